"""BN254 device arithmetic on the CPU backend (libzkevm_cpu.so: csrc/bn254_fq.hpp compiled for the host) through the zk_fr_op
known-answer hooks, against tests/bn254_ref.py (checks: tests/ecc_kat.py)."""
import pytest

from tests import ecc_kat


@pytest.fixture(scope="module")
def lib():
    from zkevm_specs_amd import _lib

    return _lib.init("cpu")


@pytest.mark.parametrize("check", ["fq_mul", "fq12_ops", "final_exp", "pairing", "g2_chain"])
def test_bn254_known_answers_cpu(lib, check):
    getattr(ecc_kat, "check_" + check)(lib)
