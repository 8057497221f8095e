"""BN254 device arithmetic on the MI355X (k_ecc.hip's zk_fr_op hooks) against tests/bn254_ref.py (checks: tests/ecc_kat.py)."""
import pytest

from tests import ecc_kat

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from zkevm_specs_amd import _lib

    return _lib.init()


@pytest.mark.parametrize("check", ["fq_mul", "fq12_ops", "final_exp", "pairing", "g2_chain"])
def test_bn254_known_answers_hip(lib, check):
    getattr(ecc_kat, "check_" + check)(lib)
