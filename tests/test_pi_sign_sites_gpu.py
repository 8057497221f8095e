"""Directed PI / PI-copy / Tx / Sig failure sites on the device (tests/golden/pi_sign_site_cases.npz, tests/pi_sign_site_cases.py): every case
makes one numbered check of csrc/pi_circuit.hpp / sign_circuit.hpp the first failure of its target row or unit, and runs with the target
where the launch arithmetic, the wrap-around and the ranges can be wrong — PI rows: rows 0, 63 / 64, 255 / 256 (the edge of a 256-thread
block) and n - 1, whose successor is row 0, with n no multiple of 64; Tx / Sig units and copy constraints: positions 0, 63, 64, 255, 256
and n - 1 of a batch, the keccak table holding the batch's rows too — through sessions, ranged sessions and the one-shot entries."""
import pytest

from tests import pi_sign_site_cases as psc

pytestmark = pytest.mark.gpu

N_SLICES = {"pi": 6, "tx": 6, "sig": 6}
SLICES = [(name, part) for name in ("pi", "tx", "sig") for part in range(N_SLICES[name])]
_ran = {}


@pytest.fixture(scope="module")
def datas(golden_dir):
    return {"pi": psc.load_pi(golden_dir), "copy": psc.load_copy(golden_dir), "tx": psc.load_sign(golden_dir, False), "sig": psc.load_sign(golden_dir, True)}


@pytest.mark.parametrize("name,part", SLICES)
def test_every_case_fails_at_its_site_on_the_device(datas, name, part):
    data = datas[name]
    if name == "pi":
        out = psc.pi_run_slice(data, None, part, N_SLICES[name])
        assert out[1] == psc.pi_expected_runs(data, part, N_SLICES[name]) and out[0] > 0
    else:
        out = psc.sign_run_slice(data, None, part, N_SLICES[name])
        assert out[1] == psc.sign_expected_runs(data, part, N_SLICES[name]) and out[0] > 0
    _ran[(name, part)] = out


def test_copy_constraints_on_the_device(datas):
    out = psc.copy_run_all(datas["copy"], None)
    assert out[0] == len(datas["copy"]) and out[1] == 6 * len(datas["copy"]) and out[2] == {1, 2}
    _ran["copy"] = out


def test_full_length_witness_on_the_device(datas):
    _ran["pifull"] = psc.pi_run_full(datas["pi"], None)


def test_no_case_was_skipped_on_the_device(datas):
    """over the tests above: cases run == cases in the file, runs made == runs declared, sites exercised == the file's census"""
    assert sorted(k for k in _ran if isinstance(k, tuple)) == sorted(SLICES) and "copy" in _ran and _ran["pifull"] == 5, "run this module as a whole"
    for name, sites in (("pi", psc.PI_SITES), ("tx", psc.TX_SITES), ("sig", psc.SIG_SITES)):
        data = datas[name]
        parts = [_ran[(name, p)] for p in range(N_SLICES[name])]
        assert sum(p[0] for p in parts) == len(data.cases)
        assert sum(p[1] for p in parts) == (psc.pi_expected_runs(data, 0, 1) if name == "pi" else psc.sign_expected_runs(data, 0, 1))
        assert sorted(set().union(*(p[2] for p in parts))) == psc.census(data.cases, sites)[0]
    assert _ran["copy"][0] == len(datas["copy"])
