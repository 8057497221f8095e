"""Directed Withdrawal sites on the MI355X (k_withdrawal.hip: withdrawal_rows_kernel, withdrawal_assign_kernel, wd_mpt_index_kernel): every (variant,
placement) of tests/withdrawal_site_cases.py through the one-shot, the session and ranged sessions with and without their halo, and the
assignment batches, bit for bit against the plain-Python model tests/withdrawal_ref.py.  Reads tests/golden/ and the tree only."""
import pytest

from tests import withdrawal_site_cases as c

pytestmark = pytest.mark.gpu
HIP = None


@pytest.fixture(scope="module")
def returned():
    """the statuses the one-shot tests got, by (variant, placement): what the coverage test counts"""
    return {}


@pytest.mark.parametrize("name", list(c.VARIANTS))
def test_oneshot_hip(name, returned):
    c.run_variant_oneshots(name, HIP, returned)


@pytest.mark.parametrize("site", c.SITES)
def test_full_session_twice_hip(site):
    for case in c.rotating_cases(site):
        c.check_session_twice(case, HIP)


@pytest.mark.parametrize("site", c.SITES[1:])
def test_shard_rows_world3_hip(site):
    for case in c.rotating_cases(site):
        c.check_shard_rows_world3(case, HIP)


@pytest.mark.parametrize("cut", c.CUTS)
def test_hand_cut_shards_hip(cut):
    cases = c.boundary_cases(cut)
    assert len(cases) >= 40
    for case in cases:
        c.check_cuts(case, (cut,), HIP)


def test_all_cuts_at_once_hip():
    """five shards, two of them of one row: [0, 64), [64, 65), [65, 256), [256, 257), [257, n)"""
    for case in c.halo_cases(64) + c.halo_cases(256):
        if c.n_eval(case.wit) > 257:
            c.check_cuts(case, c.CUTS, HIP)


@pytest.mark.parametrize("cut", c.CUTS)
def test_halo_refusal_hip(cut):
    cases = c.halo_cases(cut)
    assert len(cases) >= 10
    seen = set()
    for case in cases:
        for lo, hi in ((0, cut), (cut, c.n_eval(case.wit))):
            for st, want in c.check_halo_refusal(case, lo, hi, HIP):
                seen |= {(k == 0, k == len(st) - 1) for k, s in enumerate(st) if s == c.HALO}
    assert seen >= {(True, False), (False, True)}  # the refusal stood on a first held row and on a last one


def test_coverage_hip(returned):
    c.check_coverage(returned, HIP)


@pytest.mark.parametrize("k", range(len(c.batch_ids())), ids=c.batch_ids())
def test_assignment_hip(k):
    c.check_assignment(c.batches()[k], HIP)


@pytest.mark.parametrize("pad", (0, 3, 65))
def test_assigned_witness_verifies_and_tampers_like_the_model_hip(pad):
    c.check_assign_verify_tamper(HIP, pad)


def test_reference_judged_cases_hip():
    assert c.check_golden(HIP) >= 20
