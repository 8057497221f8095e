"""Directed Withdrawal sites on the CPU backend (libzkevm_cpu.so: csrc/withdrawal_circuit.hpp compiled for the host): every (variant,
placement) of tests/withdrawal_site_cases.py through the one-shot, the session and ranged sessions with and without their halo, and the
assignment batches, bit for bit against the plain-Python model tests/withdrawal_ref.py; then the builder's own conditions, which
need the model alone."""
import pytest

from tests import withdrawal_ref as W
from tests import withdrawal_site_cases as c

CPU = "cpu"


@pytest.fixture(scope="module")
def returned():
    """the statuses the one-shot tests got, by (variant, placement): what the coverage test counts"""
    return {}


@pytest.mark.parametrize("name", list(c.VARIANTS))
def test_oneshot_cpu(name, returned):
    c.run_variant_oneshots(name, CPU, returned)


@pytest.mark.parametrize("site", c.SITES)
def test_full_session_twice_cpu(site):
    for case in c.rotating_cases(site):
        c.check_session_twice(case, CPU)


@pytest.mark.parametrize("site", c.SITES[1:])
def test_shard_rows_world3_cpu(site):
    for case in c.rotating_cases(site):
        c.check_shard_rows_world3(case, CPU)


@pytest.mark.parametrize("cut", c.CUTS)
def test_hand_cut_shards_cpu(cut):
    cases = c.boundary_cases(cut)
    assert len(cases) >= 40
    for case in cases:
        c.check_cuts(case, (cut,), CPU)


def test_all_cuts_at_once_cpu():
    """five shards, two of them of one row: [0, 64), [64, 65), [65, 256), [256, 257), [257, n)"""
    for case in c.halo_cases(64) + c.halo_cases(256):
        if c.n_eval(case.wit) > 257:
            c.check_cuts(case, c.CUTS, CPU)


@pytest.mark.parametrize("cut", c.CUTS)
def test_halo_refusal_cpu(cut):
    cases = c.halo_cases(cut)
    assert len(cases) >= 10
    seen = set()
    for case in cases:
        for lo, hi in ((0, cut), (cut, c.n_eval(case.wit))):
            for st, want in c.check_halo_refusal(case, lo, hi, CPU):
                seen |= {(k == 0, k == len(st) - 1) for k, s in enumerate(st) if s == c.HALO}
    assert seen >= {(True, False), (False, True)}  # the refusal stood on a first held row and on a last one


def test_coverage_cpu(returned):
    c.check_coverage(returned, CPU)


@pytest.mark.parametrize("k", range(len(c.batch_ids())), ids=c.batch_ids())
def test_assignment_cpu(k):
    c.check_assignment(c.batches()[k], CPU)


@pytest.mark.parametrize("pad", (0, 3, 65))
def test_assigned_witness_verifies_and_tampers_like_the_model_cpu(pad):
    c.check_assign_verify_tamper(CPU, pad)


def test_reference_judged_cases_cpu():
    assert c.check_golden(CPU) >= 20


# ---- the builder's own conditions: the model alone ------------------------------------------------------------------------------------------
def test_builder_coverage_is_complete():
    """every required (kind, site) x placement cell is the target row's status and the first failure of its witness (case() asserts that
    for each case), every valid companion is clean, and nothing stands in an unreachable cell"""
    table = c.coverage_table()
    assert set(table) == set(c.coverage_required()) and all(c.coverage_required()[k] <= v for k, v in table.items())
    companions = [x for x in c.all_cases() if x.code == 0]
    assert len(companions) >= 80 and all(not any(x.status) for x in companions)
    assert {x.variant for x in c.all_cases()} == set(c.VARIANTS)


def test_builder_key_high_half_and_carries():
    hi = {p: [x for x in c.all_cases() if x.variant.startswith("3/table_key_hi") and x.placement == p and x.wit.rows[x.target][0] >> 128]
          for p in c.PLACEMENTS}
    assert all(hi.values()), [p for p, v in hi.items() if not v]  # key hi wrong on an id of at least 2^128, at every placement
    main = c.main()
    assert main.rows[289][0] == (1 << 128) - 1 and main.rows[290][0] == 1 << 128
    wrap = c.wrap()
    assert wrap.rows[0][0] == W.P - 290 and wrap.rows[289][0] == W.P - 1 and wrap.rows[290][0] == 0 and not any(c.status_of(wrap))


def test_builder_payload_moves_both_ways():
    moves = {c.payload_moves(x) for x in c.cases("2") if x.variant.startswith("2/payload")}
    assert any(a >= 56 and b == 55 for a, b in moves) and any(a <= 55 and b == 56 for a, b in moves)


def test_builder_assign_is_the_models():
    b = c.batches()[0]
    assert c.assign(b.wds[:70], b.roots[:70], 75, b.r) == W.assign(b.wds[:70], b.roots[:70], 75, b.r)
    assert c.assign([], [], 3, 5) == W.assign([], [], 3, 5)


def test_builder_batches_cover_the_rlp_paths():
    sweep = c.batches()[0].wds
    assert {c.payload_len(w) for w in sweep} >= set(range(4, 133)) and (W.P - 1,) * 4 in sweep
    for f in range(4):
        assert {(len(W.rlp_int(w[f])) if w[f] >= 0x80 else 0) for w in sweep} >= set(range(2, 34)), f  # byte lengths 1..32 behind a prefix
        assert {w[f] for w in sweep} >= {0, 1, 0x7F, 0x80, 0xFF}, f
    heavy_lanes = {i % 64 for i, w in enumerate(sweep) if c.heavy(w)}
    assert {0, 63} <= heavy_lanes and all(c.heavy(w) for w in sweep[len(sweep) - len(sweep) % 64:])
