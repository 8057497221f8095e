"""Directed checkpoint cases of the EVM circuit on the device (tests/golden/checkpoint_cases.npz, tests/checkpoint_cases.py): every case
makes one checkpoint of csrc/evm_circuit.hpp the first one to fail, so a checkpoint that the kernels lack, number differently or check
more weakly than the oracle shows as a wrong status code.  Tiny sessions, a few thousand per test function."""
import numpy as np
import pytest

from oracle import codes
from tests import checkpoint_cases as cc
from tests.evm_cases import oracle_status
from zkevm_specs_amd import engine

pytestmark = pytest.mark.gpu

N_SLICES = 4  # contiguous quarters of the file (cases are grouped by base, bases by golden file): no one function dominates the suite


@pytest.fixture(scope="module")
def loaded(golden_dir):
    return cc.load(golden_dir)


def _run(w, opts, state_sort=True, generic_index=False):
    with engine.open_evm(w, bool(opts[0]), bool(opts[1]), state_sort=state_sort, generic_index=generic_index) as s:
        res = s.run()
        return res, s.read_status().tolist()


def _check_tally(res, exp):  # as tests/test_evm_gpu.py
    fails = [j for j, c in enumerate(exp) if c]
    assert res.fail_count == len(fails)
    if fails:
        assert res.first_fail_row == fails[0] and res.first_fail_code == exp[fails[0]]
    else:
        assert res.first_fail_row is None


def _check(res, status, exp, c, b, where):
    assert status == exp, where
    _check_tally(res, exp)
    assert status[b.pair] == c.code and codes.kind_of(status[b.pair]) == c.ref_kind, where


@pytest.mark.parametrize("part", range(N_SLICES))
def test_every_case_fails_at_its_checkpoint_on_the_device(golden_dir, loaded, part):
    """state-sorted sessions for every case; every third case in trace order, every seventh with the generic index, every fifth through
    the one-shot entry: status of every pair == the oracle's, the tally, and the kind of the patched pair == the reference's"""
    from zkevm_specs_amd import oneshot

    n_cases = len(loaded[1])
    lo, hi = part * n_cases // N_SLICES, (part + 1) * n_cases // N_SLICES
    n = 0
    for k, c, b, name, w, opts in cc.iter_cases(golden_dir, loaded):
        if not lo <= k < hi:
            continue
        exp = oracle_status(w, opts)
        where = (k, b.file, name, b.pair, c.patches)
        assert exp[b.pair] == c.code, where
        _check(*_run(w, opts), exp, c, b, where)
        if k % 3 == 0:
            _check(*_run(w, opts, state_sort=False), exp, c, b, where + ("trace order",))
        if k % 7 == 0:
            _check(*_run(w, opts, generic_index=True), exp, c, b, where + ("generic index",))
        if k % 5 == 0:
            res, st = oneshot.evm_verify(w, bool(opts[0]), bool(opts[1]))
            _check(res, st.tolist(), exp, c, b, where + ("one-shot",))
        n += 1
    assert n == hi - lo >= 500


def test_wide_cases_are_final_in_a_caller_buffer_after_a_stream_sync(golden_dir, loaded):
    """cases whose patch makes a staged step cell >= 2^64 or a word cell >= 2^128 leave the fast kernel (deferred pairs): their verdict
    must be in a caller-provided status buffer once the stream has drained, without zk_collect, as in
    tests/test_evm_gpu.py::test_caller_status_buffer_is_final_after_a_stream_sync"""
    import torch

    wide = [k for k, c in enumerate(loaded[1]) if cc.is_wide(c)]
    assert len(wide) >= 300
    pick = set(wide[:: max(1, len(wide) // 120)])
    n = 0
    for k, c, b, name, w, opts in cc.iter_cases(golden_dir, loaded):
        if k not in pick:
            continue
        exp = oracle_status(w, opts)
        with engine.open_evm(dict(w), bool(opts[0]), bool(opts[1])) as s:
            buf = torch.full((len(exp),), 0x7fffffff, dtype=torch.int32, device="cuda")
            s.launch(status_dev=buf)
            torch.cuda.synchronize()  # the caller's own synchronisation; zk_collect has not run
            assert buf.cpu().numpy().view(np.uint32).tolist() == exp, (k, b.file, name, c.patches)
            _check_tally(s.collect(), exp)
        n += 1
    assert n >= 30


def test_equal_rw_rows_count_once_under_the_last_end_block(golden_dir):
    """a repeated RW row (tests/checkpoint_cases.py DUPLICATE_RW_ROW_WITNESSES): the device counts it while it builds the generic RW
    index (EvmDyn::agg_rw_dups) and accepts the last EndBlock pair as the reference and the oracle do — sessions in both orders, the
    generic index, and the one-shot entry"""
    from zkevm_specs_amd import oneshot

    n = 0
    for w, opts, pair in cc.duplicate_rw_row_witnesses(golden_dir):
        exp = oracle_status(w, opts)
        assert exp[pair] == 0
        for kw in ({}, {"state_sort": False}, {"generic_index": True}):
            res, status = _run(w, opts, **kw)
            assert status == exp, kw
            _check_tally(res, exp)
        res, st = oneshot.evm_verify(w, bool(opts[0]), bool(opts[1]))
        assert st.tolist() == exp
        _check_tally(res, exp)
        n += 1
    assert n == 2
