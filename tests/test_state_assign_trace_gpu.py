"""zk_state_assign_from_trace* on the device (assign_rows_trace_kernel / assign_rows_trace_pair_kernel of csrc/k_assign.hip): the cases of
tests/state_trace_cases.py and tests/state_assign_trace_cases.py against the composition on HIP (the from-RW session over the rows the
trace-witness session writes) — through host buffers and over device-resident records with guarded caller buffers and every combination
of null output pointers, in the 57-cell and the compact form, with both writers, on the fast and the generic sort, first and second pass —
against the CPU backend on the 73,729-row table, chained into open_state without a host copy, and behind SuperCircuit(state_trace=...)."""
import itertools

import numpy as np
import pytest

from tests import state_assign_trace_cases as ac
from tests import state_trace_cases as sc
from tests.test_state_assign_trace_cpu import (check_assign, check_domain_errors, check_missing_inputs, check_rejected_rows,
                                               check_rows_feed_the_state_circuit, check_two_passes, composition, expand, expanded,  # noqa: F401
                                               records_of, same_witness)
from tests.test_state_trace_cpu import verdict
from tests.test_trace_witness_gpu import dev, dev_records, guarded, guards_intact, host
from zkevm_specs_amd import _lib, engine, oneshot, trace

pytestmark = pytest.mark.gpu

WRITERS = ("lane", "pair")  # ZK_STATE_TRACE_WRITER: the lane-per-op writer (the default) and the half-cell-per-lane one


@pytest.fixture(params=WRITERS)
def writer(request, monkeypatch):
    monkeypatch.setenv("ZK_STATE_TRACE_WRITER", request.param)  # (read per launch)
    return request.param


@pytest.mark.parametrize("name", sc.TAME + sc.VALID + ac.ALL)
def test_host_buffers(name, expanded, writer):
    r = check_assign(records_of(name), *expanded(name, None), None)[0]
    assert r.ok or name in sc.TAME


def test_rejected_rows_and_failing_ops(writer):
    check_rejected_rows(None)
    for label, rec in sc.no_witness():  # a rejected tag nibble, addresses wider than 160 bits, Account field tags outside 1..4
        r = check_assign(rec, *expand(rec, None), None)[0]
        assert r.fail_count >= 1, label


def resident(name, expanded, compact, nulls=(), passes=2):
    """device-resident records; rows, flags, MPT rows and statuses into guarded caller buffers of capacity n_rw + 1 (`nulls`: the outputs the
    session owns instead); first pass, then a second one"""
    import torch

    rec = records_of(name)
    n, nc = len(rec["head"]), 15 if compact else 57
    want = composition(*expanded(name, None), None, compact)
    up = dev_records(rec)
    bufs = {"rows": guarded((nc * 4 * (n + 1),), np.uint64), "flags": guarded((n + 1,), np.uint32), "mpt": guarded((48 * (n + 1),), np.uint64)}
    f_st, status = guarded((n + 1,), np.uint32)
    own = {k: (None if k in nulls else v[1]) for k, v in bufs.items()}
    with engine.open_state_assign_from_trace(up, own["rows"], own["flags"], own["mpt"], compact=compact) as s:
        m = s.n
        assert m == len(want[1]) and s.compact == compact
        for _ in range(passes):
            s.launch(status[:m])
            r = s.collect()
            torch.cuda.synchronize()
            k = s.n_mpt()
            assert k == len(want[4])
            got = {"rows": None, "flags": None, "mpt": None}
            if own["rows"] is not None:
                got["rows"] = host(own["rows"], np.uint64)[: nc * 4 * m].reshape(nc, m, 4)
                assert bool((own["rows"][nc * 4 * m:] == -1).all())  # packed for n_ops: nothing behind them
            if own["flags"] is not None:
                got["flags"] = host(own["flags"], np.uint32)[:m]
                assert bool((own["flags"][m:] == -1).all())
            if own["mpt"] is not None:
                got["mpt"] = host(own["mpt"], np.uint64)[: 48 * k].reshape(k, 12, 4)
                assert bool((own["mpt"][48 * k:] == -1).all())
            read = s.read()
            full = [read[i] if got[key] is None else got[key] for i, key in enumerate(("rows", "flags", "mpt"))]
            same_witness((r, host(status, np.uint32)[:m], *full), want)
            same_witness((r, host(status, np.uint32)[:m], *read), want)  # (the session's read over buffers of the caller's)
            assert bool((status[m:] == -1).all()) and guards_intact(f_st) and all(guards_intact(v[0]) for v in bufs.values())
            for v in bufs.values():
                v[1].fill_(-1)
            status.fill_(-1)


@pytest.mark.parametrize("compact", (False, True))
@pytest.mark.parametrize("name", ["directed_tame", "tame_1", "tame_63", "tame_253", "tame_1025", "tame_8193", "valid_block"] + ac.ALL)
def test_resident_records_caller_buffers(name, compact, expanded, writer):
    resident(name, expanded, compact)


@pytest.mark.parametrize("nulls", [c for k in range(1, 4) for c in itertools.combinations(("rows", "flags", "mpt"), k)])
def test_null_output_pointers(nulls, expanded):
    for compact in (False, True):
        resident("aimed_257", expanded, compact, nulls=nulls)


@pytest.mark.parametrize("env", ({"ZK_REKEY_NO_FAST": "0"}, {"ZK_REKEY_NO_FAST": "1"}))
def test_sort_forms(env, monkeypatch, expanded, writer):
    for k, v in env.items():
        monkeypatch.setenv(k, v)  # (read per open)
    for name in ("directed_tame", "tame_4097", "aimed_4098", "block_edge"):
        for compact in (False, True):
            resident(name, expanded, compact)


def test_hip_equals_cpu_backend_on_the_big_table(writer):
    rec = sc.case(sc.BIG)
    for compact in (False, True):
        same_witness(oneshot.state_assign_from_trace(rec, compact=compact), oneshot.state_assign_from_trace(rec, device="cpu", compact=compact))


def test_missing_inputs(expanded):
    check_missing_inputs(None, expanded)
    rec = sc.mutable("tame_253")
    want = oneshot.state_assign_from_trace(rec)
    with engine.open_state_assign_from_trace(dev_records({**rec, "prev": None})) as s:  # resident records without prev and without steps
        r = s.run()
        same_witness((r, s.read_status(), *s.read()), want)


def test_two_passes_keep_the_heads(writer):
    check_two_passes(None)
    check_two_passes(None, to_dev=dev_records, zero=lambda t: t.zero_())


def test_rows_feed_the_state_circuit_through_host_buffers():
    check_rows_feed_the_state_circuit(None)


@pytest.mark.parametrize("compact", (False, True))
def test_rows_assigned_in_place_chain_into_open_state(compact, writer):
    """records resident in HBM -> rows, flags and MPT rows in caller buffers -> open_state over views of those buffers, no host copy: a clean
    block, and the block with three cells damaged in record space"""
    import torch

    for rec in (sc.case("valid_block"), sc.damage("valid_block", 3, seed=9)):
        n, nc = len(rec["head"]), 15 if compact else 57
        want = oneshot.state_verify_from_trace(rec)
        rows_b = torch.empty(nc * 4 * (n + 1), dtype=torch.int64, device="cuda")
        flags_b = torch.empty(n + 1, dtype=torch.int32, device="cuda")
        mpt_b = torch.empty(48 * (n + 1), dtype=torch.int64, device="cuda")
        with engine.open_state_assign_from_trace(dev_records(rec), rows_b, flags_b, mpt_b, compact=compact) as a:
            assert a.run().ok
            m, k = a.n, a.n_mpt()
        with engine.open_state(rows_b[: nc * 4 * m].view(nc, m, 4), flags_b[:m], mpt_b[: 48 * k].view(k, 12, 4), compact=compact) as s:
            r = s.run()
            assert verdict(r) == verdict(want[0]) and np.array_equal(s.read_status(), want[1])
        assert r.ok == (rec is sc.case("valid_block")) and (r.ok or r.fail_count >= 1)


def test_domain_errors_of_host_and_resident_records():
    lib = _lib.init(None)
    check_domain_errors(lib)
    check_domain_errors(lib, opts=_lib.OPT_DEVICE_PTRS, to_dev=dev_records)


def test_super_circuit_state_trace():
    """SuperCircuit(state_trace=records of the block's RW table): every circuit's (count, first row, code) is that of the same SuperCircuit
    without the keyword, in the three State forms, on the clean block and with one Memory value damaged"""
    from zkevm_specs_amd import evm_tables as ET
    from zkevm_specs_amd.super_circuit import SuperCircuit, synth_super_block

    p = synth_super_block(13, seed=7)
    rw = p["evm"]["rw"]
    assert p["state_ops"] is None

    def verdicts(**kw):
        with SuperCircuit(p, to_device=dev, **kw) as s:
            s.launch()
            return {k: (r.fail_count, r.first_fail_row, r.first_fail_code) for k, r in s.collect()[0].items()}

    j = next(i for i in range(rw.shape[0] // 2, rw.shape[0]) if int(rw[i, 2, 0]) == int(ET.Target.Memory) and int(rw[i, 1, 0]) == 0)
    for damaged in (False, True):
        if damaged:
            rw[j, 8, 0] ^= np.uint64(1)
        records = trace.rw_ops_from_wire(rw, p["evm"]["rw_flags"])  # (the caller's contract: the records expand to evm["rw"])
        for form in ({}, {"state_compact": True}, {"state_fused": True}):
            want = verdicts(**form)
            assert verdicts(state_trace=records, **form) == want
            assert (want["state"][0] != 0) == damaged
    rw[j, 8, 0] ^= np.uint64(1)
