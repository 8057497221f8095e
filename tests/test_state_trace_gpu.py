"""zk_state_verify_from_trace* / zk_state_ops_from_trace* on the device: the cases of tests/state_trace_cases.py against the composition
(the _from_rw entries over the expanded rows) on HIP — through host buffers and over device-resident records with guarded caller buffers,
on the fast and the generic sort, first pass and resident passes — against the CPU backend on the 73,729-row table, and chained with the
trace-witness session on one set of resident records."""
import numpy as np
import pytest

from tests import state_trace_cases as sc
from tests.test_state_trace_cpu import (check_domain_errors, check_missing_inputs, check_no_witness, check_ops, check_resident, check_verify,
                                        expanded, verdict)  # noqa: F401  (expanded: the module-scoped fixture)
from tests.test_trace_witness_gpu import dev, dev_records, guarded, guards_intact, host
from zkevm_specs_amd import _lib, engine, oneshot

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sc.TAME + sc.VALID)
def test_host_buffers_verdict(name, expanded):
    rec = sc.case(name)
    fails = check_verify(rec, *expanded(rec, name), None, False)
    assert fails == 0 or name not in sc.VALID


@pytest.mark.parametrize("name", sc.WILD + sc.VALID)
def test_host_buffers_op_list(name, expanded):
    rec = sc.case(name)
    check_ops(rec, *expanded(rec, name), None, False)


@pytest.mark.parametrize("name", sc.VALID)
def test_damaged_tables(name, expanded):
    rec = sc.damage(name, max(8, len(sc.case(name)["head"]) // 40), seed=3)
    assert check_verify(rec, *expanded(rec), None, False) >= 3


def test_no_witness_raises_with_the_from_rw_text(expanded):
    check_no_witness(None, expanded)


def resident_verdict(name, expanded, passes=3):
    """device-resident records, the statuses into a guarded caller buffer; first pass, then resident passes"""
    import torch

    rec = sc.case(name)
    want = oneshot.state_verify_from_rw(*expanded(rec, name), device="cpu")
    up = dev_records(rec)
    with engine.open_state_verify_from_trace(up) as s:
        assert s.n == len(want[1])
        flat, status = guarded((s.n,), np.uint32)
        for _ in range(passes):
            s.launch(status)
            r = s.collect()
            torch.cuda.synchronize()
            assert verdict(r) == verdict(want[0]) and np.array_equal(host(status, np.uint32), want[1])
            assert guards_intact(flat)
            status.fill_(-1)


def resident_op_list(name, expanded, passes=2):
    import torch

    rec = sc.case(name)
    n = len(rec["head"])
    want = oneshot.state_ops_from_rw(*expanded(rec, name), device="cpu")
    up = dev_records(rec)
    f_ops, ops = guarded((48 * (n + 1),), np.uint64)
    f_of, of = guarded((n + 1,), np.uint32)
    f_st, status = guarded((n,), np.uint32)
    with engine.open_state_ops_from_trace(up, ops_dev=ops, op_flags_dev=of) as s:
        m = s.n_ops
        assert m == want[2].shape[1]
        for _ in range(passes):
            s.launch(status)
            r = s.collect()
            torch.cuda.synchronize()
            assert verdict(r) == verdict(want[0]) and np.array_equal(host(status, np.uint32), want[1])
            assert np.array_equal(host(ops, np.uint64)[: 48 * m].reshape(12, m, 4), want[2]) and np.array_equal(host(of, np.uint32)[:m], want[3])
            assert bool((ops[48 * m:] == -1).all()) and bool((of[m:] == -1).all())  # packed for n_ops: nothing behind them
            assert guards_intact(f_ops) and guards_intact(f_of) and guards_intact(f_st)
            got_ops, got_of = s.read()
            assert np.array_equal(got_ops, want[2]) and np.array_equal(got_of, want[3])


@pytest.mark.parametrize("name", ["directed_tame", "tame_1", "tame_63", "tame_253", "tame_1025", "tame_8193", "valid_block"])
def test_resident_records_verdict(name, expanded):
    resident_verdict(name, expanded)


@pytest.mark.parametrize("name", ["directed_wild", "wild_1", "wild_64", "wild_252", "wild_1024", "wild_8193"])
def test_resident_records_op_list(name, expanded):
    resident_op_list(name, expanded)


@pytest.mark.parametrize("env", ({"ZK_REKEY_NO_FAST": "0"}, {"ZK_REKEY_NO_FAST": "1"}, {"ZK_REKEY_NO_RANKS": "1"},
                                 {"ZK_REKEY_NO_FAST": "1", "ZK_REKEY_NO_RANKS": "1"}))
def test_sort_forms(env, monkeypatch, expanded):
    """the fast sort (keys of at most 64 bits), the generic one, with and without ranked fields: first pass and two resident passes"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)  # (both are read per open)
    for name in ("directed_tame", "tame_4097", "tame_8193"):
        resident_verdict(name, expanded)
    resident_op_list("wild_8192", expanded)
    rec = sc.case("valid_directed")
    assert check_verify(rec, *expanded(rec, "valid_directed"), None, False) == 0


def test_hip_equals_cpu_backend_on_the_big_table(expanded):
    rec = sc.case(sc.BIG)
    want = oneshot.state_verify_from_trace(rec, device="cpu")
    got = oneshot.state_verify_from_trace(rec)
    assert verdict(got[0]) == verdict(want[0]) and np.array_equal(got[1], want[1])
    want = oneshot.state_ops_from_trace(rec, device="cpu")
    got = oneshot.state_ops_from_trace(rec)
    assert verdict(got[0]) == verdict(want[0]) and all(np.array_equal(a, b) for a, b in zip(got[1:], want[1:]))
    resident_verdict(sc.BIG, expanded)


def test_chained_with_the_trace_witness_session_on_one_set_of_resident_records():
    from zkevm_specs_amd import trace

    rec = trace.trace_records(sc.case("valid_block"))
    up = dev_records(rec)
    n = len(rec["head"])
    outs = {"rw": guarded((n, 14, 4), np.uint64)[1], "rw_flags": guarded((n,), np.uint32)[1]}
    with engine.open_evm_witness_from_trace(up, outs=outs) as a, engine.open_state_verify_from_trace(up) as t:
        assert a.run().ok
        got = t.run()
        got_status = t.read_status()
        with engine.open_state_verify_from_rw(outs["rw"], outs["rw_flags"]) as s:  # the State verdict over the expanded wire
            want = s.run()
            assert np.array_equal(s.read_status(), got_status)
        assert verdict(got) == verdict(want) and want.ok and want.rows_evaluated > 300
        assert verdict(t.run()) == verdict(want) and np.array_equal(t.read_status(), got_status)  # a resident pass behind the other session's


def test_missing_inputs(expanded):
    check_missing_inputs(None, expanded)
    rec = sc.mutable("tame_253")
    want = oneshot.state_verify_from_trace(rec)
    up = dev_records({**rec, "prev": None})  # resident records without prev and without steps
    with engine.open_state_verify_from_trace(up) as s:
        assert verdict(s.run()) == verdict(want[0]) and np.array_equal(s.read_status(), want[1])


def test_resident_passes_keep_the_heads():
    check_resident(None)
    check_resident(None, to_dev=dev_records, zero=lambda t: t.zero_())


def test_domain_errors_of_host_and_resident_records():
    lib = _lib.init(None)
    check_domain_errors(lib)
    check_domain_errors(lib, opts=_lib.OPT_DEVICE_PTRS, to_dev=dev_records)
