"""zk_evm_witness_from_trace on the device (csrc/k_trace_witness.hip): RW ops and step records to the wire rows — host buffers, records
resident in HBM with guarded caller-owned outputs, sessions, and the chains into the EVM circuit and the from-RW State verdict without a
host copy — against the plain-Python model of tests/trace_witness_ref.py and the CPU backend."""
import itertools
import os
import re

import numpy as np
import pytest

from tests import evm_cases
from tests import trace_witness_cases as tc
from tests.test_state_rekey import _valid_block_rw
from zkevm_specs_amd import engine, errors, oneshot, trace
from zkevm_specs_amd.wire import rows_to_rowmajor

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GUARD = 512  # words of -1 on either side of every caller-owned output


def dev(x):
    import torch

    if x is None:
        return None
    x = np.array(x)  # (a writable copy: the shared case arrays are read-only)
    return torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x.view(np.int32) if x.dtype == np.uint32 else x).cuda()


def dev_records(rec):
    return {k: dev(v) if hasattr(v, "dtype") else v for k, v in rec.items()}


def guarded(shape, dtype):
    """(flat tensor of -1 with GUARD words around the output, the output's view) in HBM"""
    import torch

    n = int(np.prod(shape))
    flat = torch.full((n + 2 * GUARD,), -1, dtype=torch.int64 if dtype == np.uint64 else torch.int32, device="cuda")
    return flat, flat[GUARD : GUARD + n].view(shape)


def guards_intact(flat):
    return bool((flat[:GUARD] == -1).all()) and bool((flat[-GUARD:] == -1).all())


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def shapes_of(rec):
    return engine.evm_witness_from_trace_shapes(rec["head"].shape[0], rec["steps"].shape[0])


def both(name="rw_257_a", steps="steps_65"):
    """an RW case and a step case in one records dict"""
    rec = tc.mutable(name)
    rec["steps"] = tc.directed(steps)["steps"].copy()
    return rec


@pytest.mark.parametrize("name", tc.NAMES)
def test_directed_host_buffers(name):
    exp = tc.expected(name)
    res, out = oneshot.evm_witness_from_trace(tc.directed(name))
    assert res.ok and res.fail_count == 0 and res.rows_evaluated == exp["rw"].shape[0]
    assert tc.same(out, exp)


@pytest.mark.parametrize("name", tc.NAMES)
def test_directed_resident_inputs_caller_buffers(name):
    import torch

    rec, exp = tc.directed(name), tc.expected(name)
    shapes = shapes_of(rec)
    bufs = {k: guarded(shp, dt) for k, (shp, dt) in shapes.items()}
    up = dev_records(rec)
    assert engine.evm_witness_from_trace_sizes(up) == (exp["rw"].shape[0], exp["steps"].shape[0])
    with engine.open_evm_witness_from_trace(up, outs={k: v[1] for k, v in bufs.items()}) as s:
        res = s.run()
        torch.cuda.synchronize()
        assert res.ok and res.rows_evaluated == exp["rw"].shape[0]
        got = {k: host(bufs[k][1], shapes[k][1]) for k in tc.OUTPUTS}
        assert tc.same(got, exp)
        assert all(guards_intact(bufs[k][0]) for k in tc.OUTPUTS)
        assert tc.same(s.read(), exp)
        assert not s.read_status().any()


def test_hip_equals_cpu_backend_on_the_long_golden_table():
    rec, rw, flags = tc.long_table()
    cpu = oneshot.evm_witness_from_trace(rec, device="cpu")
    hip = oneshot.evm_witness_from_trace(rec)
    assert hip[0].ok and hip[0].rows_evaluated == cpu[0].rows_evaluated == rw.shape[0] >= 40000
    assert tc.same(hip[1], cpu[1])
    assert np.array_equal(hip[1]["rw"], rw) and np.array_equal(hip[1]["rw_flags"], flags)


def test_two_passes_with_a_pool_word_and_a_narrow_value_changed_in_hbm():
    import torch

    rec = both()
    up = dev_records(rec)
    with engine.open_evm_witness_from_trace(up) as s:
        assert s.run().ok and tc.same(s.read(), tc.ref.model(rec))
        narrow = int(np.flatnonzero((rec["head"] & trace.H_VALUE_POOL) == 0)[40])
        rec["pool"][17] = tc.limbs(tc.P + 54321)
        rec["val"][narrow] = 0x1234567
        rec["steps"][64, 5] = 77
        up["pool"][17] = dev(rec["pool"][17:18])[0]
        up["val"][narrow] = 0x1234567
        up["steps"][64, 5] = 77
        up["head"].zero_()  # the heads were fixed at open: a rewritten head cannot move a store
        torch.cuda.synchronize()
        exp2 = tc.ref.model(rec)
        assert not np.array_equal(exp2["rw"], tc.expected("rw_257_a")["rw"])
        res = s.run()
        assert res.ok and res.launches == 1
        assert tc.same(s.read(), exp2)


@pytest.mark.parametrize("given", list(itertools.product((False, True), repeat=3)))
def test_null_members_of_out_dev(given):
    rec = both()
    exp, shapes = tc.ref.model(rec), shapes_of(rec)
    bufs = {k: guarded(*shapes[k]) for k, g in zip(tc.OUTPUTS, given) if g}
    with engine.open_evm_witness_from_trace(dev_records(rec), outs={k: v[1] for k, v in bufs.items()}) as s:
        assert s.run().ok
        got = s.read()  # the session's own buffers, or the caller's: the last pass's outputs either way
    assert tc.same(got, exp)
    for k, (flat, out) in bufs.items():
        assert np.array_equal(host(out, shapes[k][1]), exp[k]) and guards_intact(flat), k


def test_domain_errors_of_resident_records():
    from tests.test_trace_witness_cpu import domain_errors
    from zkevm_specs_amd import _lib

    for label, rec, over, code, text in domain_errors():
        if over:
            continue  # (counts that differ from the arrays' extents: the raw-call cases of the CPU suite)
        for call in (engine.evm_witness_from_trace_sizes, engine.open_evm_witness_from_trace):
            with pytest.raises(_lib.EngineError, match=re.escape(text)) as e:
                call(dev_records(rec))
            assert e.value.rc == code, label


def _golden_case(file):
    """the first case of `file` whose RW table and steps the records hold"""
    for name, w, opts, _ in evm_cases.load_cases(os.path.join(GOLDEN, file)):
        try:
            if w["rw"].shape[0]:
                return name, w, opts, trace.trace_records(trace.rw_ops_from_wire(w["rw"], w["rw_flags"]), trace.step_records_from_wire(w["steps"]))
        except errors.UnsupportedOnDevice:
            continue
    raise AssertionError(f"{file}: no such case")


@pytest.mark.parametrize("file", ["evm_add_sub.npz", "evm_memory.npz", "evm_sload.npz", "evm_callop.npz", "evm_begin_tx.npz"],
                         ids=["add_sub", "memory", "storage", "callop", "begin_tx"])
def test_chain_into_the_evm_circuit_without_a_host_copy(file):
    name, w, opts, rec = _golden_case(file)
    w = {k: np.ascontiguousarray(v) for k, v in w.items()}
    with engine.open_evm({k: dev(v) for k, v in w.items()}, bool(opts[0]), bool(opts[1])) as c:  # the golden's own tables
        assert c.run().rows_evaluated == w["steps"].shape[0] - 1
        expected = c.read_status()
    shapes = shapes_of(rec)
    outs = {k: guarded(*shapes[k])[1] for k in tc.OUTPUTS}
    wire = {k: dev(v) for k, v in w.items() if k not in outs}
    wire.update(outs)
    with engine.open_evm_witness_from_trace(dev_records(rec), outs=outs) as a:
        assert a.run().ok
        with engine.open_evm(wire, bool(opts[0]), bool(opts[1])) as c:
            res = c.run()
            status = c.read_status()
    assert status.tolist() == expected.tolist(), name
    assert res.fail_count == int((expected != 0).sum())
    for k in tc.OUTPUTS:
        assert np.array_equal(host(outs[k], w[k].dtype), w[k]), k


def test_chain_into_the_state_verdict_from_rw():
    rows, flags = _valid_block_rw(300)  # a consistent trace: the derived witness satisfies the State circuit
    rw, fl = rows_to_rowmajor(rows, 14), np.array(flags, dtype=np.uint32)
    with engine.open_state_verify_from_rw(dev(rw), dev(fl)) as s:  # over the uploaded wire
        want = s.run()
        want_status = s.read_status()
    rec = trace.trace_records(trace.rw_ops_from_wire(rw, fl))
    shapes = shapes_of(rec)
    outs = {k: guarded(*shapes[k])[1] for k in ("rw", "rw_flags")}
    with engine.open_evm_witness_from_trace(dev_records(rec), outs=outs) as a:
        assert a.run().ok
        with engine.open_state_verify_from_rw(outs["rw"], outs["rw_flags"]) as s:
            got = s.run()
            assert np.array_equal(s.read_status(), want_status)
    assert (got.fail_count, got.first_fail_row, got.rows_evaluated) == (want.fail_count, want.first_fail_row, want.rows_evaluated)
    assert want.ok and want.rows_evaluated > 300
