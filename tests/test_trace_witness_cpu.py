"""zk_evm_witness_from_trace on the CPU backend (libzkevm_cpu.so: the per-row functions of csrc/trace_witness.hpp in host loops): RW ops
and step records to the wire rows, against the reference's recorded tables (tests/golden/evm_*.npz), a plain-Python model written from
the reference's statements (tests/trace_witness_ref.py), the reference's own RWDictionary where it is staged, and a stand-alone sanitizer
build of the header."""
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from tests import trace_witness_cases as tc
from tests import trace_witness_ref as ref
from zkevm_specs_amd import _lib, arithmetic, engine, errors, flatten, objects, oneshot, trace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ref.P


def run_cpu(rec):
    return oneshot.evm_witness_from_trace(rec, device="cpu")


# ---- (a) the reference's recorded tables: records recovered from each golden case's own wires, the wires rebuilt from them
def test_golden_wires_from_recovered_records():
    n_rw = n_steps = n_rw_skipped = n_steps_skipped = 0
    for where, rw, flags, steps in tc.golden_cases():
        ops = sr = None
        if rw.shape[0]:
            try:
                ops = trace.rw_ops_from_wire(rw, flags)
            except errors.UnsupportedOnDevice:  # (anything else fails the test)
                n_rw_skipped += 1
        try:
            sr = trace.step_records_from_wire(steps)
        except errors.UnsupportedOnDevice:
            n_steps_skipped += 1
        if ops is None and sr is None:
            continue
        res, out = run_cpu(trace.trace_records(ops, sr))
        assert res.ok and res.fail_count == 0, where
        if ops is not None:
            assert res.rows_evaluated == rw.shape[0], where
            assert np.array_equal(out["rw"], rw) and np.array_equal(out["rw_flags"], flags), where
            n_rw += 1
        if sr is not None:
            assert np.array_equal(out["steps"], steps), where
            n_steps += 1
    assert n_rw >= 3000 and n_steps >= 4000, (n_rw, n_rw_skipped, n_steps, n_steps_skipped)


# ---- (b) one long table: every accepted golden table, counters rebased, at arbitrary phases of the row writer
def test_long_table_of_golden_rows():
    rec, rw, flags = tc.long_table()
    assert rw.shape[0] >= 40000
    res, out = run_cpu(rec)
    assert res.ok and res.rows_evaluated == rw.shape[0]
    assert np.array_equal(out["rw"], rw) and np.array_equal(out["rw_flags"], flags)
    assert trace.record_bytes(rec) * 6 < rw.nbytes + flags.nbytes  # what the records are for


# ---- (c) the directed sets against the model, bit for bit
@pytest.mark.parametrize("name", tc.NAMES)
def test_directed_against_model(name):
    exp = tc.expected(name)
    res, out = run_cpu(tc.directed(name))
    assert res.ok and res.fail_count == 0 and res.rows_evaluated == exp["rw"].shape[0]
    assert tc.same(out, exp)


def test_directed_sets_cover_what_they_claim():
    c = tc.coverage()
    assert c["combos"] == set(range(32)) and c["tags"] == set(range(16)) and {0, 255} <= c["fields"]
    assert c["modes"] == {True, False, "explicit"}
    assert c["flag_forms"] == {(0, 0), (0, 1), (1, 0), (1, 1)}  # (is_word bit, wide) for value and value_prev
    for slot in range(5):
        assert set(tc.EDGE_WORDS) <= c["edge_at"][slot], slot
    for combo in (31, 0):
        assert c["ends"][combo] == {"first", "last", "before16", "at16", "before64", "at64"}, combo
    assert int(tc.directed("rw_16_a")["rw_base"]) + 16 == 1 << 64 and tc.expected("rw_16_a")["rw"][-1, 0].tolist() == [tc.U64, 0, 0, 0]
    gaps = np.diff(tc.directed("rw_17_a")["rw_counter"].astype(object))
    assert (gaps >= 1).all() and (gaps > 1).any()
    for n in tc.STEP_SIZES[2:]:
        w = tc.directed(f"steps_{n}")["steps"]
        assert all({0, tc.U64} <= set(int(x) for x in w[:, k]) for k in range(1, 9)), n
    words = {sum(int(x) << (64 * k) for k, x in enumerate(r[9:13])) for n in tc.STEP_SIZES for r in tc.directed(f"steps_{n}")["steps"]}
    assert set(tc.EDGE_WORDS) <= words
    # the canonical encoder inverts the model on the directed wires it can hold (p, p + 1 and 2^256 - 1 as FQ operands have no record)
    for name in ("rw_257_a", "rw_1025_b"):
        exp = tc.expected(name)
        back = ref.model(trace.trace_records(trace.rw_ops_from_wire(exp["rw"], exp["rw_flags"])))
        assert np.array_equal(back["rw"], exp["rw"]) and np.array_equal(back["rw_flags"], exp["rw_flags"]), name


# ---- (d) the mirror of RWDictionary against the reference's, where the reference is staged
def _call_sequence(rng, n):
    """(method, args): ("W", int) a Word, ("F", int) an FQ, ("cc" / "acc" / "log" / "rcpt", k) a field tag, the rest plain ints / bools"""
    w = lambda: ("W", rng.choice((0, 1, rng.getrandbits(64), rng.getrandbits(128), rng.getrandbits(256), (1 << 256) - 1)))  # noqa: E731
    small = lambda: rng.choice((0, 1, rng.getrandbits(16), rng.getrandbits(64)))  # noqa: E731
    addr = lambda: rng.choice((small(), rng.getrandbits(160)))  # noqa: E731
    rev, calls = [10 ** 6], []

    def reversion():
        if rng.random() < 0.5:
            return None
        rev[0] -= 1
        return rev[0]
    for _ in range(n):
        m = rng.randrange(19)
        if m == 0: calls.append((rng.choice(("stack_read", "stack_write")), (small(), rng.randrange(1024), w())))
        elif m == 1: calls.append((rng.choice(("memory_read", "memory_write")), (small(), small(), rng.randrange(256))))
        elif m == 2:
            k = rng.randrange(1, 26)
            word = k in (5, 6, 11, 17)
            calls.append((rng.choice(("call_context_read", "call_context_write")), (small(), ("cc", k), w() if word else rng.choice((small(), ("F", small()))))))
        elif m == 3:
            k = rng.randrange(1, 6)
            calls.append(("tx_log_write", (small() % 1000, rng.randrange(8), ("log", k), rng.randrange(1 << 16), w() if k in (1, 2) else small())))
        elif m == 4: calls.append((rng.choice(("tx_receipt_read", "tx_receipt_write")), (small(), ("rcpt", rng.randrange(1, 4)), small())))
        elif m == 5: calls.append(("tx_refund_read", (small(), small())))
        elif m == 6: calls.append(("tx_refund_write", (small(), small(), small(), reversion())))
        elif m == 7: calls.append(("tx_access_list_account_write", (small(), addr(), bool(rng.randrange(2)), bool(rng.randrange(2)), reversion())))
        elif m == 8: calls.append(("tx_access_list_account_read", (small(), addr(), bool(rng.randrange(2)))))
        elif m == 9: calls.append(("tx_access_list_account_storage_write", (small(), addr(), w(), bool(rng.randrange(2)), bool(rng.randrange(2)), reversion())))
        elif m == 10: calls.append(("tx_access_list_account_storage_read", (small(), addr(), w(), bool(rng.randrange(2)))))
        elif m == 11: calls.append(("account_read", (addr(), ("acc", rng.randrange(1, 5)), rng.choice((small(), w(), ("F", small()))))))
        elif m == 12: calls.append(("account_write", (addr(), ("acc", rng.randrange(1, 5)), rng.choice((small(), w())), rng.choice((small(), w())), reversion())))
        elif m == 13: calls.append(("account_storage_read", (addr(), w(), w(), rng.choice((small(), ("F", small()))), w())))
        else: calls.append(("account_storage_write", (addr(), w(), w(), w(), small(), w(), reversion())))
    return calls


def test_mirror_against_the_reference_rw_dictionary():
    root = os.path.join(ROOT, "oracle", "_ref", "src")
    if not os.path.isdir(root):
        pytest.skip("no reference staged under oracle/_ref/")
    added = [os.path.join(ROOT, "oracle", "refshim"), root]
    sys.path[:0] = added
    try:
        from zkevm_specs.evm_circuit import table as rtab
        from zkevm_specs.evm_circuit import typing as rt
        from zkevm_specs.util import FQ as RFQ
        from zkevm_specs.util import Word as RWord

        ref_tags = {"cc": rtab.CallContextFieldTag, "acc": rtab.AccountFieldTag, "log": rtab.TxLogFieldTag, "rcpt": rtab.TxReceiptFieldTag}

        def conv(a, word, fq, tags):
            if isinstance(a, tuple):
                return word(a[1]) if a[0] == "W" else fq(a[1]) if a[0] == "F" else (tags[a[0]](a[1]) if tags else a[1])
            return a
        methods = set()
        for seed in (1, 2, 3):
            calls = _call_sequence(random.Random(seed), 400)
            theirs, ours = rt.RWDictionary(7), trace.RWDictionary(7)
            for m, args in calls:
                methods.add(m)
                getattr(theirs, m)(*[conv(a, RWord, RFQ, ref_tags) for a in args])
                getattr(ours, m)(*[conv(a, arithmetic.Word, arithmetic.FQ, None) for a in args])
            assert ours.rw_counter == theirs.rw_counter
            rw, flags = flatten.flatten_rw_table(theirs.rws)
            res, out = run_cpu(trace.trace_records(ours.ops()))
            assert res.ok and np.array_equal(out["rw"], rw) and np.array_equal(out["rw_flags"], flags), seed
            assert len(theirs.rws) > len(calls)  # reversion rows took part
        public = {m for m in dir(rt.RWDictionary) if not m.startswith("_")}
        assert methods == public and public == {m for m in dir(trace.RWDictionary) if not m.startswith("_")} - {"ops"}
    finally:
        for p in added:
            sys.path.remove(p)
        for m in [m for m in sys.modules if m == "zkevm_specs" or m.startswith("zkevm_specs.")]:
            del sys.modules[m]


# ---- (e) errors and API edges
def _raw_call(rec, fn="one_shot", n_rw=None, n_pool=None, n_steps=None, want=tc.OUTPUTS, opts=0):
    lib = _lib.load_cpu()
    p = _lib.ptr
    n = rec["head"].shape[0] if n_rw is None else n_rw
    m = rec["pool"].shape[0] if n_pool is None else n_pool
    k = rec["steps"].shape[0] if n_steps is None else n_steps
    t = _lib.ZkTrace(p(rec["head"]), p(rec["id"]), p(rec["addr"]), p(rec["val"]), p(rec["prev"]), p(rec["rw_counter"]), int(rec["rw_base"]), n,
                     p(rec["pool"]), m, p(rec["steps"]), k)
    shapes = engine.evm_witness_from_trace_shapes(rec["head"].shape[0], rec["steps"].shape[0])
    out = {key: np.full(shp, 0xA5A5A5A5A5A5A5A5 >> (64 - 8 * np.dtype(dt).itemsize), dtype=dt) for key, (shp, dt) in shapes.items()}  # every byte 0xA5
    w = _lib.ZkTraceWitness(*[p(out[key]) if key in want else None for key in tc.OUTPUTS])
    if fn == "sizes":
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        rc = lib.zk_evm_witness_from_trace_sizes(ctypes.byref(t), opts, ctypes.byref(a), ctypes.byref(b))
    elif fn == "open":
        hd = ctypes.c_void_p()
        rc = lib.zk_evm_witness_from_trace_open(ctypes.byref(t), None, opts, ctypes.byref(hd))
        if rc == 0:
            lib.zk_close(hd)
    else:
        rc = lib.zk_evm_witness_from_trace(ctypes.byref(t), ctypes.byref(w), opts, ctypes.byref(_lib.ZkResult()))
    return rc, lib.zk_last_error().decode(), out


def _with_steps(name="rw_65_b", steps="steps_33"):
    rec = tc.mutable(name)
    rec["steps"] = tc.directed(steps)["steps"].copy()
    return rec


def domain_errors():
    """(label, records, overrides, code, text)"""
    cases = []
    for bit in (5, 7, 18, 19, 25, 31):
        r = _with_steps()
        r["head"][40] |= np.uint32(1 << bit)
        cases.append((f"head bit {bit}", r, {}, _lib.ERR_TRC_HEAD, "head of RW op 40"))
    for bit in (10, 63):
        r = _with_steps()
        r["steps"][32, 0] |= np.uint64(1 << bit)
        cases.append((f"step w0 bit {bit}", r, {}, _lib.ERR_TRC_HEAD, "word 0 of step 32"))
    r = _with_steps("rw_17_a")  # explicit counters
    r["rw_counter"][9] = r["rw_counter"][8]
    cases.append(("equal counters", r, {}, _lib.ERR_TRC_ORDER, "rw_counter of RW op 9"))
    r = _with_steps("rw_17_a")
    r["rw_counter"][16] = 0
    cases.append(("descending counters", r, {}, _lib.ERR_TRC_ORDER, "rw_counter of RW op 16"))
    r = _with_steps()
    r["rw_base"] = (1 << 64) - 64
    cases.append(("rw_base + n_rw passes 2^64", r, {}, _lib.ERR_TRC_ORDER, "passes 2^64"))
    r = _with_steps()
    cases.append(("a pool word too few", r, {"n_pool": r["pool"].shape[0] - 1}, _lib.ERR_TRC_POOL, f"consume {r['pool'].shape[0]} pool words"))
    r = _with_steps()
    r["pool"] = np.concatenate([r["pool"], r["pool"][:1]])
    cases.append(("a pool word too many", r, {}, _lib.ERR_TRC_POOL, f"n_pool is {r['pool'].shape[0]}"))
    r = _with_steps()
    r["head"][3] ^= np.uint32(trace.H_KEY)
    cases.append(("a head flips a pool bit", r, {}, _lib.ERR_TRC_POOL, "pool words"))
    cases.append(("2^31 RW ops", _with_steps(), {"n_rw": 1 << 31}, _lib.ERR_TRC_ROWS, "2^31 rows or more"))
    cases.append(("2^31 steps", _with_steps(), {"n_steps": 1 << 31}, _lib.ERR_TRC_ROWS, "2^31 rows or more"))
    return cases


def test_domain_errors_by_code_and_text():
    for label, rec, over, code, text in domain_errors():
        for fn in ("sizes", "open", "one_shot"):
            rc, msg, out = _raw_call(rec, fn, **over)
            assert rc == code and "zk_evm_witness_from_trace" in msg and text in msg, (label, fn, rc, msg)
            assert all((a.view(np.uint8) == 0xA5).all() for a in out.values()), (label, fn)  # nothing was written
    r = _with_steps()
    r["rw_base"] = (1 << 64) - 65  # the last counter is 2^64 - 1
    assert _raw_call(r, "sizes")[0] == 0
    r = _with_steps()
    r["head"][40] |= np.uint32(1 << 6)
    for call in (engine.evm_witness_from_trace_sizes, engine.open_evm_witness_from_trace, oneshot.evm_witness_from_trace):
        with pytest.raises(_lib.EngineError) as e:
            call(r, device="cpu")
        assert e.value.rc == _lib.ERR_TRC_HEAD
    with pytest.raises(ValueError):
        bad = _with_steps()
        bad["val"] = bad["val"][:-1]
        oneshot.evm_witness_from_trace(bad, device="cpu")
    assert _raw_call(_with_steps(), "one_shot", opts=_lib.OPT_DEVICE_PTRS)[0] != 0  # no device pointers on this backend
    assert engine.evm_witness_from_trace_sizes(_with_steps(), device="cpu") == (65, 33)


def test_null_output_members():
    rec = _with_steps()
    exp = ref.model(rec)
    for skip in range(len(tc.OUTPUTS) + 1):
        want = tuple(k for i, k in enumerate(tc.OUTPUTS) if i != skip)
        rc, _, out = _raw_call(rec, want=want)
        assert rc == 0
        for k in tc.OUTPUTS:
            assert np.array_equal(out[k], exp[k]) if k in want else (out[k].view(np.uint8) == 0xA5).all(), (skip, k)
    assert _raw_call(rec, want=())[0] == 0
    empty = trace.trace_records()
    res, out = run_cpu(empty)
    assert res.ok and res.rows_evaluated == 0 and out["rw"].shape == (0, 14, 4) and out["steps"].shape == (0, 13, 4)


def test_two_passes_read_values_anew_and_keep_the_heads():
    rec = _with_steps("rw_257_a")
    with engine.open_evm_witness_from_trace(rec, device="cpu") as s:
        assert s.n == 257
        res = s.run()
        assert res.ok and res.launches == 1 and res.rows_evaluated == 257 and tc.same(s.read(), ref.model(rec))
        rec["val"][:] = rec["val"][::-1].copy()         # values: the next pass reads them
        rec["pool"][5] = tc.limbs(P + 12345)
        rec["steps"][7, 4] = 99
        assert s.run().ok and tc.same(s.read(), ref.model(rec))
        assert not s.read_status().any()
        assert list(s.read(names=("steps",))) == ["steps"]
    rec = _with_steps("rw_257_b")
    first = ref.model(rec)
    with engine.open_evm_witness_from_trace(rec, device="cpu") as s:
        assert s.run().ok and tc.same(s.read(), first)
        rec["head"][:] = 0                               # heads: fixed at open, a rewritten head cannot move a store
        assert s.run().ok and tc.same(s.read(), first)


def test_mirror_sorts_drops_duplicates_and_refuses():
    W = arithmetic.Word
    d = trace.RWDictionary(5)
    d.stack_write(1, 1023, W(7)).memory_write(1, 0, 255).account_write(0xabc, 2, W(1 << 200), W(3), rw_counter_of_reversion=900)
    d.rows.append(d.rows[0])                             # an exact duplicate is one row of the set
    d.rows.reverse()
    ops = d.ops()
    assert ops["rw_counter"].tolist() == [5, 6, 7, 900] and ops["rw_base"] == 1
    res, out = run_cpu(trace.trace_records(ops))
    assert res.ok and out["rw"][3, 8].tolist() == [3, 0, 0, 0] and out["rw"][3, 11].tolist() == [0, 1 << 8, 0, 0]  # the reversion row swaps value and value_prev
    rows = objects.rw_table_from_wire(out["rw"], out["rw_flags"])
    assert [r.key0.n for r in rows] == [8, 9, 5, 5] and rows[2].value.int_value() == 1 << 200
    dense = trace.RWDictionary(1 << 40).stack_read(1, 2, W(3)).stack_read(1, 3, W(4)).ops()
    assert dense["rw_counter"] is None and dense["rw_base"] == 1 << 40
    clash = trace.RWDictionary(5).stack_write(1, 1, W(1))
    clash.rw_counter = 5
    clash.stack_write(1, 2, W(1))
    with pytest.raises(errors.UnsupportedOnDevice):      # two different rows with one rw_counter
        clash.ops()
    with pytest.raises(errors.UnsupportedOnDevice):      # an id of 2^64 or more
        trace.RWDictionary(1).stack_read(1 << 64, 1, W(1)).ops()
    with pytest.raises(errors.UnsupportedOnDevice):      # a counter of 2^64 or more
        trace.RWDictionary(1 << 64).stack_read(1, 1, W(1)).ops()
    with pytest.raises(errors.UnsupportedOnDevice):      # a Word half of 2^128 or more
        trace.RWDictionary(1).stack_read(1, 1, W((1 << 128, 0), check=False)).ops()
    with pytest.raises(AssertionError):                  # the reference's sanity asserts
        trace.RWDictionary(1).call_context_read(1, 5, 7)
    with pytest.raises(AssertionError):
        trace.RWDictionary(1).call_context_read(1, 1, W(7))
    with pytest.raises(AssertionError):
        trace.RWDictionary(1).tx_log_write(1, 0, 1, 0, 7)
    log = trace.RWDictionary(1).tx_log_write(3, 2, 3, 9, 0xee).ops()
    assert int(log["addr"][0]) == 9 + (3 << 32) + (2 << 48)
    with pytest.raises(errors.UnsupportedOnDevice):
        trace.step_records_from_wire(np.full((1, 13, 4), 1, np.uint64))
    steps = objects.steps_from_wire(tc.expected("steps_33")["steps"])
    assert np.array_equal(trace.step_records(steps), tc.directed("steps_33")["steps"])


# ---- (f) the header's functions under AddressSanitizer + UBSan: a stand-alone host program, run as a child process
def test_sanitizer_program(tmp_path):
    exe = str(tmp_path / "trace_witness_asan")
    src = os.path.join(ROOT, "tests", "hostsim", "trace_witness_asan.cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DZK_HOSTSIM", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",  # (the runtimes inside the program: nothing to preload)
                           "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-o", exe, src])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "trace_witness_asan: ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
