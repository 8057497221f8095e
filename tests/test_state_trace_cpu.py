"""zk_state_verify_from_trace* / zk_state_ops_from_trace* on the CPU backend: the State verdict and the State op list of compact trace
records, DEFINED BY COMPOSITION — what the _from_rw entries return over the rw / rw_flags zk_evm_witness_from_trace writes for the same
records.  Every case of tests/state_trace_cases.py is compared with that composition, the smaller ones also with the plain-Python chain
(tests/trace_witness_ref.py records -> wire, oracle.rw_state_oracle, assign_oracle, state_oracle), and a stand-alone sanitizer build
runs the header's per-row functions."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import assign_oracle, rw_state_oracle, state_oracle, wire
from tests import state_trace_cases as sc
from tests import trace_witness_ref as ref
from zkevm_specs_amd import _lib, engine, oneshot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def verdict(r):
    return (r.fail_count, r.first_fail_row, r.first_fail_code, r.rows_evaluated)


@pytest.fixture(scope="module")
def expanded():
    """name -> (rw, rw_flags) of the case's records, by the CPU backend's zk_evm_witness_from_trace: computed once per case, never changed"""
    cache = {}

    def get(rec, name=None):
        if name is None or name not in cache:
            res, w = oneshot.evm_witness_from_trace({**rec, "steps": None}, device="cpu")
            assert res.ok
            if name is None:
                return w["rw"], w["rw_flags"]
            cache[name] = (w["rw"], w["rw_flags"])
        return cache[name]

    return get


def oracle_chain(rec):
    """records -> the State statuses by the plain-Python chain (oracle_statuses of tests/test_state_fused.py behind the record model)"""
    w = ref.model({**rec, "steps": np.zeros((0, 13), np.uint64)})
    ops, op_flags, _ = rw_state_oracle.rw_to_state_ops(wire.rowmajor_to_rows(w["rw"]), w["rw_flags"].tolist(), strict=True)
    st_rows, row_flags, mpt, status = assign_oracle.assign(ops, op_flags)
    assert not any(status)
    return state_oracle.verify_rows(st_rows, row_flags, mpt)


def check_verify(rec, rw, fl, device, with_oracle):
    """the verdict form against the composition on `device`; -> fail_count"""
    r, st = oneshot.state_verify_from_trace(rec, device=device)
    r2, st2 = oneshot.state_verify_from_rw(rw, fl, device=device)
    assert len(st) == len(st2) and np.array_equal(st, st2), [(j, hex(st[j]), hex(st2[j])) for j in np.nonzero(st != st2)[0][:5]]
    assert verdict(r) == verdict(r2)
    if with_oracle:
        want = oracle_chain(rec)
        assert st.tolist() == want, [(j, hex(st[j]), hex(want[j])) for j in range(len(want)) if st[j] != want[j]][:5]
    return int(r.fail_count)


def check_ops(rec, rw, fl, device, with_oracle):
    r, st, ops, of = oneshot.state_ops_from_trace(rec, device=device)
    r2, st2, ops2, of2 = oneshot.state_ops_from_rw(rw, fl, device=device)
    assert verdict(r) == verdict(r2) and np.array_equal(st, st2) and ops.shape == ops2.shape and np.array_equal(ops, ops2) and np.array_equal(of, of2)
    if with_oracle:
        w = ref.model({**rec, "steps": np.zeros((0, 13), np.uint64)})
        e_ops, e_flags, e_status = rw_state_oracle.rw_to_state_ops(wire.rowmajor_to_rows(w["rw"]), w["rw_flags"].tolist(), strict=False)
        assert st.tolist() == e_status and wire.colmajor_to_rows(ops) == e_ops and of.tolist() == e_flags
    return ops


def test_cases_cover_what_they_claim():
    sc.assert_coverage()
    _, _, ops, _ = oneshot.state_ops_from_trace(sc.case("tame_1025"), device="cpu")
    keys = ops[2:7].transpose(1, 0, 2).reshape(ops.shape[1], -1)
    edges = np.concatenate([[0, 1], 1 + np.nonzero((keys[2:] != keys[1:-1]).any(axis=1))[0] + 1, [len(keys)]])  # group starts (op 0: StartOp)
    starts, ends = edges[1:-1], edges[2:] - 1
    lengths = ends - starts + 1
    assert lengths.min() == 1 and 17 <= lengths.max() <= 40
    assert ((starts // 63) != (ends // 63)).any()    # a group across a wavefront edge of the evaluation kernel
    assert ((starts // 256) != (ends // 256)).any()  # ... and across a 256-op assignment block


@pytest.mark.parametrize("name", sc.TAME + sc.VALID)
def test_verdict_equals_the_composition(name, expanded):
    rec = sc.case(name)
    fails = check_verify(rec, *expanded(rec, name), "cpu", len(rec["head"]) <= sc.ORACLE_MAX)
    if name in sc.VALID:
        assert fails == 0  # a consistent table: the derived witness satisfies the State circuit


@pytest.mark.parametrize("name", sc.WILD + sc.TAME[:8] + sc.VALID)
def test_op_list_equals_the_composition(name, expanded):
    rec = sc.case(name)
    check_ops(rec, *expanded(rec, name), "cpu", len(rec["head"]) <= sc.ORACLE_MAX)


@pytest.mark.parametrize("name", sc.VALID)
def test_damaged_tables(name, expanded):
    rec = sc.damage(name, max(8, len(sc.case(name)["head"]) // 40), seed=3)
    assert check_verify(rec, *expanded(rec), "cpu", True) >= 3


def test_big_table(expanded):
    rec = sc.case(sc.BIG)
    assert len(rec["head"]) == sc.N_BIG
    rw, fl = expanded(rec)
    check_verify(rec, rw, fl, "cpu", False)
    check_ops(rec, rw, fl, "cpu", False)


def error_of(call, *args, **kw):
    with pytest.raises(_lib.EngineError) as e:
        call(*args, **kw)
    text = str(e.value)
    return e.value.rc, text[text.index("): ") + 3:]  # (behind "<what> failed (rc=..): ")


def retitled(text, name):
    """the from-RW / trace-witness text under the new entry's name: everything behind the first colon stays"""
    return name + text[text.index(":"):]


def check_no_witness(device, expanded):
    for label, rec in sc.no_witness():
        rw, fl = expanded(rec)
        rc, want = error_of(oneshot.state_verify_from_rw, rw, fl, device=device)
        rc2, got = error_of(oneshot.state_verify_from_trace, rec, device=device)
        assert rc == rc2 == -1 and got.startswith("zk_state_verify_from_trace") and got == retitled(want, "zk_state_verify_from_trace"), (label, got, want)
        check_ops(rec, rw, fl, device, False)  # the ops form reports the rejected rows as codes


def test_no_witness_raises_with_the_from_rw_text(expanded):
    check_no_witness("cpu", expanded)


def _raw(lib, rec, entry, n_rw=None, n_pool=None, opts=0, prev=True):
    """one raw call of a from-trace entry -> (rc, text)"""
    p = _lib.ptr
    n = rec["head"].shape[0] if n_rw is None else n_rw
    m = rec["pool"].shape[0] if n_pool is None else n_pool
    t = _lib.ZkTrace(p(rec["head"]), p(rec["id"]), p(rec["addr"]), p(rec["val"]), p(rec["prev"]) if prev else None, p(rec["rw_counter"]),
                     int(rec["rw_base"]), n, p(rec["pool"]), m, None, 0)
    cap = rec["head"].shape[0] + 1
    st, n_ops, res, h = np.zeros(cap, np.uint32), ctypes.c_uint64(), _lib.ZkResult(), ctypes.c_void_p()
    if entry == "verify_open":
        rc = lib.zk_state_verify_from_trace_open(ctypes.byref(t), opts, ctypes.byref(n_ops), ctypes.byref(h))
    elif entry == "verify":
        rc = lib.zk_state_verify_from_trace(ctypes.byref(t), opts, p(st), ctypes.byref(n_ops), ctypes.byref(res))
    elif entry == "ops_open":
        rc = lib.zk_state_ops_from_trace_open(ctypes.byref(t), None, None, opts, ctypes.byref(n_ops), ctypes.byref(h))
    else:
        ops, of = np.zeros(48 * cap, np.uint64), np.zeros(cap, np.uint32)
        rc = lib.zk_state_ops_from_trace(ctypes.byref(t), p(ops), p(of), ctypes.byref(n_ops), opts, p(st), ctypes.byref(res))
    if rc == 0 and h:
        lib.zk_close(h)
    return rc, lib.zk_last_error().decode()


def domain_errors():
    """(label, records, overrides, code, text) — the trace session's domain errors (tests/test_trace_witness_cpu.py), over RW records"""
    cases = []
    for bit in (5, 7, 18, 19, 25, 31):
        r = sc.mutable("tame_65")
        r["head"][40] |= np.uint32(1 << bit)
        cases.append((f"head bit {bit}", r, {}, _lib.ERR_TRC_HEAD, "the head of RW op 40 has a reserved bit set"))
    r = sc.mutable("tame_63")  # explicit counters
    assert r["rw_counter"] is not None
    r["rw_counter"][9] = r["rw_counter"][8]
    cases.append(("equal counters", r, {}, _lib.ERR_TRC_ORDER, "the rw_counter of RW op 9 does not exceed the one before it (rw_counters must be strictly ascending)"))
    r = sc.mutable("tame_63")
    r["rw_counter"][16] = 0
    cases.append(("descending counters", r, {}, _lib.ERR_TRC_ORDER, "the rw_counter of RW op 16 does not exceed"))
    r = sc.mutable("tame_65")
    r["rw_counter"], r["rw_base"] = None, (1 << 64) - 64
    cases.append(("rw_base + n_rw passes 2^64", r, {}, _lib.ERR_TRC_ORDER, f"rw_base {(1 << 64) - 64} + 65 RW ops passes 2^64"))
    r = sc.mutable("tame_65")
    m = r["pool"].shape[0]
    cases.append(("a pool word too few", r, {"n_pool": m - 1}, _lib.ERR_TRC_POOL, f"the heads consume {m} pool words, n_pool is {m - 1}"))
    r = sc.mutable("tame_65")
    r["pool"] = np.concatenate([r["pool"], r["pool"][:1]])
    cases.append(("a pool word too many", r, {}, _lib.ERR_TRC_POOL, f"the heads consume {m} pool words, n_pool is {m + 1}"))
    r = sc.mutable("tame_65")
    r["head"][3] ^= np.uint32(1 << 21)
    cases.append(("a head flips a pool bit", r, {}, _lib.ERR_TRC_POOL, "pool words"))
    cases.append(("2^31 RW ops", sc.mutable("tame_65"), {"n_rw": 1 << 31}, _lib.ERR_TRC_ROWS, f"{1 << 31} RW ops, 0 steps (a table of 2^31 rows or more)"))
    return cases


def check_domain_errors(lib, opts=0, to_dev=lambda rec: rec):
    for label, rec, over, code, text in domain_errors():
        rec = to_dev(rec)
        for entry in ("verify_open", "verify", "ops_open", "ops"):
            rc, msg = _raw(lib, rec, entry, opts=opts, **over)
            name = "zk_state_verify_from_trace" if entry.startswith("verify") else "zk_state_ops_from_trace"
            assert rc == code and msg.startswith(name + ": ") and text in msg, (label, entry, rc, msg)


def test_domain_errors_by_code_and_text():
    lib = _lib.load_cpu()
    check_domain_errors(lib)
    # the text is the trace session's apart from the entry's name
    r = sc.mutable("tame_65")
    r["head"][40] |= np.uint32(1 << 6)
    rc, want = error_of(oneshot.evm_witness_from_trace, {**r, "steps": None}, device="cpu")
    for call, name in ((oneshot.state_verify_from_trace, "zk_state_verify_from_trace"), (oneshot.state_ops_from_trace, "zk_state_ops_from_trace"),
                       (engine.open_state_verify_from_trace, "zk_state_verify_from_trace"), (engine.open_state_ops_from_trace, "zk_state_ops_from_trace")):
        rc2, got = error_of(call, r, device="cpu")
        assert rc == rc2 == _lib.ERR_TRC_HEAD and got == retitled(want, name)
    r = sc.mutable("tame_65")
    r["rw_counter"], r["rw_base"] = None, (1 << 64) - 65  # the last counter is 2^64 - 1
    assert _raw(lib, r, "verify")[0] == 0
    assert _raw(lib, sc.mutable("tame_65"), "verify", opts=_lib.OPT_DEVICE_PTRS)[0] != 0  # no device pointers on this backend
    with pytest.raises(ValueError):
        bad = sc.mutable("tame_65")
        bad["val"] = bad["val"][:-1]
        oneshot.state_verify_from_trace(bad, device="cpu")


def check_missing_inputs(device, expanded):
    """prev null and steps absent (neither is read); garbage in prev changes nothing"""
    rec = sc.mutable("tame_253")
    rw, fl = expanded(rec)
    want = oneshot.state_verify_from_rw(rw, fl, device=device)
    for change in ({"prev": None}, {"prev": np.full_like(rec["prev"], 0xA5A5A5A5A5A5A5A5)}, {"steps": np.zeros((0, 13), np.uint64)}):
        r, st = oneshot.state_verify_from_trace({**rec, **change}, device=device)
        assert verdict(r) == verdict(want[0]) and np.array_equal(st, want[1]), list(change)
        _, st_ops, ops, of = oneshot.state_ops_from_trace({**rec, **change}, device=device)
        w = oneshot.state_ops_from_rw(rw, fl, device=device)
        assert np.array_equal(st_ops, w[1]) and np.array_equal(ops, w[2]) and np.array_equal(of, w[3])


def test_null_prev_and_absent_steps(expanded):
    check_missing_inputs("cpu", expanded)
    lib = _lib.load_cpu()
    for entry in ("verify_open", "verify", "ops_open", "ops"):
        assert _raw(lib, sc.mutable("tame_65"), entry, prev=False)[0] == 0


@pytest.mark.parametrize("env", ({"ZK_REKEY_NO_FAST": "0"}, {"ZK_REKEY_NO_FAST": "1"}, {"ZK_REKEY_NO_RANKS": "1"}))
def test_sort_switches(env, monkeypatch, expanded):
    for k, v in env.items():
        monkeypatch.setenv(k, v)  # (both are read per open)
    for name in ("directed_tame", "tame_1025", "valid_block"):
        rec = sc.case(name)
        check_verify(rec, *expanded(rec, name), "cpu", False)
    rec = sc.case("wild_1025")
    check_ops(rec, *expanded(rec, "wild_1025"), "cpu", False)


def check_resident(device, to_dev=lambda rec: rec, zero=lambda a: a.fill(0)):
    """three passes give identical results, also with the caller's heads zeroed after open (the session keeps its own)"""
    for zero_heads in (False, True):
        rec = to_dev(sc.mutable("tame_1025"))
        want = oneshot.state_verify_from_trace(sc.case("tame_1025"), device=device)
        with engine.open_state_verify_from_trace(rec, device=device) as s:
            if zero_heads:
                zero(rec["head"])
            for _ in range(3):
                r = s.run()
                st = s.read_status()
                assert r.rows_evaluated == s.n == len(st) and verdict(r) == verdict(want[0]) and np.array_equal(st, want[1])
        rec = to_dev(sc.mutable("wild_1025"))
        want = oneshot.state_ops_from_trace(sc.case("wild_1025"), device=device)
        with engine.open_state_ops_from_trace(rec, device=device) as s:
            if zero_heads:
                zero(rec["head"])
            for _ in range(3):
                r = s.run()
                ops, of = s.read()
                assert verdict(r) == verdict(want[0]) and np.array_equal(s.read_status(), want[1]) and np.array_equal(ops, want[2]) and np.array_equal(of, want[3])


def test_resident_passes():
    check_resident("cpu")


def test_sanitizer_program(tmp_path):
    """the header's per-row functions and the CPU entry under -fsanitize=address,undefined, as a stand-alone child process"""
    exe = str(tmp_path / "state_trace_asan")
    src = os.path.join(ROOT, "tests", "hostsim", "state_trace_asan.cpp")
    # (-O0 -g1: the program holds the whole CPU backend, whose optimised sanitizer build takes a minute and a half)
    subprocess.check_call(["g++", "-O0", "-g1", "-std=c++17", "-DZK_HOSTSIM", "-fopenmp", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",  # (the runtimes inside the program: nothing to preload)
                           "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-Wno-array-bounds", "-o", exe, src, "-ldl"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "state_trace_asan: ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
