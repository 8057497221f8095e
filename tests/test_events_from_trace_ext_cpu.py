"""zk_events_from_trace_ext* on the CPU backend: the copy events of BeginTx, RETURN / REVERT and DATACOPY steps (and every event
zk_events_from_trace derives) against the plain-Python model of tests/events_from_trace_ext_ref.py, bit for bit (events, flags, both refs,
step indices, statuses, tally, counts, capacities); the domain errors with their codes and texts under this entry's name; the identity with
zk_events_from_trace on that entry's tables; the reference-recorded goldens of the three states; the derived events through
zk_copy_assign_from_sources; a stand-alone sanitizer build of the CPU entries."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import copy_sources_cases as csc
from tests import copy_sources_ref as csref
from tests import events_from_trace_cases as cc
from tests import events_from_trace_ext_cases as xc
from tests import events_from_trace_ext_ref as xref
from tests import events_from_trace_ref as ref
from tests import test_events_from_trace_cpu as old
from zkevm_specs_amd import _lib, engine, oneshot, trace
from zkevm_specs_amd.errors import UnsupportedOnDevice
from zkevm_specs_amd.evm_tables import ExecutionState as ES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = "cpu"
NAME = "zk_events_from_trace_ext"
GOLDEN_KINDS = {"return_revert": (33, 24), "begin_tx": (29, 4), "dataCopy": (1, 1)}  # cases used / cases that emit, at least
GOLDEN_UNSUPPORTED = {"create": ("CREATE", "CREATE2"), "callop": ("CALL_OP",)}


def run(c, device=DEVICE):
    return oneshot.events_from_trace_ext(c["trace"], c["codes"], c["hashes"], device=device)


def test_cases_hit_what_they_claim():
    for name in xc.NAMES:
        c, want = xc.case(name), xc.expected(name)
        assert {s: int(x) for s, x in enumerate(want["status"]) if x} == c["want"], name
    sites = xc.case("sites")["want"]
    assert {x & 0xFFFFFF for x in sites.values() if x >> 24 == ref.KIND_VALUE_ERROR} == {1, 2, 3, 4, 5}
    assert sum(1 for x in sites.values() if x == ref.UNSUPPORTED_CODE) == len(xref.STILL_UNSUPPORTED) == 3
    # the forms: both counter modes, every tag pair, both Word destinations with their refs, zero-length events, the twin hash
    assert xc.case("forms")["trace"]["rw_counter"] is None and xc.case("forms_gaps")["trace"]["rw_counter"] is not None
    for name in ("forms", "forms_gaps"):
        c, w = xc.case(name), xc.expected(name)
        ev, steps = w["copy_events"], c["trace"]["steps"]
        state = [int(steps[s, 0]) & 0xFF for s in w["copy_step"]]
        tags = {(st, int(e[2, 0]), int(e[5, 0])) for st, e in zip(state, ev)}
        assert {(int(ES.RETURN), 2, 1), (int(ES.RETURN), 2, 2), (int(ES.DATACOPY), 2, 2), (int(ES.BeginTx), 3, 5), (int(ES.BeginTx), 3, 1)} <= tags
        to_code = [(e, f, d) for e, f, d in zip(ev, w["copy_flags"], w["copy_dst_ref"]) if int(e[5, 0]) == 1]
        assert all(int(f) == 2 for _, f, _ in to_code) and {int(d) for _, _, d in to_code} == {0, 4, 5}  # H_A's first code, DEPLOYED, INIT
        assert all(int(d) == 0 for e, d in zip(ev, w["copy_dst_ref"]) if int(e[5, 0]) != 1)
        assert any(e[4].any() for e, _, _ in to_code)       # a destination hash with a non-zero upper half
        ret_mem = [e for st, e in zip(state, ev) if st == int(ES.RETURN) and int(e[5, 0]) == 2]
        assert sorted(int(e[9, 0]) for e in ret_mem) == [0, 0, 8, 20, 20] and {int(e[3, 0]) for e in ret_mem} == {2, 9}  # min(len, rl); next.call_id
        # DATACOPY(c 6, cdo 10, cdl 7, rdo 3, rdl 5): the second event 8 + min(8, 7) counters behind the first - neither 2 cdl nor 2 (rdo + rdl)
        dc = [(int(s), e) for st, s, e in zip(state, w["copy_step"], ev) if st == int(ES.DATACOPY)]
        assert dc[0][0] == dc[1][0] and int(dc[1][1][11, 0]) - int(dc[0][1][11, 0]) == 15 and int(dc[0][1][9, 0]) == 8 and int(dc[1][1][9, 0]) == 5
        assert len(dc) == 8 and sum(1 for _, e in dc if int(e[9, 0]) == 0) == 2
        # BeginTx: the create path twice (one with EndTx behind it), the other three forms silent
        bt = [s for s in range(len(steps)) if int(steps[s, 0]) & 0xFF == int(ES.BeginTx)]
        emitting = [s for s in bt if s in set(w["copy_step"].tolist())]
        assert len(bt) == 5 and len(emitting) == 2 and int(steps[emitting[1] + 1, 0]) & 0xFF == int(ES.EndTx)
        assert all(int(steps[s + 1, 1]) == int(steps[s, 1]) + 23 for s in emitting) and not w["status"][bt].any()
    assert len(xc.case("forms")["trace"]["pool"]) >= 8
    # the last-step forms, the exact fill, the ladders' edges
    for f in xc.LAST_FORMS:
        c = xc.case(f"last_{f}")
        assert set(c["want"]) <= {len(c["trace"]["steps"]) - 1}
    w = xc.expected("pairs_257")
    assert len(w["copy_step"]) == 514 == xref.capacities(xc.case("pairs_257")["trace"])[0] and not w["status"].any()
    for n in xc.LADDER_SIZES:
        for p in xc.LADDER_PATTERNS:
            c, w = xc.case(f"ladder_{n}_{p}"), xc.expected(f"ladder_{n}_{p}")
            assert len(w["status"]) == n and not w["status"][: n - 1].any()
            per_step = np.bincount(w["copy_step"], minlength=n)
            if p == "none":
                assert not len(w["copy_step"]) and not len(w["exp_step"])
                assert n < 4 or xref.capacities(c["trace"])[0] > n  # BeginTx steps that count and emit nothing
            for i, k in ((63, 2), (64, 1), (255, 2), (256, 1)):
                if p != "none" and i < n - 1:
                    assert per_step[i] == (k if p == "alt" else 3 - k), (n, p, i)
    w = xc.expected("ladder_1025_all")
    assert len(w["copy_step"]) > 1025 and len(w["exp_step"]) > 200


@pytest.mark.parametrize("name", xc.NAMES)
def test_equals_the_model(name):
    xc.check_outputs(name, *run(xc.case(name)))


def check_sizes(device):
    for name in ("forms_gaps", "pairs_257", "ladder_257_none", "ladder_1025_alt", "last_begin_tx_create"):
        c = xc.case(name)
        assert engine.events_from_trace_ext_sizes(c["trace"], c["codes"], c["hashes"], device=device) == xref.capacities(c["trace"]), name


def test_sizes():
    check_sizes(DEVICE)


def check_session(device, stream=None):
    """a session: counts before and after a pass, two passes (the second after zk_session_set_stream) with equal results, read by name"""
    for name in ("forms_gaps", "sites", "ladder_257_alt", "pairs_257"):
        c, want = xc.case(name), xc.expected(name)
        with engine.open_events_from_trace_ext(c["trace"], c["codes"], c["hashes"], device=device) as s:
            assert s.n == len(want["status"]) and s.counts() == (0, 0)
            r1 = s.run()
            out1, st1 = s.read(), s.read_status()
            assert s.counts() == (len(want["copy_step"]), len(want["exp_step"]))
            s.set_stream(stream)
            r2 = s.run()
            out2, st2 = s.read(), s.read_status()
            xc.check_outputs(name, r1, st1, out1)
            xc.check_outputs(name, r2, st2, out2)
            part = s.read(("copy_dst_ref", "exp_step"))
            assert set(part) == {"copy_dst_ref", "exp_step"} and np.array_equal(part["copy_dst_ref"], want["copy_dst_ref"])


def test_session():
    check_session(DEVICE)


def domain_errors():
    """the domain errors of zk_events_from_trace, under this entry's name"""
    return [(label, c, rc, NAME + text[text.index(": "):]) for label, c, rc, text in old.domain_errors()]


@pytest.mark.parametrize("label,c,rc,text", domain_errors(), ids=[d[0] for d in domain_errors()])
def test_domain_errors(label, c, rc, text):
    args = (c["trace"], c["codes"], c["hashes"])
    assert old.error_of(engine.events_from_trace_ext_sizes, *args, device=DEVICE) == (rc, text)
    assert old.error_of(engine.open_events_from_trace_ext, *args, device=DEVICE) == (rc, text)
    assert old.error_of(oneshot.events_from_trace_ext, *args, device=DEVICE) == (rc, text)


def check_too_many_rows(device):
    c = xc.case("forms")
    lib = _lib.init(device)
    n, m, big = ctypes.c_uint64(), ctypes.c_uint64(), 1 << 31
    ns, nb, nc = len(c["trace"]["steps"]), sum(len(x) for x in c["codes"]), len(c["codes"])
    for field, rc, text in (("n_steps", _lib.ERR_TEV_ROWS, f"{NAME}: {big} steps, {nb} code bytes, {nc} codes (2^31 or more)"),
                            ("n_code_bytes", _lib.ERR_TEV_ROWS, f"{NAME}: {ns} steps, {big} code bytes, {nc} codes (2^31 or more)"),
                            ("n_codes", _lib.ERR_TEV_ROWS, f"{NAME}: {ns} steps, {nb} code bytes, {big} codes (2^31 or more)"),
                            ("n_rw", _lib.ERR_TRC_ROWS, f"{NAME}: {big} RW ops, {ns} steps (a table of 2^31 rows or more)")):
        p = engine._wire_args(engine.TRACE_EVENTS_EXT, engine.trace_event_sources(c["trace"], c["codes"], c["hashes"]))
        setattr(p.t.trace if field in ("n_steps", "n_rw") else p.t, field, big)
        assert lib.zk_events_from_trace_ext_sizes(ctypes.byref(p.t), p.opts, ctypes.byref(n), ctypes.byref(m)) == rc, field
        assert lib.zk_last_error().decode() == text


def test_too_many_rows():
    check_too_many_rows(DEVICE)


# ---- the identity with zk_events_from_trace ---------------------------------------------------------------------------------------------
def check_identity(device):
    """On every table of tests/events_from_trace_cases.py: all outputs of zk_events_from_trace, and copy_dst_ref all zero.  Those tables
    hold a few BeginTx / RETURN / DATACOPY steps over plain ops (the old entry's UNSUPPORTED status): here they have the model's status -
    no event either - and every other status is the old entry's."""
    for name in cc.NAMES:
        c = cc.case(name)
        r0, st0, out0 = oneshot.events_from_trace(c["trace"], c["codes"], c["hashes"], device=device)
        r1, st1, out1 = run(c, device)
        for k in cc.OUTPUTS:
            assert out1[k].dtype == out0[k].dtype and np.array_equal(out1[k], out0[k]), (name, k)
        assert out1["copy_dst_ref"].shape == out0["copy_src_ref"].shape and not out1["copy_dst_ref"].any()
        new = np.isin(np.asarray(c["trace"]["steps"])[:, 0] & np.uint64(0xFF), np.array(sorted(xref.NEW_STATES), dtype=np.uint64))
        assert np.array_equal(st1[~new], st0[~new]) and (st0[new] == ref.UNSUPPORTED_CODE).all(), name
        want = xref.derive(c["trace"], c["codes"], c["hashes"])
        assert np.array_equal(st1, want["status"]), name
        if not new.any():
            assert (r1.fail_count, r1.first_fail_row, r1.first_fail_code) == (r0.fail_count, r0.first_fail_row, r0.first_fail_code)


def test_identity_with_the_old_entry():
    check_identity(DEVICE)


# ---- the reference-recorded goldens -------------------------------------------------------------------------------------------------
def _records(g):
    try:
        return dict(trace.rw_ops_from_wire(g["rw"], g["rw_flags"]), steps=trace.step_records_from_wire(g["steps"]))
    except UnsupportedOnDevice:
        return None


def with_written_codes(rec, codes, hashes):
    """The goldens' bytecode tables hold the codes that are READ; a caller of this entry also lists the codes its trace WRITES (their
    index is the dst_ref).  The hashes come from the records - every CodeHash a CallContext op or an Account write carries - and each
    gets an empty placeholder code: this entry never reads a written code's bytes."""
    codes, hashes = list(codes), list(hashes)
    for op in ref.ops_by_counter(rec).values():
        is_hash = (op["tag"] == ref.Target.CallContext and op["addr"] == int(ref.CC.CodeHash)) or (
            op["tag"] == ref.Target.Account and op["write"] and op["field"] == int(ref.AccountFieldTag.CodeHash))
        if is_hash and op["value"] not in hashes:
            codes.append(b"")
            hashes.append(op["value"])
    return codes, hashes


def check_goldens(golden_dir, device):
    """every accepted golden case of the three states that the records can hold: the derived copy events are the golden copy table's
    events as sets (the key of tests/test_events_from_trace_cpu.py) -> kind -> (cases used, cases that emit)"""
    counts = {}
    for kind in GOLDEN_KINDS:
        used = emitting = 0
        for g in old.golden_cases(golden_dir, kind):
            rec = None if g["ref_kind"].any() else _records(g)
            if rec is None:
                continue
            codes, hashes = with_written_codes(rec, *old.codes_of_bytecode_table(g["bytecode"]))
            res, status, out = run({"trace": rec, "codes": codes, "hashes": hashes}, device)

            def key(cells, tx_log):
                v = [ref._word(x) for x in cells]
                return tuple(v[:8] + ([] if tx_log else [v[8]]) + [v[9], v[10]])

            derived = {key(list(e[:10]) + [e[11]], int(e[5, 0]) == ref.TX_LOG) for e in out["copy_events"]}
            golden = {key(list(r[1:11]) + [r[12]], int(r[6, 0]) == ref.TX_LOG) for r in g["copy"]}
            assert derived == golden, (kind, used, status)
            assert len(out["copy_events"]) == len(derived)  # no event twice
            used += 1
            emitting += 1 if len(golden) else 0
        counts[kind] = (used, emitting)
    return counts


def check_unsupported_goldens(golden_dir, device):
    """evm_create / evm_callop: every step of those states is UNSUPPORTED and emits nothing"""
    seen = {}
    for kind, states in GOLDEN_UNSUPPORTED.items():
        codes_of = {int(ES[s]) for s in states}
        seen[kind] = 0
        for g in old.golden_cases(golden_dir, kind):
            rec = _records(g)
            if rec is None:
                continue
            codes, hashes = old.codes_of_bytecode_table(g["bytecode"])
            res, status, out = run({"trace": rec, "codes": codes, "hashes": hashes}, device)
            mine = np.nonzero(np.isin(rec["steps"][:, 0] & np.uint64(0xFF), np.array(sorted(codes_of), dtype=np.uint64)))[0]
            assert len(mine) and (status[mine] == ref.UNSUPPORTED_CODE).all(), (kind, seen[kind])
            assert not np.isin(out["copy_step"], mine).any() and not np.isin(out["exp_step"], mine).any()
            seen[kind] += 1
    return seen


def test_goldens(golden_dir):
    counts = check_goldens(golden_dir, DEVICE)
    assert all(counts[k][0] >= u and counts[k][1] >= e for k, (u, e) in GOLDEN_KINDS.items()), counts
    seen = check_unsupported_goldens(golden_dir, DEVICE)
    assert all(n >= 100 for n in seen.values()), seen


# ---- the derived events through zk_copy_assign_from_sources -----------------------------------------------------------------------------
def check_pipeline(device):
    """the pipeline table's events, src_ref and dst_ref into zk_copy_assign_from_sources (the code set holds the deployed code and the init
    code under the hashes the steps carry, tx 1's calldata is the init code): every output is zk_copy_assign's over the MODEL's events
    with the bytes the plain-Python gather finds"""
    c, want = xc.case("pipeline"), xc.expected("pipeline")
    res, status, out = run(c, device)
    xc.check_outputs("pipeline", res, status, out)
    assert res.ok and len(out["copy_events"]) == 7
    assert {int(d) for e, d in zip(out["copy_events"], out["copy_dst_ref"]) if int(e[5, 0]) == 1} == {c["codes"].index(xc.DEPLOYED), c["codes"].index(xc.INIT)}
    calldata = b"".join(c["calldata"])
    sources = {"code": np.frombuffer(b"".join(c["codes"]), np.uint8).copy(), "code_offsets": np.cumsum([0] + [len(x) for x in c["codes"]]).astype(np.uint64),
               "calldata": np.frombuffer(calldata, np.uint8).copy(), "calldata_offsets": np.cumsum([0] + [len(x) for x in c["calldata"]]).astype(np.uint64),
               "trace": {k: v for k, v in c["trace"].items() if k != "steps"}}
    r = 0x1234567
    model = csref.model(want["copy_events"], want["copy_src_ref"], want["copy_dst_ref"], sources)
    assert not model[2].any() and len(model[0]) == len(xc.INIT) * 2 + len(xc.DEPLOYED) + 9 + 3 + 7 + 5
    got = oneshot.copy_assign_from_sources(out["copy_events"], out["copy_flags"], out["copy_src_ref"], out["copy_dst_ref"], sources, r, device=device)
    csc.check_outputs({"events": want["copy_events"], "flags": want["copy_flags"], "r": r}, model, got, device)


def test_pipeline():
    check_pipeline(DEVICE)


def test_sanitizer_program(tmp_path):
    """the CPU entries over exactly-sized heap buffers under -fsanitize=address,undefined, as a stand-alone child process"""
    exe = str(tmp_path / "events_from_trace_ext_asan")
    src = os.path.join(ROOT, "tests", "hostsim", "events_from_trace_ext_asan.cpp")
    # (-O0 -g1: the program holds the whole CPU backend, whose optimised sanitizer build takes a minute and a half)
    subprocess.check_call(["g++", "-O0", "-g1", "-std=c++17", "-DZK_HOSTSIM", "-fopenmp", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",  # (the runtimes inside the program: nothing to preload)
                           "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-Wno-array-bounds", "-o", exe, src, "-ldl"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "events_from_trace_ext_asan: ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
