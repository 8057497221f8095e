"""zk_sha3_from_trace* on the CPU backend: the messages the SHA3 steps of compact trace records hash, their keccak rows and the status per
step against the plain-Python model of tests/trace_sha3_ref.py, bit for bit (rows, steps, data, offsets, statuses, tally, counts); the
session form, with passes after the caller rewrote its records; the domain errors with their codes and texts; the composition (the rows
are zk_keccak_table's over the returned data); the reference-recorded SHA3 goldens; a consistent synthetic block; a stand-alone
sanitizer build of the header's functions and the CPU entries."""
import collections
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import trace_sha3_cases as cc
from tests import trace_sha3_ref as ref
from zkevm_specs_amd import _lib, engine, oneshot, trace
from zkevm_specs_amd.errors import UnsupportedOnDevice
from zkevm_specs_amd.super_circuit import _digest_of_row
from zkevm_specs_amd.synth_block import synth_block_codes, synth_block_sha3_inputs, synth_block_trace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = "cpu"
GOLDEN_USED = (12, 3, 3)  # cases of tests/golden/evm_sha3.npz; accepted / rejected ones the records can hold


def run(c, device=DEVICE):
    return oneshot.sha3_from_trace(c["trace"], c["randomness"], device=device)


def messages_of(out):
    off = out["data_offsets"]
    return [bytes(out["data"][int(a):int(b)]) for a, b in zip(off[:-1], off[1:])]


def test_cases_hit_what_they_claim():
    site = lambda name: {int(x) & 0xFFFFFF for x in cc.expected(name)["status"] if x}  # noqa: E731
    assert site("sites") == {1, 2, 3, 4, 5, 6, 7} and site("sites_dense") == {2, 3, 5, 6, 7} and site("sites_dense_tail") == {1, 4}
    assert all((int(x) >> 24) == ref.KIND_VALUE_ERROR for x in cc.expected("sites")["status"] if x)
    # both counter modes; every length, duplicates kept, the empty message, both calls, pool words
    assert cc.case("lengths")["trace"]["rw_counter"] is None and cc.case("lengths_gaps")["trace"]["rw_counter"] is not None
    w, c = cc.expected("lengths"), cc.case("lengths")
    lens = [len(m) for m in w["messages"]]
    assert lens[: len(cc.LENGTHS)] == list(cc.LENGTHS) and w["messages"].count(cc.message(33, 4)) == 3
    assert {int(c["trace"]["steps"][s, 2]) for s in w["step"]} == {1, 2} and len(c["trace"]["pool"]) >= len(cc.LENGTHS)
    assert [int(x) & 0xFF for x in w["status"] if x] == [7]  # the pushed word below 2^64
    states = {int(x) & 0xFF for x in c["trace"]["steps"][:, 0]}
    assert len(states) >= 5 and len(w["step"]) < len(w["status"])
    # the single step's ops are the first and the last of the table
    c1 = cc.case("single")["trace"]
    assert len(c1["head"]) == 3 + 70 and int(c1["steps"][0, 1]) == c1["rw_base"]
    # sites 4-6 on byte 0, 63, 64 and the last
    c, w = cc.case("sites"), cc.expected("sites")
    for m, s in zip(w["messages"], w["step"]):
        code = int(w["status"][s]) & 0xFF
        if code in (4, 5, 6):
            zeros = [i for i, (a, b) in enumerate(zip(m, cc.message(100, 3))) if a != b]
            assert zeros and zeros[0] in cc.SITE_BYTES + (9, 70), (s, zeros)
    # the ladders: SHA3 steps on both sides of the wavefront and block edges; the byte batch likewise
    for n in cc.LADDER_SIZES:
        assert len(cc.expected(f"ladder_{n}_all")["step"]) == n
        edges = cc.expected(f"ladder_{n}_edges")["step"].tolist()
        assert edges == sorted({i for i in (0, 63, 64, 255, 256, n - 1) if i < n})
    ends = set(cc.expected("bytes_edges")["data_offsets"].tolist())
    assert {63, 64, 65, 255, 256, 257, 511, 512, 513} <= ends


@pytest.mark.parametrize("name", cc.NAMES)
def test_equals_the_model(name):
    c = cc.case(name)
    want = cc.expected(name)
    assert engine.sha3_from_trace_sizes(c["trace"], device=DEVICE) == (len(want["step"]), len(want["data"]))
    cc.check_outputs(name, *run(c))


def check_session(device, stream=None):
    """a session: the counts, two passes (the second after zk_session_set_stream) with equal results, read by name"""
    for name in ("lengths_gaps", "sites", "ladder_257_alt"):
        c, want = cc.case(name), cc.expected(name)
        with engine.open_sha3_from_trace(c["trace"], c["randomness"], device=device) as s:
            assert s.n == len(want["status"]) and s.counts() == (len(want["step"]), len(want["data"]))
            r1 = s.run()
            out1, st1 = s.read(), s.read_status()
            s.set_stream(stream)
            r2 = s.run()
            out2, st2 = s.read(), s.read_status()
            cc.check_outputs(name, r1, st1, out1)
            cc.check_outputs(name, r2, st2, out2)
            part = s.read(("rows", "step"))
            assert set(part) == {"rows", "step"} and np.array_equal(part["rows"], want["rows"])


def test_session():
    check_session(DEVICE)


def rewritten(c, **changes):
    """the model over the records with single entries of per-op arrays replaced: {array: (index, value)}"""
    rec = dict(c["trace"])
    for k, (i, v) in changes.items():
        rec[k] = rec[k].copy()
        rec[k][i] = v
    return ref.derive(rec, c["randomness"])


def check_rewrites(open_session, poke):
    """Passes after the caller overwrote its records.  A message byte's val: the byte, the row and site 7 follow.  The size operand's val:
    nothing moves - which steps are messages, their sizes and the offsets are the session's own (decided at open).  open_session(c) ->
    (session, the arrays the session reads); poke(arrays, name, index, value) rewrites one entry in place."""
    c = cc.case("lengths")
    tr = c["trace"]
    want0 = cc.expected("lengths")
    step = int(want0["step"][4])                     # the 33-byte message
    first = int(tr["steps"][step, 1]) - tr["rw_base"]  # (dense counters: the index of op 0)
    s, arrays = open_session(c)
    with s:
        cc.check_outputs("lengths", s.run(), s.read_status(), s.read())
        byte_op = first + 3 + 20
        poke(arrays, "val", byte_op, int(tr["val"][byte_op]) ^ 0x40)
        want1 = rewritten(c, val=(byte_op, int(tr["val"][byte_op]) ^ 0x40))
        assert int(want1["status"][step]) == ref.code_of(7) and not np.array_equal(want1["rows"][4], want0["rows"][4])
        cc.check_against(want1, s.run(), s.read_status(), s.read(), "a byte rewritten")
        poke(arrays, "val", byte_op, 300)           # no byte any more: site 6, gathered as 0
        want2 = rewritten(c, val=(byte_op, 300))
        assert int(want2["status"][step]) == ref.code_of(6)
        cc.check_against(want2, s.run(), s.read_status(), s.read(), "a byte of 300")
        poke(arrays, "val", byte_op, int(tr["val"][byte_op]))
        poke(arrays, "val", first + 1, 1)            # the size operand: read at open only
        cc.check_outputs("lengths", s.run(), s.read_status(), s.read())
        assert s.counts() == (len(want0["step"]), len(want0["data"]))


def test_passes_after_rewrites():
    def open_session(c):
        rec = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in c["trace"].items()}  # the CPU backend reads val in place
        return engine.open_sha3_from_trace(rec, c["randomness"], device=DEVICE), rec

    def poke(rec, name, i, v):
        rec[name][i] = v

    check_rewrites(open_session, poke)


def check_composition(device):
    """the rows are bit for bit zk_keccak_table's (mode 0) over the returned data / data_offsets - failing steps included"""
    for name in ("lengths", "sites", "bytes_edges"):
        c = cc.case(name)
        _, _, out = run(c, device)
        rows = engine.keccak_table(messages_of(out), c["randomness"], engine.KECCAK_MODE_CIRCUIT, device=device)
        assert np.array_equal(np.asarray(rows), out["rows"]), name


def test_rows_are_the_keccak_table_of_the_data():
    check_composition(DEVICE)


def error_of(call, *args, **kw):
    with pytest.raises(_lib.EngineError) as e:
        call(*args, **kw)
    text = str(e.value)
    return e.value.rc, text[text.index("): ") + 3:]


def domain_errors():
    """(label, trace dict, rc, text)"""
    base = cc.case("lengths_gaps")["trace"]
    out = []

    def variant(label, rc, text, **changes):
        t = dict(base)
        for k, f in changes.items():
            t[k] = f(t.get(k))
        out.append((label, t, rc, text))

    def at(i, v):
        def f(a):
            a = a.copy()
            a[i] = v
            return a
        return f

    name = "zk_sha3_from_trace: "
    n_rw, n_pool = len(base["head"]), len(base["pool"])
    variant("trace head", _lib.ERR_TRC_HEAD, name + "the head of RW op 5 has a reserved bit set", head=at(5, (8 << 1) | (1 << 30)))
    variant("trace step", _lib.ERR_TRC_HEAD, name + "word 0 of step 3 has a reserved bit set",
            steps=lambda a: np.concatenate([a[:3], a[3:4] | np.array([1 << 12] + [0] * 12, np.uint64), a[4:]]))
    variant("trace order", _lib.ERR_TRC_ORDER, name + "the rw_counter of RW op 4 does not exceed the one before it (rw_counters must be strictly ascending)",
            rw_counter=lambda a: at(4, int(a[3]))(a))
    variant("trace order wrap", _lib.ERR_TRC_ORDER, name + f"rw_base {2**64 - 5} + {n_rw} RW ops passes 2^64", rw_counter=lambda a: None,
            rw_base=lambda a: 2**64 - 5)
    variant("trace pool", _lib.ERR_TRC_POOL, name + f"the heads consume {n_pool} pool words, n_pool is {n_pool - 1}", pool=lambda a: a[:-1])
    # 2^31 message bytes: the size operand of a later SHA3 step (op 1 of step s) made 2^31 - 1; the bytes in front of it take the total over
    # the bound at that step (no byte op is looked at before the open has refused)
    steps, ctr = base["steps"], base["rw_counter"]
    sha3 = [s for s in range(len(steps)) if int(steps[s, 0]) & 0xFF == ref.SHA3]
    s = sha3[3]
    op1 = int(np.searchsorted(ctr, steps[s, 1])) + 1
    variant("message bytes", _lib.ERR_TS3_BYTES, name + f"the message of step {s} takes the hashed bytes to 2^31 or more", val=at(op1, 2**31 - 1))
    return out


@pytest.mark.parametrize("label,t,rc,text", domain_errors(), ids=[d[0] for d in domain_errors()])
def test_domain_errors(label, t, rc, text):
    assert error_of(engine.sha3_from_trace_sizes, t, device=DEVICE) == (rc, text)
    assert error_of(engine.open_sha3_from_trace, t, cc.RANDOMNESS, device=DEVICE) == (rc, text)


def check_too_many_rows(device):
    """ZK_ERR_TS3_ROWS needs no array of 2^31 entries: the counts are checked before anything is read"""
    c = cc.case("lengths")
    lib = _lib.init(device)
    a, b, big = ctypes.c_uint64(), ctypes.c_uint64(), 1 << 31
    ns, n = len(c["trace"]["steps"]), len(c["trace"]["head"])
    for field, text in (("n_steps", f"zk_sha3_from_trace: {n} RW ops, {big} steps (2^31 or more)"),
                        ("n_rw", f"zk_sha3_from_trace: {big} RW ops, {ns} steps (2^31 or more)")):
        p = engine._wire_args(engine.TRACE_SHA3, engine._trace_sha3_records(c["trace"]))
        setattr(p.t, field, big)
        assert lib.zk_sha3_from_trace_sizes(ctypes.byref(p.t), p.opts, ctypes.byref(a), ctypes.byref(b)) == _lib.ERR_TS3_ROWS, field
        assert lib.zk_last_error().decode() == text


def test_too_many_rows():
    check_too_many_rows(DEVICE)


# ---- the reference-recorded goldens -------------------------------------------------------------------------------------------------
def check_goldens(golden_dir, device):
    """The 12 reference-recorded SHA3 cases, each turned into records where the records can hold it (six carry a fuzzed cell the reference
    never looked at and that no record holds: a tag above 15, a step integer of 2^64 or more).  A case the reference accepted: every
    step is clean and the derived length and digest cells are the golden keccak row's.  A case the reference rejected (one fuzzed cell
    somewhere in its tables): the entry derives the row of the bytes the trace reads all the same; where it differs from the golden row,
    the golden row is the fuzzed one - it is not the keccak row of those bytes.  The fixture does not record the keccak randomness the
    reference drew (rand_fq()), and the sibling golden tests never need it (the wire rows carry the RLCs already), so the RLC cell is
    not compared here: tests/trace_sha3_ref.py covers it.  -> (cases seen, accepted cases compared, rejected cases compared)"""
    g = np.load(os.path.join(golden_dir, "evm_sha3.npz"))
    n = sum(1 for k in g.files if k.endswith("_steps"))
    used = [0, 0]
    for i in range(n):
        case = {f: g[f"c{i:04d}_{f}"] for f in ("steps", "rw", "rw_flags", "keccak", "ref_kind")}
        try:
            rec = dict(trace.rw_ops_from_wire(case["rw"], case["rw_flags"]), steps=trace.step_records_from_wire(case["steps"]))
        except UnsupportedOnDevice:
            continue
        res, status, out = oneshot.sha3_from_trace(rec, cc.RANDOMNESS, device=device)
        assert len(out["rows"]) == len(case["keccak"]) == 1
        same = np.array_equal(out["rows"][:, [0, 2, 3, 4]], case["keccak"][:, [0, 2, 3, 4]])
        model = ref.keccak_row(messages_of(out)[0], cc.RANDOMNESS)
        assert np.array_equal(out["rows"][0], model), i
        if not case["ref_kind"].any():
            assert res.ok and not status.any() and same, (i, status)
        else:
            assert same or not np.array_equal(case["keccak"][0][[0, 2, 3, 4]], model[[0, 2, 3, 4]]), i
        used[1 if case["ref_kind"].any() else 0] += 1
    return n, used[0], used[1]


def test_goldens(golden_dir):
    assert check_goldens(golden_dir, DEVICE) == GOLDEN_USED


# ---- a consistent synthetic block ---------------------------------------------------------------------------------------------------
N_BLOCK_STEPS = 1 << 10


def check_block(device):
    """synth_block_trace with block ops at 2^10 steps.  The generator's sha3_inputs lists what its programs hash once per program position;
    a trace that loops executes a position several times, so the derived messages equal that list as a set, and as a multiset they equal
    the bytes of the generator's own per-step SHA3 copy events."""
    r, kw = 0x1234567, dict(seed=9, seg_len=96, n_contracts=2, block_ops=24)
    programs = synth_block_codes(**kw)
    msgs = sorted(set(synth_block_sha3_inputs(**kw)))
    rows = engine.keccak_table(list(programs) + msgs, r, engine.KECCAK_MODE_CIRCUIT, device=device)
    digest = {m: _digest_of_row(rows[len(programs) + i]).to_bytes(32, "big") for i, m in enumerate(msgs)}
    evm = synth_block_trace(N_BLOCK_STEPS, code_hashes=[_digest_of_row(rows[i]) for i in range(len(programs))],
                            digest_of=lambda ms: [digest[m] for m in ms], randomness=r, **kw)
    rec = dict(trace.rw_ops_from_wire(evm["rw"], evm["rw_flags"]), steps=trace.step_records_from_wire(evm["steps"]))
    res, status, out = oneshot.sha3_from_trace(rec, r, device=device)
    assert res.ok and not status.any() and res.rows_evaluated == N_BLOCK_STEPS
    derived = messages_of(out)
    assert len(derived) >= 8 and set(derived) == set(evm["sha3_inputs"])
    ce = evm["copy_events"]
    hashed = [bytes((ce["data"][int(a):int(b)] & 0xFF).astype(np.uint8)) for e, a, b in zip(ce["events"], ce["offsets"][:-1], ce["offsets"][1:])
              if int(e[5, 0]) == 5]  # the events whose destination is RlcAcc: the SHA3 steps'
    assert collections.Counter(m for m in derived if m) == collections.Counter(hashed)
    states = evm["steps"][:, 0, 0]
    assert out["step"].tolist() == [s for s in range(N_BLOCK_STEPS) if int(states[s]) == ref.SHA3]
    # the derived rows in place of the generator's keccak rows: the same clean verdict
    evm["keccak"] = np.ascontiguousarray(rows[len(programs):])
    from tests.test_events_from_trace_cpu import codes_of_bytecode_table

    codes, hashes = codes_of_bytecode_table(evm["bytecode"])
    sources = {"code": np.frombuffer(b"".join(codes), np.uint8).copy(), "code_offsets": np.cumsum([0] + [len(c) for c in codes]).astype(np.uint64),
               "calldata": None, "calldata_offsets": None, "trace": {k: v for k, v in rec.items() if k != "steps"}}
    r1, _, ev_out = oneshot.events_from_trace(rec, codes, hashes, device=device)
    r2, st2, _, _, copy_table, *_ = oneshot.copy_assign_from_sources(ev_out["copy_events"], ev_out["copy_flags"], ev_out["copy_src_ref"], None, sources,
                                                                     ce["r"], device=device)
    assert r1.ok and r2.ok and not st2.any()
    verdicts = []
    for keccak in (evm["keccak"], out["rows"]):
        r4, st4 = oneshot.evm_verify(dict(evm, copy=copy_table, keccak=np.ascontiguousarray(keccak)), device=device)
        verdicts.append((r4.ok, r4.fail_count, r4.rows_evaluated, st4.tolist()))
    assert verdicts[0] == verdicts[1] and verdicts[0][:3] == (True, 0, N_BLOCK_STEPS - 1), verdicts[0][:3]
    # the SHA3 steps that emit a copy event in zk_events_from_trace are the derived messages with size != 0
    emitting = {int(s) for s, e in zip(ev_out["copy_step"], ev_out["copy_events"]) if int(e[5, 0]) == 5}
    assert emitting == {int(s) for s, m in zip(out["step"], derived) if m}


def test_consistent_block():
    check_block(DEVICE)


def test_sanitizer_program(tmp_path):
    """the header's functions and the CPU entries under -fsanitize=address,undefined, as a stand-alone child process"""
    exe = str(tmp_path / "trace_sha3_asan")
    src = os.path.join(ROOT, "tests", "hostsim", "trace_sha3_asan.cpp")
    # (-O0 -g1: the program holds the whole CPU backend, whose optimised sanitizer build takes a minute and a half)
    subprocess.check_call(["g++", "-O0", "-g1", "-std=c++17", "-DZK_HOSTSIM", "-fopenmp", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",  # (the runtimes inside the program: nothing to preload)
                           "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-Wno-array-bounds", "-o", exe, src, "-ldl"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "trace_sha3_asan: ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
