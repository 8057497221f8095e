"""zk_events_from_trace* on the CPU backend: the copy and EXP events of the steps of compact trace records against the plain-Python model
of tests/events_from_trace_ref.py, bit for bit (events, flags, refs, step indices, statuses, tally); the domain errors with their codes and
texts; the reference-recorded EVM goldens, whose copy and exp tables the derived events must be; a consistent synthetic block, whose own
event lists they must equal and whose EVM circuit accepts the tables assigned from them; a stand-alone sanitizer build of the header's
functions and the CPU entries."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import events_from_trace_cases as cc
from tests import events_from_trace_ref as ref
from zkevm_specs_amd import _lib, engine, oneshot, trace
from zkevm_specs_amd.errors import UnsupportedOnDevice
from zkevm_specs_amd.super_circuit import _digest_of_row
from zkevm_specs_amd.synth_block import synth_block_codes, synth_block_sha3_inputs, synth_block_trace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = "cpu"
GOLDEN_KINDS = {"sha3": 3, "calldatacopy": 18, "codecopy": 5, "extcodecopy": 31, "returndatacopy": 7, "logs": 21, "exp": 40}  # cases used, at least


def run(c, device=DEVICE):
    return oneshot.events_from_trace(c["trace"], c["codes"], c["hashes"], device=device)


def test_cases_hit_what_they_claim():
    for name in cc.NAMES:
        c, want = cc.case(name), cc.expected(name)
        assert {s: int(x) for s, x in enumerate(want["status"]) if x} == c["want"], name
    sites = cc.case("sites")["want"]
    assert {x & 0xFFFFFF for x in sites.values() if x >> 24 == ref.KIND_VALUE_ERROR} == {1, 2, 3, 4}
    assert sum(1 for x in sites.values() if x == ref.UNSUPPORTED_CODE) == len(ref.UNSUPPORTED) == 6
    # both counter modes, pool-word operands, every copy kind, LOG0..LOG4, both lists
    assert cc.case("kinds")["trace"]["rw_counter"] is None and cc.case("kinds_gaps")["trace"]["rw_counter"] is not None
    k = cc.expected("kinds")
    assert len(cc.case("kinds")["trace"]["pool"]) >= 4
    ev = k["copy_events"]
    assert {(int(e[2, 0]), int(e[5, 0])) for e in ev} == {(2, 5), (3, 2), (2, 2), (1, 2), (2, 4)}
    assert sorted(int(e[11, 0]) - int(cc.case("kinds")["trace"]["steps"][s, 1]) for e, s in zip(ev, k["copy_step"]) if int(e[5, 0]) == 4) == [7, 9, 11, 13, 15]
    assert any(e[1].any() for e in ev if int(e[2, 0]) == 1) and any(not e[0].any() and not e[1].any() for e in ev if int(e[2, 0]) == 1)  # a wide and the zero hash
    assert any(e[2, 1] and e[4, 1] for e in k["exp_events"])  # a 256-bit base and exponent: the hi halves reach their upper words
    assert any(int(e[9, 0]) == 0 for e in ev)  # RETURNDATACOPY with size 0
    dup = [e for e in ev if int(e[2, 0]) == 1 and ref._word(e[0]) | (ref._word(e[1]) << 128) == cc.H_A]
    assert dup and all(int(e[7, 0]) == len(cc.CODE_A) for e in dup)  # of the two codes with H_A the first
    # the ladders: the emitting steps at the wavefront and block edges, in both lists
    for n in cc.LADDER_SIZES:
        emits = cc.ladder_emits(n, "alt")
        assert emits[0] and emits[n - 1] and all(emits[i] for i in (63, 64, 255, 256) if i < n)
        w = cc.expected(f"ladder_{n}_alt")
        assert sorted(w["copy_step"].tolist() + w["exp_step"].tolist()) == [i for i, e in enumerate(emits) if e]
        assert len(cc.expected(f"ladder_{n}_all")["status"]) == n and not len(cc.expected(f"ladder_{n}_none")["copy_step"])
    w = cc.expected("ladder_1025_all")
    assert len(w["copy_step"]) + len(w["exp_step"]) == 1025 and len(w["exp_step"]) > 256 and len(w["copy_step"]) > 512


@pytest.mark.parametrize("name", cc.NAMES)
def test_equals_the_model(name):
    cc.check_outputs(name, *run(cc.case(name)))


def check_session(device, stream=None):
    """a session: counts before and after a pass, two passes (the second after zk_session_set_stream) with equal results, read by name"""
    for name in ("kinds_gaps", "sites", "ladder_257_alt"):
        c, want = cc.case(name), cc.expected(name)
        with engine.open_events_from_trace(c["trace"], c["codes"], c["hashes"], device=device) as s:
            assert s.n == len(want["status"]) and s.counts() == (0, 0)
            r1 = s.run()
            out1, st1 = s.read(), s.read_status()
            assert s.counts() == (len(want["copy_step"]), len(want["exp_step"]))
            s.set_stream(stream)
            r2 = s.run()
            out2, st2 = s.read(), s.read_status()
            cc.check_outputs(name, r1, st1, out1)
            cc.check_outputs(name, r2, st2, out2)
            part = s.read(("exp_events", "copy_step"))
            assert set(part) == {"exp_events", "copy_step"} and np.array_equal(part["exp_events"], want["exp_events"])


def test_session():
    check_session(DEVICE)


def error_of(call, *args, **kw):
    with pytest.raises(_lib.EngineError) as e:
        call(*args, **kw)
    text = str(e.value)
    return e.value.rc, text[text.index("): ") + 3:]


def domain_errors():
    """(label, case dict, rc, text)"""
    base = cc.case("kinds_gaps")
    out = []

    def variant(label, rc, text, **changes):
        c = {"trace": dict(base["trace"]), "codes": {"code": np.frombuffer(b"".join(base["codes"]), np.uint8).copy(),
                                                     "code_offsets": np.cumsum([0] + [len(x) for x in base["codes"]]).astype(np.uint64)},
             "hashes": list(base["hashes"])}
        for k, f in changes.items():
            if k.startswith("trace_"):
                c["trace"][k[6:]] = f(c["trace"].get(k[6:]))
            else:
                c["codes"][k] = f(c["codes"][k])
        out.append((label, c, rc, text))

    def at(i, v):
        def f(a):
            a = a.copy()
            a[i] = v
            return a
        return f

    name = "zk_events_from_trace: "
    n_rw, n_bytes = len(base["trace"]["head"]), sum(len(x) for x in base["codes"])
    variant("code offsets start", _lib.ERR_TEV_OFFSETS, name + "code_offsets[0] is 1, not 0", code_offsets=at(0, 1))
    variant("code offsets decrease", _lib.ERR_TEV_OFFSETS, name + "code_offsets decrease at entry 2", code_offsets=at(1, n_bytes))
    variant("code offsets end", _lib.ERR_TEV_OFFSETS, name + f"code_offsets[n_codes] is {n_bytes}, n_code_bytes is {n_bytes + 1}",
            code=lambda a: np.concatenate([a, a[:1]]))
    variant("trace head", _lib.ERR_TRC_HEAD, name + "the head of RW op 5 has a reserved bit set", trace_head=at(5, (8 << 1) | (1 << 30)))
    variant("trace step", _lib.ERR_TRC_HEAD, name + "word 0 of step 3 has a reserved bit set",
            trace_steps=lambda a: np.concatenate([a[:3], a[3:4] | np.array([1 << 12] + [0] * 12, np.uint64), a[4:]]))
    variant("trace order", _lib.ERR_TRC_ORDER, name + "the rw_counter of RW op 4 does not exceed the one before it (rw_counters must be strictly ascending)",
            trace_rw_counter=lambda a: at(4, int(a[3]))(a))
    variant("trace order wrap", _lib.ERR_TRC_ORDER, name + f"rw_base {2**64 - 5} + {n_rw} RW ops passes 2^64", trace_rw_counter=lambda a: None,
            trace_rw_base=lambda a: 2**64 - 5)
    n_pool = len(base["trace"]["pool"])
    variant("trace pool", _lib.ERR_TRC_POOL, name + f"the heads consume {n_pool} pool words, n_pool is {n_pool - 1}", trace_pool=lambda a: a[:-1])
    return out


@pytest.mark.parametrize("label,c,rc,text", domain_errors(), ids=[d[0] for d in domain_errors()])
def test_domain_errors(label, c, rc, text):
    args = (c["trace"], c["codes"], c["hashes"])
    assert error_of(engine.events_from_trace_sizes, *args, device=DEVICE) == (rc, text)
    assert error_of(engine.open_events_from_trace, *args, device=DEVICE) == (rc, text)


def check_too_many_rows(device):
    """ZK_ERR_TEV_ROWS / ZK_ERR_TRC_ROWS need no array of 2^31 entries: the counts are checked before anything is read"""
    c = cc.case("kinds")
    lib = _lib.init(device)
    n, big = ctypes.c_uint64(), 1 << 31
    ns, nb, nc = len(c["trace"]["steps"]), sum(len(x) for x in c["codes"]), len(c["codes"])
    for field, rc, text in (("n_steps", _lib.ERR_TEV_ROWS, f"zk_events_from_trace: {big} steps, {nb} code bytes, {nc} codes (2^31 or more)"),
                            ("n_code_bytes", _lib.ERR_TEV_ROWS, f"zk_events_from_trace: {ns} steps, {big} code bytes, {nc} codes (2^31 or more)"),
                            ("n_codes", _lib.ERR_TEV_ROWS, f"zk_events_from_trace: {ns} steps, {nb} code bytes, {big} codes (2^31 or more)"),
                            ("n_rw", _lib.ERR_TRC_ROWS, f"zk_events_from_trace: {big} RW ops, {ns} steps (a table of 2^31 rows or more)")):
        p = engine._wire_args(engine.TRACE_EVENTS, engine.trace_event_sources(c["trace"], c["codes"], c["hashes"]))
        setattr(p.t.trace if field in ("n_steps", "n_rw") else p.t, field, big)
        assert lib.zk_events_from_trace_sizes(ctypes.byref(p.t), p.opts, ctypes.byref(n)) == rc, field
        assert lib.zk_last_error().decode() == text


def test_too_many_rows():
    check_too_many_rows(DEVICE)


# ---- the reference-recorded goldens -------------------------------------------------------------------------------------------------
def golden_cases(golden_dir, kind):
    g = np.load(os.path.join(golden_dir, f"evm_{kind}.npz"))
    for i in range(sum(1 for k in g.files if k.endswith("_steps"))):
        yield {f: g[f"c{i:04d}_{f}"] for f in ("steps", "rw", "rw_flags", "bytecode", "copy", "exp", "ref_kind")}


def codes_of_bytecode_table(bt):
    """the code set of a bytecode table uint64[n, 6, 4] (hash lo, hi, tag, index, is_code, value): a Header row gives a code's hash and
    length, the Byte rows of that hash its bytes.  (Some goldens carry a fuzzed row - another tag, a value that is no byte - which the
    reference never looked at: such a row is left out.)"""
    lengths, data = {}, {}
    for row in bt:
        lo, hi, tag, index, _, value = (ref._word(c) for c in row)
        if tag == 1 and value < 1 << 24:
            lengths.setdefault(lo | (hi << 128), value)
        elif tag == 2 and value < 256:
            data.setdefault((lo | (hi << 128), index), value)
    return [bytes(data.get((h, i), 0) for i in range(n)) for h, n in lengths.items()], list(lengths)


def check_goldens(golden_dir, device):
    """every accepted golden case the records can hold: the derived copy events are the golden copy table's rows (as sets, on src id, tags,
    dst id, addresses, length and rw_counter; the TxLog dst_addr packing left out), every derived EXP event is in the golden exp table"""
    used = {}
    for kind in GOLDEN_KINDS:
        used[kind] = 0
        for g in golden_cases(golden_dir, kind):
            if g["ref_kind"].any():
                continue
            try:
                rec = dict(trace.rw_ops_from_wire(g["rw"], g["rw_flags"]), steps=trace.step_records_from_wire(g["steps"]))
            except UnsupportedOnDevice:
                continue
            codes, hashes = codes_of_bytecode_table(g["bytecode"])
            res, status, out = run({"trace": rec, "codes": codes, "hashes": hashes}, device)
            assert not (status & 0xFFFFFF)[status >> 24 == ref.KIND_VALUE_ERROR].any(), (kind, used[kind], status)

            def key(cells, tx_log):
                v = [ref._word(x) for x in cells]
                return tuple(v[:8] + ([] if tx_log else [v[8]]) + [v[9], v[10]])

            derived = {key(list(e[:10]) + [e[11]], int(e[5, 0]) == ref.TX_LOG) for e in out["copy_events"]}
            golden = {key(list(r[1:11]) + [r[12]], int(r[6, 0]) == ref.TX_LOG) for r in g["copy"]}
            assert derived == golden, (kind, used[kind])
            table = {tuple(ref._word(x) for x in r[[1, 3, 4, 5, 6, 7, 8]]) for r in g["exp"]}
            for e in out["exp_events"]:
                ident, blo, bhi, elo, ehi = (ref._word(x) for x in e)
                base = blo | (bhi << 128)
                assert (ident, *[(base >> (64 * k)) & (2**64 - 1) for k in range(4)], elo, ehi) in table, (kind, used[kind])
            used[kind] += 1
    return used


def test_goldens(golden_dir):
    used = check_goldens(golden_dir, DEVICE)
    assert all(used[k] >= n for k, n in GOLDEN_KINDS.items()), used


# ---- a consistent synthetic block ---------------------------------------------------------------------------------------------------
N_BLOCK_STEPS = 3000


def block_case(device):
    """synth_block with block_ops at 3,000 steps: the code hashes and the digests the SHA3 steps push are the keccak table's (the EVM
    circuit looks them up), the trace records those of its RW wire, the code set that of its bytecode table"""
    r, kw = 0x1234567, dict(seed=9, seg_len=96, n_contracts=2, block_ops=24)
    programs = synth_block_codes(**kw)
    msgs = sorted(set(synth_block_sha3_inputs(**kw)))
    rows = engine.keccak_table(list(programs) + msgs, r, engine.KECCAK_MODE_CIRCUIT, device=device)
    digest = {m: _digest_of_row(rows[len(programs) + i]).to_bytes(32, "big") for i, m in enumerate(msgs)}
    evm = synth_block_trace(N_BLOCK_STEPS, code_hashes=[_digest_of_row(rows[i]) for i in range(len(programs))],
                            digest_of=lambda ms: [digest[m] for m in ms], randomness=r, **kw)
    evm["keccak"] = np.ascontiguousarray(rows[len(programs):])
    rec = dict(trace.rw_ops_from_wire(evm["rw"], evm["rw_flags"]), steps=trace.step_records_from_wire(evm["steps"]))
    codes, hashes = codes_of_bytecode_table(evm["bytecode"])
    return evm, rec, codes, hashes


def check_block(device):
    evm, rec, codes, hashes = block_case(device)
    ce = evm["copy_events"]
    res, status, out = oneshot.events_from_trace(rec, codes, hashes, device=device)
    assert res.ok and not status.any() and res.rows_evaluated == N_BLOCK_STEPS
    # the generator's own lists: cells, flags and refs
    index = {h: j for j, h in reversed(list(enumerate(hashes)))}
    refs = [index[ref._word(e[0]) | (ref._word(e[1]) << 128)] if int(e[2, 0]) == ref.BYTECODE else 0 for e in ce["events"]]
    tags = {(int(e[2, 0]), int(e[5, 0])) for e in ce["events"]}
    assert (1, 2) in tags and (2, 5) in tags and len(ce["events"]) >= 8 and len(evm["exp_events"]) >= 4
    assert np.array_equal(out["copy_events"], ce["events"]) and np.array_equal(out["copy_flags"], ce["flags"])
    assert out["copy_src_ref"].tolist() == refs
    assert np.array_equal(out["exp_events"], evm["exp_events"])
    states = evm["steps"][:, 0, 0]
    assert all(int(states[s]) in (int(ref.ES.SHA3), int(ref.ES.CODECOPY)) for s in out["copy_step"]) and all(int(states[s]) == int(ref.ES.EXP) for s in out["exp_step"])
    # the derived lists through the assignments: the EVM circuit accepts the block with the copy and exp tables they produce
    sources = {"code": np.frombuffer(b"".join(codes), np.uint8).copy(), "code_offsets": np.cumsum([0] + [len(c) for c in codes]).astype(np.uint64),
               "calldata": None, "calldata_offsets": None, "trace": {k: v for k, v in rec.items() if k != "steps"}}
    r2, st2, _, _, copy_table, *_ = oneshot.copy_assign_from_sources(out["copy_events"], out["copy_flags"], out["copy_src_ref"], None, sources, ce["r"],
                                                                     device=device)
    assert r2.ok and not st2.any()
    r3, _, exp_table = oneshot.exp_assign(out["exp_events"], device=device)
    assert r3.ok
    r4, st4 = oneshot.evm_verify(dict(evm, copy=copy_table, exp=exp_table), device=device)
    assert r4.ok and not st4.any() and r4.rows_evaluated == N_BLOCK_STEPS - 1, r4


def test_consistent_block():
    check_block(DEVICE)


def test_sanitizer_program(tmp_path):
    """the header's functions and the CPU entries under -fsanitize=address,undefined, as a stand-alone child process"""
    exe = str(tmp_path / "events_from_trace_asan")
    src = os.path.join(ROOT, "tests", "hostsim", "events_from_trace_asan.cpp")
    # (-O0 -g1: the program holds the whole CPU backend, whose optimised sanitizer build takes a minute and a half)
    subprocess.check_call(["g++", "-O0", "-g1", "-std=c++17", "-DZK_HOSTSIM", "-fopenmp", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",  # (the runtimes inside the program: nothing to preload)
                           "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-Wno-array-bounds", "-o", exe, src, "-ldl"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "events_from_trace_asan: ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
