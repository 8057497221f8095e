#!/usr/bin/env python3
"""The copy and EXP event lists of a block from its compact trace records (zk_events_from_trace) against a host loop over the same trace.
Block: the bench's config 5 (synth_super_block: synth_block with block_ops, 2^18 steps at --log2-total 20), whose events are those of
its SHA3, CODECOPY and EXP steps.

In one process on one stream, REPS times:
  host     the per-step work synth_block.py does for these kinds beside its trace, as a loop of its own over the trace's wire rows: find the
           step's stack rows by counter, pop the operands, append the event (Python, by the host clock)
  one-shot zk_events_from_trace with the records, the code set and the caller's output buffers resident (ZK_OPT_DEVICE_PTRS), between
           two device events: open (checks, directory, buffers) + one pass + the counts
  resident PASSES launches of an open_events_from_trace session -> ms per pass
The device's lists must equal the host loop's and the generator's own.  Prints one JSON line and writes profiles/events_from_trace.json.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from zkevm_specs_amd import _lib, engine, trace
from zkevm_specs_amd.evm_tables import ExecutionState as ES
from zkevm_specs_amd.super_circuit import synth_super_block


def up(x):
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32, np.dtype(np.uint8): np.uint8}[x.dtype]
    return torch.from_numpy(np.ascontiguousarray(x).view(view)).cuda()


def timed(fn, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(stream)
    out = fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def host_loop(steps, rw, code_len):
    """the event lists of the SHA3 / CODECOPY / EXP steps, as synth_block.py appends them: steps / rw are the wire arrays, code_len maps a
    code hash to its length -> (copy events [12 ints], flags, EXP events [5 ints])"""
    M = (1 << 128) - 1
    sha3, codecopy, exp = int(ES.SHA3), int(ES.CODECOPY), int(ES.EXP)
    base = int(rw[0, 0, 0])
    value = lambda k: int(rw[k, 8, 0]) | (int(rw[k, 8, 1]) << 64) | (int(rw[k, 9, 0]) << 128) | (int(rw[k, 9, 1]) << 192)  # noqa: E731
    copy, flags, exps = [], [], []
    for s in range(steps.shape[0]):
        state = int(steps[s, 0, 0])
        if state != sha3 and state != codecopy and state != exp:
            continue
        rwc, call_id = int(steps[s, 1, 0]), int(steps[s, 2, 0])
        k = rwc - base  # (the block's counters are consecutive)
        if state == sha3:
            off, size = value(k), value(k + 1)
            copy.append([call_id, 0, 2, call_id, 0, 5, off, off + size, 0, size, 0, rwc + 3])
            flags.append(0)
        elif state == codecopy:
            moff, coff, size = value(k), value(k + 1), value(k + 2)
            h = (int(steps[s, 5, 0]) | (int(steps[s, 5, 1]) << 64), int(steps[s, 6, 0]) | (int(steps[s, 6, 1]) << 64))
            copy.append([h[0], h[1], 1, call_id, 0, 2, coff, code_len[h], moff, size, 0, rwc + 3])
            flags.append(1)
        else:
            b, e = value(k), value(k + 1)
            exps.append([rwc + 3, b & M, b >> 128, e & M, e >> 128])
    return copy, flags, exps


def cells(rows, n):
    raw = b"".join(int(x).to_bytes(32, "little") for r in rows for x in r)
    return np.frombuffer(raw, dtype="<u8").astype(np.uint64).reshape(len(rows), n, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-total", type=int, default=20)
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "events_from_trace.json"))
    args = ap.parse_args()
    lib = _lib.init(0)
    stream = torch.cuda.Stream()
    import ctypes

    _lib.check(lib.zk_set_stream(ctypes.c_void_p(stream.cuda_stream)), "zk_set_stream", lib)
    p = synth_super_block(args.log2_total, seed=5)
    evm, ce = p["evm"], p["copy_events"]
    heads = [row for row in evm["bytecode"] if int(row[2, 0]) == 1]
    word = lambda c: int.from_bytes(c.tobytes(), "little")  # noqa: E731
    hashes = [word(h[0]) | (word(h[1]) << 128) for h in heads]
    codes, at = [], 0
    for h in heads:  # the Byte rows follow their Header row
        n = int(h[5, 0])
        codes.append(bytes(evm["bytecode"][at + 1: at + 1 + n, 5, 0].astype(np.uint8)))
        at += 1 + n
    code_len = {(h & ((1 << 128) - 1), h >> 128): len(c) for h, c in zip(hashes, codes)}
    rec = dict(trace.rw_ops_from_wire(evm["rw"], evm["rw_flags"]), steps=trace.step_records_from_wire(evm["steps"]))
    assert rec["rw_counter"] is None
    x = engine.trace_event_sources(rec, codes, hashes)
    d_tr = {k: (up(v) if hasattr(v, "dtype") else v) for k, v in rec.items() if k != "prev"}
    d_codes, d_hashes = {"code": up(x["code"]), "code_offsets": up(x["code_offsets"])}, up(x["code_hashes"])
    ns = int(rec["steps"].shape[0])
    shapes = engine.events_from_trace_shapes(ns)
    view = {np.uint64: torch.int64, np.uint32: torch.int32}
    outs = {k: torch.zeros(shp, dtype=view[dt], device="cuda") for k, (shp, dt) in shapes.items()}
    prepared = engine._wire_args(engine.TRACE_EVENTS, engine.trace_event_sources(d_tr, d_codes, d_hashes), (), outs)
    d_status = torch.zeros(ns, dtype=torch.int32, device="cuda")

    def one_shot():
        res, a, b = _lib.ZkResult(), ctypes.c_uint64(), ctypes.c_uint64()
        _lib.check(lib.zk_events_from_trace(ctypes.byref(prepared.t), ctypes.byref(prepared.w), prepared.opts, _lib.ptr(d_status), ctypes.byref(a),
                                            ctypes.byref(b), ctypes.byref(res)), "zk_events_from_trace", lib)
        return engine.Result(res), int(a.value), int(b.value)

    times = {"host_loop": [], "one_shot": []}
    for rep in range(-1, args.reps):  # (rep -1: warm-up)
        t0 = time.perf_counter()
        copy, flags, exps = host_loop(evm["steps"], evm["rw"], code_len)
        ms_host = (time.perf_counter() - t0) * 1e3
        with torch.cuda.stream(stream):
            ms_dev, (res, n_copy, n_exp) = timed(one_shot, stream)
        assert res.ok and (n_copy, n_exp) == (len(copy), len(exps))
        got = engine.cut_trace_events({k: t.cpu().numpy().view(shapes[k][1]) for k, t in outs.items()}, n_copy, n_exp)
        assert np.array_equal(got["copy_events"], cells(copy, 12)) and got["copy_flags"].tolist() == flags
        assert np.array_equal(got["exp_events"], cells(exps, 5))
        assert np.array_equal(got["copy_events"], ce["events"]) and np.array_equal(got["exp_events"], p["exp_events"])
        if rep >= 0:
            times["host_loop"].append(ms_host)
            times["one_shot"].append(ms_dev)
    with engine.open_events_from_trace(d_tr, d_codes, d_hashes, outs) as s:
        assert s.run().ok

        def passes():
            for _ in range(args.passes):
                s.launch()

        resident = []
        for _ in range(args.reps):
            resident.append(round(timed(passes, stream)[0] / args.passes, 5))
            s.collect()
    rnd = lambda v: [round(t, 4) for t in v]  # noqa: E731
    out = {"tool": "bench_events_from_trace", "block": f"synth_super_block(2^{args.log2_total}, seed=5)", "n_steps": ns, "n_rw_ops": int(rec["head"].shape[0]),
           "n_pool_words": int(rec["pool"].shape[0]), "n_copy_events": n_copy, "n_exp_events": n_exp, "n_codes": len(codes),
           "code_bytes": int(x["code"].shape[0]), "record_bytes": trace.record_bytes(rec), "passes": args.passes, "reps": args.reps,
           "host_loop_ms": rnd(times["host_loop"]), "one_shot_ms": rnd(times["one_shot"]),
           "median_ms": {"host_loop": round(statistics.median(times["host_loop"]), 4), "one_shot": round(statistics.median(times["one_shot"]), 4)},
           "resident_pass_ms": resident, "lists_equal": True, "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
