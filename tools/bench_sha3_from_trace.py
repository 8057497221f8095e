#!/usr/bin/env python3
"""The keccak rows of a block's SHA3 steps from its compact trace records (zk_sha3_from_trace) against the path a producer of traces took
so far.  Block: the bench's config 5 (synth_super_block: synth_block with block_ops, 2^18 steps at --log2-total 20).

In one process on one stream, REPS times, the legs alternating:
  A  host loop   collect the SHA3 inputs from the trace's wire rows: per SHA3 step the two stack operands by counter, then the value of
                 the Memory row at each of the size counters behind them, concatenated (Python, by the host clock)
     upload      the bytes and their offsets to HBM (host clock around the copies and a synchronisation)
     keccak      the zk_keccak_table one-shot over the resident bytes, rows into a resident buffer, between two device events
  B  one-shot    zk_sha3_from_trace with the records and the caller's output buffers resident (ZK_OPT_DEVICE_PTRS), between two device
                 events: open (checks, statuses and sizes, scan, records) + one pass
     resident    PASSES launches of an open_sha3_from_trace session -> ms per pass
Every output of both legs is compared equal.  Prints one JSON line and writes profiles/sha3_from_trace.json.
"""
import argparse
import ctypes
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


def host_loop(steps, rw):
    """the SHA3 inputs of the trace, step by step: steps / rw are the wire arrays -> (list of bytes, the steps)"""
    sha3 = int(ES.SHA3)
    base = int(rw[0, 0, 0])  # (the block's counters are consecutive)
    msgs, at = [], []
    for s in np.nonzero(steps[:, 0, 0] == sha3)[0]:
        k = int(steps[s, 1, 0]) - base
        size = int(rw[k + 1, 8, 0])
        msgs.append(bytes(int(rw[k + 3 + i, 8, 0]) for i in range(size)))
        at.append(int(s))
    return msgs, at


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-total", type=int, default=20)
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sha3_from_trace.json"))
    args = ap.parse_args()
    lib = _lib.init(0)
    stream = torch.cuda.Stream()
    _lib.check(lib.zk_set_stream(ctypes.c_void_p(stream.cuda_stream)), "zk_set_stream", lib)
    p = synth_super_block(args.log2_total, seed=5)
    evm, r = p["evm"], int(p["copy_events"]["r"])
    rec = dict(trace.rw_ops_from_wire(evm["rw"], evm["rw_flags"]), steps=trace.step_records_from_wire(evm["steps"]))
    assert rec["rw_counter"] is None
    d_tr = {k: (up(v) if hasattr(v, "dtype") else v) for k, v in rec.items() if k != "prev"}
    ns = int(rec["steps"].shape[0])
    counts = engine.sha3_from_trace_sizes(d_tr)
    shapes = engine.sha3_from_trace_shapes(*counts)
    view = {np.uint64: torch.int64, np.uint32: torch.int32, np.uint8: torch.uint8}
    outs = {k: torch.zeros(shp, dtype=view[dt], device="cuda") for k, (shp, dt) in shapes.items()}
    prepared = engine._wire_args(engine.TRACE_SHA3, engine._trace_sha3_records(d_tr, counts), (r,), outs)
    d_status = torch.zeros(ns, dtype=torch.int32, device="cuda")
    rows_a = torch.zeros((counts[0], 5, 4), dtype=torch.int64, device="cuda")

    def one_shot():
        res, a, b = _lib.ZkResult(), ctypes.c_uint64(), ctypes.c_uint64()
        _lib.check(lib.zk_sha3_from_trace(ctypes.byref(prepared.t), _lib.ptr(prepared.keep[-1]), ctypes.byref(prepared.w), prepared.opts, _lib.ptr(d_status),
                                          ctypes.byref(a), ctypes.byref(b), ctypes.byref(res)), "zk_sha3_from_trace", lib)
        return engine.Result(res), int(a.value), int(b.value)

    times = {"host_loop": [], "upload": [], "keccak_table": [], "one_shot": []}
    for rep in range(-1, args.reps):  # (rep -1: warm-up)
        t0 = time.perf_counter()
        msgs, at = host_loop(evm["steps"], evm["rw"])
        data, offsets = engine.pack_messages(msgs)
        t1 = time.perf_counter()
        with torch.cuda.stream(stream):
            d_data, d_off = up(data), up(offsets)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            args_k, opts_k, keep_k = engine._keccak_args(d_data, d_off, r, engine.KECCAK_MODE_CIRCUIT, rows_a)

            def keccak():
                res = _lib.ZkResult()
                _lib.check(lib.zk_keccak_table(*args_k, opts_k, None, ctypes.byref(res)), "zk_keccak_table", lib)
                return engine.Result(res)

            ms_keccak, res_a = timed(keccak, stream)
            ms_dev, (res, n_msgs, n_bytes) = timed(one_shot, stream)
        assert res_a.ok and res.ok and (n_msgs, n_bytes) == counts == (len(msgs), len(data)) and not bool(d_status.any())
        got = {k: t.cpu().numpy().view(shapes[k][1]) for k, t in outs.items()}
        assert np.array_equal(got["rows"], rows_a.cpu().numpy().view(np.uint64)) and np.array_equal(got["data"], data)
        assert np.array_equal(got["data_offsets"], offsets) and got["step"].tolist() == at
        if rep >= 0:
            times["host_loop"].append((t1 - t0) * 1e3)
            times["upload"].append((t2 - t1) * 1e3)
            times["keccak_table"].append(ms_keccak)
            times["one_shot"].append(ms_dev)
    with engine.open_sha3_from_trace(d_tr, r, outs) as s:
        assert s.run().ok

        def passes():
            for _ in range(args.passes):
                s.launch()

        resident = []
        for _ in range(args.reps):
            resident.append(round(timed(passes, stream)[0] / args.passes, 5))
            s.collect()
    got = {k: t.cpu().numpy().view(shapes[k][1]) for k, t in outs.items()}
    assert np.array_equal(got["rows"], rows_a.cpu().numpy().view(np.uint64)) and np.array_equal(got["data"], data)
    rnd = lambda v: [round(t, 4) for t in v]  # noqa: E731
    out = {"tool": "bench_sha3_from_trace", "block": f"synth_super_block(2^{args.log2_total}, seed=5)", "n_steps": ns, "n_rw_ops": int(rec["head"].shape[0]),
           "n_msgs": counts[0], "n_bytes": counts[1], "record_bytes": trace.record_bytes(rec), "passes": args.passes, "reps": args.reps,
           "leg_a_ms": {k: rnd(times[k]) for k in ("host_loop", "upload", "keccak_table")}, "leg_b_ms": {"one_shot": rnd(times["one_shot"]), "resident_pass": resident},
           "median_ms": {k: round(statistics.median(v), 4) for k, v in times.items()}, "outputs_equal": True, "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
