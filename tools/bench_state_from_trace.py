#!/usr/bin/env python3
"""The State verdict from compact trace records (zk_state_verify_from_trace) against the way it took before: the expansion to wire rows
(zk_evm_witness_from_trace) followed by zk_state_verify_from_rw over them.  Two tables: the RW records of bench.py's 2^18-step trace
(synth_evm_trace(2^18, seed=3)) and the RW table of synth_block_trace(2^18, seed=7) through trace.rw_ops_from_wire.

Per table, in one process on one stream, device events around each leg, legs alternating, REPS times:
  A   one pass of a resident zk_evm_witness_from_trace session (records and outputs in HBM), then the one-shot zk_state_verify_from_rw
      over its output (ZK_OPT_DEVICE_PTRS)
  B   the one-shot zk_state_verify_from_trace over the same resident records
  resident pass: PASSES launches of the from-RW fused session and of the from-trace session between two events -> ms per pass
The statuses and results of A and B must be equal.  Also: the bytes each form reads as input and the bytes the from-trace session holds
beyond the from-RW session's own buffers (counted from the sizes).  Prints one JSON line and writes profiles/state_from_trace.json.
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from zkevm_specs_amd import _lib, engine, trace
from zkevm_specs_amd.synth_block import synth_block_trace
from zkevm_specs_amd.synth_evm import synth_evm_trace


def up(x):
    return torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x.view(np.int32) if x.dtype == np.uint32 else x).cuda()


def timed(fn, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(stream)
    out = fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def first_pass(open_fn):
    s = open_fn()
    return s, s.run()


def one_shot_rw(lib, rw, fl, status):
    r, n_ops = _lib.ZkResult(), ctypes.c_uint64()
    _lib.check(lib.zk_state_verify_from_rw(_lib.ptr(rw), _lib.ptr(fl), int(rw.shape[0]), _lib.OPT_DEVICE_PTRS, _lib.ptr(status), ctypes.byref(n_ops),
                                           ctypes.byref(r)), "zk_state_verify_from_rw", lib)
    return engine.Result(r), int(n_ops.value)


def one_shot_trace(lib, t, status):
    r, n_ops = _lib.ZkResult(), ctypes.c_uint64()
    _lib.check(lib.zk_state_verify_from_trace(ctypes.byref(t), _lib.OPT_DEVICE_PTRS, _lib.ptr(status), ctypes.byref(n_ops), ctypes.byref(r)),
               "zk_state_verify_from_trace", lib)
    return engine.Result(r), int(n_ops.value)


def bench_table(lib, label, rw, fl, stream, args):
    rec = trace.trace_records(trace.rw_ops_from_wire(rw, fl))
    n = int(rw.shape[0])
    d_rec = {k: (up(v) if hasattr(v, "dtype") else v) for k, v in rec.items()}
    outs = {"rw": torch.full((n, 14, 4), -1, dtype=torch.int64, device="cuda"), "rw_flags": torch.full((n,), -1, dtype=torch.int32, device="cuda")}
    st_a = torch.full((n + 1,), -1, dtype=torch.int32, device="cuda")
    st_b = torch.full((n + 1,), -1, dtype=torch.int32, device="cuda")
    t, opts, keep, _ = engine._state_from_trace_args(d_rec)
    assert opts == _lib.OPT_DEVICE_PTRS
    expand = engine.open_evm_witness_from_trace(d_rec, outs=outs)

    def leg_a():
        expand.launch()
        return one_shot_rw(lib, outs["rw"], outs["rw_flags"], st_a)

    def leg_b():
        return one_shot_trace(lib, t, st_b)

    leg_a(), leg_b()  # warm-up (code objects, the fast sort's LDS attribute)
    assert expand.collect().ok
    a_ms, b_ms = [], []
    for _ in range(args.reps):
        ms, (ra, na) = timed(leg_a, stream)
        a_ms.append(ms)
        assert expand.collect().ok
        ms, (rb, nb) = timed(leg_b, stream)
        b_ms.append(ms)
        torch.cuda.synchronize()
        assert na == nb and (ra.fail_count, ra.first_fail_row, ra.first_fail_code) == (rb.fail_count, rb.first_fail_row, rb.first_fail_code)
        assert bool(torch.equal(st_a[:na], st_b[:nb])), "the two legs disagree on the statuses"
    # resident passes: the from-RW fused session over the expanded rows against the from-trace session over the records
    s_rw, r_rw = first_pass(lambda: engine.open_state_verify_from_rw(outs["rw"], outs["rw_flags"]))
    s_tr, r_tr = first_pass(lambda: engine.open_state_verify_from_trace(d_rec))
    assert s_rw.n == s_tr.n and np.array_equal(s_rw.read_status(), s_tr.read_status())

    def passes(s):
        for _ in range(args.passes):
            s.launch()

    res_rw, res_tr = [], []
    for _ in range(args.reps):
        res_rw.append(timed(lambda: passes(s_rw), stream)[0] / args.passes)
        s_rw.collect()
        res_tr.append(timed(lambda: passes(s_tr), stream)[0] / args.passes)
        s_tr.collect()
    assert np.array_equal(s_rw.read_status(), s_tr.read_status())
    n_ops = s_rw.n
    for s in (s_rw, s_tr, expand):
        s.close()
    rec_bytes = trace.record_bytes(rec) - int(rec["steps"].nbytes) - int(rec["prev"].nbytes)
    return {"table": label, "n_rw": n, "n_ops": n_ops, "n_pool": int(rec["pool"].shape[0]), "fail_count": int(r_tr.fail_count),
            "A_expand_then_verify_from_rw_ms": [round(v, 4) for v in a_ms], "B_verify_from_trace_ms": [round(v, 4) for v in b_ms],
            "resident_pass_from_rw_ms": [round(v, 5) for v in res_rw], "resident_pass_from_trace_ms": [round(v, 5) for v in res_tr],
            # what each session reads, and what the from-trace session holds beyond the from-RW session's own buffers (its copy of the heads,
            # the pool offsets, the 48-byte op stream; explicit counters would add 8 bytes per row): counted, not measured
            "input_bytes": {"rows_from_rw_reads": n * 452, "records_from_trace_reads": rec_bytes},
            "from_trace_session_extra_bytes": n * 12 + n_ops * 48,
            "legs_equal": True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-steps", type=int, default=18)
    ap.add_argument("--passes", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "state_from_trace.json"))
    args = ap.parse_args()
    lib = _lib.init(0)
    stream = torch.cuda.Stream()
    _lib.check(lib.zk_set_stream(ctypes.c_void_p(stream.cuda_stream)), "zk_set_stream", lib)  # sessions and one-shots of this thread: this stream
    tables = []
    w = synth_evm_trace(1 << args.log2_steps, seed=3)
    tables.append(bench_table(lib, f"synth_evm_trace(2^{args.log2_steps}, seed=3)", np.ascontiguousarray(w["rw"]), np.ascontiguousarray(w["rw_flags"]), stream, args))
    w = synth_block_trace(1 << args.log2_steps, seed=7)
    tables.append(bench_table(lib, f"synth_block_trace(2^{args.log2_steps}, seed=7)", np.ascontiguousarray(w["rw"]), np.ascontiguousarray(w["rw_flags"]), stream, args))
    out = {"tool": "bench_state_from_trace", "passes": args.passes, "reps": args.reps, "tables": tables, "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
