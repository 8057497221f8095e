#!/usr/bin/env python3
"""The State WITNESS from compact trace records (zk_state_assign_from_trace) against the only route there was: the expansion to wire rows
(zk_evm_witness_from_trace) followed by the from-RW assignment (zk_state_assign_from_rw_open) over them.  Table: the RW table of
synth_block_trace(2^18, seed=7) through trace.rw_ops_from_wire (DESIGN.md §3.StateFromTrace's block table).

In one process on one stream, device events around each leg, legs alternating, REPS times, in the 57-cell and the compact form:
  A   one pass of a resident zk_evm_witness_from_trace session (records and outputs in HBM), then the from-RW assignment as a one-shot over
      its output: open, launch, collect, the MPT row count, close (ZK_OPT_DEVICE_PTRS, the caller's row / flag / MPT buffers)
  B   the one-shot zk_state_assign_from_trace over the same resident records into buffers of the same kind, the records' checks and the
      pool-offset scan included; with either row writer (ZK_STATE_TRACE_WRITER=lane, the default, and =pair)
  resident pass: PASSES launches of the from-RW session and of the from-trace session between two events -> ms per pass
The rows, flags, MPT rows, statuses and results of A and B must be equal.  Prints one JSON line and writes
profiles/state_assign_from_trace.json.

  --trace-run N           only N one-shots of leg B (57-cell form), nothing timed: the run to put under a kernel trace of its own
  --kernel-stats CSV      fold the per-kernel statistics of such a trace (name, calls, total / average ns) into the JSON written
  --merge                 no run: read the JSON written before, add --kernel-stats, write it back
"""
import argparse
import csv
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from zkevm_specs_amd import _lib, engine, trace
from zkevm_specs_amd.synth_block import synth_block_trace


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


class Buffers:
    """the caller's outputs of one leg: capacity n_rw + 1 rows"""

    def __init__(self, n, nc):
        self.nc = nc
        self.rows = torch.full((nc * 4 * (n + 1),), -1, dtype=torch.int64, device="cuda")
        self.flags = torch.full((n + 1,), -1, dtype=torch.int32, device="cuda")
        self.mpt = torch.full((48 * (n + 1),), -1, dtype=torch.int64, device="cuda")
        self.status = torch.full((n + 1,), -1, dtype=torch.int32, device="cuda")

    def views(self, n_ops, n_mpt):
        return self.rows[: self.nc * 4 * n_ops], self.flags[:n_ops], self.mpt[: 48 * n_mpt], self.status[:n_ops]


def one_shot_rw(rw, fl, b, compact):
    with engine.open_state_assign_from_rw(rw, fl, b.rows, b.flags, b.mpt, compact=compact) as s:
        s.launch(b.status[: s.n])
        r = s.collect()
        return r, s.n, s.n_mpt()


def one_shot_trace(lib, t, b, compact):
    r, n_ops, n_mpt = _lib.ZkResult(), ctypes.c_uint64(), ctypes.c_uint64()
    opts = _lib.OPT_DEVICE_PTRS | (_lib.OPT_STATE_COMPACT if compact else 0)
    _lib.check(lib.zk_state_assign_from_trace(ctypes.byref(t), _lib.ptr(b.rows), _lib.ptr(b.flags), _lib.ptr(b.mpt), ctypes.byref(n_mpt),
                                              ctypes.byref(n_ops), opts, _lib.ptr(b.status), ctypes.byref(r)), "zk_state_assign_from_trace", lib)
    return engine.Result(r), int(n_ops.value), int(n_mpt.value)


def verdict(r):
    return (r.fail_count, r.first_fail_row, r.first_fail_code, r.rows_evaluated)


def bench_form(lib, d_rec, outs, expand, n, compact, stream, args):
    nc = 15 if compact else 57
    buf_a, buf_b = Buffers(n, nc), Buffers(n, nc)
    t, opts, keep, _ = engine._state_from_trace_args(d_rec)
    assert opts == _lib.OPT_DEVICE_PTRS

    def leg_a():
        expand.launch()
        return one_shot_rw(outs["rw"], outs["rw_flags"], buf_a, compact)

    def leg_b():
        return one_shot_trace(lib, t, buf_b, compact)

    def equal(a, b):
        (ra, na, ma), (rb, nb, mb) = a, b
        assert (na, ma) == (nb, mb) and verdict(ra) == verdict(rb), "the two legs disagree on the counts or the result"
        for x, y in zip(buf_a.views(na, ma), buf_b.views(nb, mb)):
            assert bool(torch.equal(x, y)), "the two legs disagree on an output"

    times = {"A": [], "B_pair": [], "B_lane": []}
    for rep in range(-1, args.reps):  # (rep -1: warm-up — code objects, the fast sort's LDS attribute)
        ms_a, out_a = timed(leg_a, stream)
        assert expand.collect().ok
        for writer in ("lane", "pair"):
            os.environ["ZK_STATE_TRACE_WRITER"] = writer  # (read per launch)
            buf_b.rows.fill_(-1)
            ms_b, out_b = timed(leg_b, stream)
            equal(out_a, out_b)
            if rep >= 0:
                times["B_" + writer].append(ms_b)
        if rep >= 0:
            times["A"].append(ms_a)
    # resident passes of the two sessions (every pass runs the session's whole chain)
    res = {}
    for key, writer, open_fn in (("from_rw", "pair", lambda: engine.open_state_assign_from_rw(outs["rw"], outs["rw_flags"], buf_a.rows, buf_a.flags, buf_a.mpt, compact=compact)),
                                 ("from_trace_pair", "pair", lambda: engine.open_state_assign_from_trace(d_rec, buf_b.rows, buf_b.flags, buf_b.mpt, compact=compact)),
                                 ("from_trace_lane", "lane", lambda: engine.open_state_assign_from_trace(d_rec, buf_b.rows, buf_b.flags, buf_b.mpt, compact=compact))):
        os.environ["ZK_STATE_TRACE_WRITER"] = writer
        with open_fn() as s:
            assert s.run().ok

            def passes():
                for _ in range(args.passes):
                    s.launch()

            res[key] = []
            for _ in range(args.reps):
                res[key].append(round(timed(passes, stream)[0] / args.passes, 5))
                s.collect()
    os.environ.pop("ZK_STATE_TRACE_WRITER", None)
    _, n_ops, n_mpt = out_a
    rnd = lambda v: [round(x, 4) for x in v]  # noqa: E731
    return {"form": "compact (15 cells)" if compact else "57 cells", "n_ops": n_ops, "n_mpt": n_mpt, "row_bytes_written": n_ops * nc * 32,
            "A_expand_then_assign_from_rw_ms": rnd(times["A"]), "B_assign_from_trace_ms": rnd(times["B_lane"]),
            "B_assign_from_trace_pair_writer_ms": rnd(times["B_pair"]),
            "A_median_ms": round(statistics.median(times["A"]), 4), "B_median_ms": round(statistics.median(times["B_lane"]), 4),
            "B_pair_writer_median_ms": round(statistics.median(times["B_pair"]), 4),
            "B_not_slower_than_A": statistics.median(times["B_lane"]) <= statistics.median(times["A"]),
            "resident_pass_ms": res, "legs_equal": True}


def kernel_stats(path):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append({"name": r.get("Name", ""), "calls": int(r.get("Calls", 0)), "total_ns": int(float(r.get("TotalDurationNs", 0))),
                         "average_ns": round(float(r.get("AverageNs", 0)), 1)})
    return sorted(rows, key=lambda r: -r["total_ns"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-steps", type=int, default=18)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trace-run", type=int, default=0)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--merge", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "state_assign_from_trace.json"))
    args = ap.parse_args()
    if args.merge:
        out = json.load(open(args.out))
        out["kernel_trace_of_three_one_shots"] = kernel_stats(args.kernel_stats)
    else:
        lib = _lib.init(0)
        stream = torch.cuda.Stream()
        _lib.check(lib.zk_set_stream(ctypes.c_void_p(stream.cuda_stream)), "zk_set_stream", lib)  # sessions and one-shots of this thread: this stream
        w = synth_block_trace(1 << args.log2_steps, seed=7)
        rw, fl = np.ascontiguousarray(w["rw"]), np.ascontiguousarray(w["rw_flags"])
        rec = trace.trace_records(trace.rw_ops_from_wire(rw, fl))
        n = int(rw.shape[0])
        d_rec = {k: (up(v) if hasattr(v, "dtype") else v) for k, v in rec.items()}
        if args.trace_run:
            t, _, _, _ = engine._state_from_trace_args(d_rec)
            b = Buffers(n, 57)
            for _ in range(args.trace_run):
                assert one_shot_trace(lib, t, b, False)[0].ok
            torch.cuda.synchronize()
            print(json.dumps({"tool": "bench_state_assign_from_trace", "trace_run": args.trace_run, "n_rw": n}))
            return
        outs = {"rw": torch.full((n, 14, 4), -1, dtype=torch.int64, device="cuda"), "rw_flags": torch.full((n,), -1, dtype=torch.int32, device="cuda")}
        expand = engine.open_evm_witness_from_trace(d_rec, outs=outs)
        forms = [bench_form(lib, d_rec, outs, expand, n, compact, stream, args) for compact in (False, True)]
        expand.close()
        out = {"tool": "bench_state_assign_from_trace", "table": f"synth_block_trace(2^{args.log2_steps}, seed=7)", "n_rw": n,
               "n_pool": int(rec["pool"].shape[0]), "passes": args.passes, "reps": args.reps, "forms": forms, "device": torch.cuda.get_device_name(0)}
        if args.kernel_stats:
            out["kernel_trace_of_three_one_shots"] = kernel_stats(args.kernel_stats)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
