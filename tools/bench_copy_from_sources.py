#!/usr/bin/env python3
"""The Copy witness of a block from its raw inputs (zk_copy_assign_from_sources) against the route there was: the host gather of the
`data` array, its upload and zk_copy_assign.  Block: the bench's config 5 (synth_super_block: synth_block with block_ops), whose copy
events are CODECOPY (Bytecode -> Memory) and SHA3 (Memory -> RlcAcc) steps.

In one process on one stream, legs alternating, REPS times:
  A   the parent's path: the host gather (CopyEvents.copy's loop per byte over the contracts' bytes and the memory values, with the host
      is_code scan of every contract a Bytecode copy reads) by the host clock; then the upload of `data` and the zk_copy_assign one-shot
      over resident events (ZK_OPT_DEVICE_PTRS, the caller's output buffers) between two device events
  B   the zk_copy_assign_from_sources one-shot with the sources resident (code set, trace records), into buffers of the same kind
  resident pass: PASSES launches of an open_copy_assign session and of an open_copy_assign_from_sources session -> ms per pass
The rows, flags, table and RW rows of A and B must be equal, and B's gathered data must be A's.  Prints one JSON line and writes
profiles/copy_from_sources.json.

  --trace-run N           only N one-shots of leg B, nothing timed: the run to put under a kernel trace of its own
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
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from zkevm_specs_amd import _lib, engine, trace
from zkevm_specs_amd.copy_circuit import CopyEvents
from zkevm_specs_amd.super_circuit import synth_super_block


def up(x):
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16, np.dtype(np.uint8): np.uint8}[x.dtype]
    return torch.from_numpy(np.ascontiguousarray(x).view(view)).cuda()


def timed(fn, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(stream)
    out = fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def init_is_code(code):
    out, left = [], 0
    for b in code:
        out.append(1 if left == 0 else 0)
        left = (b - 0x5F if 0x60 <= b <= 0x7F else 0) if left == 0 else left - 1
    return out


class CodeView:
    """src_data of a Bytecode copy: address -> (byte, is_code)"""

    def __init__(self, code, is_code):
        self.code, self.is_code = code, is_code

    def __contains__(self, a):
        return a < len(self.code)

    def __getitem__(self, a):
        return self.code[a], self.is_code[a]


def host_gather(ev_rows, flags, codes, code_ref, mem_values, r):
    """the parent's host pass: every event through CopyEvents.copy (a Python loop per byte); the is_code scan of a contract when the first
    copy reads it -> (data uint16[], offsets uint64[])"""
    ce = CopyEvents(r)
    views = {}
    for e, row in enumerate(ev_rows):
        s_lo, s_hi, s_tag, d_lo, d_hi, d_tag, src_addr, src_end, dst_addr, length, log_id, rwc = row
        if s_tag == 1:
            j = code_ref[e]
            if j not in views:
                views[j] = CodeView(codes[j], init_is_code(codes[j]))
            src = views[j]
        else:
            src = mem_values[e]
        ce.copy(rwc, s_lo, s_tag, d_lo, d_tag, src_addr, src_end, dst_addr, length, src, log_id)
    return np.array(ce.data, dtype=np.uint16), np.array(ce.offsets, dtype=np.uint64)


class Outs:
    def __init__(self, sizes):
        n_rows, n_table, n_rw, n_data = sizes
        i64, i32 = dict(dtype=torch.int64, device="cuda"), dict(dtype=torch.int32, device="cuda")
        self.rows, self.rf = torch.full((20, n_rows, 4), -1, **i64), torch.full((n_rows,), -1, **i32)
        self.table = torch.full((n_table, 14, 4), -1, **i64)
        self.rw, self.rwf = torch.full((n_rw, 14, 4), -1, **i64), torch.full((n_rw,), -1, **i32)
        self.data = torch.full((n_data,), -1, dtype=torch.int16, device="cuda")

    def five(self):
        return self.rows, self.rf, self.table, self.rw, self.rwf


def kernel_stats(path):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append({"name": r.get("Name", ""), "calls": int(r.get("Calls", 0)), "total_ns": int(float(r.get("TotalDurationNs", 0))),
                         "average_ns": round(float(r.get("AverageNs", 0)), 1)})
    return sorted(rows, key=lambda r: -r["total_ns"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-total", type=int, default=20)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trace-run", type=int, default=0)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--merge", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "copy_from_sources.json"))
    args = ap.parse_args()
    if args.merge:
        out = json.load(open(args.out))
        out["kernel_trace_of_one_shots"] = kernel_stats(args.kernel_stats)
    else:
        lib = _lib.init(0)
        stream = torch.cuda.Stream()
        _lib.check(lib.zk_set_stream(ctypes.c_void_p(stream.cuda_stream)), "zk_set_stream", lib)
        p = synth_super_block(args.log2_total, seed=5)
        ce, evm, codes = p["copy_events"], p["evm"], [bytes(c) for c in p["codes"]]
        events, flags, r = np.ascontiguousarray(ce["events"]), np.ascontiguousarray(ce["flags"]), ce["r"]
        n = int(events.shape[0])
        ev_rows = [[int.from_bytes(events[e, k].tobytes(), "little") for k in range(12)] for e in range(n)]
        # the refs: a contract's index in the code set, by the hash its Header row carries
        bt = evm["bytecode"]
        heads = [row for row in bt if int(row[2, 0]) == 1]
        assert len(heads) == len(codes)
        index = {(int.from_bytes(h[0].tobytes(), "little"), int.from_bytes(h[1].tobytes(), "little")): j for j, h in enumerate(heads)}
        code_ref = [index[(row[0], row[1])] if row[2] == 1 else 0 for row in ev_rows]
        # what the parent's builder is handed for a Memory source: the memory values at the event's addresses
        mem_values = [None] * n
        for e, row in enumerate(ev_rows):
            if row[2] == 2:
                lo = int(ce["offsets"][e])
                mem_values[e] = {row[6] + i: int(ce["data"][lo + i]) & 0xFF for i in range(int(ce["offsets"][e + 1]) - lo)}
        ops = trace.rw_ops_from_wire(evm["rw"], evm["rw_flags"])
        sources = {"code": np.frombuffer(b"".join(codes), np.uint8).copy(), "code_offsets": np.cumsum([0] + [len(c) for c in codes]).astype(np.uint64),
                   "calldata": None, "calldata_offsets": None, "trace": {k: ops[k] for k in ("head", "id", "addr", "val", "rw_counter", "rw_base")}}
        d_ev, d_fl, d_ref = up(events), up(flags), up(np.array(code_ref, dtype=np.uint32))
        d_src = {k: (up(v) if v is not None else None) for k, v in sources.items() if k != "trace"}
        d_src["trace"] = {k: (up(v) if hasattr(v, "dtype") else v) for k, v in sources["trace"].items()}
        sizes = engine.copy_assign_from_sources_sizes(d_ev, d_fl, d_ref, None, d_src)
        out_a, out_b = Outs(sizes), Outs(sizes)
        t_b, opts_b, keep_b = engine._copy_sources_args(d_ev, d_fl, d_ref, None, d_src, r)
        d_status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        h_offsets = np.zeros(n + 1, dtype=np.uint64)

        def leg_b():
            res = _lib.ZkResult()
            _lib.check(lib.zk_copy_assign_from_sources(ctypes.byref(t_b), *(_lib.ptr(x) for x in out_b.five()), _lib.ptr(out_b.data), _lib.ptr(h_offsets),
                                                       opts_b, _lib.ptr(d_status), ctypes.byref(res)), "zk_copy_assign_from_sources", lib)
            return engine.Result(res)

        if args.trace_run:
            for _ in range(args.trace_run):
                assert leg_b().ok
            torch.cuda.synchronize()
            print(json.dumps({"tool": "bench_copy_from_sources", "trace_run": args.trace_run, "n_events": n, "sizes": sizes}))
            return

        d_r = engine._randomness_cells(r, d_ev)

        def leg_a_device(data, offsets):
            d_data, d_off = up(data), up(offsets)  # the upload the new entry drops
            t_a = _lib.ZkCopyEvents(_lib.ptr(d_ev), _lib.ptr(d_fl), n, _lib.ptr(d_data, len(data)), _lib.ptr(d_off), _lib.ptr(d_r))
            res = _lib.ZkResult()
            _lib.check(lib.zk_copy_assign(ctypes.byref(t_a), *(_lib.ptr(x) for x in out_a.five()), _lib.OPT_DEVICE_PTRS, ctypes.byref(res)), "zk_copy_assign", lib)
            return engine.Result(res)

        times = {"A_host_gather": [], "A_upload_and_assign": [], "B_from_sources": []}
        for rep in range(-1, args.reps):  # (rep -1: warm-up)
            t0 = time.perf_counter()
            data, offsets = host_gather(ev_rows, flags, codes, code_ref, mem_values, r)
            ms_gather = (time.perf_counter() - t0) * 1e3
            assert np.array_equal(data, ce["data"]) and np.array_equal(offsets, ce["offsets"])
            with torch.cuda.stream(stream):
                ms_a, res_a = timed(lambda: leg_a_device(data, offsets), stream)
                ms_b, res_b = timed(leg_b, stream)
            assert res_a.ok and res_b.ok
            for x, y in zip(out_a.five(), out_b.five()):
                assert bool(torch.equal(x, y)), "the two legs disagree on an output"
            assert np.array_equal(out_b.data.cpu().numpy().view(np.uint16), data) and np.array_equal(h_offsets, offsets)
            if rep >= 0:
                times["A_host_gather"].append(ms_gather)
                times["A_upload_and_assign"].append(ms_a)
                times["B_from_sources"].append(ms_b)
        resident = {}
        d_data, d_off = up(data), up(offsets)
        for key, open_fn in (("copy_assign", lambda: engine.open_copy_assign(d_ev, d_fl, d_data, d_off, r, *out_a.five())),
                             ("copy_assign_from_sources", lambda: engine.open_copy_assign_from_sources(d_ev, d_fl, d_ref, None, d_src, r, *out_b.five(), out_b.data))):
            with open_fn() as s:
                assert s.run().ok

                def passes():
                    for _ in range(args.passes):
                        s.launch()

                resident[key] = []
                for _ in range(args.reps):
                    resident[key].append(round(timed(passes, stream)[0] / args.passes, 5))
                    s.collect()
        rnd = lambda v: [round(x, 4) for x in v]  # noqa: E731
        med = lambda k: round(statistics.median(times[k]), 4)  # noqa: E731
        out = {"tool": "bench_copy_from_sources", "block": f"synth_super_block(2^{args.log2_total}, seed=5)", "n_events": n, "n_rows": sizes[0],
               "n_table": sizes[1], "n_rw_rows": sizes[2], "n_data": sizes[3], "code_bytes": int(sources["code"].shape[0]), "n_codes": len(codes),
               "trace_ops": int(ops["head"].shape[0]), "data_upload_bytes": 2 * sizes[3], "passes": args.passes, "reps": args.reps,
               "A_host_gather_ms": rnd(times["A_host_gather"]), "A_upload_and_assign_ms": rnd(times["A_upload_and_assign"]),
               "B_from_sources_ms": rnd(times["B_from_sources"]),
               "A_median_ms": {"host_gather": med("A_host_gather"), "upload_and_assign": med("A_upload_and_assign")},
               "B_median_ms": med("B_from_sources"), "resident_pass_ms": resident, "legs_equal": True, "device": torch.cuda.get_device_name(0)}
        if args.kernel_stats:
            out["kernel_trace_of_one_shots"] = kernel_stats(args.kernel_stats)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
