#!/usr/bin/env python3
"""The EVM circuit's RW table and step table from compact trace records (zk_evm_witness_from_trace) against the upload of the wire arrays
it replaces, on the RW table and steps of bench.py's 2^18-step trace (synth_evm_trace(2^18, seed=3)).

Legs, in one process, alternating, REPS times:
  A   the upload of the wire arrays rw / rw_flags / steps from page-locked memory (device events)
  B   the upload of the records (head, id, addr, val, prev, pool, steps; page-locked) + one pass of the session, device events around
      both together
Also: PASSES passes of the resident session between two events -> ms per pass and the bytes it writes per second (448-byte row + 4-byte
flag + 4-byte status per RW row, 416 bytes per step), to hold against the 6.0-6.3 TB/s that streamed 16-byte stores reach on an MI355X
and the 3.5 TB/s of btb_rows_kernel.  The arrays of A and B must be equal.  Prints one JSON line and writes
profiles/evm_witness_from_trace.json.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from zkevm_specs_amd import _lib, engine, trace
from zkevm_specs_amd.synth_evm import synth_evm_trace


def as_torch(x):
    return torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x.view(np.int32) if x.dtype == np.uint32 else x)


def timed(fn, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(stream)
    fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-steps", type=int, default=18)
    ap.add_argument("--passes", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evm_witness_from_trace.json"))
    args = ap.parse_args()
    _lib.init(0)
    w = synth_evm_trace(1 << args.log2_steps, seed=3)
    wire = {k: np.ascontiguousarray(w[k]) for k in ("rw", "rw_flags", "steps")}
    rec = trace.trace_records(trace.rw_ops_from_wire(wire["rw"], wire["rw_flags"]), trace.step_records_from_wire(wire["steps"]))
    arrays = {k: v for k, v in rec.items() if hasattr(v, "dtype")}
    n_rw, n_steps = wire["rw"].shape[0], wire["steps"].shape[0]
    shapes = engine.evm_witness_from_trace_shapes(n_rw, n_steps)
    stream = torch.cuda.Stream()
    # B: page-locked records, their device tensors (the session uses them in place), caller-owned outputs
    pinned = {k: as_torch(v).pin_memory() for k, v in arrays.items()}
    d_rec = {k: torch.empty_like(v, device="cuda") for k, v in pinned.items()}
    for k in d_rec:
        d_rec[k].copy_(pinned[k])
    outs = {k: torch.full(shp, -1, dtype=torch.int64 if dt == np.uint64 else torch.int32, device="cuda") for k, (shp, dt) in shapes.items()}
    torch.cuda.synchronize()
    s = engine.open_evm_witness_from_trace(dict(rec, **d_rec), outs=outs)
    s.set_stream(stream)
    # A: page-locked wire arrays and their destination
    p_wire = {k: as_torch(v).pin_memory() for k, v in wire.items()}
    a_wire = {k: torch.full_like(v, -1, device="cuda") for k, v in p_wire.items()}

    def leg_a():
        with torch.cuda.stream(stream):
            for k in a_wire:
                a_wire[k].copy_(p_wire[k], non_blocking=True)

    def leg_b():
        with torch.cuda.stream(stream):
            for k in d_rec:
                d_rec[k].copy_(pinned[k], non_blocking=True)
        s.launch()

    def passes(n):
        for _ in range(n):
            s.launch()

    passes(args.warmup)
    assert s.collect().ok
    a_ms, b_ms, pass_ms = [], [], []
    for _ in range(args.reps):
        a_ms.append(timed(leg_a, stream))
        b_ms.append(timed(leg_b, stream))
        assert s.collect().ok
        pass_ms.append(timed(lambda: passes(args.passes), stream) / args.passes)
        assert s.collect().ok
    torch.cuda.synchronize()
    equal = all(bool(torch.equal(a_wire[k], outs[k])) for k in a_wire)
    s.close()
    pass_bytes = n_rw * (448 + 4 + 4) + n_steps * 416
    wire_b = sum(int(v.nbytes) for v in wire.values())
    rec_b = trace.record_bytes(rec)
    rw_rec_b = rec_b - int(rec["steps"].nbytes)
    out = {"tool": "bench_evm_witness_from_trace", "n_steps": n_steps, "n_rw": n_rw, "n_pool": int(rec["pool"].shape[0]),
           "rw_counter_explicit": rec["rw_counter"] is not None, "passes": args.passes, "reps": args.reps,
           "A_upload_wire_ms": [round(v, 4) for v in a_ms], "B_upload_records_plus_pass_ms": [round(v, 4) for v in b_ms],
           "pass_ms": [round(v, 5) for v in pass_ms],
           "upload_bytes": {"A_wire": wire_b, "B_records": rec_b},
           "record_bytes_per_rw_row": round(rw_rec_b / n_rw, 2), "wire_bytes_per_rw_row": 452,
           "record_bytes_per_step": 104, "wire_bytes_per_step": 416,
           "pass_bytes_written": pass_bytes, "pass_write_TB_per_s": [round(pass_bytes / (v * 1e-3) / 1e12, 3) for v in pass_ms],
           "streamed_store_reference_TB_per_s": [6.0, 6.3], "btb_rows_kernel_TB_per_s": 3.5, "outputs_equal": equal,
           "device": torch.cuda.get_device_name(0)}
    assert equal, "the uploaded wire and the session disagree on the timed inputs"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
