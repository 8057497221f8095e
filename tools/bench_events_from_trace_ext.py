#!/usr/bin/env python3
"""zk_events_from_trace_ext: the copy and EXP event lists of a table that holds BeginTx, RETURN and DATACOPY steps, and the cost of the
wider per-step function on a block that holds none of them.

In one process on one stream, REPS times each:
  ladder   a table of 2^LOG2_STEPS steps, a tile of 16 steps repeated: a DATACOPY (two events), a RETURN to a caller, a deployment (a
           dst_ref lookup), a SHA3 and an EXP step, a BeginTx that emits nothing (it counts in the copy capacity) and ten plain steps -
           5 emitters and 6 events per 16 steps
             host      the plain-Python model's loop over the records (tests/events_from_trace_ext_ref.py, by the host clock)
             one-shot  zk_events_from_trace_ext with records, code set and output buffers resident (ZK_OPT_DEVICE_PTRS), between two
                       device events: open (checks, the capacity count, directory, buffers) + one pass + the counts
             resident  PASSES launches of an open session -> ms per pass
           the device's lists must equal the model's every time
  block    the bench's config 5 (synth_super_block: SHA3, CODECOPY and EXP events, none of the new states): a resident pass of
           zk_events_from_trace_ext beside one of zk_events_from_trace, alternating in the same job; equal lists
Prints one JSON line and writes profiles/events_from_trace_ext.json."""
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

from tests import events_from_trace_ext_cases as xc
from tests import events_from_trace_ext_ref as xref
from zkevm_specs_amd import _lib, engine, trace
from zkevm_specs_amd.super_circuit import synth_super_block

TILE = 16


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


def ladder(n_steps):
    """the tile's records (dense counters) repeated: every copy of the tile has its counters moved behind the one before"""
    b = xc.Builder()
    b.datacopy(6, 10, 7, 3, 5)
    b.ret(32, 8, ro=100, rl=20, follow=False)
    b.ret(4, 10, create=1, h=xc.H_DEP)
    b.sha3(64, 32)
    b.exp(3, 200)
    b.begin_tx("empty")
    while len(b.steps) < TILE:
        b.plain()
    c = b.case()
    t = c["trace"]
    assert t["rw_counter"] is None and t["rw_base"] == 1 and n_steps % TILE == 0
    reps, n_ops = n_steps // TILE, len(t["head"])
    steps = np.tile(t["steps"], (reps, 1))
    steps[:, 1] += np.repeat(np.arange(reps, dtype=np.uint64) * np.uint64(n_ops), TILE)
    rec = {k: np.tile(t[k], reps) for k in ("head", "id", "addr", "val")}
    rec.update(rw_counter=None, rw_base=1, pool=np.tile(t["pool"], (reps, 1)), steps=steps)
    return rec, c["codes"], c["hashes"]


def resident_inputs(rec, codes, hashes):
    x = engine.trace_event_sources(rec, codes, hashes)
    d_tr = {k: (up(v) if hasattr(v, "dtype") else v) for k, v in rec.items() if k != "prev"}
    return d_tr, {"code": up(x["code"]), "code_offsets": up(x["code_offsets"])}, up(x["code_hashes"])


def buffers(shapes):
    view = {np.uint64: torch.int64, np.uint32: torch.int32}
    return {k: torch.zeros(shp, dtype=view[dt], device="cuda") for k, (shp, dt) in shapes.items()}


def host_lists(outs, shapes, n_copy, n_exp):
    return engine.cut_trace_events({k: t.cpu().numpy().view(shapes[k][1]) for k, t in outs.items()}, n_copy, n_exp)


def pass_ms(s, stream, passes, reps):
    def run():
        for _ in range(passes):
            s.launch()

    out = []
    for _ in range(reps):
        out.append(round(timed(run, stream)[0] / passes, 5))
        s.collect()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-steps", type=int, default=18)
    ap.add_argument("--log2-total", type=int, default=20)
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "events_from_trace_ext.json"))
    args = ap.parse_args()
    lib = _lib.init(0)
    stream = torch.cuda.Stream()
    _lib.check(lib.zk_set_stream(ctypes.c_void_p(stream.cuda_stream)), "zk_set_stream", lib)
    fam = engine.TRACE_EVENTS_EXT

    # ---- the ladder
    rec, codes, hashes = ladder(1 << args.log2_steps)
    ns = int(rec["steps"].shape[0])
    d_tr, d_codes, d_hashes = resident_inputs(rec, codes, hashes)
    caps = engine.events_from_trace_ext_sizes(d_tr, d_codes, d_hashes)
    assert caps == xref.capacities(rec)
    shapes = engine.events_from_trace_ext_shapes(*caps)
    outs = buffers(shapes)
    x = dict(engine.trace_event_sources(d_tr, d_codes, d_hashes), copy_capacity=caps[0])
    prepared = engine._wire_args(fam, x, (), outs)
    d_status = torch.zeros(ns, dtype=torch.int32, device="cuda")

    def one_shot():
        res, a, b = _lib.ZkResult(), ctypes.c_uint64(), ctypes.c_uint64()
        _lib.check(lib.zk_events_from_trace_ext(ctypes.byref(prepared.t), ctypes.byref(prepared.w), prepared.opts, _lib.ptr(d_status), ctypes.byref(a),
                                                ctypes.byref(b), ctypes.byref(res)), "zk_events_from_trace_ext", lib)
        return engine.Result(res), int(a.value), int(b.value)

    times = {"host_model": [], "one_shot": []}
    for rep in range(args.reps):
        t0 = time.perf_counter()
        want = xref.derive(rec, codes, hashes)
        times["host_model"].append((time.perf_counter() - t0) * 1e3)
        for t in outs.values():
            t.zero_()
        with torch.cuda.stream(stream):
            if rep == 0:
                one_shot()  # warm-up
            ms_dev, (res, n_copy, n_exp) = timed(one_shot, stream)
        times["one_shot"].append(ms_dev)
        got = host_lists(outs, shapes, n_copy, n_exp)
        assert res.ok and np.array_equal(d_status.cpu().numpy().view(np.uint32), want["status"])
        assert all(np.array_equal(got[k], want[k]) for k in xc.OUTPUTS)
    with engine.open_events_from_trace_ext(d_tr, d_codes, d_hashes, outs) as s:
        assert s.run().ok
        ladder_pass = pass_ms(s, stream, args.passes, args.reps)
        assert s.counts() == (n_copy, n_exp) and all(np.array_equal(host_lists(outs, shapes, n_copy, n_exp)[k], want[k]) for k in xc.OUTPUTS)
    ladder_out = {"n_steps": ns, "n_rw_ops": int(rec["head"].shape[0]), "emitting_steps": ns // TILE * 5, "n_copy_events": n_copy, "n_exp_events": n_exp,
                  "copy_capacity": caps[0], "host_model_ms": [round(t, 1) for t in times["host_model"]], "one_shot_ms": [round(t, 4) for t in times["one_shot"]],
                  "median_ms": {k: round(statistics.median(v), 4) for k, v in times.items()}, "resident_pass_ms": ladder_pass, "lists_equal": True}
    del outs, d_tr, d_codes, d_hashes, prepared

    # ---- the block without the new states: the wider per-step function beside the old one
    p = synth_super_block(args.log2_total, seed=5)
    evm = p["evm"]
    heads = [row for row in evm["bytecode"] if int(row[2, 0]) == 1]
    word = lambda c: int.from_bytes(c.tobytes(), "little")  # noqa: E731
    hashes = [word(h[0]) | (word(h[1]) << 128) for h in heads]
    codes, at = [], 0
    for h in heads:  # the Byte rows follow their Header row
        n = int(h[5, 0])
        codes.append(bytes(evm["bytecode"][at + 1: at + 1 + n, 5, 0].astype(np.uint8)))
        at += 1 + n
    rec = dict(trace.rw_ops_from_wire(evm["rw"], evm["rw_flags"]), steps=trace.step_records_from_wire(evm["steps"]))
    ns = int(rec["steps"].shape[0])
    d_tr, d_codes, d_hashes = resident_inputs(rec, codes, hashes)
    caps = engine.events_from_trace_ext_sizes(d_tr, d_codes, d_hashes)
    assert caps == (ns, ns)  # none of the two-event states
    shapes_old, shapes_new = engine.events_from_trace_shapes(ns), engine.events_from_trace_ext_shapes(*caps)
    outs_old, outs_new = buffers(shapes_old), buffers(shapes_new)
    block = {"old": [], "new": []}
    with engine.open_events_from_trace(d_tr, d_codes, d_hashes, outs_old) as s0, engine.open_events_from_trace_ext(d_tr, d_codes, d_hashes, outs_new) as s1:
        assert s0.run().ok and s1.run().ok
        for _ in range(args.reps):  # alternating
            block["old"] += pass_ms(s0, stream, args.passes, 1)
            block["new"] += pass_ms(s1, stream, args.passes, 1)
        c0, c1 = s0.counts(), s1.counts()
        assert c0 == c1
        a, b = host_lists(outs_old, shapes_old, *c0), host_lists(outs_new, shapes_new, *c1)
        assert all(np.array_equal(a[k], b[k]) for k in a) and not b["copy_dst_ref"].any()
    block_out = {"block": f"synth_super_block(2^{args.log2_total}, seed=5)", "n_steps": ns, "n_copy_events": c0[0], "n_exp_events": c0[1],
                 "resident_pass_ms": {"zk_events_from_trace": block["old"], "zk_events_from_trace_ext": block["new"]},
                 "median_ms": {"zk_events_from_trace": statistics.median(block["old"]), "zk_events_from_trace_ext": statistics.median(block["new"])},
                 "lists_equal": True}
    out = {"tool": "bench_events_from_trace_ext", "passes": args.passes, "reps": args.reps, "ladder": ladder_out, "block": block_out,
           "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
