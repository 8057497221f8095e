#!/usr/bin/env python3
"""Bytecode table / circuit rows / keccak rows from raw contract code (zk_bytecode_from_code) against the row path it replaces, on a
code set of 2^17 table rows (the size behind DESIGN.md §6's Bytecode-assignment figure), everything resident in HBM.

Legs, timed in one process with device events around PASSES passes each, alternating, REPS times:
  A   the row path: a zk_keccak_table session over the codes + a zk_bytecode_assign session over the resident 192-byte rows
  B   the new session writing `rows` and `keccak` into caller buffers, `table` left to the session
  B'  the new session with `table` in a caller buffer as well
The outputs of A and B on the timed inputs must be equal.  Also reported: the bytes each form needs uploaded (192 n against n).
Prints one JSON line and writes profiles/bytecode_from_code.json.
"""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from zkevm_specs_amd import _lib, engine

R = 0x2A3B4C5D6E7F8091A2B3C4D5E6F708192A3B4C5D6E7F8091A2B3C4D5E6F70819 % 21888242871839275222246405745257275088548364400416034343698204186575808495617


def code_set(n_rows, n_codes=16, seed=5):
    """n_codes codes with n_rows table rows in total: lengths of 2..24 KiB, 30 % of the bytes PUSH1..PUSH32"""
    rng = random.Random(seed)
    while True:
        lengths = [rng.randrange(2 << 10, 24 << 10) for _ in range(n_codes - 1)]
        rest = n_rows - n_codes - sum(lengths)
        if (2 << 10) <= rest <= (24 << 10):
            break
    lengths.append(rest)
    g = np.random.default_rng(seed)
    codes = []
    for n in lengths:
        b = g.integers(0, 256, n, dtype=np.uint8)
        push = g.random(n) < 0.3
        b[push] = g.integers(0x60, 0x80, int(push.sum()), dtype=np.uint8)
        codes.append(b.tobytes())
    return codes


def dev(x):
    return torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).cuda()


def timed(launch, passes, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(stream)
    launch(passes)
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / passes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-rows", type=int, default=17)
    ap.add_argument("--passes", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bytecode_from_code.json"))
    args = ap.parse_args()
    _lib.init(0)
    k = args.log2_rows
    codes = code_set(1 << k)
    code, off = engine.pack_messages(codes)
    n_bytes, n_codes = len(code), len(codes)
    d_code, d_off = dev(code), dev(off)
    new = lambda shape: torch.full(shape, -1, dtype=torch.int64, device="cuda")  # noqa: E731
    shapes = engine.bytecode_from_code_shapes(n_bytes, n_codes, k)
    b_rows, b_keccak = new(shapes["rows"]), new(shapes["keccak"])
    b2_table, b2_rows, b2_keccak = new(shapes["table"]), new(shapes["rows"]), new(shapes["keccak"])
    a_rows, a_keccak = new(shapes["rows"]), new(shapes["keccak"])
    # every session rides one stream of its own, so that the events around the passes are in order with them
    stream = torch.cuda.Stream()
    sB = engine.open_bytecode_from_code(d_code, d_off, k, R, rows_dev=b_rows, keccak_dev=b_keccak)
    sB2 = engine.open_bytecode_from_code(d_code, d_off, k, R, table_dev=b2_table, rows_dev=b2_rows, keccak_dev=b2_keccak)
    for s in (sB, sB2):
        s.set_stream(stream)
    assert sB2.run().ok
    torch.cuda.synchronize()
    # the row path's inputs, resident: the 192-byte rows (as B' made them), their row offsets and the byte lengths
    d_row_off = dev(off + np.arange(n_codes + 1, dtype=np.uint64))
    d_len = dev(np.diff(off))
    sAk = engine.open_keccak(d_code, d_off, R, rows_dev=a_keccak)
    sAb = engine.open_bytecode_assign(b2_table, d_row_off, d_len, k, R, rows_dev=a_rows)
    for s in (sAk, sAb):
        s.set_stream(stream)

    def leg_a(n):
        for _ in range(n):
            sAk.launch()
            sAb.launch()
        assert sAk.collect().ok and sAb.collect().ok

    def leg(s):
        def run(n):
            for _ in range(n):
                s.launch()
            assert s.collect().ok
        return run

    legs = {"A": leg_a, "B": leg(sB), "B_table": leg(sB2)}
    for f in legs.values():
        f(args.warmup)
    ms = {name: [] for name in legs}
    for _ in range(args.reps):
        for name, f in legs.items():
            ms[name].append(timed(f, args.passes, stream))
    torch.cuda.synchronize()
    equal = bool(torch.equal(a_rows, b_rows)) and bool(torch.equal(a_keccak, b_keccak)) and bool(torch.equal(a_rows, b2_rows))
    for s in (sB, sB2, sAk, sAb):
        s.close()
    spread_a = max(ms["A"]) - min(ms["A"])
    rec = {"tool": "bench_bytecode_from_code", "table_rows": 1 << k, "n_codes": n_codes, "code_bytes": n_bytes, "passes": args.passes,
           "reps": args.reps, "ms_per_pass": {n: [round(v, 5) for v in vs] for n, vs in ms.items()},
           "ms_per_pass_best": {n: round(min(vs), 5) for n, vs in ms.items()}, "A_spread_ms": round(spread_a, 5),
           "B_no_slower_than_A_within_spread": bool(min(ms["B"]) <= min(ms["A"]) + spread_a),
           "upload_bytes": {"A_rows": 192 * (1 << k), "A_keccak_data": n_bytes, "B": n_bytes},
           "outputs_equal": equal, "device": torch.cuda.get_device_name(0)}
    assert equal, "the row path and the new session disagree on the timed inputs"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
