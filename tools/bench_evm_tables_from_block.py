#!/usr/bin/env python3
"""The EVM circuit's tx table from raw block data (zk_evm_tables_from_block) against the host path it replaces, on a block of 2^10 txs
with 2^20 calldata bytes in all (skewed lengths: many empty and short txs, a few of hundreds of KiB).

Legs, in one process, alternating, REPS times:
  A   the host path: Transaction.table_assignments() over the mirror objects + flatten_tx_table (host clock), then the upload of the
      160-byte rows and their flags from page-locked memory (device events); the two parts are reported separately
  B   the upload of the raw inputs (tx fields, flags, access counts, calldata, offsets; page-locked) + one pass of the session, device
      events around both together
Also: PASSES passes of the resident session between two events -> ms per pass and the bytes it writes per second (160-byte row + 4-byte
flag + 4-byte status per tx-table row; the block and withdrawal tables are a few KB), to hold against the 6.0-6.3 TB/s that streamed
16-byte stores reach on an MI355X.  The tables of A and B must be equal.  Prints one JSON line and writes
profiles/evm_tables_from_block.json.
"""
import argparse
import json
import os
import random
import sys
import time
from itertools import chain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from zkevm_specs_amd import _lib, block_tables as bt, engine, flatten


def block_of(n_txs, total, seed=3):
    """n_txs txs with `total` calldata bytes: a third empty, most below 200 bytes, four that share what is left"""
    rng = random.Random(seed)
    lengths = [0 if rng.random() < 0.33 else rng.randrange(1, 200) for _ in range(n_txs - 4)]
    rest = total - sum(lengths)
    cuts = sorted(rng.randrange(rest) for _ in range(3))
    lengths += [cuts[0], cuts[1] - cuts[0], cuts[2] - cuts[1], rest - cuts[2]]
    rng.shuffle(lengths)
    g = np.random.default_rng(seed)
    txs = []
    for i, n in enumerate(lengths):
        data = g.integers(0, 256, n, dtype=np.uint8)
        data[g.random(n) < 0.4] = 0
        txs.append(bt.Transaction(id=i + 1, nonce=rng.getrandbits(64), gas=rng.getrandbits(64), gas_price=rng.getrandbits(256),
                                  caller_address=rng.getrandbits(160), callee_address=None if i % 7 == 0 else rng.getrandbits(160),
                                  value=rng.getrandbits(256), call_data=data.tobytes(), invalid_tx=i % 2))
    blk = bt.Block(number=1 << 30, history_hashes=[rng.getrandbits(256) for _ in range(256)])
    wds = [bt.Withdrawal(id=i, validator_id=i, amount=rng.getrandbits(64)) for i in range(16)]
    return blk, txs, wds


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
    ap.add_argument("--log2-txs", type=int, default=10)
    ap.add_argument("--log2-bytes", type=int, default=20)
    ap.add_argument("--passes", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evm_tables_from_block.json"))
    args = ap.parse_args()
    _lib.init(0)
    blk, txs, wds = block_of(1 << args.log2_txs, 1 << args.log2_bytes)
    raw = bt.raw_block_data(blk, txs, wds)
    n_rows = 12 * len(txs) + len(raw["calldata"])
    shapes = engine.evm_tables_from_block_shapes(len(txs), len(raw["calldata"]), 256, len(wds))
    stream = torch.cuda.Stream()
    # B: page-locked raw inputs, their device tensors (the session uses them in place), caller-owned outputs
    pinned = {k: as_torch(v).pin_memory() for k, v in raw.items()}
    d_raw = {k: torch.empty_like(v, device="cuda") for k, v in pinned.items()}
    for k in d_raw:
        d_raw[k].copy_(pinned[k])
    outs = {k: torch.full(shp, -1, dtype=torch.int64 if dt == np.uint64 else torch.int32, device="cuda") for k, (shp, dt) in shapes.items()}
    torch.cuda.synchronize()
    s = engine.open_evm_tables_from_block(d_raw, outs=outs)
    s.set_stream(stream)
    # A: the destination of the uploaded rows
    a_rows = torch.full(shapes["tx"][0], -1, dtype=torch.int64, device="cuda")
    a_flags = torch.full(shapes["tx_flags"][0], -1, dtype=torch.int32, device="cuda")

    def leg_b():
        with torch.cuda.stream(stream):
            for k in d_raw:
                d_raw[k].copy_(pinned[k], non_blocking=True)
        s.launch()

    def passes(n):
        for _ in range(n):
            s.launch()

    passes(args.warmup)
    assert s.collect().ok
    a_host_s, a_upload_ms, b_ms, pass_ms = [], [], [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        rows, flags = flatten.flatten_tx_table(list(chain(*[t.table_assignments() for t in txs])))
        a_host_s.append(time.perf_counter() - t0)
        p_rows, p_flags = as_torch(rows).pin_memory(), as_torch(flags).pin_memory()

        def leg_a_upload():
            with torch.cuda.stream(stream):
                a_rows.copy_(p_rows, non_blocking=True)
                a_flags.copy_(p_flags, non_blocking=True)

        a_upload_ms.append(timed(leg_a_upload, stream))
        b_ms.append(timed(leg_b, stream))
        assert s.collect().ok
        pass_ms.append(timed(lambda: passes(args.passes), stream) / args.passes)
        assert s.collect().ok
    torch.cuda.synchronize()
    equal = bool(torch.equal(a_rows, outs["tx"])) and bool(torch.equal(a_flags, outs["tx_flags"]))
    s.close()
    pass_bytes = n_rows * (160 + 4 + 4) + shapes["block"][0][0] * (128 + 4) + len(wds) * 128
    upload_b = sum(int(v.numel()) * v.element_size() for v in pinned.values())
    rec = {"tool": "bench_evm_tables_from_block", "n_txs": len(txs), "calldata_bytes": int(len(raw["calldata"])), "tx_table_rows": n_rows,
           "longest_tx_bytes": int(np.diff(raw["offsets"]).max()), "passes": args.passes, "reps": args.reps,
           "A_host_flatten_s": [round(v, 3) for v in a_host_s], "A_upload_ms": [round(v, 4) for v in a_upload_ms],
           "B_upload_plus_pass_ms": [round(v, 4) for v in b_ms], "pass_ms": [round(v, 5) for v in pass_ms],
           "upload_bytes": {"A_rows_and_flags": n_rows * 164, "B_raw_inputs": upload_b},
           "pass_bytes_written": pass_bytes, "pass_write_TB_per_s": [round(pass_bytes / (v * 1e-3) / 1e12, 3) for v in pass_ms],
           "streamed_store_reference_TB_per_s": [6.0, 6.3], "outputs_equal": equal, "device": torch.cuda.get_device_name(0)}
    assert equal, "the host path and the session disagree on the timed inputs"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
