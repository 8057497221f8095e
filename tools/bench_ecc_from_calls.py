#!/usr/bin/env python3
"""zk_ecc_from_calls on one MI355X: one pass over 2^12 ecAdd, 2^12 ecMul and 256 two-pair ecPairing calls resident in HBM, HIP events
around the pass (zk_result.kernel_ms of a collect after one launch), three repetitions after a warm-up pass; for comparison
zk_ecc_open's verify pass over the same ops and rows (the entry's own outputs, in place).  The calls are made with the engine itself
(k G from a first ecMul batch), so nothing but this package is needed.  Writes one JSON record (default profiles/ecc_from_calls.json).

    python tools/bench_ecc_from_calls.py [--out PATH] [--adds N] [--muls N] [--pairings N] [--reps K]
"""
import argparse
import json
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zkevm_specs_amd import ecc_circuit, engine, oneshot  # noqa: E402

P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
G = (1, 2)
# the generator of G2 in the input's word order (x.c1, x.c0, y.c1, y.c0), EIP-197
Q = (11559732032986387107991004021392285783925812861821192530917403151452391805634, 10857046999023057135944570762232829481370756359578518086990519993285655852781,
     4082367875863433681332203403145435568316851327593401208105741076214120093531, 8495653923123431417604973247489272438418190587263600148770280649306958101930)
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617  # the group's order, and the cells' modulus
RANDOMNESS = 0x0123456789ABCDEF0123456789ABCDEF0123456789ABCDEF0123456789ABCDEF % R


def word(cell):
    return sum(int(cell[k]) << (64 * k) for k in range(4))


def make_calls(n_add, n_mul, n_pairing, rng):
    n_pts = 2 * n_add + n_mul + n_pairing
    _, _, out = oneshot.ecc_from_calls(ecc_circuit.ecc_calls_wire([], [(G, rng.randrange(1, 1 << 254)) for _ in range(n_pts)], []), RANDOMNESS)
    pts = [(word(w[4]), word(w[5])) for w in out["points"]]
    adds = [(pts[2 * k], pts[2 * k + 1]) for k in range(n_add)]
    # scalars below p: above it the ECC circuit rejects the row at its copy constraint and the compared verify pass would skip its chain
    muls = [(pts[2 * n_add + k], rng.randrange(P)) for k in range(n_mul)]
    pairings = []
    for k in range(n_pairing):  # e(A, Q) e(-A, Q) = 1
        a = pts[2 * n_add + n_mul + k]
        pairings.append(([a, (a[0], P - a[1])], [Q, Q]))
    return adds, muls, pairings


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ecc_from_calls.json"))
    ap.add_argument("--adds", type=int, default=1 << 12)
    ap.add_argument("--muls", type=int, default=1 << 12)
    ap.add_argument("--pairings", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import torch

    adds, muls, pairings = make_calls(a.adds, a.muls, a.pairings, random.Random(2026))
    host = ecc_circuit.ecc_calls_wire(adds, muls, pairings)
    dev = {k: torch.from_numpy(v.view({8: np.int64, 4: np.int32}[v.dtype.itemsize])).cuda() for k, v in host.items()}
    n = a.adds + a.muls + a.pairings
    tdt = {np.uint64: torch.int64, np.uint32: torch.int32}
    outs = {k: torch.zeros(shp, dtype=tdt[dt], device="cuda") for k, (shp, dt) in engine.ecc_calls_shapes(a.adds, a.muls, a.pairings).items()}
    rec = {"what": "tools/bench_ecc_from_calls.py on one MI355X: one zk_ecc_from_calls pass (calls and outputs in HBM) and zk_ecc_open's verify "
                   "pass over the same ops and rows; kernel_ms = HIP events around a pass, one launch per collect, after one warm-up pass",
           "calls": {"add": a.adds, "mul": a.muls, "pairing": a.pairings, "pairs_per_pairing": 2}}
    with engine.open_ecc_from_calls(dev, RANDOMNESS, outs=outs) as s:
        s.run()
        ms = [s.run().kernel_ms for _ in range(a.reps)]
        out = s.read()
        rec["from_calls_kernel_ms"] = [round(x, 4) for x in ms]
        rec["table_rows"] = int(out["ecc_table"].shape[0])
    valid = out["rows"][:, 12, 0]
    rec["valid_calls"] = int(valid.sum())
    rec["pairings_accepted"] = int(out["pair_out"][:, 0].sum())
    assert rec["valid_calls"] == n and rec["pairings_accepted"] == a.pairings and rec["table_rows"] == n, rec
    wire = {"points": outs["points"], "n_add": a.adds, "n_mul": a.muls, "pair_pts": dev["pair_pts"], "pair_off": dev["pair_off"],
            "pair_out": outs["pair_out"], "max_ok": np.ones(3, dtype=np.uint32)}
    with engine.open_ecc(wire, outs["rows"], RANDOMNESS) as v:
        v.run()
        res = [v.run() for _ in range(a.reps)]
        rec["verify_kernel_ms"] = [round(r.kernel_ms, 4) for r in res]
        rec["verify_fail_count"] = int(res[-1].fail_count)
        assert rec["verify_fail_count"] == 0, rec
    rec["from_calls_median_ms"] = round(float(np.median(rec["from_calls_kernel_ms"])), 4)
    rec["verify_median_ms"] = round(float(np.median(rec["verify_kernel_ms"])), 4)
    rec["calls_per_s"] = int(n / (rec["from_calls_median_ms"] * 1e-3))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
