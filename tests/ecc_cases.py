"""Shared helpers of the ECC circuit tests: the golden cases of tests/golden/ecc_cases.npz (tools/gen_golden_ecc.py), random ops,
and the ops behind the EccTableRows the EVM fixtures carry."""
import json
import os
import random

import numpy as np

from tests import bn254_ref as b

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ecc_cases.npz")
KEYS = ("points", "pair_pts", "pair_off", "pair_out", "max_ok")


def golden_cases():
    g = np.load(GOLDEN)
    meta = json.loads(str(g["meta"]))
    r = int(meta["randomness"], 16)
    for i, m in enumerate(meta["cases"]):
        w = {k: g[f"{i}_{k}"] for k in KEYS}
        w["n_add"], w["n_mul"] = m["n_add"], m["n_mul"]
        yield m, w, g[f"{i}_rows"], g[f"{i}_assigned"], g[f"{i}_status"], r


def word(cell):
    return sum(int(cell[k]) << (64 * k) for k in range(4))


def rows_to_ints(rows):
    return [[word(c) for c in row] for row in rows]


def random_point_ops(rng, n_add, n_mul):
    """valid and invalid add / mul ops: on-curve multiples of G, infinity, off-curve points (some (x, 0)), coordinates >= p, right
    and wrong outputs"""
    F, P = b.Fq, b.P

    def point():
        t = rng.random()
        if t < 0.6:
            return b.multiply(b.G1, rng.randrange(1, 1 << 20), F)
        if t < 0.7:
            return (0, 0)
        if t < 0.8:
            return (rng.randrange(P), 0)
        if t < 0.9:
            return (rng.randrange(P), rng.randrange(P))
        x, y = b.multiply(b.G1, rng.randrange(1, 1000), F)
        return (x + P, y) if rng.random() < 0.5 else (x, y + P)

    def out_for(res):
        res = (0, 0) if res is None else res
        t = rng.random()
        return res if t < 0.6 else ((res[0] + 1) % P, res[1]) if t < 0.8 else (rng.randrange(1 << 256), res[1])

    def g1(p):
        return b._g1(p[0] % P, p[1] % P)

    adds = []
    for _ in range(n_add):
        p, q = point(), point()
        adds.append((p, q, out_for(b.add(g1(p), g1(q), F))))
    muls = []
    for _ in range(n_mul):
        p = point()
        s = rng.choice([rng.randrange(1 << 256), rng.randrange(b.R), rng.randrange(16), b.R, P - 1 + rng.randrange(3)])
        muls.append((p, s, out_for(b.multiply(g1(p), s % P, F))))
    return adds, muls


def ops_from_table_rows(rows):
    """EccTableRows (uint64[m, 13, 4]) of ecAdd / ecMul -> (add_ops, mul_ops) whose chips are the rows' own words"""
    adds, muls = [], []
    for r in rows_to_ints(rows):
        # (a fixture's cell may exceed 128 bits: the op's word is then whatever the row's limbs make mod 2^256, and the row fails
        # its copy constraint as it would against any op)
        px, py, qx, qy = ((r[c] + (r[c + 1] << 128)) % (1 << 256) for c in (1, 3, 5, 7))
        if r[0] == 1:
            adds.append(((px, py), (qx, qy), (r[10], r[11])))
        elif r[0] == 2:
            muls.append(((px, py), qx, (r[10], r[11])))
    return adds, muls


def rng(seed):
    return random.Random(seed)
