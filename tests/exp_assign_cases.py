"""The golden cases of tools/gen_golden_exp_assign.py (tests/golden/exp_assign_cases.npz), seeded random EXP events and an independent
model of the Exp circuit's witness: every row from Python's own pow(base, e, 2**256), no square-and-multiply recursion."""
import json
import os
import random

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exp_assign_cases.npz")
POW2 = 1 << 256
M128 = (1 << 128) - 1
FR_P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
DUMMY_ROW = (1, 0, 0, 0, 1, 1, 1, 1, 1, 0, 1, 0, 1)
DUMMY_TABLE_ROW = (1, 0, 0, 1, 0, 0, 0, 1, 0, 1, 0)


def golden_cases():
    """-> list of dicts: name, max_exp_steps, calls ("fill" or (base, exponent, identifier)), exc (class name or "", call index),
    rows uint64[21, n, 4] and table (sorted, uint64[m, 11, 4]) where nothing raised"""
    g = np.load(GOLDEN)
    out = []
    for ci, name in enumerate(g["names"].tolist()):
        calls = [c if c == "fill" else tuple(int(v) for v in c) for c in json.loads(str(g[f"c{ci}_calls"]))]
        exc, at = g[f"c{ci}_exc"].tolist()
        c = {"name": name, "max_exp_steps": int(g[f"c{ci}_max"][0]), "calls": calls, "exc": (exc, int(at)), "rows": None, "table": None}
        if not exc:
            c["rows"], c["table"] = g[f"c{ci}_rows"], g[f"c{ci}_table"]
        out.append(c)
    return out


def events_of(calls):
    """the (identifier, base, exponent) of a case's add_event calls, identifier reduced as FQ() does"""
    return [(i % FR_P, b, e) for (b, e, i) in (c for c in calls if c != "fill")]


def cells(values):
    raw = b"".join(int(v).to_bytes(32, "little") for v in values)
    return np.frombuffer(raw, dtype="<u8").reshape(len(values), 4).copy()


def events_wire(events):
    """[(identifier, base, exponent)] -> uint64[n, 5, 4]"""
    flat = [v for (i, b, e) in events for v in (i, b & M128, b >> 128, e & M128, e >> 128)]
    return cells(flat).reshape(len(events), 5, 4)


def model(events, max_exp_steps):
    """-> (rows as 13-tuples of ints in ExpCircuitRow order, table rows as 11-tuples in first-seen order)"""
    rows, table = [], []
    for ident, base, exponent in events:
        chain, e = [], exponent
        while e > 1:
            chain.append(e)
            e = e // 2 if e % 2 == 0 else e - 1
        for k, e in enumerate(chain):
            d = pow(base, e, POW2)
            a, b = (pow(base, e // 2, POW2),) * 2 if e % 2 == 0 else (pow(base, e - 1, POW2), base)
            assert a * b % POW2 == d
            last = int(k == len(chain) - 1)
            rows.append((1, 1, ident, last, base, e, d, a, b, 0, d, e // 2, e % 2))
            table.append((1, ident, last) + tuple((base >> (64 * q)) & (2**64 - 1) for q in range(4)) + (e & M128, e >> 128, d & M128, d >> 128))
    if len(rows) < 7 * max_exp_steps:
        table.append(DUMMY_TABLE_ROW)
        rows += [DUMMY_ROW] * (7 * max_exp_steps - len(rows))
    return rows, table


def rows_wire(rows):
    """13-tuples -> uint64[21, n, 4]"""
    flat = []
    for r in rows:
        flat += list(r[:4])
        for w in r[4:12]:
            flat += [w & M128, w >> 128]
        flat.append(r[12])
    return np.ascontiguousarray(cells(flat).reshape(len(rows), 21, 4).transpose(1, 0, 2))


def table_wire(table):
    return cells([v for t in table for v in t]).reshape(len(table), 11, 4)


def sorted_table(table):
    """uint64[m, 11, 4] -> the sorted list of int tuples (the set the reference builds)"""
    t = np.asarray(table)
    ints = [[int(c[0]) | int(c[1]) << 64 | int(c[2]) << 128 | int(c[3]) << 192 for c in row] for row in t]
    return sorted(tuple(r) for r in ints)


def random_events(rng, n, max_bits=256, empty_share=0.0):
    """n events with strictly increasing identifiers, exponents of up to max_bits bits, `empty_share` of them 0 or 1"""
    out, ident = [], 0
    for _ in range(n):
        ident += rng.randrange(1, 1000)
        e = rng.randrange(2) if rng.random() < empty_share else rng.getrandbits(rng.randrange(2, max_bits + 1)) | 2
        b = rng.choice([rng.getrandbits(256), rng.getrandbits(256), rng.getrandbits(64), rng.getrandbits(256) << rng.randrange(200) & (POW2 - 1)])
        out.append((ident, b, e))
    return out


def random_events_wire(seed, n, max_bits):
    """a large seeded event array without Python big-int loops: identifiers 3, 6, 9, ..., random 256-bit bases, exponents below 2^max_bits"""
    rng = np.random.default_rng(seed)
    ev = np.zeros((n, 5, 4), dtype=np.uint64)
    ev[:, 0, 0] = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(3)
    ev[:, 1:5, 0:2] = rng.integers(0, 2**64, size=(n, 4, 2), dtype=np.uint64)
    if max_bits <= 64:
        ev[:, 3, 1] = 0
        ev[:, 4] = 0
        ev[:, 3, 0] &= np.uint64((1 << max_bits) - 1)
    return ev
