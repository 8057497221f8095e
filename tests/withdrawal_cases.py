"""Shared helpers of the Withdrawal-circuit tests: the golden cases (tests/golden/withdrawal_cases.npz, tools/gen_golden_withdrawal.py),
random honest witnesses built with the plain-Python model (tests/withdrawal_ref.py), and their wire form."""
import json
import os
import random

import numpy as np

from tests import withdrawal_ref as W

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "withdrawal_cases.npz")


def cells(rows, nc):
    return np.array([[[(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in r] for r in rows], dtype=np.uint64).reshape(
        len(rows), nc, 4)


def ints(a):
    """uint64[n, c, 4] -> list of tuples of ints"""
    return [tuple(sum(int(x[k]) << (64 * k) for k in range(4)) for x in r) for r in np.asarray(a)]


def golden_cases():
    """(meta, wire dict, expected status uint32[n], randomness) of every golden case"""
    z = np.load(GOLDEN)
    meta = json.loads(str(z["meta"]))
    r = int(meta["randomness"], 16)
    for i, m in enumerate(meta["cases"]):
        w = {k: z[f"{i}_{k}"] for k in ("rows", "mpt", "keccak", "block")}
        w.update(max_withdrawals=m["max_withdrawals"], total_rows=m["total_rows"], row_base=0)
        yield m, w, z[f"{i}_status"], r


def honest_witness(n, seed, max_withdrawals=None, r=None, id0=None):
    """a witness withdrawals2witness would build for n random withdrawals (model form): withdrawals, roots, rows, mpt, keccak, block"""
    rng = random.Random(seed)
    m = n if max_withdrawals is None else max_withdrawals
    id0 = rng.randrange(0, 2**64) if id0 is None else id0
    wds = [((id0 + i) % W.P, rng.randrange(0, 2**64), rng.randrange(1, 2**160), rng.randrange(1, 2**64)) for i in range(n)]
    roots = [5 * (i + 1) for i in range(n)]
    rows, krows = W.assign(wds, roots, m, r)
    keccak = set(krows) | {(0, 0, 0, 0, 0)}
    block = [(W.WITHDRAWAL_ROOT_TAG, 0) + W.split(roots[-1] if n else 0)]
    return wds, roots, rows, W.mock_mpt(wds, roots), keccak, block


def wire(rows, mpt, keccak, block, max_withdrawals, total_rows=None):
    return {"rows": cells(rows, 8), "mpt": cells(sorted(set(mpt)), 12), "keccak": cells(sorted(set(keccak)), 5),
            "block": cells(sorted(set(block)), 4), "max_withdrawals": max_withdrawals,
            "total_rows": len(rows) if total_rows is None else total_rows, "row_base": 0}


def withdrawal_inputs(wds, roots):
    """zk_withdrawal_assign's input uint64[n, 5, 4]"""
    return cells([tuple(wd) + (root,) for wd, root in zip(wds, roots)], 5)


def tamper(rows, rng, k):
    """k random cell changes (id / validator / address / amount mod p, hash / root halves below 2^128) -> (rows, touched rows)"""
    t = [list(r) for r in rows]
    for _ in range(k):
        i, f = rng.randrange(len(t)), rng.randrange(8)
        t[i][f] = (t[i][f] + 1 + rng.randrange(1 << 20)) % (W.P if f < 4 else 1 << 128)
    return [tuple(r) for r in t]


def big_witness(n, seed, r, device):
    """an honest witness of n random withdrawals assigned by the backend `device` (zk_withdrawal_assign), its tables built in numpy:
    wire dict (rows, mpt, keccak with the zero row, block), and the assignment's input"""
    from zkevm_specs_amd import oneshot

    rng = np.random.default_rng(seed)
    inp = np.zeros((n, 5, 4), dtype=np.uint64)
    id0 = int(rng.integers(0, 2**62))
    inp[:, 0, 0] = np.arange(id0, id0 + n, dtype=np.uint64)
    inp[:, 1, 0] = rng.integers(0, 2**63, n, dtype=np.uint64)
    inp[:, 2, 0] = rng.integers(1, 2**63, n, dtype=np.uint64)  # 160-bit addresses: two more limbs below
    inp[:, 2, 1] = rng.integers(0, 2**63, n, dtype=np.uint64)
    inp[:, 2, 2] = rng.integers(0, 2**32, n, dtype=np.uint64)
    inp[:, 3, 0] = rng.integers(1, 2**63, n, dtype=np.uint64)
    inp[:, 4, 0] = 5 * np.arange(1, n + 1, dtype=np.uint64)
    rows, krows = oneshot.withdrawal_assign(inp, n, r, device=device)
    mpt = np.zeros((n, 12, 4), dtype=np.uint64)
    mpt[:, 0] = rows[:, 2]
    mpt[:, 1, 0] = 8
    mpt[:, 2, :2] = rows[:, 0, :2]
    mpt[:, 3, :2] = rows[:, 0, 2:]
    mpt[:, 4:6] = rows[:, 6:8]
    mpt[1:, 6:8] = rows[:-1, 6:8]
    mpt[:, 8:10] = rows[:, 4:6]
    keccak = np.concatenate([np.zeros((1, 5, 4), dtype=np.uint64), krows])
    block = np.zeros((1, 4, 4), dtype=np.uint64)
    block[0, 0, 0] = 9
    block[0, 2:4] = rows[-1, 6:8]
    w = {"rows": rows, "mpt": mpt, "keccak": keccak, "block": block, "max_withdrawals": n, "total_rows": n, "row_base": 0}
    return w, inp


def tamper_cells(rows, rng, k):
    """k random cell changes of wire rows uint64[n, 8, 4] (low limb bumped: stays canonical for ids / amounts of 64 bits and for Word
    halves) -> a new array"""
    t = rows.copy()
    n = t.shape[0]
    for _ in range(k):
        i, f = int(rng.integers(0, n)), int(rng.integers(0, 8))
        t[i, f, 0] ^= np.uint64(1 + int(rng.integers(0, 1 << 20)))
    return t
