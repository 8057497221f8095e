"""Plain-Python model of zk_ecc_from_calls (include/zkevm_hip.h "ECC precompile calls"), written from the reference's statements over
tests/bn254_ref.py: is_valid as EccCircuitRow.assign_add / assign_mul / assign_pairing compute it (ecc_circuit.py:49-232), the
precompile's result for a valid call per EIP-196 / EIP-197 and zero for an invalid one (ecadd.py:29-35, ecpairing.py:34-61), the rows
through bn254_ref.assign_rows (circuit2rows), the EVM circuit's table as a set in first-occurrence order and the aux rows in
flatten_step_aux's layout.  Test infrastructure only: nothing in the package imports it.

Calls: adds [(p, q)], muls [(p, s)], pairings [(g1_pts, g2_pts)] with G2 tuples in EIP-197 order (x.c1, x.c0, y.c1, y.c0).
Results are memoised per distinct call: the directed batches repeat a small set of calls."""
import functools

import numpy as np

from tests import bn254_ref as b

P, R, FR = b.P, b.R, b.FR
M128 = (1 << 128) - 1


def _valid_g1(pt):
    return pt[0] < P and pt[1] < P and b.is_on_curve(b._g1(*pt), b.Fq, b.B1)


@functools.lru_cache(maxsize=None)
def add_result(p, q):
    """(is_valid, out) of ecAdd(p, q)"""
    if not (_valid_g1(p) and _valid_g1(q)):
        return False, (0, 0)
    return True, b.add(b._g1(*p), b._g1(*q), b.Fq) or (0, 0)


@functools.lru_cache(maxsize=None)
def mul_result(p, s):
    """(is_valid, out) of ecMul(p, s): the group has order R, so [s]P = [s mod R]P for the full 256-bit s"""
    if not _valid_g1(p):
        return False, (0, 0)
    return True, b.multiply(b._g1(*p), s % R, b.Fq) or (0, 0)


@functools.lru_cache(maxsize=None)
def _pair_valid(g1, g2):
    """assign_pairing's per-pair validity; the points (None = infinity) when valid"""
    if not all(c < P for c in g1 + g2):
        return False, None, None
    p, q = b._g1(*g1), b._g2(g2)
    ok = (b.is_on_curve(p, b.Fq, b.B1) and b.is_on_curve(q, b.Fq2, b.B2) and b.multiply(p, R, b.Fq) is None
          and b.multiply(q, R, b.Fq2) is None)
    return ok, p, q


@functools.lru_cache(maxsize=None)
def pairing_result(g1s, g2s):
    """(is_valid, out) of ecPairing over the pairs: 1 when the product of the pairings is one (the empty product included)"""
    pts = []
    for g1, g2 in zip(g1s, g2s):
        ok, p, q = _pair_valid(tuple(g1), tuple(g2))
        if not ok:
            return False, 0
        pts.append((p, q))
    return True, int(b.pairing_product_is_one(pts))


def _tup(pairing):
    return tuple(tuple(g) for g in pairing[0]), tuple(tuple(g) for g in pairing[1])


def cells(rows, width):
    """rows of ints -> uint64[n, width, 4]"""
    out = np.zeros((len(rows), width, 4), dtype=np.uint64)
    for i, row in enumerate(rows):
        for c, v in enumerate(row):
            for k in range(4):
                out[i, c, k] = (v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF
    return out


@functools.lru_cache(maxsize=None)
def _row(kind, call, r):
    """circuit2rows' row of one call with its result filled in (bn254_ref.assign_rows), and the op"""
    if kind == 1:
        op = (call[0], call[1], add_result(*call)[1])
        return b.assign_rows([op], [], [], r)[0], op
    if kind == 2:
        op = (call[0], call[1], mul_result(*call)[1])
        return b.assign_rows([], [op], [], r)[0], op
    op = (list(call[0]), list(call[1]), pairing_result(*call)[1])
    return b.assign_rows([], [], [op], r)[0], op


def model(adds, muls, pairings, r):
    """-> dict of the six outputs as arrays (ecc_table cut to its rows) plus `ops`: (add_ops, mul_ops, pairing_ops) with out filled"""
    calls = [(1, (tuple(p), tuple(q))) for p, q in adds] + [(2, (tuple(p), s)) for p, s in muls] + [(3, _tup(pr)) for pr in pairings]
    rows, ops, valid = [], ([], [], []), []
    for kind, call in calls:
        row, op = _row(kind, call, r)
        rows.append(row)
        ops[kind - 1].append(op)
        valid.append((add_result, mul_result, pairing_result)[kind - 1](*call)[0])
    add_ops, mul_ops, pair_ops = ops
    assert [row[12] for row in rows] == [int(v) for v in valid], "assign_rows' is_valid and the call's own disagree"
    table, seen = [], set()
    for row in rows:
        t = tuple(row[:10]) + (row[10] % FR, row[11] % FR, row[12])
        if t not in seen:
            seen.add(t)
            table.append(list(t))
    aux, kinds = [], []
    for p, q, o in add_ops:
        aux.append([v for w in (p[0], p[1], q[0], q[1]) for v in (w & M128, w >> 128)] + [o[0] % FR, o[1] % FR])
        kinds.append(6)
    for p, s, o in mul_ops:
        aux.append([v for w in (p[0], p[1], s) for v in (w & M128, w >> 128)] + [o[0] % FR, o[1] % FR])
        kinds.append(7)
    for (g1s, g2s, o), row in zip(pair_ops, rows[len(add_ops) + len(mul_ops):]):
        aux.append([row[9], len(list(zip(g1s, g2s))), row[12], o])
        kinds.append(8)
    points = b.point_ops(add_ops, mul_ops)
    return {"points": cells(points, 6), "pair_out": cells([[o] for _, _, o in pair_ops], 1).reshape(len(pair_ops), 4),
            "rows": cells(rows, 13), "ecc_table": cells(table, 13), "aux": cells(aux, 12), "aux_kind": np.array(kinds, dtype=np.uint32),
            "ops": (add_ops, mul_ops, pair_ops)}


OUTPUTS = ("points", "pair_out", "rows", "ecc_table", "aux", "aux_kind")


def assert_equal(got, want, what=""):
    """all six outputs and both counts (the calls and the table's rows), bit for bit"""
    for k in OUTPUTS:
        g, w = np.asarray(got[k]), want[k]
        assert g.shape == w.shape, f"{what}: {k} has shape {g.shape}, expected {w.shape}"
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)[0]
            raise AssertionError(f"{what}: {k} differs first at {tuple(bad)}: got {g[tuple(bad)]:#x}, expected {w[tuple(bad)]:#x}")
