"""Known-answer checks of the BN254 device arithmetic (csrc/bn254_fq.hpp through the zk_fr_op hooks 18..25) against the plain-Python
model tests/bn254_ref.py.  Each check takes the library to run on, so test_ecc_kat_cpu.py (libzkevm_cpu.so) and
test_ecc_kat_gpu.py (the HIP library) run the same cases."""
import math

from tests import bn254_ref as b
from tests.ecc_cases import (FINAL_EXP_M, f12_easy, f12_final_exp, f12_frob, f12_inv, fr_op, g2_words, order3_point, rng,
                             tower_to_w, w_to_tower, zero_y_chain_point)

P, R = b.P, b.R


def fq_operands():
    """(a, c) pairs: random residues, random raw words (some in [5p, 2^256)), and every pair of an edge set"""
    g = rng(18)
    edges = [0, 1, 2, P - 1, P, P + 1, 2 * P - 1, 5 * P, 5 * P + 1, (1 << 256) - 1, (P - 1) // 2, (1 << 256) % P, (1 << 512) % P]
    for k in range(32, 256, 32):
        edges += [1 << k, (1 << k) - 1]
    a = [g.randrange(P) for _ in range(8000)] + [g.randrange(1 << 256) for _ in range(8000)] + [g.randrange(5 * P, 1 << 256) for _ in range(4000)]
    c = [g.randrange(P) for _ in range(8000)] + [g.randrange(1 << 256) for _ in range(8000)] + [g.randrange(1 << 256) for _ in range(4000)]
    for x in edges:
        for y in edges:
            a.append(x)
            c.append(y)
    return a, c


def check_fq_mul(lib):
    a, c = fq_operands()
    assert len(a) >= 20000 and sum(1 for x in a if x >= 5 * P) >= 4000
    assert fr_op(lib, 18, a, c) == [(x % P) * (y % P) % P for x, y in zip(a, c)]


def fq12_elements(n_random=1700):
    """elements of the model's Fq12 (w-basis): random, one nonzero Fq2 coefficient, the 0/3/4 shape of a line, coefficients p - 1,
    0 and 1, and members of the cyclotomic subgroup"""
    g = rng(12)
    out = [[0] * 12, list(b.ONE12)]
    out += [[g.randrange(P) for _ in range(12)] for _ in range(n_random)]
    for k in range(6):
        for _ in range(24):
            t = [0] * 12
            t[2 * k], t[2 * k + 1] = g.choice([0, 1, P - 1, g.randrange(P)]), g.randrange(P)
            out.append(tower_to_w(t))
    for _ in range(128):
        t = [0] * 12
        for k in (0, 3, 4):
            t[2 * k], t[2 * k + 1] = g.randrange(P), g.randrange(P)
        out.append(tower_to_w(t))
    out.append(tower_to_w([P - 1] * 12))
    for _ in range(63):
        out.append(tower_to_w([g.choice([0, 1, P - 1, P - 2, g.randrange(P)]) for _ in range(12)]))
    out += [f12_easy([g.randrange(P) for _ in range(12)]) for _ in range(64)]
    return out


def _flat(elems):
    return [v for e in elems for v in w_to_tower(e)]


def _unflat(vals):
    return [tower_to_w(vals[12 * i:12 * i + 12]) for i in range(len(vals) // 12)]


def check_fq12_ops(lib):
    xs = fq12_elements()
    assert len(xs) >= 2048
    ys = list(reversed(xs))
    fx, fy = _flat(xs), _flat(ys)
    assert _unflat(fr_op(lib, 19, fx, fy)) == [b.f12_mul(x, y) for x, y in zip(xs, ys)]
    assert _unflat(fr_op(lib, 20, fx)) == [b.f12_mul(x, x) for x in xs]
    inv = _unflat(fr_op(lib, 21, fx))
    for x, v in zip(xs, inv):
        assert (v == [0] * 12) if x == [0] * 12 else b.f12_mul(x, v) == b.ONE12
    frob = _unflat(fr_op(lib, 22, fx))
    assert frob == [f12_frob(x) for x in xs]
    for x, v in list(zip(xs, frob))[:8]:  # the Frobenius map of the check itself, against the model's power
        assert v == b.f12_pow(x, P)


def check_final_exp(lib):
    """op 23 is f^((p^12 - 1) / r * m) for the one pinned m"""
    assert math.gcd(FINAL_EXP_M, R) == 1
    xs = fq12_elements(16)
    xs = xs[:18] + xs[18::24][:14]
    got = _unflat(fr_op(lib, 23, _flat(xs)))
    assert got[:2] == [[0] * 12, list(b.ONE12)]
    assert got == [f12_final_exp(x) for x in xs]
    assert got[2] == b.f12_pow(xs[2], b.FINAL_EXP * FINAL_EXP_M)  # the exponent of the check, unsplit


def _g2_mul(q, n):
    return b.multiply(q, n, b.Fq2)


def check_pairing(lib):
    """op 24: e(aG1, bG2) as the exact value e(G1, G2)^(ab m), full-width a and b, small and r - 1 scalars, P negated"""
    g = rng(24)
    A = [g.randrange(1, R) for _ in range(16)]
    B = [g.randrange(1, R) for _ in range(16)]
    pa = {a: b.multiply(b.G1, a, b.Fq) for a in A + [1, 2, R - 1]}
    qb = {c: _g2_mul(b.G2, c) for c in B + [1, 2, R - 1]}
    cases = [(a, c, False) for a in A for c in B] + [(a, c, False) for a in (1, 2, R - 1) for c in (1, 2, R - 1)]
    cases += [(A[i], B[i], True) for i in range(8)]
    words = []
    for a, c, negate in cases:
        p = b.neg(pa[a], b.Fq) if negate else pa[a]
        words += list(p) + list(g2_words(qb[c])) + [0] * 6
    got = _unflat(fr_op(lib, 24, words))
    assert len(set(tuple(map(tuple, [pa[a], qb[c]])) for a, c, _ in cases)) >= 256
    e = b.pairing(b.G2, b.G1)
    em = b.f12_pow(e, FINAL_EXP_M)
    for (a, c, negate), v in zip(cases, got):
        assert v == b.f12_pow(em, (-a if negate else a) * c % R), (a, c, negate)
        assert v != b.ONE12
    for (a, c, negate), v in list(zip(cases, got))[:: len(cases) // 8][:8]:  # the model's own pairing, directly
        p = b.neg(pa[a], b.Fq) if negate else pa[a]
        assert v == b.f12_pow(b.pairing(qb[c], p), FINAL_EXP_M)
    for v in got[::9]:
        assert b.f12_pow(v, R) == b.ONE12


def g2_chain_points():
    """twist-field points whose py_ecc chain leaves the group law: (x, 0) (y = 0 at once), (0, y) (order 3 on its curve), and
    points first reaching y = 0 after one doubling; plus G2 and a point of the twist outside G2"""
    g = rng(25)
    pts = [((g.randrange(P), g.randrange(P)), (0, 0)) for _ in range(2)]
    pts += [order3_point(b.Fq2, g) for _ in range(2)]
    pts += [zero_y_chain_point(b.Fq2, 1, g) for _ in range(3)]
    return pts


def chain_scalars(j, g):
    ss = list(range(0, 1 << (j + 3)))
    for bits in (max(j - 1, 1), j + 1, j + 2, 254):
        ss.append(g.randrange(1 << (bits - 1), 1 << bits))
    ss += [R, R - 1, R + 1, P - 1, P, P + 3, (1 << 256) - 1, g.randrange(P, 1 << 256), g.randrange(1 << 256)]
    return ss


def check_g2_chain(lib):
    """op 25 against py_ecc's multiply over Fq2 (the chain of the circuit's G2 subgroup check)"""
    g = rng(26)
    words, exp = [], []
    for q in g2_chain_points() + [b.G2]:
        j = 0
        t = q
        while j < 4 and t[1] != (0, 0):
            t, j = b.double(t, b.Fq2), j + 1
        for n in chain_scalars(j, g):
            words += list(g2_words(q)) + [n] + [0] * 7
            r = _g2_mul(q, n)
            exp.append([0, 0, 0, 0, 1] if r is None else [r[0][0], r[0][1], r[1][0], r[1][1], 0])
    got = fr_op(lib, 25, words)
    assert [got[12 * i:12 * i + 5] for i in range(len(exp))] == exp
    assert not any(any(got[12 * i + 5:12 * i + 12]) for i in range(len(exp)))
