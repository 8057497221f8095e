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


# ---- Fq12: the device's tower and the model's w-basis -------------------------------------------------------------------
# tower order (c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2) holds the Fq2 coefficients of w^0, w^2, w^4, w^1, w^3, w^5, and
# u = w^6 - 9 (w^6 = xi = 9 + u), so a0 + a1 u at w^e is (a0 - 9 a1) w^e + a1 w^(e + 6)
TOWER_W_POWER = (0, 2, 4, 1, 3, 5)
BN_X = 4965661367192848881
# the device's final exponentiation is f^((p^12 - 1) / r * FINAL_EXP_M): the x-chain of its hard part (Fuentes-Castaneda, Knapp,
# Rodriguez-Henriquez) computes this multiple of (p^4 - p^2 + 1) / r; gcd(FINAL_EXP_M, r) = 1
FINAL_EXP_M = 2 * BN_X * (6 * BN_X * BN_X + 3 * BN_X + 1)


def tower_to_w(x):
    """12 tower-order Fq elements -> the model's 12 coefficients of w^0 .. w^11"""
    P = b.P
    f = [0] * 12
    for k, e in enumerate(TOWER_W_POWER):
        a0, a1 = x[2 * k], x[2 * k + 1]
        f[e] = (f[e] + a0 - 9 * a1) % P
        f[e + 6] = (f[e + 6] + a1) % P
    return f


def w_to_tower(f):
    P = b.P
    x = [0] * 12
    for k, e in enumerate(TOWER_W_POWER):
        x[2 * k], x[2 * k + 1] = (f[e] + 9 * f[e + 6]) % P, f[e + 6] % P
    return x


def fq12_tower_mul(x, y):
    return w_to_tower(b.f12_mul(tower_to_w(x), tower_to_w(y)))


F12_MOD = [82, 0, 0, 0, 0, 0, -18, 0, 0, 0, 0, 0, 1]  # w^12 - 18 w^6 + 82, low to high


def f12_inv(a):
    """a^-1 in the model's Fq12 by the extended Euclidean algorithm on polynomials over Fq (0 -> 0)"""
    P = b.P

    def trim(v):
        v = [c % P for c in v]
        while v and v[-1] == 0:
            v.pop()
        return v

    r0, r1 = trim(F12_MOD), trim(a)
    if not r1:
        return [0] * 12
    s0, s1 = [], [1]
    while len(r1) > 1:
        q = [0] * (len(r0) - len(r1) + 1)
        rem = list(r0)
        li = pow(r1[-1], P - 2, P)
        for d in range(len(rem) - len(r1), -1, -1):
            c = rem[d + len(r1) - 1] * li % P
            q[d] = c
            for i, v in enumerate(r1):
                rem[d + i] = (rem[d + i] - c * v) % P
        prod = [0] * (len(q) + len(s1))
        for i, u in enumerate(q):
            for j, v in enumerate(s1):
                prod[i + j] += u * v
        s_next = trim([(s0[i] if i < len(s0) else 0) - (prod[i] if i < len(prod) else 0) for i in range(max(len(s0), len(prod)))])
        r0, r1, s0, s1 = r1, trim(rem), s1, s_next
    c = pow(r1[0], P - 2, P)
    out = [v * c % P for v in s1] + [0] * 12
    return out[:12]


_FROB = {}


def f12_frob(a, k=1):
    """a^(p^k): linear over Fq, with the powers of w^(p^k) from the model's f12_pow (cached)"""
    if k not in _FROB:
        wp = b.f12_pow([0, 1] + [0] * 10, b.P ** k)
        pw = [b.ONE12]
        for _ in range(11):
            pw.append(b.f12_mul(pw[-1], wp))
        _FROB[k] = pw
    out = [0] * 12
    for c, row in zip(a, _FROB[k]):
        if c:
            out = [(o + c * v) for o, v in zip(out, row)]
    return [o % b.P for o in out]


def f12_easy(f):
    """f^((p^6 - 1)(p^2 + 1)): an element of the cyclotomic subgroup (0 -> 0)"""
    g = b.f12_mul(f12_frob(f, 6), f12_inv(f))
    return b.f12_mul(f12_frob(g, 2), g)


def f12_final_exp(f):
    """the value the device's final exponentiation must give: f^((p^12 - 1) / r * FINAL_EXP_M), the easy part by Frobenius maps"""
    return b.f12_pow(f12_easy(f), (b.P ** 4 - b.P ** 2 + 1) // b.R * FINAL_EXP_M)


# ---- the zk_fr_op known-answer hooks -----------------------------------------------------------------------------------
def words(vals):
    return np.array([[(x >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for x in vals], dtype=np.uint64).reshape(-1, 4)


def fr_op(lib, op, a, c=None):
    """zk_fr_op(op) on the ints a (and c) through `lib` (either backend): the output words as ints"""
    from zkevm_specs_amd import _lib

    xa = words(a)
    xc = words(c) if c is not None else xa
    out = np.zeros_like(xa)
    _lib.check(lib.zk_fr_op(op, _lib.ptr(xa), _lib.ptr(xc), _lib.ptr(out), len(a), 0), f"zk_fr_op {op}", lib)
    return [word(w) for w in out]


def g2_words(q):
    """a twist point ((x.c0, x.c1), (y.c0, y.c1)) or None -> EIP-197 order (x.c1, x.c0, y.c1, y.c0)"""
    return (0, 0, 0, 0) if q is None else (q[0][1], q[0][0], q[1][1], q[1][0])


# ---- off-curve points whose py_ecc chain doubles a point with y = 0 --------------------------------------------------------
def _poly_trim(v, F):
    while v and v[-1] == F.zero:
        v.pop()
    return v


def _poly_divmod(a, m, F):
    """(q, r) of a / m over the field F (polynomials low to high)"""
    a = list(a)
    if len(a) < len(m):
        return [F.zero], a
    li = F.inv(m[-1])
    q = [F.zero] * (len(a) - len(m) + 1)
    for d in range(len(a) - len(m), -1, -1):
        c = F.mul(a[d + len(m) - 1], li)
        q[d] = c
        for i, v in enumerate(m):
            a[d + i] = F.sub(a[d + i], F.mul(c, v))
    return q, _poly_trim(a[:len(m) - 1], F)


def _poly_mul(a, c, F):
    out = [F.zero] * (len(a) + len(c) - 1)
    for i, u in enumerate(a):
        for j, v in enumerate(c):
            out[i + j] = F.add(out[i + j], F.mul(u, v))
    return out


def _poly_powmod(base, e, m, F):
    acc = [F.one]
    while e:
        if e & 1:
            acc = _poly_divmod(_poly_mul(acc, base, F), m, F)[1] or [F.zero]
        base = _poly_divmod(_poly_mul(base, base, F), m, F)[1] or [F.zero]
        e >>= 1
    return acc


def _poly_gcd(a, c, F):
    a, c = _poly_trim(list(a), F), _poly_trim(list(c), F)
    while c:
        a, c = c, _poly_divmod(a, c, F)[1]
    li = F.inv(a[-1])
    return [F.mul(v, li) for v in a]


def _field_order(F):
    return b.P if F is b.Fq else b.P * b.P


def _rand_elem(F, rng):
    return rng.randrange(b.P) if F is b.Fq else (rng.randrange(b.P), rng.randrange(b.P))


def poly_roots(f, F, rng):
    """the roots in F of a squarefree-or-not polynomial f: gcd(X^q - X, f), split by Cantor-Zassenhaus"""
    q = _field_order(F)
    f = _poly_trim(list(f), F)
    xq = _poly_powmod([F.zero, F.one], q, f, F)
    g = _poly_gcd(_poly_sub(xq, [F.zero, F.one], F), f, F)
    out = []

    def split(h):
        if len(h) == 1:
            return
        if len(h) == 2:
            out.append(F.neg(h[0]))
            return
        while True:
            t = _poly_powmod([_rand_elem(F, rng), F.one], (q - 1) // 2, h, F)
            d = _poly_gcd(_poly_sub(t, [F.one], F), h, F)
            if 1 < len(d) < len(h):
                split(d)
                split(_poly_divmod(h, d, F)[0])
                return

    split(g)
    return out


def _poly_sub(a, c, F):
    n = max(len(a), len(c))
    return _poly_trim([F.sub(a[i] if i < len(a) else F.zero, c[i] if i < len(c) else F.zero) for i in range(n)], F)


def field_sqrt(a, F):
    if F is b.Fq:
        y = pow(a, (b.P + 1) // 4, b.P)  # p = 3 mod 4
        return y if y * y % b.P == a else None
    return fq2_sqrt(a)


def fq2_sqrt(a):
    # p = 3 mod 4: Algorithm 9 of Adj and Rodriguez-Henriquez, "Square root computation over even extension fields"
    F, P = b.Fq2, b.P

    def pw(x, e):
        acc = (1, 0)
        while e:
            if e & 1:
                acc = F.mul(acc, x)
            x = F.mul(x, x)
            e >>= 1
        return acc

    a1 = pw(a, (P - 3) // 4)
    alpha = F.mul(a1, F.mul(a1, a))
    x0 = F.mul(a1, a)
    if alpha == (P - 1, 0):
        x = F.mul((0, 1), x0)
    else:
        x = F.mul(pw(F.add((1, 0), alpha), (P - 1) // 2), x0)
    return x if F.mul(x, x) == a else None


def halve(t_pt, bp, F, rng):
    """a point H of y^2 = x^3 + bp with py_ecc's double(H) == t_pt, or None: x(2H) = x_T is the quartic
    x^4 - 4 x_T x^3 - 8 bp x - 4 x_T bp = 0, and y = sqrt(x^3 + bp)"""
    xt = t_pt[0]
    four = F.small(4)
    quartic = [F.neg(F.mul(four, F.mul(xt, bp))), F.neg(F.mul(F.small(8), bp)), F.zero, F.neg(F.mul(four, xt)), F.one]
    for x in poly_roots(quartic, F, rng):
        y = field_sqrt(F.add(F.mul(F.mul(x, x), x), bp), F)
        if y is None or y == F.zero:
            continue
        for h in ((x, y), (x, F.neg(y))):
            if b.double(h, F) == t_pt:
                return h
    return None


def zero_y_depth(pt, F, limit=8):
    """the first k with double^k(pt) having y = 0 (py_ecc's chain), or None"""
    for k in range(limit + 1):
        if pt[1] == F.zero:
            return k
        pt = b.double(pt, F)
    return None


def zero_y_chain_point(F, depth, rng):
    """an off-curve point whose affine doubling chain first reaches y = 0 at P_depth: (t, 0) lies on y^2 = x^3 - t^3, halved depth
    times on that curve (a fresh t when a halving does not exist).  Over Fq only depth 0 exists: the halving quartic of (t, 0) is
    (x^2 - 2 t x - 2 t^2)^2, whose roots t (1 +- sqrt 3) are not in Fq (3 is a non-residue mod p), so no curve y^2 = x^3 + b' over Fq
    has a point of order 4 and py_ecc's G1 chain can meet y = 0 only at its first point."""
    assert depth == 0 or F is b.Fq2
    while True:
        t = _rand_elem(F, rng)
        bp = F.neg(F.mul(F.mul(t, t), t))
        pt = (t, F.zero)
        for _ in range(depth):
            pt = halve(pt, bp, F, rng)
            if pt is None:
                break
        if pt is not None and not b.is_on_curve(pt, F, b.B1 if F is b.Fq else b.B2):
            assert zero_y_depth(pt, F) == depth
            return pt


def order3_point(F, rng):
    """(0, y): order 3 on y^2 = x^3 + y^2 (it doubles to (0, -y)); off the curve / twist for a random y"""
    return (F.zero, _rand_elem(F, rng))
