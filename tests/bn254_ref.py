"""Plain-Python BN254 (alt_bn128) model for the ECC circuit tests, written from the curve's definition (EIP-196 / EIP-197) and
from py_ecc's published affine formulas (bn128_curve.py: double / add / multiply, inverse(0) = 0), which the reference's
ecc_circuit.py computes with also for points that are off the curve.  Test infrastructure only: nothing in the package imports it.

* Fq = Z / p, Fq2 = Fq[u] / (u^2 + 1) as (c0, c1) tuples, Fq12 = Fq[w] / (w^12 - 18 w^6 + 82) as 12-coefficient lists (py_ecc's
  representation: u = w^6 - 9).  The pairing is the ate pairing of py_ecc's bn128_pairing (Miller loop over 6x + 2 on the
  untwisted points, lines evaluated from the twist, then f^((p^12 - 1) / r)).
* `assign_rows` / `verify_status`: the ECC circuit's circuit2rows + EccCircuitRow.verify (ecc_circuit.py:35-433) on the wire
  layout of include/zkevm_hip.h (zk_ecc_ops), status codes as csrc/ecc_circuit.hpp numbers the checks.
"""
P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617  # curve order
FR = R  # the circuit's cells live in the scalar field
ATE_LOOP_COUNT = 29793968203157093288
LOG_ATE_LOOP_COUNT = 63
G1 = (1, 2)
G2 = ((10857046999023057135944570762232829481370756359578518086990519993285655852781,
       11559732032986387107991004021392285783925812861821192530917403151452391805634),
      (8495653923123431417604973247489272438418190587263600148770280649306958101930,
       4082367875863433681332203403145435568316851327593401208105741076214120093531))


def inv(a):
    return pow(a, P - 2, P)  # 0 -> 0, as py_ecc's prime_field_inv


class Fq:
    """Field ops over Z / p (elements are ints)."""
    zero = 0
    one = 1

    @staticmethod
    def add(a, b): return (a + b) % P
    @staticmethod
    def sub(a, b): return (a - b) % P
    @staticmethod
    def mul(a, b): return a * b % P
    @staticmethod
    def neg(a): return -a % P
    @staticmethod
    def inv(a): return inv(a)
    @staticmethod
    def small(k): return k % P


class Fq2:
    """Field ops over Fq[u] / (u^2 + 1) (elements are (c0, c1))."""
    zero = (0, 0)
    one = (1, 0)

    @staticmethod
    def add(a, b): return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)
    @staticmethod
    def sub(a, b): return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)
    @staticmethod
    def mul(a, b): return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)
    @staticmethod
    def neg(a): return (-a[0] % P, -a[1] % P)
    @staticmethod
    def inv(a):
        d = inv((a[0] * a[0] + a[1] * a[1]) % P)
        return (a[0] * d % P, -a[1] * d % P)
    @staticmethod
    def small(k): return (k % P, 0)


B1 = 3
B2 = Fq2.mul((3, 0), Fq2.inv((9, 1)))


# ---- py_ecc's affine chains (None = infinity) -------------------------------------------------------------------------
def is_on_curve(pt, F, b):
    if pt is None:
        return True
    x, y = pt
    return F.sub(F.mul(y, y), F.mul(F.mul(x, x), x)) == b


def double(pt, F):
    if pt is None:
        return pt
    x, y = pt
    m = F.mul(F.mul(F.small(3), F.mul(x, x)), F.inv(F.mul(F.small(2), y)))
    nx = F.sub(F.mul(m, m), F.mul(F.small(2), x))
    ny = F.sub(F.add(F.mul(F.neg(m), nx), F.mul(m, x)), y)
    return (nx, ny)


def add(p1, p2, F):
    if p1 is None or p2 is None:
        return p1 if p2 is None else p2
    x1, y1 = p1
    x2, y2 = p2
    if x2 == x1 and y2 == y1:
        return double(p1, F)
    if x2 == x1:
        return None
    m = F.mul(F.sub(y2, y1), F.inv(F.sub(x2, x1)))
    nx = F.sub(F.sub(F.mul(m, m), x1), x2)
    ny = F.sub(F.add(F.mul(F.neg(m), nx), F.mul(m, x1)), y1)
    return (nx, ny)


def multiply(pt, n, F):
    if n == 0:
        return None
    if n == 1:
        return pt
    if not n % 2:
        return multiply(double(pt, F), n // 2, F)
    return add(multiply(double(pt, F), n // 2, F), pt, F)


def neg(pt, F):
    return None if pt is None else (pt[0], F.neg(pt[1]))


# ---- Fq12 and the pairing (py_ecc's bn128_pairing, from its definition) ------------------------------------------------


def f12_mul(a, b):
    t = [0] * 23
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                t[i + j] += x * y
    for k in range(22, 11, -1):
        c = t[k]
        if c:
            t[k] = 0
            t[k - 6] += 18 * c
            t[k - 12] -= 82 * c
    return [x % P for x in t[:12]]


ONE12 = [1] + [0] * 11


def f12_pow(a, e):
    acc, base = ONE12, a
    while e:
        if e & 1:
            acc = f12_mul(acc, base)
        base = f12_mul(base, base)
        e >>= 1
    return acc


XI = (9, 1)


def fq2_to_12(a):  # a0 + a1 u = (a0 - 9 a1) + a1 w^6
    out = [0] * 12
    out[0] = (a[0] - 9 * a[1]) % P
    out[6] = a[1] % P
    return out


def _fq2_pow(a, e):
    acc = (1, 0)
    while e:
        if e & 1:
            acc = Fq2.mul(acc, a)
        a = Fq2.mul(a, a)
        e >>= 1
    return acc


FROB_X = _fq2_pow(XI, (P - 1) // 3)  # w^(2(p - 1)) = xi^((p - 1) / 3)
FROB_Y = _fq2_pow(XI, (P - 1) // 2)  # w^(3(p - 1)) = xi^((p - 1) / 2)


def twist_frob(q):  # the p-power Frobenius of the untwisted point, expressed on the twist again
    (x, y) = q
    return (Fq2.mul((x[0], -x[1] % P), FROB_X), Fq2.mul((y[0], -y[1] % P), FROB_Y))


def linefunc(r1, r2, p):
    """py_ecc's linefunc(R1, R2, P) for R1, R2 untwisted from the twist ((x, y) -> (x w^2, y w^3)): every slope is m' w with m' the
    slope on the twist, so the line is evaluated without an Fq12 inversion."""
    (x1, y1), (x2, y2) = r1, r2
    xt, yt = p
    if x1 != x2:
        m = Fq2.mul(Fq2.sub(y2, y1), Fq2.inv(Fq2.sub(x2, x1)))
    elif y1 == y2:
        m = Fq2.mul(Fq2.mul((3, 0), Fq2.mul(x1, x1)), Fq2.inv(Fq2.mul((2, 0), y1)))
    else:  # vertical: xt - x1 w^2
        v = [0] * 12
        v[0] = xt
        return [(a - b) % P for a, b in zip(v, f12_mul(fq2_to_12(x1), W2))]
    # m w (xt - x1 w^2) - (yt - y1 w^3)
    mw = f12_mul(fq2_to_12(m), W1)
    t = [0] * 12
    t[0] = xt
    t = [(a - b) % P for a, b in zip(t, f12_mul(fq2_to_12(x1), W2))]
    u = [0] * 12
    u[0] = yt
    u = [(a - b) % P for a, b in zip(u, f12_mul(fq2_to_12(y1), W3))]
    return [(a - b) % P for a, b in zip(f12_mul(mw, t), u)]


W1 = [0, 1] + [0] * 10
W2 = [0, 0, 1] + [0] * 9
W3 = [0, 0, 0, 1] + [0] * 8


def miller_loop(q, p):
    """py_ecc's miller_loop(twist(Q), P) for Q on the twist and P in G1 (both finite), without the final exponentiation."""
    r_pt, f = q, ONE12
    for i in range(LOG_ATE_LOOP_COUNT, -1, -1):
        f = f12_mul(f12_mul(f, f), linefunc(r_pt, r_pt, p))
        r_pt = double(r_pt, Fq2)
        if ATE_LOOP_COUNT & (2 ** i):
            f = f12_mul(f, linefunc(r_pt, q, p))
            r_pt = add(r_pt, q, Fq2)
    q1 = twist_frob(q)
    nq2 = neg(twist_frob(q1), Fq2)
    f = f12_mul(f, linefunc(r_pt, q1, p))
    r_pt = add(r_pt, q1, Fq2)
    f = f12_mul(f, linefunc(r_pt, nq2, p))
    return f


FINAL_EXP = (P ** 12 - 1) // R


def pairing_product_is_one(pairs):
    """prod e(Q_i, P_i) == 1 for [(P in G1 affine or None, Q in G2 affine over Fq2 or None)], both on their curves."""
    f = ONE12
    for p, q in pairs:
        if p is not None and q is not None:
            f = f12_mul(f, miller_loop(q, p))
    return f12_pow(f, FINAL_EXP) == ONE12


def pairing(q, p):
    return ONE12 if p is None or q is None else f12_pow(miller_loop(q, p), FINAL_EXP)


# ---- the ECC circuit on the wire layout ---------------------------------------------------------------------------------
NCELLS = 13
A = 1 << 24  # AssertionError kind
ATTR = 13 << 24  # AttributeError kind
(OP_TYPE, NO_CHIP, COPY_PX, COPY_PY, COPY_QX, COPY_QY, COPY_OUT_X, COPY_OUT_Y, RLC_ZERO, PAIR_PX_ZERO, PAIR_PY_ZERO, PAIR_QX_ZERO,
 PAIR_QY_ZERO, IS_VALID_BOOL, MAX_ADD, MAX_MUL, MAX_PAIRING, ADD_RESULT, MUL_QY_ZERO, MUL_RESULT, PAIR_OUT_X, PAIR_OUT_Y,
 PAIR_SUBGROUP, PAIR_RLC, PAIR_ON_CURVE, PAIR_RESULT) = range(1, 27)
M128 = (1 << 128) - 1


def _g1(x, y):
    return None if x == 0 and y == 0 else (x % P, y % P)


def _g2(g):  # EIP-197 order (x.c1, x.c0, y.c1, y.c0) -> ((x.c0, x.c1), (y.c0, y.c1)) reduced; all zero -> None
    q = ((g[1] % P, g[0] % P), (g[3] % P, g[2] % P))
    return None if q == ((0, 0), (0, 0)) else q


def _rlc(pairs_words, r):
    acc = 0
    for g1, g2 in pairs_words:
        for v in (g1[0], g1[1], g2[1], g2[0], g2[3], g2[2]):
            for byte in v.to_bytes(32, "little"):
                acc = (acc * r + byte) % FR
    return acc


def point_ops(add_ops, mul_ops):
    """[(p, q, out)] / [(p, s, out)] -> the uniform six-word ops (p.x, p.y, q.x | s, q.y | 0, out.x, out.y)"""
    return [(p[0], p[1], q[0], q[1], o[0], o[1]) for p, q, o in add_ops] + [(p[0], p[1], s, 0, o[0], o[1]) for p, s, o in mul_ops]


def assign_rows(add_ops, mul_ops, pairing_ops, r):
    """circuit2rows: add_ops [(p, q, out)], mul_ops [(p, s, out)], pairing_ops [(g1_pts, g2_pts, out)] -> rows of 13 ints"""
    rows = []
    for k, w in enumerate(point_ops(add_ops, mul_ops)):
        is_add = k < len(add_ops)
        pts = [(w[0], w[1])] + ([(w[2], w[3])] if is_add else [])
        valid = all(c < P for pt in pts for c in pt) and all(is_on_curve(_g1(*pt), Fq, B1) for pt in pts)
        qy = w[3] if is_add else 0
        rows.append([1 if is_add else 2, w[0] & M128, w[0] >> 128, w[1] & M128, w[1] >> 128, w[2] & M128, w[2] >> 128, qy & M128,
                     qy >> 128, 0, w[4] % P, w[5] % P, int(valid)])
    for g1s, g2s, out in pairing_ops:
        valid = True
        pairs = list(zip(g1s, g2s))
        for g1, g2 in pairs:
            pre = all(c < P for c in tuple(g1) + tuple(g2))
            p, q = _g1(*g1), (None if all(c == 0 for c in g2) else _g2(g2))
            ok = (pre and is_on_curve(p, Fq, B1) and is_on_curve(q, Fq2, B2) and multiply(p, R, Fq) is None
                  and multiply(q, R, Fq2) is None)
            valid = valid and ok
        rows.append([3, 0, 0, 0, 0, 0, 0, 0, 0, _rlc(pairs, r), out >> 128, out & M128, int(valid)])
    return rows


def verify_status(add_ops, mul_ops, pairing_ops, rows, r, max_add=1, max_mul=1, max_pairing=1):
    """EccCircuitRow.verify of every row (rows in circuit2rows order, chips from the ops): status code per row."""
    pops = point_ops(add_ops, mul_ops)
    out = []
    for i, row in enumerate(rows):
        out.append(_verify_row(i, row, pops, pairing_ops, r, (max_add, max_mul, max_pairing)))
    return out


def _verify_row(i, row, pops, pairing_ops, r, maxes):
    op = row[0]
    kind = {1: 1, 2: 2, 3: 3}.get(op, 0)
    if not kind:
        return A | OP_TYPE
    if kind != 3:
        if i >= len(pops):
            return ATTR | NO_CHIP
        w = pops[i]
        for c in range(4):
            v = w[c] % P
            if (row[1 + 2 * c], row[2 + 2 * c]) != (v & M128, v >> 128):
                return A | (COPY_PX + c)
        if (w[4] - row[10]) % P:
            return A | COPY_OUT_X
        if (w[5] - row[11]) % P:
            return A | COPY_OUT_Y
        if row[9]:
            return A | RLC_ZERO
    else:
        for c in range(4):
            if row[1 + 2 * c] or row[2 + 2 * c]:
                return A | (PAIR_PX_ZERO + c)
    if row[12] not in (0, 1):
        return A | IS_VALID_BOOL
    if maxes[kind - 1] < 1:
        return A | (MAX_ADD + kind - 1)
    if kind == 1:
        got = add(_g1(w[0] % P, w[1] % P), _g1(w[2] % P, w[3] % P), Fq)
        return A | ADD_RESULT if int(((0, 0) if got is None else got) == (w[4] % P, w[5] % P)) != row[12] else 0
    if kind == 2:
        if row[7] or row[8]:
            return A | MUL_QY_ZERO
        got = multiply(_g1(w[0] % P, w[1] % P), w[2] % P, Fq)
        return A | MUL_RESULT if int(((0, 0) if got is None else got) == (w[4] % P, w[5] % P)) != row[12] else 0
    if row[10]:
        return A | PAIR_OUT_X
    if i < len(pops):
        return ATTR | NO_CHIP
    g1s, g2s, o = pairing_ops[i - len(pops)]
    if row[11] != o & M128:
        return A | PAIR_OUT_Y
    pairs = list(zip(g1s, g2s))
    pts = [(_g1(g1[0] % P, g1[1] % P), _g2(g2)) for g1, g2 in pairs]
    for p, q in pts:
        if not (multiply(p, R, Fq) is None and multiply(q, R, Fq2) is None):
            return A | PAIR_SUBGROUP
    red = [((g1[0] % P, g1[1] % P), tuple(c % P for c in g2)) for g1, g2 in pairs]
    if row[9] != _rlc(red, r):
        return A | PAIR_RLC
    for p, q in pts:
        if not is_on_curve(q, Fq2, B2) or not is_on_curve(p, Fq, B1):
            return A | PAIR_ON_CURVE
    one = pairing_product_is_one(pts)
    return 0 if row[11] == int(one) else A | PAIR_RESULT
