#!/usr/bin/env python3
"""Write tests/golden/ecc_site_cases.npz: a directed failing case per numbered check of csrc/ecc_circuit.hpp (EccSite), laid out on
sheets of 131 add / mul rows and 67 pairing ops (tests/ecc_site_cases.py) so that every site stands on the wavefront and block edges
of each launch form.  Every expected value is the plain-Python model's (tests/bn254_ref.py assign_rows / verify_status): nothing of
the code under test runs here.

* Fault table: FAULTS_POINT / FAULTS_PAIRING below, one entry per (site, variant).  Each is asserted to be the first failure of its
  row by the model; a variant whose expected code is 0 is a clean control.
* Sheets: on the pairing slots sheet s puts PAIRING_SITES[(s + j) mod 15] on slot j; on the point slots each row takes the site
  that still has most of that row's slot classes to stand in, a new variant of the site at every visit, until every (site, slot
  class) of tests/ecc_site_cases.required_cells is covered (17 sheets).  Two more sheets with max_*_ops = 0 carry sites 15, 16 and 17.
  The per-pair sites (23, 25) also place their offending PAIR on pairs 0, 63, 64 and the last one of the points array (filler pair
  counts are bent for that; one entry per site stands on pair 65 as well, lane 64 of a stage 1 that starts at pair 1), first, middle
  and last of a 3-pair op.  Site 20's visits of the mul slots (the first mul, also as row 64 of a 64-add sheet, rows 127, 128, 130)
  take an (x, 0) base with s = r, p - 1 or a 190-bit scalar, so that the aff_mul_slow fallback runs on those lanes.  Variants that no slot took, the clean controls and the
  precedence cases stand on other rows.  Fillers are clean rows from small pools (a few live pairing ops, the rest zero- or
  infinity-pair ops).  main() asserts the coverage and writes it into the file's metadata (site:slot -> sheets).
* Reference outcomes: with --ref-root (a staged reference, as tools/gen_golden_ecc.py takes it) every add / mul site is also built
  as a circuit of at most 3 rows with that one fault and given to the unmodified reference's verify_circuit under oracle/refshim;
  the exception's class name is recorded.  Without it the names already in the output file are kept.  (Pairing rows carry only the
  model's verdict: the shim has no Fq2.)

SEED fixes every choice; the file is written with fixed zip dates and re-creates byte for byte.  Run time: about 1 min 40 s (pure
Python; model verdicts are cached per distinct row).
Run: python tools/gen_golden_ecc_sites.py [--ref-root oracle/_ref]
"""
import argparse
import io
import json
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import bn254_ref as b  # noqa: E402
from tests import ecc_site_cases as sc  # noqa: E402
from tests.ecc_cases import fq2_sqrt, g2_words, order3_point, rng, zero_y_chain_point  # noqa: E402
from zkevm_specs_amd.flatten import flatten_ecc_ops  # noqa: E402

SEED = 20261020
RANDOMNESS = 0x17A0C3B5D2E4F60718293A4B5C6D7E8F9FAEBDCCDBEAF90817263544536271 % b.R
P, R, F, F2 = b.P, b.R, b.Fq, b.Fq2
A, ATTR = b.A, b.ATTR
M128 = (1 << 128) - 1
B64, B128, B192, B200 = 1 << 64, 1 << 128, 1 << 192, 1 << 200
INF1, INF2 = (0, 0), (0, 0, 0, 0)


def pt(x):
    return (0, 0) if x is None else x


# ---- points and clean ops -----------------------------------------------------------------------------------------------------------
G = rng(SEED)
MULT = [b.multiply(b.G1, a, F) for a in (5, 1234567, 0x1F2E3D4C5B6A7988, 77, 3, 9)]
G2W = g2_words(b.G2)
A2 = [g2_words(b.multiply(b.G2, a, F2)) for a in (5, 1234567)]
NG1 = b.neg(b.G1, F)
X0 = zero_y_chain_point(F, 0, G)          # (t, 0): its doubling chain meets y = 0 at once (the aff_mul_slow fallback)
O3 = order3_point(F, G)                    # (0, y): order 3 off the curve
OFF = (2, 3)                               # off the curve, [r]OFF is not None
SCALARS = [7, 0x1F2E3D4C5B6A79887766554433221100FFEEDDCCBBAA99, P - 1, 0x2A3B4C5D6E7F8091A2B3C4D5E6F708192A3B4C5D6E7F809 % R]
ADD_POOL = [(MULT[i], MULT[j], b.add(MULT[i], MULT[j], F)) for i, j in ((0, 1), (1, 2), (2, 3), (3, 0))]
MUL_POOL = [(MULT[i], s, b.multiply(MULT[i], s, F)) for i, s in enumerate(SCALARS)]


def twist_point_outside_g2():
    for i in range(1, 50):
        x = (i, 1)
        y = fq2_sqrt(F2.add(F2.mul(F2.mul(x, x), x), b.B2))
        if y is not None and b.multiply((x, y), R, F2) is not None:
            return g2_words((x, y))
    raise AssertionError("no twist point found")


BAD_Q = twist_point_outside_g2()
OFF_TWIST = g2_words(((1, 0), (2, 0)))    # off the twist with [r]Q = None (the golden corpus's construction)
X0_P = (5, 0)                              # off the curve, y = 0 (trap4_pairing_x0): [r]P is (x, 0), not None
ISO_P = (49 * MULT[0][0] % P, 343 * MULT[0][1] % P)  # (c^2 x, c^3 y), c = 7: off the curve with [r]P = None
assert b.multiply(OFF, R, F) is not None and b.multiply(X0_P, R, F) is not None and b.multiply(b._g2(OFF_TWIST), R, F2) is None
assert b.multiply(ISO_P, R, F) is None and not b.is_on_curve(ISO_P, F, b.B1)
assert not b.is_on_curve(b._g2(OFF_TWIST), F2, b.B2) and b.is_on_curve(b._g2(BAD_Q), F2, b.B2)

PAIR_VALID2 = ([MULT[0], NG1], [G2W, A2[0]], 1)             # e(5 G1, G2) e(-G1, 5 G2) = 1
PAIR_VALID3 = ([MULT[0], INF1, NG1], [G2W, G2W, A2[0]], 1)  # the same around an infinity pair
PAIR_LIVE1 = ([b.G1], [G2W], 0)                             # one live pair, product != 1
PAIR_FILL = {0: ([], [], 1), 1: ([MULT[1]], [INF2], 1), 2: ([MULT[1], INF1], [INF2, A2[1]], 1)}
PAIR_FILL_ALT = {1: ([INF1], [A2[1]], 1)}


def clean(rk, k=0):
    return (ADD_POOL if rk == "add" else MUL_POOL)[k % 4]


# ---- faults: name -> (site code, fn(rk, k) -> (op, tampers) or None); a tamper is (cell, value or fn(old value)) -------------------------
def label(rk):
    return 1 if rk == "add" else 2


def words_of(op, rk):
    return [op[0][0], op[0][1], op[1][0], op[1][1]] if rk == "add" else [op[0][0], op[0][1], op[1], 0]


def with_word(op, rk, c, v):
    """op with coordinate word c (p.x, p.y, q.x | s, q.y) replaced; None where a mul op has no such word"""
    if rk == "add":
        p, q = list(op[0]), list(op[1])
        (p if c < 2 else q)[c % 2] = v
        return (tuple(p), tuple(q), op[2])
    if c == 3:
        return None
    p = list(op[0])
    if c < 2:
        p[c] = v
        return (tuple(p), op[1], op[2])
    return (op[0], v, op[2])


def small_op(rk):
    """a clean op whose coordinate words are all small enough that word + 5p fits 256 bits"""
    two = b.add(b.G1, b.G1, F)
    return (b.G1, b.G1, two) if rk == "add" else (b.G1, 2, two)


def _small_out():
    lim = (1 << 256) - 5 * P - 1
    for k in range(3, 2000):
        o = b.multiply(b.G1, k, F)
        if o[0] < lim and o[1] < lim:
            return k, b.multiply(b.G1, k - 1, F), o
    raise AssertionError("no small multiple found")


SMALL_K, SMALL_PREV, SMALL_OUT = _small_out()


def small_out_op(rk):
    """a clean op whose output coordinates are small enough that out + 5p + 1 fits 256 bits (fq_reduce's fifth subtraction)"""
    return (SMALL_PREV, b.G1, SMALL_OUT) if rk == "add" else (b.G1, SMALL_K, SMALL_OUT)


FAULTS_POINT = {}


def fp(name, site, kind=A):
    def deco(fn):
        FAULTS_POINT[name] = ((kind | site) if site else 0, fn)
        return fn
    return deco


for nm, v in (("zero", lambda rk: 0), ("four", lambda rk: 4), ("limb1", lambda rk: label(rk) + B64), ("limb3", lambda rk: label(rk) + B192)):
    fp(f"1/{nm}", 1)(lambda rk, k, v=v: (clean(rk, k), [(0, v(rk))]))


@fp("2/none_as_pairing", 2, ATTR)
def _(rk, k):  # all-zero words labelled pairing: past the zero-word checks and out_x, then `None.output`
    return ((INF1, INF1, INF1) if rk == "add" else (INF1, 0, INF1)), [(0, 3)]


for c in range(4):
    lo, hi = 1 + 2 * c, 2 + 2 * c
    fp(f"{3 + c}/lo", 3 + c)(lambda rk, k, lo=lo: (clean(rk, k), [(lo, lambda x: x ^ 1)]))
    fp(f"{3 + c}/hi_only", 3 + c)(lambda rk, k, hi=hi: (clean(rk, k), [(hi, lambda x: x ^ 1)]))
    fp(f"{3 + c}/limb2", 3 + c)(lambda rk, k, lo=lo: (clean(rk, k), [(lo, lambda x: x + B128)]))
    fp(f"{3 + c}/limb3", 3 + c)(lambda rk, k, hi=hi: (clean(rk, k), [(hi, lambda x: x + B192)]))
    for kp in range(1, 6):  # the op's coordinate x + k p: the row holds the raw word, the chip the residue
        def shifted(rk, k, c=c, kp=kp):
            op = small_op(rk)
            w = words_of(op, rk)[c] + kp * P
            assert w < 1 << 256
            op = with_word(op, rk, c, w)
            return None if op is None else (op, [])
        fp(f"{3 + c}/plus_{kp}p", 3 + c)(shifted)
    fp(f"{3 + c}/word_max", 3 + c)(lambda rk, k, c=c: (lambda op: None if op is None else (op, []))(with_word(clean(rk, k), rk, c, (1 << 256) - 1)))

for c, site in ((10, 7), (11, 8)):
    fp(f"{site}/off_by_one", site)(lambda rk, k, c=c: (clean(rk, k), [(c, lambda x: x + 1)]))
    fp(f"{site}/cell_plus_p_clean", 0)(lambda rk, k, c=c: (clean(rk, k), [(c, lambda x: x + P)]))

    def out_ge_p(rk, k, c=c, tamper=False):
        op = clean(rk, k)
        out = list(op[2])
        out[c - 10] += P
        return (op[0], op[1], tuple(out)), ([(c, lambda x: x + 1)] if tamper else [])
    fp(f"{site}/op_out_ge_p_clean", 0)(out_ge_p)
    fp(f"{site}/op_out_ge_p_off_by_one", site)(lambda rk, k, f=out_ge_p: f(rk, k, tamper=True))
    fp(f"{site}/cell_plus_5p_off_by_one", site)(lambda rk, k, c=c: (small_out_op(rk), [(c, lambda x: x + 5 * P + 1)]))
    fp(f"{site}/cell_plus_5p_clean", 0)(lambda rk, k, c=c: (small_out_op(rk), [(c, lambda x: x + 5 * P)]))

    def out_plus_5p(rk, k, c=c):
        op = small_out_op(rk)
        out = list(op[2])
        out[c - 10] += 5 * P
        return (op[0], op[1], tuple(out)), []
    fp(f"{site}/op_out_plus_5p_clean", 0)(out_plus_5p)

for nm, v in (("one", 1), ("limb1", B64), ("limb3", B200)):
    fp(f"9/{nm}", 9)(lambda rk, k, v=v: (clean(rk, k), [(9, v)]))
for nm, v in (("two", 2), ("limb1", 1 + B64), ("limb2", B128), ("limb3", 1 + B192)):
    fp(f"14/{nm}", 14)(lambda rk, k, v=v: (clean(rk, k), [(12, v)]))


# the relabelled point rows that reach the pairing-only sites
@fp("10/relabel", 10)
def _(rk, k):
    return clean(rk, k), [(0, 3)]


@fp("11/relabel", 11)
def _(rk, k):
    return ((O3, INF1, O3) if rk == "add" else (O3, 1, O3)), [(0, 3)]


@fp("12/relabel", 12)
def _(rk, k):
    return ((INF1, MULT[0], MULT[0]) if rk == "add" else (INF1, 5, INF1)), [(0, 3)]


@fp("13/relabel", 13)
def _(rk, k):
    return ((INF1, O3, O3), [(0, 3)]) if rk == "add" else None


@fp("21/relabel", 21)
def _(rk, k):  # zero words, a non-zero out_x
    return ((INF1, INF1, (5, 0)) if rk == "add" else (INF1, 0, (5, 0))), [(0, 3)]


# sites 18 / 20: `valid1_wrong` = is_valid 1 with a wrong output, `valid0_right` = is_valid 0 with the right one
def wrong(o):
    return ((o[0] + 1) % P, o[1])


ADD_CASES = {
    "neg": (MULT[0], b.neg(MULT[0], F)), "double": (MULT[1], MULT[1]), "inf_p": (INF1, MULT[2]), "inf_inf": (INF1, INF1),
    "general": (MULT[0], MULT[1]), "x0": (X0, MULT[0]),
}
for nm, (p0, p1) in ADD_CASES.items():
    res = pt(b.add(b._g1(*p0), b._g1(*p1), F))
    on = nm != "x0"  # (the assignment says is_valid = 1 exactly for on-curve inputs)

    def add_case(rk, k, p0=p0, p1=p1, res=res, on=on, right=True, valid=1):
        if rk != "add":
            return None
        t = [] if valid == int(on) else [(12, valid)]
        return (p0, p1, res if right else wrong(res)), t
    fp(f"18/{nm}_valid1_wrong", 18)(lambda rk, k, f=add_case: f(rk, k, right=False, valid=1))
    fp(f"18/{nm}_valid0_right", 18)(lambda rk, k, f=add_case: f(rk, k, right=True, valid=0))
    fp(f"18/{nm}_valid0_wrong_clean", 0)(lambda rk, k, f=add_case: f(rk, k, right=False, valid=0))
    fp(f"18/{nm}_valid1_right_clean", 0)(lambda rk, k, f=add_case: f(rk, k, right=True, valid=1))


@fp("18/relabel_mul", 18)
def _(rk, k):  # a mul op's row labelled add: the chip adds p and (s, 0), the row says is_valid = 1
    return (None if rk == "add" else (clean(rk, k), [(0, 1)]))


MUL_CASES = {"s0": (MULT[0], 0), "s1": (MULT[1], 1), "sr": (MULT[2], R), "sp_minus_1": (MULT[3], P - 1), "sp_plus_7": (MULT[0], P + 7),
             "x0_r": (X0, R), "x0_p_minus_1": (X0, P - 1), "x0_big": (X0, SCALARS[1]), "order3_r": (O3, R), "order3_p_minus_1": (O3, P - 1),
             "order3_r_plus_1": (O3, R + 1)}
MOD_R_DIFFERS = []
for nm, (p0, s) in MUL_CASES.items():
    res = pt(b.multiply(b._g1(*p0), s % P, F))
    on = b.is_on_curve(b._g1(*p0), F, b.B1)
    if s >= R and pt(b.multiply(b._g1(*p0), s % R, F)) != res:
        MOD_R_DIFFERS.append(nm)

    def mul_case(rk, k, p0=p0, s=s, res=res, on=on, right=True, valid=1):
        if rk != "mul":
            return None
        t = [] if valid == int(on) else [(12, valid)]
        if s >= P:  # the row must hold the residue to get past the copy of the scalar
            t += [(5, (s % P) & M128), (6, (s % P) >> 128)]
        return (p0, s, res if right else wrong(res)), t
    fp(f"20/{nm}_valid1_wrong", 20)(lambda rk, k, f=mul_case: f(rk, k, right=False, valid=1))
    fp(f"20/{nm}_valid0_right", 20)(lambda rk, k, f=mul_case: f(rk, k, right=True, valid=0))
    fp(f"20/{nm}_valid1_right_clean", 0)(lambda rk, k, f=mul_case: f(rk, k, right=True, valid=1))
assert len(MOD_R_DIFFERS) >= 4, MOD_R_DIFFERS  # scalars in [r, p) on off-curve bases: [s mod r]P is another point


@fp("20/relabel_add", 20)
def _(rk, k):  # an add op with q = (s, 0) labelled mul: the chip multiplies p by s
    return ((MULT[0], (9, 0), MULT[1]), [(0, 2), (12, 1)]) if rk == "add" else None


for nm, qy in (("lo", 7), ("hi", 3 << 128)):
    fp(f"19/qy_{nm}", 19)(lambda rk, k, qy=qy: ((MULT[0], (5, qy), INF1), [(0, 2)]) if rk == "add" else None)


@fp("15/natural", 15)
def _(rk, k):
    return (clean(rk, k), []) if rk == "add" else None


@fp("15/relabel", 15)
def _(rk, k):
    return (clean(rk, k), [(0, 1)]) if rk == "mul" else None


@fp("16/natural", 16)
def _(rk, k):
    return (clean(rk, k), []) if rk == "mul" else None


# max_*_ops = 0 sheets only: the assert comes before verify_add / verify_mul
fp("15/prec_15+18", 15)(lambda rk, k: ((MULT[0], MULT[1], wrong(ADD_POOL[0][2])), []) if rk == "add" else None)
fp("16/prec_16+20", 16)(lambda rk, k: ((MULT[0], 7, wrong(MUL_POOL[0][2])), []) if rk == "mul" else None)
fp("16/prec_16+19", 16)(lambda rk, k: ((MULT[0], (5, 7), INF1), [(0, 2)]) if rk == "add" else None)


@fp("16/relabel", 16)
def _(rk, k):
    return ((MULT[0], (9, 0), MULT[1]), [(0, 2)]) if rk == "add" else None


# precedence: one row violating two checks adjacent in EccCircuitRow.verify's order; the model reports the earlier
def both(name, first, *tampers, op=None, kinds=("add", "mul")):
    fp(name, first)(lambda rk, k: ((op or clean(rk, k)), list(tampers)) if rk in kinds else None)


inc = lambda x: x + 1  # noqa: E731
both("prec/1+3", 1, (0, 0), (1, inc))
both("prec/3+4", 3, (1, inc), (3, inc))
both("prec/4+5", 4, (3, inc), (5, inc))
both("prec/5+6", 5, (5, inc), (7, inc))
both("prec/6+7", 6, (7, inc), (10, inc))
both("prec/7+8", 7, (10, inc), (11, inc))
both("prec/8+9", 8, (11, inc), (9, 1))
both("prec/9+14", 9, (9, 1), (12, 2))
both("prec/14+18", 14, (12, 2), op=(MULT[0], MULT[1], wrong(ADD_POOL[0][2])), kinds=("add",))
both("prec/14+19", 14, (12, 2), (0, 2), op=(MULT[0], (5, 7), INF1), kinds=("add",))
both("prec/19+20", 19, (0, 2), (12, 1), op=(MULT[0], (5, 7), INF1), kinds=("add",))
both("prec/1+10_point", 1, (0, 3 + B64))

FAULTS_PAIRING = {}


def fq(name, site, kind=A, pair=None):
    def deco(fn):
        FAULTS_PAIRING[name] = ((kind | site) if site else 0, fn, pair)
        return fn
    return deco


def pbase(k):
    return (PAIR_LIVE1, PAIR_VALID3, PAIR_VALID2, PAIR_FILL[1])[k % 4]


fq("1/zero", 1)(lambda k: (pbase(k), [(0, 0)]))
fq("1/limb1", 1)(lambda k: (pbase(k), [(0, 3 + B64)]))
fq("2/pairing_as_add", 2, ATTR)(lambda k: (pbase(k), [(0, 1)]))
fq("2/pairing_as_mul", 2, ATTR)(lambda k: (pbase(k), [(0, 2)]))
for c in range(4):
    fq(f"{10 + c}/lo", 10 + c)(lambda k, c=c: (pbase(k), [(1 + 2 * c, 1)]))
    fq(f"{10 + c}/hi_only", 10 + c)(lambda k, c=c: (pbase(k), [(2 + 2 * c, 1)]))
    fq(f"{10 + c}/limb1", 10 + c)(lambda k, c=c: (pbase(k), [(1 + 2 * c, B64)]))
    fq(f"{10 + c}/limb3", 10 + c)(lambda k, c=c: (pbase(k), [(2 + 2 * c, B200)]))
fq("14/two", 14)(lambda k: (pbase(k), [(12, 2)]))
fq("14/limb1", 14)(lambda k: (pbase(k), [(12, 1 + B64)]))
fq("17/natural", 17)(lambda k: (pbase(k), []))
fq("21/one", 21)(lambda k: (pbase(k), [(10, 1)]))
fq("21/limb1", 21)(lambda k: (pbase(k), [(10, B64)]))
fq("21/op_out_hi", 21)(lambda k: ((PAIR_VALID2[0], PAIR_VALID2[1], B128 + 1), []))
fq("22/cell_flipped", 22)(lambda k: (pbase(k), [(11, lambda x: x ^ 1)]))
fq("22/limb2", 22)(lambda k: (pbase(k), [(11, lambda x: x + B128)]))
fq("22/limb3", 22)(lambda k: (pbase(k), [(11, lambda x: x + B192)]))
# max_pairing_ops = 0 sheets only: the assert comes before verify_pairing's out_x check
fq("17/prec_17+21", 17)(lambda k: (pbase(k), [(10, 1)]))
fq("26/says0_is1", 26)(lambda k: ((PAIR_VALID2[0], PAIR_VALID2[1], 0), []))
fq("26/says1_is0", 26)(lambda k: ((PAIR_LIVE1[0], PAIR_LIVE1[1], 1), []))
fq("26/says0_is1_inf_pair", 26)(lambda k: ((PAIR_VALID3[0], PAIR_VALID3[1], 0), []))
fq("24/off_by_one", 24)(lambda k: (PAIR_VALID3, [(9, lambda x: (x + 1) % R)]))
fq("24/limb3", 24)(lambda k: (PAIR_VALID3, [(9, lambda x: x ^ B200)]))


def three(j, bad_p=None, bad_q=None, out=0):
    """a 3-pair op whose pair j holds the offending point, between pairs that are fine"""
    g1s, g2s = [MULT[0], b.G1, NG1], [G2W, A2[0], G2W]
    if bad_p is not None:
        g1s[j] = bad_p
    if bad_q is not None:
        g2s[j] = bad_q
    return (g1s, g2s, out)


for j, pos in enumerate(("first", "middle", "last")):
    fq(f"23/off_curve_p_{pos}", 23, pair=j)(lambda k, j=j: (three(j, bad_p=OFF), []))
    fq(f"23/twist_outside_g2_{pos}", 23, pair=j)(lambda k, j=j: (three(j, bad_q=BAD_Q), []))
    fq(f"25/iso_p_{pos}", 25, pair=j)(lambda k, j=j: (three(j, bad_p=ISO_P, out=1), []))
    fq(f"25/off_twist_q_{pos}", 25, pair=j)(lambda k, j=j: (three(j, bad_q=OFF_TWIST), []))
flip = lambda x: x ^ 1  # noqa: E731
bump = lambda x: (x + 1) % R  # noqa: E731
fq("prec/1+10", 1)(lambda k: (pbase(k), [(0, 0), (1, 1)]))
fq("prec/2+14", 2, ATTR)(lambda k: (pbase(k), [(0, 1), (12, 2)]))
fq("prec/10+11", 10)(lambda k: (pbase(k), [(2, 1), (3, 1)]))
fq("prec/11+12", 11)(lambda k: (pbase(k), [(4, 1), (5, 1)]))
fq("prec/12+13", 12)(lambda k: (pbase(k), [(6, 1), (7, 1)]))
fq("prec/13+14", 13)(lambda k: (pbase(k), [(8, 1), (12, 2)]))
fq("prec/14+21", 14)(lambda k: (pbase(k), [(12, 2), (10, 1)]))
fq("prec/21+22", 21)(lambda k: (pbase(k), [(10, 1), (11, flip)]))
fq("prec/22+23", 22)(lambda k: (three(1, bad_p=OFF), [(11, flip)]))
fq("prec/23+24", 23)(lambda k: (three(1, bad_q=BAD_Q), [(9, bump)]))
fq("prec/24+25", 24)(lambda k: (three(1, bad_p=ISO_P), [(9, bump)]))
fq("23/x0_p", 23)(lambda k: (([X0_P], [G2W], 1), []))
fq("prec/24+26", 24)(lambda k: ((PAIR_VALID2[0], PAIR_VALID2[1], 0), [(9, bump)]))
# two checks on DIFFERENT pairs: the subgroup loop runs over every pair before the on-curve loop sees the first
fq("prec/23_last+25_first", 23)(lambda k: (([ISO_P, b.G1, NG1], [G2W, A2[0], BAD_Q], 0), []))
fq("prec/24+25_other_pair", 24)(lambda k: (([MULT[0], b.G1, NG1], [G2W, OFF_TWIST, A2[0]], 0), [(9, bump)]))
fq("prec/22+25", 22)(lambda k: (three(0, bad_q=OFF_TWIST), [(11, flip)]))

POINT_SITES = [1, 2, 3, 4, 5, 6, 7, 8, 9, 14, 18, 19, 20, 10, 21]      # rotated over the point slots
# rotated over the pairing slots; the per-pair entries stand three or more apart, so that one sheet never has two of them on ops 0 / 63 /
# 64, and two before each stands a site whose op 0 has one pair (a ranged pass from pairing op 1 then starts at pair 1)
PAIRING_SITES = ["23/off_curve_p", "1", "2", "24", "25/iso_p", "10", "11", "26", "23/twist_outside_g2", "12", "13", "22", "25/off_twist_q",
                 "14", "21"]
SECOND = ("23/twist_outside_g2", "25/off_twist_q")
# where the offending pair of a per-pair target stands: position in its op, and the op's first pair in the points array.  Op 64's
# two entries per site stand on pairs 64 and 65: lanes 63 and 64 of a stage 1 that starts at pair 1, lane 0 of one that starts at op 64
PAIR_PLACE = {("op0", 0): (0, None), ("op0", 1): (0, None), ("op63", 0): (1, 62), ("op63", 1): (2, 61), ("op64", 0): (0, 64), ("op64", 1): (1, 64),
              ("op66", 0): (2, None), ("op66", 1): (2, None)}


# ---- the model, cached per distinct row -----------------------------------------------------------------------------------------------
_VERDICT = {}


def freeze(x):
    return tuple(freeze(v) for v in x) if isinstance(x, (list, tuple)) else x


def model(adds, muls, pairs, tampers, maxes):
    """(assigned rows, rows to verify, status) of one circuit; tampers: {row: [(cell, value or fn)]}"""
    assigned = b.assign_rows(adds, muls, pairs, RANDOMNESS)
    rows = [list(r) for r in assigned]
    for i, ts in tampers.items():
        for c, v in ts:
            rows[i][c] = v(rows[i][c]) if callable(v) else v
            assert 0 <= rows[i][c] < 1 << 256
    pops = b.point_ops(adds, muls)
    status = []
    for i, row in enumerate(rows):
        op = pops[i] if i < len(pops) else pairs[i - len(pops)]
        key = (i < len(pops), freeze(op), tuple(row), maxes)
        if key not in _VERDICT:  # a row's verdict depends on its own op and cells only
            if i < len(pops):
                _VERDICT[key] = b._verify_row(0, row, [op], [], RANDOMNESS, maxes)
            else:
                _VERDICT[key] = b._verify_row(0, row, [], [op], RANDOMNESS, maxes)
        status.append(_VERDICT[key])
    return assigned, rows, status


def rows_array(rows):
    return np.array([[[(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in row] for row in rows], dtype=np.uint64).reshape(
        len(rows), 13, 4)


# ---- sheets ------------------------------------------------------------------------------------------------------------------------
class Plan:
    """what stands where on one sheet: {row: (variant, code, op, tampers)} for point rows and pairing ops"""

    def __init__(self, s, n_add, maxes=(1, 1, 1)):
        self.s, self.n_add, self.n_mul, self.maxes = s, n_add, sc.N_POINT - n_add, maxes
        self.points, self.pairings, self.pair_first = {}, {}, {}

    def rk(self, row):
        return "add" if row < self.n_add else "mul"

    def free_point_rows(self, rk):
        slots = set(sc.point_slots(self.n_add).values())
        lo, hi = (1, self.n_add) if rk == "add" else (self.n_add, sc.N_POINT)
        return [r for r in range(lo, hi) if r not in slots and r not in self.points]

    def free_pairing_ops(self):
        return [k for k in range(1, sc.N_PAIRING) if k not in sc.PAIR_SLOTS.values() and k not in self.pairings and k not in (5, 30, 65)]

    def put_point(self, row, name):
        code, fn = FAULTS_POINT[name]
        made = fn(self.rk(row), row)
        if made is None:
            return False
        self.points[row] = (name, code, made[0], made[1])
        return True

    def put_pairing(self, k, name, first=None):
        code, fn, pair = FAULTS_PAIRING[name]
        op, tampers = fn(k)
        self.pairings[k] = (name, code, op, tampers, pair)
        if first is not None:
            self.pair_first[k] = first


def build_sheet(plan):
    adds = [plan.points[r][2] if r in plan.points else clean("add", r) for r in range(plan.n_add)]
    muls = [plan.points[r][2] if r in plan.points else clean("mul", r) for r in range(plan.n_add, sc.N_POINT)]
    # pairing fillers: one infinity pair each (so that op k starts at pair k), a few live ones, then counts bent to the wanted starts
    pairs, adjustable = [], []
    for k in range(sc.N_PAIRING):
        if k in plan.pairings:
            pairs.append(plan.pairings[k][2])
        elif k in (5, 30, 65):
            pairs.append((PAIR_VALID2, PAIR_LIVE1, PAIR_VALID3)[(k + plan.s) % 3])
        else:
            pairs.append((PAIR_FILL_ALT if k % 2 else PAIR_FILL)[1])
            adjustable.append(k)
    prev = 0
    for k, first in sorted(plan.pair_first.items()):
        diff = first - sum(len(p[0]) for p in pairs[:k])
        for j in [a for a in adjustable if prev < a < k][:abs(diff)]:
            pairs[j] = PAIR_FILL[0] if diff < 0 else PAIR_FILL[2]
        assert sum(len(p[0]) for p in pairs[:k]) == first, (plan.s, k, first)
        prev = k
    assert len(pairs[0][0]) >= 1  # a ranged pass that starts at pairing op 1 starts past pair 0
    tampers = {r: v[3] for r, v in plan.points.items()}
    tampers.update({sc.N_POINT + k: v[3] for k, v in plan.pairings.items()})
    assigned, rows, status = model(adds, muls, pairs, tampers, plan.maxes)
    w = flatten_ecc_ops(adds, muls, pairs, *plan.maxes)
    targets = []
    for r, (name, code, _, _) in sorted(plan.points.items()):
        assert status[r] == code, (plan.s, r, name, hex(status[r]), hex(code))
        targets.append([r, code, name, -1])
    for k, (name, code, _, _, pair) in sorted(plan.pairings.items()):
        assert status[sc.N_POINT + k] == code, (plan.s, k, name, hex(status[sc.N_POINT + k]), hex(code))
        targets.append([sc.N_POINT + k, code, name, -1 if pair is None else int(w["pair_off"][k]) + pair])
    target_rows = {t[0] for t in targets}
    if plan.maxes == (1, 1, 1):  # every filler is clean
        assert all(st == 0 for i, st in enumerate(status) if i not in target_rows), plan.s
    w.update(rows=rows_array(rows), assigned=rows_array(assigned), status=np.array(status, dtype=np.uint32))
    meta = {"name": f"sheet{plan.s:02d}", "n_add": plan.n_add, "n_mul": plan.n_mul, "maxes": list(plan.maxes), "targets": targets}
    return meta, w


def variants_of(table, site):
    return [n for n in table if n.split("/")[0] == str(site) and not n.endswith("_clean")]


def plans():
    n_rot = len(PAIRING_SITES)
    used, turn, out = set(), {}, []
    needed = {(int(c.split(":")[0]), c.split(":")[1]) for c in sc.required_cells() if c.split(":")[1] not in sc.PAIR_SLOTS}
    needed = {c for c in needed if c[0] in POINT_SITES}
    # site 20 on a mul slot takes an (x, 0) base while there are any (the aff_mul_slow fallback on an edge lane), then a (0, y) base
    slow = sorted((n for n in variants_of(FAULTS_POINT, 20) if n.startswith(sc.SLOW_PREFIXES)), key=lambda n: not n.startswith("20/x0_"))
    s = 0
    while needed or s < n_rot:
        plan = Plan(s, 64 if s % 3 == 2 else 65)
        here = set()
        if s == 2:  # the first mul as row 64 (a wavefront's first lane) of a 64-add sheet
            assert plan.n_add == 64 and plan.put_point(64, slow[turn.get("slow", 0)])
            used.add(slow[turn.get("slow", 0)])
            turn["slow"] = turn.get("slow", 0) + 1
            here.add(20)
            needed -= {(20, cl) for cl in sc.slot_classes(64, 64)}
        for row in sorted(set(sc.point_slots(plan.n_add).values())):
            if row in plan.points:
                continue
            classes = sc.slot_classes(row, plan.n_add)
            # the site with most slot classes still to stand in on this row; ties go round with the sheet number
            order = sorted((x for x in POINT_SITES if x not in here),
                           key=lambda x: (-sum((x, cl) in needed for cl in classes), (POINT_SITES.index(x) - s - row) % len(POINT_SITES)))
            for site in order:
                key = "slow" if site == 20 and plan.rk(row) == "mul" else site
                names = slow if key == "slow" else variants_of(FAULTS_POINT, site)
                done = False
                for _ in names:  # the site's next variant that this kind of row can carry
                    name = names[turn.get(key, 0) % len(names)]
                    turn[key] = turn.get(key, 0) + 1
                    if plan.put_point(row, name):
                        done = True
                        break
                if done:
                    used.add(name)
                    here.add(site)
                    needed -= {(site, cl) for cl in classes}
                    break
        for j, (cl, k) in enumerate(sc.PAIR_SLOTS.items()):
            entry = PAIRING_SITES[(s + j) % n_rot]
            if "/" in entry:
                pos, first = PAIR_PLACE[(cl, int(entry in SECOND))]
                name = f"{entry}_{('first', 'middle', 'last')[pos]}"
                plan.put_pairing(k, name, first)
            else:
                names = variants_of(FAULTS_PAIRING, entry)
                name = names[turn.get("q" + entry, 0) % len(names)]
                turn["q" + entry] = turn.get("q" + entry, 0) + 1
                plan.put_pairing(k, name)
            used.add(name)
        out.append(plan)
        s += 1
    n_rot = len(out)
    # everything no slot took, the controls and the precedence cases, on free rows, round robin over the sheets
    rest = [n for n in FAULTS_POINT if n not in used and n.split("/")[0] not in ("15", "16")]
    assert all(variants_of(FAULTS_POINT, x) for x in POINT_SITES)
    for i, name in enumerate(rest):
        for d in range(n_rot):
            plan = out[(i + d) % n_rot]
            placed = False
            for rk in ("add", "mul"):
                free = plan.free_point_rows(rk)
                if free and plan.put_point(free[(7 * i) % len(free)], name):
                    placed = True
                    break
            if placed:
                break
        assert placed, name
    rest = [n for n in FAULTS_PAIRING if n not in used and not n.startswith("17/")]
    for i, name in enumerate(rest):
        plan = out[(3 * i + 1) % n_rot]
        free = plan.free_pairing_ops()
        plan.put_pairing(free[(5 * i) % len(free)], name)
    # max_*_ops = 0: sites 15 / 16 / 17 on every slot (a row of the other kind relabelled where the slot's own kind cannot reach)
    for s, (n_add, relabel) in enumerate(((65, ("first_mul",)), (64, ("row0", "row63", "last_add", "row127", "row128", "row130")))):
        plan = Plan(n_rot + s, n_add, (0, 0, 0))
        for cl, row in sc.point_slots(n_add).items():
            if row in plan.points and cl not in relabel:
                continue
            natural = "15" if plan.rk(row) == "add" else "16"
            other = "16" if natural == "15" else "15"
            assert plan.put_point(row, f"{other}/relabel" if cl in relabel else f"{natural}/natural")
        for k in sc.PAIR_SLOTS.values():
            plan.put_pairing(k, "17/natural")
        plan.put_point(2, "prec/9+14")       # an earlier check still wins over the max_*_ops assert
        plan.put_point(100, "14/two")
        plan.put_pairing(7, "14/two")
        plan.put_pairing(8, "13/lo")
        assert plan.put_point(3, "15/prec_15+18") and plan.put_point(4, "16/prec_16+19") and plan.put_point(101, "16/prec_16+20")
        plan.put_pairing(9, "17/prec_17+21")
        out.append(plan)
    return out


# ---- the reference's own outcome of the add / mul sites -----------------------------------------------------------------------------------
REF_VARIANTS = ["1/zero", "2/none_as_pairing", "3/lo", "4/hi_only", "5/lo", "6/lo", "7/off_by_one", "8/off_by_one", "9/one", "14/two",
                "15/natural", "16/natural", "18/general_valid1_wrong", "18/x0_valid0_right", "19/qy_lo", "20/sr_valid0_right",
                "20/x0_r_valid0_right", "3/plus_1p", "10/relabel", "21/relabel"]


def reference_outcomes(ref_root):
    for p in (os.path.join(ROOT, "oracle", "refshim"), os.path.join(ref_root, "src")):
        sys.path.insert(0, p)
    import zkevm_specs.ecc_circuit as ec
    from zkevm_specs.evm_circuit import EccTableRow
    from zkevm_specs.util import FQ, Word

    def ints(row):
        r = row.row
        return [r.op_type.n, r.px.lo.n, r.px.hi.n, r.py.lo.n, r.py.hi.n, r.qx.lo.n, r.qx.hi.n, r.qy.lo.n, r.qy.hi.n, r.input_rlc.n, r.out_x.n,
                r.out_y.n, r.is_valid.n]

    out = {}
    original = ec.circuit2rows
    for name in REF_VARIANTS:
        code, fn = FAULTS_POINT[name]
        rk = "add" if fn("add", 0) is not None else "mul"
        op, tampers = fn(rk, 0)
        adds, muls = [clean("add", 1)], [clean("mul", 1)]
        (adds if rk == "add" else muls).append(op)
        target = 1 if rk == "add" else 2
        maxes = tuple(0 if (code & 0xFFFFFF) == 15 + i else 1 for i in range(3))
        adds, muls = (adds[1:], muls[1:]) if 0 in maxes else (adds, muls)  # (with a max of 0 every row of that kind fails)
        target = target if 0 not in maxes else 0
        assigned, rows, status = model(adds, muls, [], {target: tampers}, maxes)
        assert [i for i, st in enumerate(status) if st] == [target] and status[target] == code, (name, status)

        def tampered(circuit, r, rows=rows, assigned=assigned):
            made = original(circuit, r)
            assert [ints(m) for m in made] == [[v % R for v in a] for a in assigned], name  # the model's assignment is the reference's
            for m, row in zip(made, rows):
                c = [FQ(v) for v in row]
                w = [Word((c[1 + 2 * k], c[2 + 2 * k]), check=False) for k in range(4)]
                m.row = EccTableRow(c[0], w[0], w[1], w[2], w[3], c[9], c[10], c[11], c[12])
            return made

        circuit = ec.EccCircuit(*maxes)
        for o in adds:
            circuit.append_add(ec.EcAdd(*o))
        for o in muls:
            circuit.append_mul(ec.EcMul(*o))
        ec.circuit2rows = tampered
        try:
            ec.verify_circuit(circuit, FQ(RANDOMNESS))
            raise SystemExit(f"{name}: the reference accepts the circuit")
        except (AssertionError, AttributeError) as e:  # the reference's own outcome, recorded as it is
            out[name] = [code, type(e).__name__]
        finally:
            ec.circuit2rows = original
    return out


def write_npz(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, arr in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arr), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


class _Rec:
    """a built sheet as tests/ecc_site_cases.coverage_of reads one"""

    def __init__(self, meta, w):
        self.name, self.n_add, self.w, self.status = meta["name"], meta["n_add"], w, w["status"]
        self.targets = [tuple(t) for t in meta["targets"]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-root", default=None, help="a staged reference (oracle/_ref): record its outcome of the add / mul sites")
    ap.add_argument("--out", default=sc.GOLDEN)
    args = ap.parse_args()
    ref = reference_outcomes(args.ref_root) if args.ref_root else json.loads(str(np.load(args.out)["meta"]))["ref_outcomes"]
    built = [build_sheet(p) for p in plans()]
    recs = [_Rec(m, w) for m, w in built]
    table, pair_table, seen = sc.coverage_of(recs, lambda s: s.status)
    missing = sc.required_cells() - set(table)
    assert not missing, sorted(missing)
    assert {f"{s}:{c}" for s in sc.PAIR_SITES for c in sc.PAIR_INDEX_CLASSES} <= set(pair_table), sorted(pair_table)
    assert seen >= {(1, s) for s in sc.ALL_SITES if s != 2} | {(13, 2)}, sorted(seen)
    assert {(s, lane) for s in sc.PAIR_SITES for lane in (0, 63, 64)} <= sc.ranged_lane_hits(recs), sorted(sc.ranged_lane_hits(recs))
    slow = sc.slow_path_cells(recs, lambda s: s.status)
    assert set(slow) >= set(sc.SLOW_CLASSES), sorted(slow)
    assert all(any(v.startswith("20/x0_") for v, _ in slow[cl]) for cl in sc.SLOW_CLASSES), slow  # the (x, 0) base on each of them
    placed = {t[2] for m, _ in built for t in m["targets"]}
    assert placed == set(FAULTS_POINT) | set(FAULTS_PAIRING), sorted((set(FAULTS_POINT) | set(FAULTS_PAIRING)) ^ placed)
    for site in sc.PAIR_SITES:  # first, middle and last pair of a 3-pair op
        assert {v.rsplit("_", 1)[1] for v in placed if v.startswith(f"{site}/")} >= {"first", "middle", "last"}
    arrays, metas = {}, []
    for i, (meta, w) in enumerate(built):
        metas.append(meta)
        for k in sc.KEYS + ("rows", "assigned", "status"):
            arrays[f"{i}_{k}"] = w[k]
    n_targets = sum(len(m["targets"]) for m in metas)
    arrays["meta"] = np.array(json.dumps({
        "randomness": hex(RANDOMNESS), "seed": SEED, "sheets": metas, "coverage": {k: sorted(v) for k, v in sorted(table.items())},
        "pair_coverage": {k: sorted(v) for k, v in sorted(pair_table.items())},
        "slow_path_coverage": {k: sorted(v) for k, v in sorted(slow.items())}, "variants": sorted(placed), "n_targets": n_targets,
        "mod_r_differs": MOD_R_DIFFERS, "ref_outcomes": ref}, sort_keys=True))
    write_npz(args.out, arrays)
    print(f"{len(built)} sheets, {n_targets} targets, {len(placed)} variants, {len(table)} site x slot cells -> {args.out} "
          f"({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()
