#!/usr/bin/env python3
"""Write tests/golden/ecc_cases.npz: ECC-circuit cases on the zk_ecc_ops wire (include/zkevm_hip.h) with their expected outcome.

Runs where the reference is (it imports the reference's tests/test_ecc_circuit.py through oracle/refshim's stand-ins):
* `ref_*` cases: the parametrised data of the reference's test_ecc_add / test_ecc_mul / test_ecc_pairing, built up as those tests
  build them (op k is verified in a circuit holding ops 0..k), with each step's expected success.  For add / mul the outcome of the
  unmodified reference's verify_circuit under the shim is recorded too (`ref_outcome`: the exception's class name, "" for none);
  the shim has no Fq2 arithmetic, so pairing steps carry only the tests' expectation.
* `trap_*` cases: variants labelled by tests/bn254_ref.py for the traps of the ECC port (coordinates >= p, a mul scalar >= p, an
  is_valid witness on off-curve rows, the (x, 0) doubling chain, max_*_ops of 0, pairing subgroup / RLC / out checks), and tampered
  rows (each row's cells as the device must judge them).
Every case: points / pair_pts / pair_off / pair_out / max_ok (flatten.flatten_ecc_ops), rows uint64[n, 13, 4] to verify (the
oracle's assignment, tampered for `tamper` cases), `assigned` (untampered rows), status uint32[n] (the oracle's codes).
Run: python tools/gen_golden_ecc.py [--ref-root <reference checkout>]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import bn254_ref as b  # noqa: E402
from tests.ecc_cases import fq2_sqrt, g2_words, order3_point, rng, zero_y_chain_point  # noqa: E402
from tests.ecc_kat import chain_scalars  # noqa: E402
from zkevm_specs_amd.flatten import flatten_ecc_ops  # noqa: E402

RANDOMNESS = 0x2F1E0D0C0B0A09080706050403020100F0E0D0C0B0A090807060504030201  # < r
P = b.P


def rows_array(rows):
    return np.array([[[(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in row] for row in rows], dtype=np.uint64).reshape(
        len(rows), 13, 4)


def case(name, add_ops, mul_ops, pair_ops, maxes=(1, 1, 1), tamper=None, expect_success=None, ref_outcome=None):
    assigned = b.assign_rows(add_ops, mul_ops, pair_ops, RANDOMNESS)
    rows = [list(r) for r in assigned]
    for (i, c, v) in tamper or ():
        rows[i][c] = v
    status = b.verify_status(add_ops, mul_ops, pair_ops, rows, RANDOMNESS, *maxes)
    if expect_success is not None:
        assert (not any(status)) == expect_success, (name, status)
    w = flatten_ecc_ops(add_ops, mul_ops, pair_ops, *maxes)
    w.update(rows=rows_array(rows), assigned=rows_array(assigned), status=np.array(status, dtype=np.uint32))
    meta = {"name": name, "n_add": len(add_ops), "n_mul": len(mul_ops), "expect_success": expect_success, "ref_outcome": ref_outcome}
    return meta, w


def reference_cases(ref_root):
    for p in (os.path.join(ROOT, "oracle", "refshim"), os.path.join(ref_root, "src"), os.path.join(ref_root, "tests")):
        sys.path.insert(0, p)
    import test_ecc_circuit as t
    from zkevm_specs.ecc_circuit import EccCircuit, verify_circuit
    from zkevm_specs.util import FQ

    out = []
    for kind, data, maxes in (("add", t.gen_ecAdd_testing_data(), (1, 0, 0)), ("mul", t.gen_ecMul_testing_data(), (0, 1, 0)),
                              ("pairing", t.gen_ecPairing_testing_data(), (0, 0, 1))):
        circuit = EccCircuit(*maxes)
        for k, (op, success) in enumerate(data):
            getattr(circuit, "append_" + kind)(op)
            ref_outcome = None
            if kind != "pairing":
                try:
                    verify_circuit(circuit, FQ(RANDOMNESS))
                    ref_outcome = ""
                except Exception as e:  # the reference's own outcome, recorded as it is
                    ref_outcome = type(e).__name__
            adds = [(tuple(o.p), tuple(o.q), tuple(o.out)) for o in circuit.add_ops]
            muls = [(tuple(o.p), o.s, tuple(o.out)) for o in circuit.mul_ops]
            pairs = [([tuple(g) for g in o.g1_pts], [tuple(g) for g in o.g2_pts], o.out) for o in circuit.pairing_ops]
            out.append(case(f"ref_{kind}_{k}", adds, muls, pairs, maxes, expect_success=success, ref_outcome=ref_outcome))
    return out


def trap_cases():
    F = b.Fq
    g, g2 = b.G1, b.G2
    g7 = b.multiply(g, 7, F)
    g2_5 = b.multiply(g2, 5, b.Fq2)
    q5 = (g2_5[0][1], g2_5[0][0], g2_5[1][1], g2_5[1][0])  # EIP-197 order
    q1 = (g2[0][1], g2[0][0], g2[1][1], g2[1][0])
    a5 = b.multiply(g, 5, F)
    na = b.neg(a5, F)
    off = (5, 0)  # off the curve, y = 0: the affine chain doubles it to (-10, 0)
    out = []
    # 1. coordinates >= p: assign says is_valid = 0, verify fails at the copy constraint
    out.append(case("trap1_add_px_ge_p", [((1 + P, 2), g, (0, 0))], [], []))
    out.append(case("trap1_mul_py_ge_p", [], [((1, 2 + P), 3, (0, 0))], []))
    out.append(case("trap1_pairing_coord_ge_p", [], [], [([g], [(q1[0] + P,) + q1[1:]], 0)]))
    out.append(case("trap1_out_ge_p", [((1, 2), (1, 2), (b.multiply(g, 2, F)[0] + P, b.multiply(g, 2, F)[1]))], [], []))
    # 2. ecMul's scalar mod p, not mod r
    out.append(case("trap2_s_plus_r", [], [(g, b.R + 7, g7)], []))
    out.append(case("trap2_s_ge_p", [], [(g, P + 7, g7)], []))
    out.append(case("trap2_s_is_p_minus_1", [], [(g, P - 1, b.multiply(g, P - 1, F))], []))
    # 3. is_valid is a witness: off-curve rows pass iff the chain does not land on out
    for name, op in (("trap3_off_curve_miss", ((2, 3), g, (0, 0))), ("trap3_off_curve_hit", ((2, 3), g, b.add((2, 3), g, F)))):
        out.append(case(name, [op], [], []))
        out.append(case(name + "_valid1", [op], [], [], tamper=[(0, 12, 1)]))
    # 4. the (x, 0) chain: py_ecc doubles (x, 0) to (-2x, 0)
    for s in (2, 3, 12345, b.R, P - 2):
        hit = b.multiply(off, s, F)
        hit = (0, 0) if hit is None else hit
        out.append(case(f"trap4_x0_mul_{s % 100000}", [], [(off, s, hit), (off, s, (0, 0))], []))
    out.append(case("trap4_x0_add_double", [(off, off, b.add(off, off, F))], [], []))
    out.append(case("trap4_pairing_x0", [], [], [([off], [q1], 1)]))
    # 5. max_*_ops: locals of verify, fire only for a max of 0
    out.append(case("trap5_max_add_0", [(g, g, b.multiply(g, 2, F))], [], [], maxes=(0, 1, 1)))
    out.append(case("trap5_max_mul_0", [], [(g, 7, g7)], [], maxes=(1, 0, 1)))
    out.append(case("trap5_max_pairing_0", [], [], [([g], [q1], 0)], maxes=(1, 1, 0)))
    out.append(case("trap5_max_2_many", [(g, g, b.multiply(g, 2, F))] * 3, [(g, 7, g7)] * 3, [], maxes=(2, 2, 2)))
    # 6. pairings: bilinear identities, infinity, off-twist Q, G2 points outside the subgroup, wrong out, empty pairing op
    out.append(case("trap6_bilinear", [], [], [([a5, g], [q1, b_neg_q(q5)], 1), ([a5, g], [q1, q5], 1), ([na, g], [q1, q5], 1)]))
    out.append(case("trap6_infinity", [], [], [([(0, 0), g], [q1, (0, 0, 0, 0)], 1), ([(0, 0)], [(0, 0, 0, 0)], 0)]))
    out.append(case("trap6_off_twist", [], [], [([g], [(1, 2, 3, 4)], 0)]))
    out.append(case("trap6_twist_not_g2", [], [], [([g], [non_subgroup_g2()], 0)]))
    out.append(case("trap6_empty", [], [], [([], [], 1), ([], [], 0)]))
    # tampered rows of a mixed circuit: every kind of cell
    mixed = ([(g, g, b.multiply(g, 2, F)), (g, (0, 0), g), ((2, 3), g, (0, 0))], [(g, 7, g7), (g, 0, (0, 0)), (off, 3, b.multiply(off, 3, F))],
             [([a5, g], [q1, b_neg_q(q5)], 1), ([g], [q1], 0)])
    out.append(case("mixed_untampered", *mixed))
    for i, c, v in ((0, 0, 2), (0, 0, 4), (1, 1, 7), (2, 12, 2), (3, 7, 1), (3, 10, 5), (4, 9, 3), (6, 9, 1), (6, 11, 0), (7, 11, 1),
                    (6, 0, 1), (0, 0, 3), (6, 1, 1), (7, 10, 1), (5, 12, 1), (2, 12, 1)):
        out.append(case(f"mixed_tamper_r{i}_c{c}", *mixed, tamper=[(i, c, v)]))
    return out


def b_neg_q(q):
    return (q[0], q[1], (-q[2]) % P, (-q[3]) % P)


def non_subgroup_g2():
    """a point on the twist outside G2 (the twist's cofactor is 2p - r): x = c, y from the curve equation"""
    for c in range(1, 100):
        x = (c, 1)
        rhs = b.Fq2.add(b.Fq2.mul(b.Fq2.mul(x, x), x), b.B2)
        y = fq2_sqrt(rhs)
        if y is not None and b.multiply((x, y), b.R, b.Fq2) is not None:
            return (x[1], x[0], y[1], y[0])
    raise AssertionError("no non-subgroup twist point found")


def _right_and_wrong(pt, scalars, g):
    """mul ops of pt: each scalar with the model's result and with a wrong one (is_valid tampered to 1: off-curve rows pass iff the
    chain lands on out)"""
    ops = []
    for s in scalars:
        r = b.multiply(b._g1(pt[0] % P, pt[1] % P), s % P, b.Fq)
        r = (0, 0) if r is None else r
        ops.append((pt, s, r))
        ops.append((pt, s, ((r[0] + 1) % P, r[1]) if g.random() < 0.5 else (r[0], (r[1] + 7) % P)))
    return ops


def chain_cases():
    """off-curve chains that leave the group law: G1 (x, 0) and (0, y) as mul and add rows; (x, 0), (0, y) and depth-1 twist-field
    points as P or Q of pairing ops (PAIR_SUBGROUP or PAIR_ON_CURVE by the model).  (A G1 chain can meet y = 0 only at its first
    point: see zero_y_chain_point.)"""
    F, F2 = b.Fq, b.Fq2
    g = rng(44)
    out = []
    for name, pt in (("x0", (g.randrange(1, P), 0)), ("x0b", (g.randrange(1, P), 0)), ("order3", order3_point(F, g)),
                     ("order3b", order3_point(F, g))):
        muls = _right_and_wrong(pt, chain_scalars(0, g), g)
        out.append(case(f"chain_g1_{name}_mul", [], muls, [], tamper=[(i, 12, 1) for i in range(len(muls))]))
        out.append(case(f"chain_g1_{name}_mul_assigned", [], muls[:16], []))
    y = order3_point(F, g)
    y2 = b.double(y, F)
    adds = [(y, y, y2), (y, b.neg(y, F), (0, 0)), (y, y2, (0, 0)), (y2, y, (1, 1)), (y, (0, 0), y), (y, y, (0, 0))]
    out.append(case("chain_g1_order3_add", adds, [], [], tamper=[(i, 12, 1) for i in range(len(adds))]))
    q1 = g2_words(b.G2)
    qs = [g2_words(((g.randrange(P), g.randrange(P)), (0, 0))), g2_words(order3_point(F2, g)), g2_words(zero_y_chain_point(F2, 1, g)),
          g2_words(zero_y_chain_point(F2, 1, g))]
    ps = [(g.randrange(1, P), 0), order3_point(F, g), (2, 3)]
    # order r off the curve / twist: [r] of the chain is None, so these pass the subgroup check and fail the on-curve check
    ops = [([b.G1], [g2_words(((1, 0), (2, 0)))], 0), ([iso_image(b.G1, F, g)], [q1], 1), ([b.G1], [g2_words(iso_image(b.G2, F2, g))], 0),
           ([b.G1, iso_image(b.multiply(b.G1, 5, F), F, g)], [q1, q1], 1)]
    ops += [([b.G1], [q], g.choice([0, 1])) for q in qs] + [([p], [q1], 0) for p in ps]
    ops += [([b.G1, p], [q1, q], 1) for p, q in zip(ps, qs)] + [([b.G1, ps[0]], [q1, (0, 0, 0, 0)], 1), ([(0, 0)], [qs[2]], 1)]
    out.append(case("chain_pairing_offcurve", [], [], ops))
    return out


def iso_image(pt, F, g):
    """(c^2 x, c^3 y) for a random c: on y^2 = x^3 + c^6 b, off the curve of pt, of pt's order"""
    c = (g.randrange(2, P), g.randrange(P)) if F is b.Fq2 else g.randrange(2, P)
    c2 = F.mul(c, c)
    return (F.mul(c2, pt[0]), F.mul(F.mul(c2, c), pt[1]))


def pairing_volume_cases():
    """160 pairing ops with 0..4 pairs, the count changing between neighbouring lanes: true products (sum a_i b_i = 0 mod r), the same
    off by one, infinity in either slot, off-curve points"""
    F, F2 = b.Fq, b.Fq2
    g = rng(45)
    pool_a = [g.randrange(1, b.R) for _ in range(6)]
    pool_b = [g.randrange(1, b.R) for _ in range(6)]
    ga = {a: b.multiply(b.G1, a, F) for a in pool_a}
    gb = {c: b.multiply(b.G2, c, F2) for c in pool_b}
    odd = [g2_words(((g.randrange(P), g.randrange(P)), (0, 0))), g2_words(zero_y_chain_point(F2, 1, g)), g2_words(iso_image(b.G2, F2, g))]
    ops = []
    for k in range(160):
        n = (0, 3, 1, 4, 2)[k % 5]
        kind = k % 4
        if n == 0:
            ops.append(([], [], k & 1))
            continue
        a = [g.choice(pool_a) for _ in range(n)]
        c = [g.choice(pool_b) for _ in range(n - 1)]
        s = sum(x * y for x, y in zip(a, c)) % b.R
        last = (-s * pow(a[-1], -1, b.R)) % b.R if kind != 1 else (-s * pow(a[-1], -1, b.R) + 1) % b.R
        g1s = [ga[x] for x in a]
        g2s = [g2_words(gb[y]) for y in c] + [g2_words(b.multiply(b.G2, last, F2))]
        if kind == 2:  # infinity in either slot of one pair
            i = g.randrange(n)
            if g.random() < 0.5:
                g1s[i] = (0, 0)
            else:
                g2s[i] = (0, 0, 0, 0)
        if kind == 3 and k % 8 == 3:
            g2s[g.randrange(n)] = g.choice(odd)
        if kind == 3 and k % 8 == 7:
            g1s[g.randrange(n)] = g.choice([(g.randrange(1, P), 0), order3_point(F, g), iso_image(b.G1, F, g)])
        ops.append((g1s, g2s, g.choice([0, 1]) if kind == 2 else int(kind != 1)))
    return [case("pairing_volume", [], [], ops)]


def mixed_wave_cases():
    """229 add / mul rows (not a multiple of 64), the muls shuffled so that every wave mixes Jacobian-only lanes, replay lanes ((x, 0): the
    y = 0 step at j = 0), order-3 chains, infinity and failing lanes; some outputs are words >= 5p"""
    F = b.Fq
    g = rng(46)
    adds, muls = [], []
    for _ in range(24):
        p = b.multiply(b.G1, g.randrange(1, 1 << 20), F)
        adds.append((p, b.G1, b.add(p, b.G1, F) if g.random() < 0.8 else (1, 2)))
    for _ in range(205):
        t = g.random()
        if t < 0.3:
            p, s = b.multiply(b.G1, g.randrange(1, 1 << 16), F), g.randrange(1 << 256)
        elif t < 0.55:
            p, s = (g.randrange(1, P), 0), g.choice([g.randrange(64), g.randrange(1 << 256), b.R, P - 1])
        elif t < 0.7:
            p, s = order3_point(F, g), g.choice([g.randrange(64), g.randrange(1 << 256)])
        elif t < 0.85:
            p, s = g.choice([((0, 0), g.randrange(1 << 256)), (b.G1, 0), (b.G1, b.R)])
        else:
            p, s = (g.randrange(P), g.randrange(P)), g.randrange(1 << 256)
        r = b.multiply(b._g1(p[0] % P, p[1] % P), s % P, F)
        r = (0, 0) if r is None else r
        if g.random() < 0.2 and max(r) < (1 << 256) - 5 * P:  # the same residues as words in [5p, 2^256): fq_reduce's fifth step
            r = (r[0] + 5 * P, r[1] + 5 * P)
        muls.append((p, s, r if g.random() < 0.75 else ((r[0] + 1) % P, r[1])))
    g.shuffle(muls)
    tamper = [(i, 12, 1) for i in range(24, 229) if g.random() < 0.5]
    return [case("mixed_wave_229", adds, muls, [], tamper=tamper)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-root", default=os.path.join(ROOT, "oracle", "_ref"), help="the reference checkout (build() stages one here)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ecc_cases.npz"))
    args = ap.parse_args()
    cases = reference_cases(args.ref_root) + trap_cases() + chain_cases() + pairing_volume_cases() + mixed_wave_cases()
    arrays, metas = {}, []
    for i, (meta, w) in enumerate(cases):
        metas.append(meta)
        for k in ("points", "pair_pts", "pair_off", "pair_out", "max_ok", "rows", "assigned", "status"):
            arrays[f"{i}_{k}"] = w[k]
    arrays["meta"] = np.array(json.dumps({"randomness": hex(RANDOMNESS), "cases": metas}))
    np.savez_compressed(args.out, **arrays)
    fails = sum(1 for m, w in cases if w["status"].any())
    print(f"{len(cases)} cases ({fails} with a failing row) -> {args.out}")


if __name__ == "__main__":
    main()
