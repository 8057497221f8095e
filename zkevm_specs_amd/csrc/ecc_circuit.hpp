// ECC circuit (src/zkevm_specs/ecc_circuit.py): assignment (EccCircuitRow.assign_add / assign_mul / assign_pairing :35-232,
// circuit2rows :386-421) and verification (EccCircuitRow.verify :234-333 with util/ec.py's ECCVerifyChip :120-166 and
// ECCPairingVerifyChip :168-201), one row per call.  Rows are in circuit2rows order: the adds, the muls, then the pairings.
//
// Wire (include/zkevm_hip.h, zk_ecc_ops): add / mul ops uint64[n_add + n_mul][6][4] as 256-bit words — add: p.x, p.y, q.x, q.y,
// out.x, out.y; mul: p.x, p.y, s, 0, out.x, out.y — so that a row's chip is uniform: p0 = (FP(w0), FP(w1)), p1 = (FP(w2), FP(w3)),
// output = (FP(w4), FP(w5)) (FP() = reduction mod the base field p).  Pairing points uint64[n_pts][6][4] in EIP-197 order (p.x,
// p.y, x.c1, x.c0, y.c1, y.c0), op k owning points [off[k], off[k + 1]), and its output word uint64[n_pairing][4].
// A row is uint64[13][4]: op_type, px lo / hi, py lo / hi, qx lo / hi, qy lo / hi, input_rlc, out_x, out_y, is_valid (flatten.py
// flatten_ecc_table).
//
// Status code of a row: (kind << 24) | site, the first check of EccCircuitRow.verify that fails, in its order.
#pragma once
#include "bn254_fq.hpp"
#include "common.hpp"

enum EccSite : u32 {
    ECC_OP_TYPE = 1,        // constrain_equal(is_add + is_mul + is_pairing, 1)
    ECC_NO_CHIP = 2,        // AttributeError: the row's op has no chip of the kind its op_type asks for (`None.p0` / `None.output`)
    ECC_COPY_PX = 3,        // constrain_equal_word(Word(chip.p0[0].n), row.px) ... (a coordinate >= p fails here)
    ECC_COPY_PY = 4,
    ECC_COPY_QX = 5,
    ECC_COPY_QY = 6,
    ECC_COPY_OUT_X = 7,     // constrain_equal(chip.output[0], row.out_x)
    ECC_COPY_OUT_Y = 8,
    ECC_RLC_ZERO = 9,       // add / mul: constrain_zero(row.input_rlc)
    ECC_PAIR_PX_ZERO = 10,  // pairing: constrain_zero_word(row.px) ... qy
    ECC_PAIR_PY_ZERO = 11,
    ECC_PAIR_QX_ZERO = 12,
    ECC_PAIR_QY_ZERO = 13,
    ECC_IS_VALID_BOOL = 14, // constrain_bool(row.is_valid)
    ECC_MAX_ADD = 15,       // assert num_add <= max_add_ops (the counters are locals of verify: they only fire for a max of 0)
    ECC_MAX_MUL = 16,
    ECC_MAX_PAIRING = 17,
    ECC_ADD_RESULT = 18,    // verify_add: FQ(add(p0, p1) == out) == is_valid
    ECC_MUL_QY_ZERO = 19,   // verify_mul: constrain_zero_word(row.qy)
    ECC_MUL_RESULT = 20,    // FQ(multiply(p0, s) == out) == is_valid
    ECC_PAIR_OUT_X = 21,    // verify_pairing: constrain_zero(row.out_x)
    ECC_PAIR_OUT_Y = 22,    // constrain_equal(chip.output, row.out_y)
    ECC_PAIR_SUBGROUP = 23, // constrain_equal(valid_p + valid_q, 2): [r]P and [r]Q by the affine chain
    ECC_PAIR_RLC = 24,      // constrain_equal(row.input_rlc, RLC(reversed(bytes), r))
    ECC_PAIR_ON_CURVE = 25, // py_ecc's pairing(): assert is_on_curve(Q, b2); assert is_on_curve(P, b)
    ECC_PAIR_RESULT = 26,   // constrain_equal(FQ(prod e(Q_i, P_i) == 1), row.out_y)
};
#define ECC_CODE(site) ((1u << 24) | (u32)(site))
#define ECC_ATTR_CODE(site) ((13u << 24) | (u32)(site))
#define ECC_NCELLS 13

struct EccArgs {
    const u64* pts;        // uint64[n_add + n_mul][6][4]
    u64 n_add, n_mul;
    const u64* pair_pts;   // uint64[n_pair_pts][6][4]
    const u32* pair_off;   // uint32[n_pairing + 1]
    const u64* pair_out;   // uint64[n_pairing][4]
    u64 n_pairing;
    Fr randomness;         // keccak randomness (canonical)
    u32 max_ok;            // bit0 max_add_ops >= 1, bit1 max_mul_ops >= 1, bit2 max_pairing_ops >= 1
    const u64* rows;       // verify: uint64[n][13][4]
    u64* rows_out;         // assign: uint64[n][13][4]
};

namespace bn {

ZK_HD Fq fq_raw_word(const u64* w) { return fq_load_raw(w); }
ZK_HD bool fq_word_is_zero(const u64* w) { return (w[0] | w[1] | w[2] | w[3]) == 0; }
// the residue FP(w) of a 256-bit word, in Montgomery form
ZK_HD Fq fq_word_mont(const u64* w) { return fq_to_mont(fq_reduce(fq_load_raw(w))); }
ZK_HD Aff<Fq> g1_from_words(const u64* x, const u64* y) {  // (FP(x), FP(y)); (0, 0) -> None
    Aff<Fq> a;
    a.x = fq_word_mont(x);
    a.y = fq_word_mont(y);
    a.inf = f_is_zero(a.x) && f_is_zero(a.y);
    return a;
}
// multiply(pt, n) == its comparison target (x, y) ((0, 0) for None), exactly as the affine chain
template <class F> ZK_HD bool mul_equals(const Aff<F>& pt, const Fq& n, const F& x, const F& y) {
    int j;
    const Jac<F> r = jac_mul_checked(pt, n, &j);
    if (j < 0) return jac_eq_xy(r, x, y);
    return aff_eq_xy(aff_mul_slow(pt, n, j), x, y);
}
template <class F> ZK_HD bool mul_by_r_is_inf(const Aff<F>& pt) {  // multiply(pt, curve_order) is None
    const Fq rr = {BN_R_LIMBS};
    int j;
    const Jac<F> r = jac_mul_checked(pt, rr, &j);
    if (j < 0) return jac_is_inf(r);
    return aff_mul_slow(pt, rr, j).inf;
}

}  // namespace bn

ZK_HD void ecc_put_cell(u64* c, u64 a, u64 b, u64 d, u64 e) {
    c[0] = a;
    c[1] = b;
    c[2] = d;
    c[3] = e;
}
ZK_HD void ecc_put_word(u64* row, int cell, const u64* w) {  // Word(w): lo = w[0..1], hi = w[2..3]
    ecc_put_cell(row + 4 * cell, w[0], w[1], 0, 0);
    ecc_put_cell(row + 4 * (cell + 1), w[2], w[3], 0, 0);
}
ZK_HD void ecc_put_fr(u64* row, int cell, const Fr& f) {
    for (int k = 0; k < 4; k++) row[4 * cell + k] = (u64)f.v[2 * k] | ((u64)f.v[2 * k + 1] << 32);
}
ZK_HD void ecc_put_fq(u64* row, int cell, const bn::Fq& f) { bn::fq_store_raw(f, row + 4 * cell); }

// ---- assignment ---------------------------------------------------------------------------------------------------------------
// add / mul row i (< n_add + n_mul): the row holds the words as given, out reduced mod p, is_valid = every coordinate < p and the
// point(s) on the curve (EccCircuitRow.assign_add :44-95, assign_mul :97-139; mul's scalar is unconstrained)
ZK_HD void ecc_assign_point_row(const EccArgs& a, u64 i, u64* row) {
    using namespace bn;
    const u64* w = a.pts + i * 24;
    const bool is_add = i < a.n_add;
    bool valid = fq_lt_p(fq_raw_word(w)) && fq_lt_p(fq_raw_word(w + 4)) && on_curve(g1_from_words(w, w + 4));
    if (is_add) valid = valid && fq_lt_p(fq_raw_word(w + 8)) && fq_lt_p(fq_raw_word(w + 12)) && on_curve(g1_from_words(w + 8, w + 12));
    for (int c = 0; c < ECC_NCELLS; c++) ecc_put_cell(row + 4 * c, 0, 0, 0, 0);
    row[0] = is_add ? 1 : 2;
    ecc_put_word(row, 1, w);
    ecc_put_word(row, 3, w + 4);
    ecc_put_word(row, 5, w + 8);
    if (is_add) ecc_put_word(row, 7, w + 12);  // mul: Word(0)
    ecc_put_fq(row, 10, fq_reduce(fq_raw_word(w + 16)));
    ecc_put_fq(row, 11, fq_reduce(fq_raw_word(w + 20)));
    row[4 * 12] = valid ? 1 : 0;
}

// RLC of the pairing inputs: 32 little-endian bytes each of p.x, p.y, x.c0, x.c1, y.c0, y.c1 per pair, reversed, with the keccak
// randomness (Horner over the bytes in their original order)
ZK_HD Fr ecc_rlc_step(Fr acc, const Fr& rM, const bn::Fq& v) {
    for (int b = 0; b < 32; b++) acc = fr_add(fr_mont(acc, rM), fr_from_u64((v.v[b >> 2] >> (8 * (b & 3))) & 0xffu));
    return acc;
}
// the six coordinates of pair `k` of the points array: raw words in RLC order (p.x, p.y, x.c0, x.c1, y.c0, y.c1)
ZK_HD void ecc_pair_words(const u64* pt, bn::Fq* c) {
    c[0] = bn::fq_raw_word(pt);
    c[1] = bn::fq_raw_word(pt + 4);
    c[2] = bn::fq_raw_word(pt + 12);
    c[3] = bn::fq_raw_word(pt + 8);
    c[4] = bn::fq_raw_word(pt + 20);
    c[5] = bn::fq_raw_word(pt + 16);
}
ZK_HD void ecc_pair_points(const bn::Fq* c, bn::Aff<bn::Fq>& p, bn::Aff<bn::Fq2>& q) {  // c: residues (not Montgomery)
    using namespace bn;
    p.x = fq_to_mont(c[0]);
    p.y = fq_to_mont(c[1]);
    p.inf = f_is_zero(p.x) && f_is_zero(p.y);
    q.x = fq2_make(fq_to_mont(c[2]), fq_to_mont(c[3]));
    q.y = fq2_make(fq_to_mont(c[4]), fq_to_mont(c[5]));
    q.inf = f_is_zero(q.x) && f_is_zero(q.y);
}

// pairing op k (EccCircuitRow.assign_pairing :141-232)
ZK_HD void ecc_assign_pairing_row(const EccArgs& a, u64 k, u64* row) {
    using namespace bn;
    const Fr rM = fr_to_mont(a.randomness);
    Fr rlc = fr_zero();
    bool valid = true;
    for (u32 t = a.pair_off[k]; t < a.pair_off[k + 1]; t++) {
        Fq c[6];
        ecc_pair_words(a.pair_pts + (u64)t * 24, c);
        bool pre = true;
        for (int e = 0; e < 6; e++) {
            pre = pre && fq_lt_p(c[e]);
            rlc = ecc_rlc_step(rlc, rM, c[e]);
        }
        if (valid && pre) {  // (the coordinates are residues here: `None` of the raw words == `None` of the reduced ones)
            Aff<Fq> p;
            Aff<Fq2> q;
            ecc_pair_points(c, p, q);
            // on the curve and in G1 (cofactor 1: an on-curve point's chain is the group law's, [r]P = None); on the twist and in G2
            valid = on_curve(p) && on_curve(q) && mul_by_r_is_inf(q);
        } else {
            valid = false;
        }
    }
    const u64* out = a.pair_out + 4 * k;
    for (int c = 0; c < ECC_NCELLS; c++) ecc_put_cell(row + 4 * c, 0, 0, 0, 0);
    row[0] = 3;
    ecc_put_fr(row, 9, rlc);
    ecc_put_cell(row + 4 * 10, out[2], out[3], 0, 0);  // out.hi
    ecc_put_cell(row + 4 * 11, out[0], out[1], 0, 0);  // out.lo
    row[4 * 12] = valid ? 1 : 0;
}

// ---- verification -------------------------------------------------------------------------------------------------------------
ZK_HD bool ecc_cell_is(const u64* c, u64 v) { return c[0] == v && (c[1] | c[2] | c[3]) == 0; }
ZK_HD bool ecc_cell_zero(const u64* c) { return (c[0] | c[1] | c[2] | c[3]) == 0; }
// constrain_equal_word(Word(x), (lo, hi)) for a residue x
ZK_HD bool ecc_word_eq(const bn::Fq& x, const u64* lo, const u64* hi) {
    u64 w[4];
    bn::fq_store_raw(x, w);
    return lo[0] == w[0] && lo[1] == w[1] && (lo[2] | lo[3]) == 0 && hi[0] == w[2] && hi[1] == w[3] && (hi[2] | hi[3]) == 0;
}

// Everything of EccCircuitRow.verify up to the per-kind checks; returns 0 and the row's kind (1 add, 2 mul, 3 pairing) or a code.
ZK_HD u32 ecc_verify_common(const EccArgs& a, u64 i, const u64* row, int* kind) {
    using namespace bn;
    const u64* op = row;
    *kind = ecc_cell_is(op, 1) ? 1 : ecc_cell_is(op, 2) ? 2 : ecc_cell_is(op, 3) ? 3 : 0;
    if (!*kind) return ECC_CODE(ECC_OP_TYPE);
    const bool point_op = i < a.n_add + a.n_mul;
    if (*kind != 3) {
        if (!point_op) return ECC_ATTR_CODE(ECC_NO_CHIP);
        const u64* w = a.pts + i * 24;
        for (int c = 0; c < 4; c++)
            if (!ecc_word_eq(fq_reduce(fq_raw_word(w + 4 * c)), row + 4 * (1 + 2 * c), row + 4 * (2 + 2 * c))) return ECC_CODE(ECC_COPY_PX + c);
        // constrain_equal(FP output, FQ cell): FP - FQ is taken mod p
        if (!fq_eq(fq_reduce(fq_raw_word(w + 16)), fq_reduce(fq_raw_word(row + 40)))) return ECC_CODE(ECC_COPY_OUT_X);
        if (!fq_eq(fq_reduce(fq_raw_word(w + 20)), fq_reduce(fq_raw_word(row + 44)))) return ECC_CODE(ECC_COPY_OUT_Y);
        if (!ecc_cell_zero(row + 36)) return ECC_CODE(ECC_RLC_ZERO);
    } else {
        for (int c = 0; c < 4; c++)
            if (!ecc_cell_zero(row + 4 * (1 + 2 * c)) || !ecc_cell_zero(row + 4 * (2 + 2 * c))) return ECC_CODE(ECC_PAIR_PX_ZERO + c);
    }
    if (!ecc_cell_is(row + 48, 0) && !ecc_cell_is(row + 48, 1)) return ECC_CODE(ECC_IS_VALID_BOOL);
    if (!((a.max_ok >> (*kind - 1)) & 1u)) return ECC_CODE(ECC_MAX_ADD + (*kind - 1));
    return 0;
}

// verify_add / verify_mul (the row passed ecc_verify_common with kind 1 / 2; the chip's coordinates are the words mod p)
ZK_HD u32 ecc_verify_point_ops(const EccArgs& a, u64 i, const u64* row, int kind) {
    using namespace bn;
    const u64* w = a.pts + i * 24;
    const Fq ox = fq_word_mont(w + 16), oy = fq_word_mont(w + 20);
    const bool is_valid = row[48] == 1;
    const Aff<Fq> p0 = g1_from_words(w, w + 4);
    bool ok;
    if (kind == 1) {
        ok = aff_eq_xy(aff_add(p0, g1_from_words(w + 8, w + 12)), ox, oy);
        return ok == is_valid ? 0 : ECC_CODE(ECC_ADD_RESULT);
    }
    if (!ecc_cell_zero(row + 28) || !ecc_cell_zero(row + 32)) return ECC_CODE(ECC_MUL_QY_ZERO);
    const Fq s = fq_reduce(fq_raw_word(w + 8));  // chip.p1[0].n: the scalar mod p
    ok = mul_equals(p0, s, ox, oy);
    return ok == is_valid ? 0 : ECC_CODE(ECC_MUL_RESULT);
}

// verify_pairing for pairing op k (the row passed ecc_verify_common with kind 3)
ZK_HD u32 ecc_verify_pairing_op(const EccArgs& a, u64 i, const u64* row) {
    using namespace bn;
    if (!ecc_cell_zero(row + 40)) return ECC_CODE(ECC_PAIR_OUT_X);
    if (i < a.n_add + a.n_mul) return ECC_ATTR_CODE(ECC_NO_CHIP);  // `self.ecc_pairing_chip.output` of a point op's row
    const u64 k = i - a.n_add - a.n_mul;
    const u64* out = a.pair_out + 4 * k;
    if (!(row[44] == out[0] && row[45] == out[1] && (row[46] | row[47]) == 0)) return ECC_CODE(ECC_PAIR_OUT_Y);
    const u32 t0 = a.pair_off[k], t1 = a.pair_off[k + 1];
    for (u32 t = t0; t < t1; t++) {
        Fq c[6];
        ecc_pair_words(a.pair_pts + (u64)t * 24, c);
        for (int e = 0; e < 6; e++) c[e] = fq_reduce(c[e]);
        Aff<Fq> p;
        Aff<Fq2> q;
        ecc_pair_points(c, p, q);
        // an on-curve G1 point is in the subgroup; anything else runs the chain
        const bool valid_p = on_curve(p) || mul_by_r_is_inf(p);
        const bool valid_q = mul_by_r_is_inf(q);
        if (!(valid_p && valid_q)) return ECC_CODE(ECC_PAIR_SUBGROUP);
    }
    const Fr rM = fr_to_mont(a.randomness);
    Fr rlc = fr_zero();
    for (u32 t = t0; t < t1; t++) {
        Fq c[6];
        ecc_pair_words(a.pair_pts + (u64)t * 24, c);
        for (int e = 0; e < 6; e++) rlc = ecc_rlc_step(rlc, rM, fq_reduce(c[e]));
    }
    if (!fr_eq(rlc, fr_load(row + 36))) return ECC_CODE(ECC_PAIR_RLC);
    Fq12 f = fq12_one();
    for (u32 t = t0; t < t1; t++) {
        Fq c[6];
        ecc_pair_words(a.pair_pts + (u64)t * 24, c);
        for (int e = 0; e < 6; e++) c[e] = fq_reduce(c[e]);
        Aff<Fq> p;
        Aff<Fq2> q;
        ecc_pair_points(c, p, q);
        if (!on_curve(q) || !on_curve(p)) return ECC_CODE(ECC_PAIR_ON_CURVE);
        if (!p.inf && !q.inf) f = fq12_mul(f, miller_loop(p.x, p.y, q.x, q.y));
    }
    const bool one = fq12_is_one(final_exp(f));
    return ecc_cell_is(row + 44, one ? 1 : 0) ? 0 : ECC_CODE(ECC_PAIR_RESULT);
}

// one row of the circuit, rows in circuit2rows order.  The add / mul rows (i < n_add + n_mul) and the pairing rows are split so
// that each kernel carries only its own arithmetic: a point op's row never reaches the pairing math (a pairing op_type there ends in
// `None.output` after the out_x check), a pairing op's row never reaches the point math (its chip is None before that).
ZK_HD u32 ecc_verify_point_row(const EccArgs& a, u64 i) {
    const u64* row = a.rows + i * (ECC_NCELLS * 4);
    int kind;
    const u32 st = ecc_verify_common(a, i, row, &kind);
    if (st) return st;
    if (kind == 3) return ecc_cell_zero(row + 40) ? ECC_ATTR_CODE(ECC_NO_CHIP) : ECC_CODE(ECC_PAIR_OUT_X);
    return ecc_verify_point_ops(a, i, row, kind);
}
ZK_HD u32 ecc_verify_pairing_row(const EccArgs& a, u64 i) {
    const u64* row = a.rows + i * (ECC_NCELLS * 4);
    int kind;
    const u32 st = ecc_verify_common(a, i, row, &kind);
    if (st) return st;
    return ecc_verify_pairing_op(a, i, row);  // kind 3 (an add / mul op_type ended in ECC_NO_CHIP)
}
ZK_HD u32 ecc_verify_row(const EccArgs& a, u64 i) {
    return i < a.n_add + a.n_mul ? ecc_verify_point_row(a, i) : ecc_verify_pairing_row(a, i);
}

// ---- verification of a session's pairing rows in two stages (zk_ecc_open) ----------------------------------------------------------
// Stage 1, one call per pair of the points array: everything of ecc_verify_pairing_op that depends on one pair alone — the flags its
// three loops test and the pair's Miller value — into the session's per-pair record.  Stage 2, one call per pairing row: the checks
// of ecc_verify_pairing_op in their order, over the records.  Both run the functions the one-lane form runs, on the same values, so
// the code of a row is the same bit for bit.
enum EccPairFlag : u32 {
    ECC_PF_VALID_P = 1u,      // on_curve(p) || [r]P == None
    ECC_PF_VALID_Q = 2u,      // [r]Q == None
    ECC_PF_Q_ON_CURVE = 4u,
    ECC_PF_P_ON_CURVE = 8u,
    ECC_PF_INF = 16u,         // p or q is None: the pair is left out of the product
    ECC_PF_MILLER = 32u,      // the record's Fq12 holds miller_loop(p, q)
};
struct EccPairArgs {
    EccArgs a;
    u32* pair_flags;       // uint32[n_pair_pts]
    bn::Fq12* pair_f;      // [n_pair_pts] (Montgomery form, tower order)
};

ZK_HD void ecc_pair_stage1(const EccPairArgs& s, u32 t) {
    using namespace bn;
    Fq c[6];
    ecc_pair_words(s.a.pair_pts + (u64)t * 24, c);
    for (int e = 0; e < 6; e++) c[e] = fq_reduce(c[e]);
    Aff<Fq> p;
    Aff<Fq2> q;
    ecc_pair_points(c, p, q);
    const bool p_on = on_curve(p), q_on = on_curve(q);
    u32 fl = (p_on ? ECC_PF_P_ON_CURVE : 0u) | (q_on ? ECC_PF_Q_ON_CURVE : 0u) | ((p.inf || q.inf) ? ECC_PF_INF : 0u);
    if (p_on || mul_by_r_is_inf(p)) fl |= ECC_PF_VALID_P;
    if (mul_by_r_is_inf(q)) fl |= ECC_PF_VALID_Q;
    // the Miller value is read only by an op that got past its subgroup and on-curve loops: a pair that fails either on its own, or
    // that the product skips, needs none (what OTHER pairs of the op do is stage 2's business)
    const u32 need = ECC_PF_VALID_P | ECC_PF_VALID_Q | ECC_PF_P_ON_CURVE | ECC_PF_Q_ON_CURVE;
    if ((fl & need) == need && !(fl & ECC_PF_INF)) {
        s.pair_f[t] = miller_loop(p.x, p.y, q.x, q.y);
        fl |= ECC_PF_MILLER;
    }
    s.pair_flags[t] = fl;
}

// pairing row i (>= n_add + n_mul) of the session: ecc_verify_pairing_row with the per-pair work read from the records
ZK_HD u32 ecc_pair_stage2(const EccPairArgs& s, u64 i) {
    using namespace bn;
    const EccArgs& a = s.a;
    const u64* row = a.rows + i * (ECC_NCELLS * 4);
    int kind;
    const u32 st = ecc_verify_common(a, i, row, &kind);
    if (st) return st;
    if (!ecc_cell_zero(row + 40)) return ECC_CODE(ECC_PAIR_OUT_X);
    const u64 k = i - a.n_add - a.n_mul;
    const u64* out = a.pair_out + 4 * k;
    if (!(row[44] == out[0] && row[45] == out[1] && (row[46] | row[47]) == 0)) return ECC_CODE(ECC_PAIR_OUT_Y);
    const u32 t0 = a.pair_off[k], t1 = a.pair_off[k + 1];
    for (u32 t = t0; t < t1; t++) {
        const u32 fl = s.pair_flags[t];
        if (!((fl & ECC_PF_VALID_P) && (fl & ECC_PF_VALID_Q))) return ECC_CODE(ECC_PAIR_SUBGROUP);
    }
    const Fr rM = fr_to_mont(a.randomness);
    Fr rlc = fr_zero();
    for (u32 t = t0; t < t1; t++) {
        Fq c[6];
        ecc_pair_words(a.pair_pts + (u64)t * 24, c);
        for (int e = 0; e < 6; e++) rlc = ecc_rlc_step(rlc, rM, fq_reduce(c[e]));
    }
    if (!fr_eq(rlc, fr_load(row + 36))) return ECC_CODE(ECC_PAIR_RLC);
    Fq12 f = fq12_one();
    for (u32 t = t0; t < t1; t++) {
        const u32 fl = s.pair_flags[t];
        if (!(fl & ECC_PF_Q_ON_CURVE) || !(fl & ECC_PF_P_ON_CURVE)) return ECC_CODE(ECC_PAIR_ON_CURVE);
        if (!(fl & ECC_PF_INF)) f = fq12_mul(f, s.pair_f[t]);  // (ECC_PF_MILLER is set: the pair passed both loops)
    }
    const bool one = fq12_is_one(final_exp(f));
    return ecc_cell_is(row + 44, one ? 1 : 0) ? 0 : ECC_CODE(ECC_PAIR_RESULT);
}

// zk_fr_op known-answer hooks (ops 18 .. 25): Fq product, Fq12 operations of residues (words are reduced first), the pairing of one
// pair and the G2 scalar chain
ZK_HD Fr ecc_fq_mul_hook(const Fr& x, const Fr& y) {
    using namespace bn;
    Fq a, b;
    for (int k = 0; k < 8; k++) {
        a.v[k] = x.v[k];
        b.v[k] = y.v[k];
    }
    const Fq r = fq_from_mont(fq_mont(fq_to_mont(fq_reduce(a)), fq_to_mont(fq_reduce(b))));
    Fr o;
    for (int k = 0; k < 8; k++) o.v[k] = r.v[k];
    return o;
}
ZK_HD bn::Fq12 ecc_fq12_load(const u64* p) {
    using namespace bn;
    Fq c[12];
    for (int e = 0; e < 12; e++) c[e] = fq_to_mont(fq_reduce(fq_load_raw(p + 4 * e)));
    Fq12 r;
    r.c0 = fq6_make(fq2_make(c[0], c[1]), fq2_make(c[2], c[3]), fq2_make(c[4], c[5]));
    r.c1 = fq6_make(fq2_make(c[6], c[7]), fq2_make(c[8], c[9]), fq2_make(c[10], c[11]));
    return r;
}
ZK_HD void ecc_fq12_store(const bn::Fq12& r, u64* out) {
    using namespace bn;
    const Fq2* c = &r.c0.c0;  // the six Fq2 coefficients are contiguous in tower order
    for (int e = 0; e < 6; e++) {
        fq_store_raw(fq_from_mont(c[e].c0), out + 8 * e);
        fq_store_raw(fq_from_mont(c[e].c1), out + 8 * e + 4);
    }
}
ZK_HD void ecc_fq12_mul_hook(const u64* a, const u64* b, u64* out) { ecc_fq12_store(bn::fq12_mul(ecc_fq12_load(a), ecc_fq12_load(b)), out); }
// zk_fr_op 25: the G2 scalar chain of the circuit (mul_by_r_is_inf / mul_equals over Fq2) on Q = words 0..3 (EIP-197 order x.c1,
// x.c0, y.c1, y.c0; reduced mod p, all zero = None) and the 256-bit scalar word 4 (as it is).  Out: affine x.c0, x.c1, y.c0, y.c1
// and an infinity flag (coordinates 0 for None), words 5..11 zero.
ZK_HD void ecc_g2_chain_hook(const u64* a, u64* out) {
    using namespace bn;
    Aff<Fq2> q;
    q.x = fq2_make(fq_word_mont(a + 4), fq_word_mont(a));
    q.y = fq2_make(fq_word_mont(a + 12), fq_word_mont(a + 8));
    q.inf = f_is_zero(q.x) && f_is_zero(q.y);
    const Fq n = fq_raw_word(a + 16);
    int j;
    const Jac<Fq2> r = jac_mul_checked(q, n, &j);
    Aff<Fq2> o;
    if (j >= 0) {
        o = aff_mul_slow(q, n, j);
    } else {
        o.inf = jac_is_inf(r);
        const Fq2 zi = f_inv(r.Z), zi2 = f_sqr(zi);  // (0 for None)
        o.x = f_mul(r.X, zi2);
        o.y = f_mul(r.Y, f_mul(zi2, zi));
    }
    if (o.inf) {
        f_zero(o.x);
        f_zero(o.y);
    }
    for (int e = 0; e < 12; e++) fq_store_raw(fq_zero(), out + 4 * e);
    fq_store_raw(fq_from_mont(o.x.c0), out);
    fq_store_raw(fq_from_mont(o.x.c1), out + 4);
    fq_store_raw(fq_from_mont(o.y.c0), out + 8);
    fq_store_raw(fq_from_mont(o.y.c1), out + 12);
    out[16] = o.inf ? 1 : 0;
}
// zk_fr_op 19..25 on one lane's 12 words (see include/zkevm_hip.h): the functions the circuit's kernels run
ZK_HD void ecc_fq12_op_hook(int op, const u64* a, const u64* b, u64* out) {
    using namespace bn;
    switch (op) {
    case 19: ecc_fq12_mul_hook(a, b, out); return;
    case 20: ecc_fq12_store(fq12_sqr(ecc_fq12_load(a)), out); return;
    case 21: ecc_fq12_store(fq12_inv(ecc_fq12_load(a)), out); return;
    case 22: ecc_fq12_store(fq12_frob(ecc_fq12_load(a)), out); return;
    case 23: ecc_fq12_store(final_exp(ecc_fq12_load(a)), out); return;
    case 24: {  // one pair, words in the wire's EIP-197 order (p.x, p.y, x.c1, x.c0, y.c1, y.c0), as the verifier reads them
        Fq c[6];
        ecc_pair_words(a, c);
        for (int e = 0; e < 6; e++) c[e] = fq_reduce(c[e]);
        Aff<Fq> p;
        Aff<Fq2> q;
        ecc_pair_points(c, p, q);
        ecc_fq12_store(final_exp(p.inf || q.inf ? fq12_one() : miller_loop(p.x, p.y, q.x, q.y)), out);
        return;
    }
    case 25: ecc_g2_chain_hook(a, out); return;
    }
}

// Host-side argument check of both backends (zk_ecc_ops is host memory); returns the problem or nullptr.  Fills the args.
#ifdef ZKEVM_HIP_H
static inline const char* ecc_args_from_ops(const zk_ecc_ops* o, EccArgs& a) {
    if (!o || !o->randomness) return "null ops / randomness";
    if ((o->n_add + o->n_mul) && !o->points) return "points is null";
    if (o->n_pairing && (!o->pair_off || !o->pair_out)) return "pair_off / pair_out is null";
    const u64 n = o->n_add + o->n_mul + o->n_pairing;
    if (n == 0 || n >= (1ull << 32) || o->n_add >= (1ull << 32) || o->n_mul >= (1ull << 32)) return "bad row count";
    if (o->n_pairing) {
        if (o->pair_off[0] != 0) return "pair_off[0] != 0";
        for (u64 k = 0; k < o->n_pairing; k++)
            if (o->pair_off[k + 1] < o->pair_off[k]) return "pair_off decreases";
        if (o->pair_off[o->n_pairing] && !o->pair_pts) return "pair_pts is null";
    }
    a.pts = o->points;
    a.n_add = o->n_add;
    a.n_mul = o->n_mul;
    a.pair_pts = o->pair_pts;
    a.pair_off = o->pair_off;
    a.pair_out = o->pair_out;
    a.n_pairing = o->n_pairing;
    for (int k = 0; k < 4; k++) {
        a.randomness.v[2 * k] = (u32)o->randomness[k];
        a.randomness.v[2 * k + 1] = (u32)(o->randomness[k] >> 32);
    }
    const u32 rmod[8] = FR_P_LIMBS;  // (host code: the ZK_HD helpers are device functions in the HIP build)
    bool lt = false;
    for (int k = 0; k < 8; k++) lt = a.randomness.v[k] < rmod[k] || (a.randomness.v[k] == rmod[k] && lt);
    if (!lt) return "randomness is not a canonical field element";
    a.max_ok = (o->max_add ? 1u : 0u) | (o->max_mul ? 2u : 0u) | (o->max_pairing ? 4u : 0u);
    a.rows = nullptr;
    a.rows_out = nullptr;
    return nullptr;
}
#endif
