// ECC precompile calls on the device: from the input words of ecAdd / ecMul / ecPairing calls to everything both circuits derive
// from them — the ECC circuit's ops (zk_ecc_ops: `points`, `pair_out`) and rows (circuit2rows), and the EVM circuit's ecc table
// (zk_evm_tables.ecc) and aux rows of kinds 6 / 7 / 8.  The reference computes the results in its tests with py_ecc and copies them
// into rows (src/zkevm_specs/ecc_circuit.py: EccCircuitRow.assign_add :49-99, assign_mul :101-142, assign_pairing :144-232,
// circuit2rows :386-421; tests/evm/precompiles/test_ecAdd.py / test_ecMul.py / test_ecPairing.py build the table row and the aux list).
//
// Per call (include/zkevm_hip.h, zk_ecc_calls):
//   add      is_valid = every coordinate < p and both points on the curve ((0, 0) = infinity); out = p + q, else (0, 0)
//   mul      is_valid = both coordinates < p and the point on the curve; out = [s] P for the full 256-bit s, else (0, 0)
//   pairing  is_valid = per pair all six coordinates < p, P on the curve, Q on the twist and [r] Q = infinity (an on-curve P is in
//            G1: cofactor 1); out = 1 when the product of the pairings is one (the empty product included), else 0; 0 when invalid.
//            input_rlc = assign_pairing's: Horner over the pairs' 32-byte little-endian words in the order p.x, p.y, x.c0, x.c1, y.c0,
//            y.c1, the LAST byte of the last word as the highest power (RLC(reversed(bytes)))
// All curve and field arithmetic is bn254_fq.hpp / ecc_circuit.hpp's; the pairing ops run ecc_pair_stage1 (the verifying session's
// per-pair record: flags + Miller value) and a per-op stage of their own over the records.
//
// The rows carry out as the residue mod the BASE modulus p (EccTableRow of the ECC circuit holds FP values).  The EVM circuit's ecc
// table and the aux rows hold FQ(out): the same integer reduced mod the SCALAR modulus (one subtraction: p < 2 * that modulus).
#pragma once
#include "ecc_circuit.hpp"

#define ECL_AUX_CELLS 12                 // the EVM wire's wide aux row (evm_tables.h)
#define ECL_ROW_WORDS (ECC_NCELLS * 4)   // one 13-cell row
#define ECL_AUX_ADD 6u
#define ECL_AUX_MUL 7u
#define ECL_AUX_PAIRING 8u

struct EccCallArgs {
    const u64* add_in;     // uint64[n_add][4][4]: p.x, p.y, q.x, q.y
    const u64* mul_in;     // uint64[n_mul][3][4]: p.x, p.y, s
    const u64* pair_pts;   // uint64[n_pairs][6][4], EIP-197 order
    const u32* pair_off;   // uint32[n_pairing + 1]
    u64 n_add, n_mul, n_pairing;
    Fr randomness;         // canonical
    // outputs (never null here: a member the caller left null is the session's own buffer)
    u64* points;           // uint64[n_add + n_mul][6][4]
    u64* pair_out;         // uint64[n_pairing][4]
    u64* rows;             // uint64[n][13][4]
    u64* ecc_table;        // uint64[<= n][13][4]: first occurrences of tcand's rows, input order
    u64* aux;              // uint64[n][12][4]
    u32* aux_kind;         // uint32[n]
    // work
    u64* tcand;            // uint64[n][13][4]: every call's ecc-table row
    u32* tdup;             // uint32[n]: an equal row comes before it
    u32* n_table;
    u32* pair_flags;       // ecc_pair_stage1's records
    bn::Fq12* pair_f;
};

// the integer of an Fq residue as a cell of the scalar field: FQ(x) for x < p < 2 * (scalar modulus)
ZK_HD void ecl_put_fq_as_fr(u64* row, int cell, const bn::Fq& x) {
    Fr v, t;
#pragma unroll
    for (int k = 0; k < 8; k++) v.v[k] = x.v[k];
    const u32 bw = u256_sub(t, v, fr_modulus());
    ecc_put_fr(row, cell, bw ? v : t);
}
ZK_HD void ecl_zero(u64* p, int words) {
    for (int k = 0; k < words; k++) p[k] = 0;
}
// the table candidate of a row: the row with out_x / out_y as FQ cells
ZK_HD void ecl_table_row(const u64* row, u64* cand) {
    for (int k = 0; k < ECL_ROW_WORDS; k++) cand[k] = row[k];
    ecl_put_fq_as_fr(cand, 10, bn::fq_raw_word(row + 40));
    ecl_put_fq_as_fr(cand, 11, bn::fq_raw_word(row + 44));
}

// add / mul call i (< n_add + n_mul): the `points` entry, the row, the table candidate and the aux row
ZK_HD void ecc_call_point(const EccCallArgs& a, u64 i) {
    using namespace bn;
    const bool is_add = i < a.n_add;
    const u64* in = is_add ? a.add_in + i * 16 : a.mul_in + (i - a.n_add) * 12;
    const int n_in = is_add ? 16 : 12;
    const Aff<Fq> p0 = g1_from_words(in, in + 4);
    bool valid = fq_lt_p(fq_raw_word(in)) && fq_lt_p(fq_raw_word(in + 4)) && on_curve(p0);
    Aff<Fq> out;
    out.inf = true;
    if (is_add) {
        const Aff<Fq> p1 = g1_from_words(in + 8, in + 12);
        valid = valid && fq_lt_p(fq_raw_word(in + 8)) && fq_lt_p(fq_raw_word(in + 12)) && on_curve(p1);
        if (valid) out = aff_add(p0, p1);  // (one inversion; on the curve py_ecc's add is the group law)
    } else if (valid) {
        // [s] P for the 256-bit s as it is: the group has order r, so no reduction of s is needed.  A point on the curve never meets
        // the affine chain's y = 0 doubling (no point of order 2): the replay is kept for exactness, never taken here
        const Fq s = fq_raw_word(in + 8);
        int j;
        const Jac<Fq> r = jac_mul_checked(p0, s, &j);
        if (j >= 0) {
            out = aff_mul_slow(p0, s, j);
        } else {
            out.inf = jac_is_inf(r);
            const Fq zi = f_inv(r.Z), zi2 = f_sqr(zi);
            out.x = f_mul(r.X, zi2);
            out.y = f_mul(r.Y, f_mul(zi2, zi));
        }
    }
    const Fq ox = out.inf ? fq_zero() : fq_from_mont(out.x), oy = out.inf ? fq_zero() : fq_from_mont(out.y);
    u64* w = a.points + i * 24;
    for (int k = 0; k < n_in; k++) w[k] = in[k];
    for (int k = n_in; k < 16; k++) w[k] = 0;
    fq_store_raw(ox, w + 16);
    fq_store_raw(oy, w + 20);
    u64* row = a.rows + i * ECL_ROW_WORDS;
    ecl_zero(row, ECL_ROW_WORDS);
    row[0] = is_add ? 1 : 2;
    ecc_put_word(row, 1, in);
    ecc_put_word(row, 3, in + 4);
    ecc_put_word(row, 5, in + 8);
    if (is_add) ecc_put_word(row, 7, in + 12);
    ecc_put_fq(row, 10, ox);
    ecc_put_fq(row, 11, oy);
    row[48] = valid ? 1 : 0;
    ecl_table_row(row, a.tcand + i * ECL_ROW_WORDS);
    u64* aux = a.aux + i * (ECL_AUX_CELLS * 4);
    ecl_zero(aux, ECL_AUX_CELLS * 4);
    const int n_words = is_add ? 4 : 3;
    for (int c = 0; c < n_words; c++) ecc_put_word(aux, 2 * c, in + 4 * c);
    ecl_put_fq_as_fr(aux, 2 * n_words, ox);
    ecl_put_fq_as_fr(aux, 2 * n_words + 1, oy);
    a.aux_kind[i] = is_add ? ECL_AUX_ADD : ECL_AUX_MUL;
}

// pairing call k, after ecc_pair_stage1 has left the records of its pairs: validity, RLC, product, final exponentiation
ZK_HD void ecc_call_pairing(const EccCallArgs& a, u64 k) {
    using namespace bn;
    const u32 t0 = a.pair_off[k], t1 = a.pair_off[k + 1];
    const Fr rM = fr_to_mont(a.randomness);
    Fr rlc = fr_zero();
    bool valid = true;
    // (with every coordinate below p the record's flags, taken on the reduced words, are those of the words themselves)
    const u32 need = ECC_PF_P_ON_CURVE | ECC_PF_Q_ON_CURVE | ECC_PF_VALID_Q;
    for (u32 t = t0; t < t1; t++) {
        Fq c[6];
        ecc_pair_words(a.pair_pts + (u64)t * 24, c);
        bool pre = true;
        for (int e = 0; e < 6; e++) {
            pre = pre && fq_lt_p(c[e]);
            rlc = ecc_rlc_step(rlc, rM, c[e]);
        }
        valid = valid && pre && (a.pair_flags[t] & need) == need;
    }
    bool one = false;
    if (valid) {
        Fq12 f = fq12_one();
        bool any = false;
        for (u32 t = t0; t < t1; t++)
            if (!(a.pair_flags[t] & ECC_PF_INF)) {  // (ECC_PF_MILLER is set: the pair passed every check of stage 1)
                f = fq12_mul(f, a.pair_f[t]);
                any = true;
            }
        one = any ? fq12_is_one(final_exp(f)) : true;
    }
    const u64 o = one ? 1 : 0;
    ecc_put_cell(a.pair_out + 4 * k, o, 0, 0, 0);
    const u64 i = a.n_add + a.n_mul + k;
    u64* row = a.rows + i * ECL_ROW_WORDS;
    ecl_zero(row, ECL_ROW_WORDS);
    row[0] = 3;
    ecc_put_fr(row, 9, rlc);
    row[44] = o;  // out_y = out.lo (out_x = out.hi = 0)
    row[48] = valid ? 1 : 0;
    u64* cand = a.tcand + i * ECL_ROW_WORDS;
    for (int q = 0; q < ECL_ROW_WORDS; q++) cand[q] = row[q];
    u64* aux = a.aux + i * (ECL_AUX_CELLS * 4);
    ecl_zero(aux, ECL_AUX_CELLS * 4);
    ecc_put_fr(aux, 0, rlc);
    aux[4] = t1 - t0;
    aux[8] = valid ? 1 : 0;
    aux[12] = o;
    a.aux_kind[i] = ECL_AUX_PAIRING;
}

ZK_HD bool ecl_row_eq(const u64* x, const u64* y) {
    for (int q = 0; q < ECL_ROW_WORDS; q++)
        if (x[q] != y[q]) return false;
    return true;
}

// Host-side argument check of both backends: `in` with pair_off and randomness readable on the host.  Returns 0 and fills the
// counts and the randomness of `a`, or the error code with its text in *err.
#ifdef ZKEVM_HIP_H
static inline int ecc_calls_check(const zk_ecc_calls* in, EccCallArgs& a, const char** err) {
    *err = nullptr;
    if (!in || !in->randomness) { *err = "null calls / randomness"; return -1; }
    const u64 lim = 1ull << 31;
    if (in->n_add >= lim || in->n_mul >= lim || in->n_pairing >= lim || in->n_add + in->n_mul + in->n_pairing >= lim) {
        *err = "2^31 calls or more";
        return ZK_ERR_ECL_ROWS;
    }
    if (in->n_add + in->n_mul + in->n_pairing == 0) { *err = "no calls"; return -1; }
    if ((in->n_add && !in->add_in) || (in->n_mul && !in->mul_in) || (in->n_pairing && !in->pair_off)) { *err = "null input array"; return -1; }
    if (in->n_pairing) {
        if (in->pair_off[0] != 0) { *err = "pair_off[0] != 0"; return ZK_ERR_ECL_OFFSETS; }
        for (u64 k = 0; k < in->n_pairing; k++)
            if (in->pair_off[k + 1] < in->pair_off[k]) { *err = "pair_off decreases"; return ZK_ERR_ECL_OFFSETS; }
        if (in->pair_off[in->n_pairing] >= lim) { *err = "2^31 pairs or more"; return ZK_ERR_ECL_ROWS; }
        if (in->pair_off[in->n_pairing] && !in->pair_pts) { *err = "pair_pts is null"; return -1; }
    }
    for (int k = 0; k < 4; k++) {
        a.randomness.v[2 * k] = (u32)in->randomness[k];
        a.randomness.v[2 * k + 1] = (u32)(in->randomness[k] >> 32);
    }
    const u32 rmod[8] = FR_P_LIMBS;  // (host code: the ZK_HD helpers are device functions in the HIP build)
    bool lt = false;
    for (int k = 0; k < 8; k++) lt = a.randomness.v[k] < rmod[k] || (a.randomness.v[k] == rmod[k] && lt);
    if (!lt) { *err = "randomness is not a canonical field element"; return ZK_ERR_ECL_RANDOMNESS; }
    a.n_add = in->n_add;
    a.n_mul = in->n_mul;
    a.n_pairing = in->n_pairing;
    return 0;
}
#endif
