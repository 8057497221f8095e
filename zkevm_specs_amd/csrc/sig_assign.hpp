// Sig circuit witness assignment on the device: signed data (msg_hash, v, r, s) -> the Sig circuit's units (zk_sign_units' Sig
// layout), its keccak table, and — from the same key recovery — the EVM circuit's sig table and the aux cells of the ecRecover
// precompile (aux kind 5).  The reference builds these in its tests (signedData2witness, the ecRecover test's SigTableRow and
// PrecompileAuxData); the contract is the data they produce.
//
// Per signature:
//   1. the key is recovered as eth_keys does it, through the Tx assignment's preparation and finish (tx_assign.hpp
//      tx_recover_prepare / tx_recover_exact / tx_recover_finish_to) and the ECDSA kernel's joint multiplication: parity =
//      v - v_offset in {0, 1} and 0 < r, s < N (else site 1), a curve point with x = r (else site 3), Q not at infinity (else site 4).
//      msg_hash is the word of the hash's 32 bytes (little-endian); z is the same bytes read big-endian;
//   2. keccak(Q) gives the recovered address; the unit's nine byte rows, eight cells and four meta words, its KeccakTable.add row,
//      its sig-table row and its aux row (with the two RLCs over the precompile's input and output bytes) are written.
// A signature with a non-zero status has defined outputs too: key rows and the key hash zero, everything taken from the input as
// given, recovered address 0, is_valid 0, output_rlc 0, no keccak row.
// The keccak table is a sorted set (keccak_set.hpp); the sig table holds the first occurrences of its rows in input order.
#pragma once
#include "tx_assign.hpp"

#define SIG_NFIELDS 4        // per signature: msg_hash, sig_v, sig_r, sig_s (256-bit words)
#define SIG_TABLE_CELLS 9    // msg_hash lo, hi, sig_v, sig_r lo, hi, sig_s lo, hi, recovered_addr, is_valid (SigTableRow)
#define SIG_TABLE_WORDS (SIG_TABLE_CELLS * 4)
#define SIG_AUX_CELLS 12     // the EVM wire's aux row (evm_tables.h), kind 5
#define SIG_PARITY_SAT 0xffffffffu  // meta[:, 3] of a v whose distance from v_offset does not fit 32 bits (flatten_sig_witness saturates alike)

struct SigAssignArgs {
    const u64* fields;        // [n][SIG_NFIELDS][4]
    const u64* addr;          // nullable [n][4]: the claimed address -> cells[0]
    const u32* expect_valid;  // nullable [n] -> meta[:, 1]
    u64 n;
    u64 v_offset;
    u64 rand[4];              // keccak_randomness as given (aux cell 11)
    const u64* rpow;          // [KT_RPOW_ROWS][4] (keccak_table.hpp)
    // work
    u64* pk;                  // [n][8]: Q.x, Q.y
    u32* status;              // [n]
    SecpLanes lanes;          // the recovery's lane form (secp_lanes.hpp)
    // outputs
    uint8_t* bytes;           // [n][9][32]
    u64* cells;               // column-major [8][n][4]
    u32* meta;                // [n][4]
    u64* kcand;               // [n + 1][5][4]: the zero row, then every signature's KeccakTable.add row (unsorted)
    u32* kfirst;              // [n + 1]
    u64* keccak;              // [<= n + 1][5][4]: sorted, without duplicates
    u32* n_keccak;
    u64* scand;               // [n][9][4]: every signature's sig-table row
    u32* sdup;                // [n]: an equal row comes before it
    u64* sig_table;           // [<= n][9][4]: the first occurrences, in input order
    u32* n_sig_rows;
    u64* aux;                 // [n][12][4]
};

SECP_HOST_DEVICE SecpRecoverArgs sig_recover_args(const SigAssignArgs& a) {  // (host code: the launcher's)
    SecpRecoverArgs q;
    q.lanes = a.lanes; q.n = a.n;
    q.vrs = a.fields + 4; q.vrs_stride = SIG_NFIELDS * 4;
    for (int k = 0; k < 8; k++) q.v_base.v[k] = 0u;
    q.v_base.v[0] = (u32)a.v_offset; q.v_base.v[1] = (u32)(a.v_offset >> 32);
    q.hash = a.fields; q.hash_stride = SIG_NFIELDS * 4; q.hash_bytes = 1;
    q.pk = a.pk; q.status = a.status;
    return q;
}

// acc += sum over the 8 bytes of w (first byte lowest) of byte_k * r^(top - k), top >= 7: lazily reduced, as kt_chunk / tx_pk_rlc
ZK_HD void sig_rlc_word(u32 acc[9], u64 w, u32 top, const u64* rpow) {
#pragma unroll
    for (u32 k = 0; k < 8; k++) {
        const u32 byte = (u32)(w >> (8u * k)) & 0xffu;
        const Fr pw = fr_load(rpow + 4 * (top - k));
        u64 c = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            c += (u64)acc[j] + (u64)pw.v[j] * byte;
            acc[j] = (u32)c;
            c >>= 32;
        }
        acc[8] += (u32)c;
    }
}
// a 256-bit integer mod the BN254 scalar field; limb-wise selects (tx_mod_fr's whole-value ones cost the unit kernel stack slots)
ZK_HD Fr sig_mod_fr(Fr x) {
    const Fr p = fr_modulus();
#pragma unroll
    for (int it = 0; it < 5; it++) {  // x < 2^256 < 6p
        Fr t;
        const u32 bw = u256_sub(t, x, p);
#pragma unroll
        for (int j = 0; j < 8; j++) x.v[j] = bw ? x.v[j] : t.v[j];
    }
    return x;
}
ZK_HD Fr sig_rlc_reduce(const u32 acc[9]) {
    Fr lo;
#pragma unroll
    for (int j = 0; j < 8; j++) lo.v[j] = acc[j];
    // acc[8] * 2^256 mod p: 2^256 mod p is the Montgomery one in canonical form
    return fr_add(sig_mod_fr(lo), fr_mul(fr_from_u64(acc[8]), frm_one()));
}
// Horner over 64 bytes, first byte highest power: sum byte_k r^(63 - k).  The bytes are the eight little-endian words w[0..8) in
// order — or, KEY, the key x || y big-endian, of which w holds the limbs (x's four, then y's four, little-endian)
template <bool KEY>
ZK_HD Fr sig_rlc64(const u64* w, const u64* rpow) {
    u32 acc[9];
#pragma unroll
    for (int j = 0; j < 9; j++) acc[j] = 0;
#pragma unroll 1
    for (u32 q = 0; q < 8; q++) sig_rlc_word(acc, KEY ? kt_bswap64(w[q < 4 ? 3u - q : 11u - q]) : w[q], 63u - 8u * q, rpow);
    return sig_rlc_reduce(acc);
}
// the precompile's output: the address as 32 little-endian bytes, first byte highest power (bytes 20 .. 31 are zero)
ZK_HD Fr sig_rlc_addr(const Fr& addr, const u64* rpow) {
    u32 acc[9];
#pragma unroll
    for (int j = 0; j < 9; j++) acc[j] = 0;
#pragma unroll
    for (u32 q = 0; q < 3; q++) sig_rlc_word(acc, tx_limb64(addr, (int)q), 31u - 8u * q, rpow);
    return sig_rlc_reduce(acc);
}

// signature i: its unit, its keccak candidate row kcand[i + 1], its sig-table candidate row and its aux row
ZK_HD void sig_write_unit(const SigAssignArgs& a, u64 i) {
    const u64* f = a.fields + i * (SIG_NFIELDS * 4);
    const Fr m = fr_load(f), v = fr_load(f + 4), r = fr_load(f + 8), s = fr_load(f + 12);
    const Fr x = fr_load(a.pk + i * 8), y = fr_load(a.pk + i * 8 + 4);  // zero unless recovered
    const bool ok = a.status[i] == 0u;
    const Fr z0 = fr_zero();
    u64 h[4] = {0, 0, 0, 0};
    Fr rec = z0;
    if (ok) {
        tx_pk_digest(x, y, h);
        // int.from_bytes(keccak(pk)[-20:], "big"): the low 160 bits of the digest read big-endian
        const u64 l0 = kt_bswap64(h[3]), l1 = kt_bswap64(h[2]), l2 = kt_bswap64(h[1]);
        rec.v[0] = (u32)l0; rec.v[1] = (u32)(l0 >> 32); rec.v[2] = (u32)l1; rec.v[3] = (u32)(l1 >> 32); rec.v[4] = (u32)l2;
    }
    // FQ(v.lo) - FQ(v_offset): the parity of a recovered signature; the sig table's cell of every signature
    const Fr voff = fr_from_u64(a.v_offset);
    const Fr vcell = fr_sub(tx_lo128(v), voff);
    Fr par;
    const u32 bw = u256_sub(par, v, voff);
    const u32 parity = (bw || !fr_fits32(par)) ? SIG_PARITY_SAT : par.v[0];

    uint8_t* ub = a.bytes + i * TX_UNIT_BYTES;
    tx_store_bytes_fr(ub + 0, x);
    tx_store_bytes_fr(ub + 32, y);
    tx_store_bytes_fr(ub + 64, x);
    tx_store_bytes_fr(ub + 96, y);
    tx_store_bytes_fr(ub + 128, m);  // the hash's bytes as they are
    tx_store_bytes_fr(ub + 160, m);
    tx_store_bytes_row(ub + 192, h[0], h[1], h[2], h[3]);
    tx_store_bytes_fr(ub + 224, r);
    tx_store_bytes_fr(ub + 256, s);
    const Fr mlo = tx_lo128(m), mhi = tx_hi128(m), rlo = tx_lo128(r), rhi = tx_hi128(r), slo = tx_lo128(s), shi = tx_hi128(s);
    kt_store(a.cells + ((u64)0 * a.n + i) * 4, a.addr ? fr_load(a.addr + i * 4) : rec);
    kt_store(a.cells + ((u64)1 * a.n + i) * 4, mlo);
    kt_store(a.cells + ((u64)2 * a.n + i) * 4, mhi);
    kt_store(a.cells + ((u64)3 * a.n + i) * 4, vcell);
    kt_store(a.cells + ((u64)4 * a.n + i) * 4, rlo);
    kt_store(a.cells + ((u64)5 * a.n + i) * 4, rhi);
    kt_store(a.cells + ((u64)6 * a.n + i) * 4, slo);
    kt_store(a.cells + ((u64)7 * a.n + i) * 4, shi);
    u32* mt = a.meta + i * 4;
    mt[0] = TX_META_PENDING; mt[1] = a.expect_valid ? a.expect_valid[i] : 1u; mt[2] = 0u; mt[3] = parity;

    // KeccakTable.add(pk_bytes): (1, RLC(reversed(pk)), 64, Word(digest bytes)); none for a signature without a key (the zero row)
    u64* kr = a.kcand + (i + 1) * (KT_NCELLS * 4);
    if (ok) {
        kt_store(kr, fr_from_u64(1));
        kt_store(kr + 4, sig_rlc64<true>(a.pk + i * 8, a.rpow));
        kt_store(kr + 8, fr_from_u64(64));
        kr[12] = h[0]; kr[13] = h[1]; kr[14] = 0; kr[15] = 0;
        kr[16] = h[2]; kr[17] = h[3]; kr[18] = 0; kr[19] = 0;
    } else {
#pragma unroll
        for (int q = 0; q < KT_NCELLS * 4; q++) kr[q] = 0;
    }
    // SigTableRow(Word(msg_hash), FQ(v) - v_offset, Word(r), Word(s), FQ(recovered address), FQ(recovered))
    u64* sr = a.scand + i * SIG_TABLE_WORDS;
    kt_store(sr, mlo);
    kt_store(sr + 4, mhi);
    kt_store(sr + 8, vcell);
    kt_store(sr + 12, rlo);
    kt_store(sr + 16, rhi);
    kt_store(sr + 20, slo);
    kt_store(sr + 24, shi);
    kt_store(sr + 28, rec);
    kt_store(sr + 32, fr_from_u64(ok ? 1 : 0));
    // PrecompileAuxData + randomness: the input words as given, the address, RLC(reversed(input)), RLC(reversed(output))
    u64* ar = a.aux + i * (SIG_AUX_CELLS * 4);
    kt_store(ar, mlo);
    kt_store(ar + 4, mhi);
    kt_store(ar + 8, tx_lo128(v));
    kt_store(ar + 12, tx_hi128(v));
    kt_store(ar + 16, rlo);
    kt_store(ar + 20, rhi);
    kt_store(ar + 24, slo);
    kt_store(ar + 28, shi);
    kt_store(ar + 32, rec);
    // the 128 input bytes are the signature's four words as they lie in memory: two chunks of 64, the first times r^64
    const Fr r64M = fr_load(a.rpow + 4 * 65);
    kt_store(ar + 36, fr_add(fr_mulc(sig_rlc64<false>(f, a.rpow), r64M), sig_rlc64<false>(f + 8, a.rpow)));
    kt_store(ar + 40, sig_rlc_addr(rec, a.rpow));
    ar[44] = a.rand[0]; ar[45] = a.rand[1]; ar[46] = a.rand[2]; ar[47] = a.rand[3];
}
ZK_HD void sig_write_zero_candidate(const SigAssignArgs& a) {
#pragma unroll
    for (int q = 0; q < KT_NCELLS * 4; q++) a.kcand[q] = 0;
}
// sig-table rows compare for equality only (the table keeps input order)
ZK_HD bool sig_row_eq(const u64* x, const u64* y) {
    for (int q = 0; q < SIG_TABLE_WORDS; q++)
        if (x[q] != y[q]) return false;
    return true;
}
