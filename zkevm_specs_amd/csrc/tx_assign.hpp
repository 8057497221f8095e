// Tx circuit witness assignment on the device: replaces txs2witness (src/zkevm_specs/tx_circuit.py:332-481; tx2witness :332-406,
// padding_tx :315-329, the dummy SignVerify chip :409-425 / :461-478).
//
// Per transaction:
//   1. the signing payload rlp([nonce, gas_price, gas, to_bytes, value, data, chain_id, 0, 0]) (:343-345) is absorbed into a Keccak
//      sponge as it is encoded: the list header and the int items from registers, the calldata streamed from the caller's buffer in
//      aligned 64-bit words (keccak_table.hpp's KtStream) — the message is never staged;  the CallDataGasCost (:360-368) is counted
//      in the same pass;
//   2. the sender's public key is recovered as eth_keys does it (oracle/refshim/eth_keys/__init__.py:99-140): parity =
//      v - 35 - 2 chain_id in {0, 1} and 0 < r, s < N (else BadSignature, site 1); R = (r, y) with y^2 = r^3 + 7 (no square root:
//      site 3) and y chosen by parity; Q = (s / r) R + (-z / r) G through the ECDSA kernel's joint multiplication (secp256k1.hpp
//      ecdsa_partial / ecdsa_partial4: GLV split of s / r, the comb of G for -z / r); Q at infinity: site 4; then to affine;
//   3. keccak(Q) gives the address; the tx's 12 fixed rows, its SignVerify unit (zk_sign_units layout) and its KeccakTable.add row
//      (tx_circuit.py:48-58) are written.  Slots from len(txs) to MAX_TXS get padding_tx rows and the dummy unit; the CallData rows
//      follow in tx order, padded with (0, CallData, 0, 0) rows to MAX_CALLDATA_BYTES (:441-456).
// The keccak table is a set: its rows are emitted sorted and without duplicates (flatten.flatten_keccak_tuples), the all-zero row
// included.
#pragma once
#include "keccak_table.hpp"
#include "secp256k1.hpp"

#define TX_NFIELDS 8         // per tx: nonce, gas_price, gas, to, value, sig_v, sig_r, sig_s (256-bit words)
#define TX_ROW_CELLS 5       // tx_id, tag, index, value lo, value hi
#define TX_FIXED_ROWS 12     // Nonce .. TxSignHash (TxContextFieldTag, evm_circuit/table.py:153-167)
#define TX_TAG_CALLDATA 13u
#define TX_UNIT_BYTES 288u   // 9 byte rows of 32
#define TX_UNIT_CELLS 8
#define TX_META_PENDING 0xffffffffu  // meta[:, 0] until the ECDSA pass fills it (flatten.ECDSA_STATUS_PENDING)
#define TX_BAD_SIGNATURE ZK_CODE(ZK_UNSUPPORTED, 1)   // eth_keys BadSignature: parity outside {0, 1}, r or s outside (0, N)
#define TX_NO_CURVE_POINT ZK_CODE(ZK_UNSUPPORTED, 3)  // eth_keys BadSignature: r^3 + 7 has no square root mod P
#define TX_Q_INFINITY ZK_CODE(ZK_UNSUPPORTED, 4)      // eth_keys BadSignature: the recovered point is the point at infinity
#define TX_RECOVER_EXACT 0xfffffffdu                  // internal: the GLV split did not fit, the plain chains run instead

struct TxAssignArgs {
    const u64* fields;      // [n][TX_NFIELDS][4]
    const u32* to_none;     // [n]: 1 where tx.to is None
    const uint8_t* data;    // calldata, back to back
    const u64* off;         // [n + 1] byte offsets into data (off[0] == 0)
    u64 n, max_txs, max_calldata;
    u64 chain_id;
    const u64* rpow;        // [KT_RPOW_ROWS][4] (keccak_table.hpp)
    // work
    u64* hash;              // [n][4]: the sign hash as a 256-bit integer (int.from_bytes(digest, "big"))
    u64* gas_cost;          // [n]
    u64* pk;                // [n][8]: Q.x, Q.y (256-bit integers)
    u32* status;            // [n]
    SecpLanes lanes;        // the recovery's lane form (secp_lanes.hpp)
    // outputs (the wire of flatten_tx_witness)
    u64* tx_rows;           // [max_txs * 12 + max_calldata][5][4]
    u32* tx_flags;          // [...]: is_word
    uint8_t* bytes;         // [max_txs][9][32]
    u64* cells;             // column-major [8][max_txs][4]
    u32* meta;              // [max_txs][4]
    u64* kcand;             // [n + 1][5][4]: the zero row, then every tx's KeccakTable.add row (unsorted)
    u32* kfirst;            // [n + 1] (device: first occurrence of its row)
    u64* keccak;            // [<= n + 1][5][4]: the table, sorted, without duplicates
    u32* n_keccak;
};

ZK_HD u64 tx_limb64(const Fr& x, int q) { return (u64)x.v[2 * q] | ((u64)x.v[2 * q + 1] << 32); }
ZK_HD Fr tx_from_limbs(const u64* p) { return fr_load(p); }
ZK_HD Fr tx_bswap256(const Fr& x) {  // the 32 bytes of x in reverse order
    Fr r;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const u64 w = kt_bswap64(tx_limb64(x, 3 - q));
        r.v[2 * q] = (u32)w; r.v[2 * q + 1] = (u32)(w >> 32);
    }
    return r;
}
ZK_HD Fr tx_mod_fr(Fr x) {  // a 256-bit integer mod the BN254 scalar field (FQ(x))
    const Fr p = fr_modulus();
#pragma unroll
    for (int it = 0; it < 5; it++) {
        Fr t;
        const u32 bw = u256_sub(t, x, p);
        x = bw ? x : t;
    }
    return x;
}
ZK_HD u32 tx_byte_len(const Fr& x) {  // minimal big-endian length, 0 for 0
    u32 L = 0;
#pragma unroll
    for (int j = 7; j >= 0; j--)
        if (L == 0 && x.v[j]) L = 4u * (u32)j + 4u - (zk_clz32(x.v[j]) >> 3);
    return L;
}
ZK_HD Fr tx_shl_bytes(Fr x, u32 s) {  // x << 8 s (mod 2^256), s < 32; constant limb indices only (no scratch)
#pragma unroll
    for (int b = 4; b >= 2; b--) {
        const int m = 1 << (b - 2);
        if (s & (1u << b)) {
#pragma unroll
            for (int j = 7; j >= 0; j--) x.v[j] = j >= m ? x.v[j - m] : 0u;
        }
    }
    const u32 r = 8u * (s & 3u);
    if (r) {
#pragma unroll
        for (int j = 7; j > 0; j--) x.v[j] = (x.v[j] << r) | (x.v[j - 1] >> (32u - r));
        x.v[0] <<= r;
    }
    return x;
}

// ---- Keccak-256 sponge fed bit-aligned: whole bytes, up to 8 at a time -------------------------------------------------
struct TxSponge {
    u64 a[25];
    u64 cur;  // pending bytes of the next rate word
    u32 nb;   // their bit count (a multiple of 8, < 64)
    u32 k;    // rate word the next full word goes to (0..16)
};
ZK_HD void txs_init(TxSponge& s) {
#pragma unroll
    for (int j = 0; j < 25; j++) s.a[j] = 0;
    s.cur = 0; s.nb = 0; s.k = 0;
}
ZK_HD void txs_word(TxSponge& s, u64 w) {
#pragma unroll
    for (int j = 0; j < 17; j++) s.a[j] ^= (j == (int)s.k) ? w : 0ull;
    if (++s.k == 17u) {
        keccak_f1600_regs(s.a);
        s.k = 0;
    }
}
// append the low `bits` (8..64, a multiple of 8) bits of w; bits above them must be zero
ZK_HD void txs_push(TxSponge& s, u64 w, u32 bits) {
    const u64 lo = s.cur | (w << s.nb);
    const u32 tot = s.nb + bits;
    if (tot >= 64u) {
        txs_word(s, lo);
        s.cur = s.nb ? (w >> (64u - s.nb)) : 0ull;
        s.nb = tot - 64u;
    } else {
        s.cur = lo;
        s.nb = tot;
    }
}
ZK_HD void txs_byte(TxSponge& s, u32 b) { txs_push(s, (u64)(b & 0xffu), 8u); }
// the L (<= 32) low-order bytes of x, most significant first
ZK_HD void txs_push_be(TxSponge& s, const Fr& x, u32 L) {
    if (!L) return;
    const Fr y = tx_shl_bytes(x, 32u - L);
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int rem = (int)L * 8 - 64 * q;
        if (rem > 0) {
            const u64 w = kt_bswap64(tx_limb64(y, 3 - q));
            const u32 bits = rem >= 64 ? 64u : (u32)rem;
            txs_push(s, bits == 64u ? w : (w & ((1ull << bits) - 1ull)), bits);
        }
    }
}
ZK_HD u32 tx_int_item_len(const Fr& x) {  // rlp of a non-negative int: b"" -> 0x80, a byte < 0x80 alone, else 0x80 + len, bytes
    const u32 L = tx_byte_len(x);
    return (L == 1u && x.v[0] < 0x80u) ? 1u : 1u + L;
}
ZK_HD void txs_push_int(TxSponge& s, const Fr& x) {
    const u32 L = tx_byte_len(x);
    if (L == 1u && x.v[0] < 0x80u) {
        txs_byte(s, x.v[0]);
    } else {
        txs_byte(s, 0x80u + L);
        txs_push_be(s, x, L);
    }
}
ZK_HD void txs_push_len(TxSponge& s, u64 len, u32 base /* 0x80 string, 0xc0 list */) {
    if (len < 56) {
        txs_byte(s, base + (u32)len);
        return;
    }
    const Fr f = fr_from_u64(len);
    const u32 L = tx_byte_len(f);
    txs_byte(s, base + 55u + L);
    txs_push_be(s, f, L);
}
// pad (0x01 .. 0x80), permute; the digest's four little-endian words -> out
ZK_HD void txs_finish(TxSponge& s, u64 out[4]) {
    const u64 w = s.cur ^ (1ull << s.nb);
#pragma unroll
    for (int j = 0; j < 17; j++) s.a[j] ^= (j == (int)s.k) ? w : 0ull;
    s.a[16] ^= 0x80ull << 56;
    keccak_f1600_regs(s.a);
#pragma unroll
    for (int q = 0; q < 4; q++) out[q] = s.a[q];
}

// ---- stage 1: RLP + sign hash + calldata gas cost ------------------------------------------------------------------------
ZK_HD void tx_sign_hash(const TxAssignArgs& a, u64 i) {
    const u64* f = a.fields + i * (TX_NFIELDS * 4);
    const Fr nonce = fr_load(f), gas_price = fr_load(f + 4), gas = fr_load(f + 8), to = fr_load(f + 12), value = fr_load(f + 16);
    const bool none = a.to_none[i] != 0u;
    const u64 o0 = a.off[i], d = a.off[i + 1] - o0;
    const uint8_t* p = a.data + o0;
    const u32 b0 = d ? (u32)p[0] : 0u;
    const Fr chain = fr_from_u64(a.chain_id);
    const bool single = d == 1 && b0 < 0x80u;
    const u64 dlen = single ? 1 : d < 56 ? 1 + d : 1 + tx_byte_len(fr_from_u64(d)) + d;
    const u64 payload = (u64)tx_int_item_len(nonce) + tx_int_item_len(gas_price) + tx_int_item_len(gas) + (none ? 1u : 21u) +
                        tx_int_item_len(value) + dlen + tx_int_item_len(chain) + 2u;
    TxSponge s;
    txs_init(s);
    txs_push_len(s, payload, 0xc0u);
    txs_push_int(s, nonce);
    txs_push_int(s, gas_price);
    txs_push_int(s, gas);
    if (none) {
        txs_byte(s, 0x80u);  // encode_to(): bytes(0)
    } else {
        txs_byte(s, 0x80u + 20u);
        txs_push_be(s, to, 20u);
    }
    txs_push_int(s, value);
    u64 zeros = 0;
    if (single) {
        txs_byte(s, b0);
        zeros = b0 == 0u;
    } else {
        txs_push_len(s, d, 0x80u);
        KtStream st = kt_stream(p, d);
        while (st.left) {
            const u32 nbytes = st.left < 8 ? (u32)st.left : 8u;
            const u64 w = kt_next(st);
#pragma unroll
            for (u32 k = 0; k < 8; k++) zeros += (k < nbytes && ((w >> (8u * k)) & 0xffull) == 0ull) ? 1u : 0u;
            txs_push(s, w, 8u * nbytes);
        }
    }
    txs_push_int(s, chain);
    txs_byte(s, 0x80u);
    txs_byte(s, 0x80u);
    u64 h[4];
    txs_finish(s, h);
    u64* out = a.hash + i * 4;
#pragma unroll
    for (int q = 0; q < 4; q++) out[q] = kt_bswap64(h[3 - q]);  // int.from_bytes(digest, "big")
    a.gas_cost[i] = 4 * zeros + 16 * (d - zeros);                // GAS_COST_TX_CALL_DATA_PER_ZERO_BYTE / _NON_ZERO_BYTE
}

// ---- stage 2: public-key recovery -----------------------------------------------------------------------------------------
// a^e for the fixed exponents of P (libsecp256k1's addition chains: blocks of ones x2 .. x223, then the tail)
ZK_HD Fr tx_sqr_n(Fr x, int n) {
    for (int k = 0; k < n; k++) x = spf_sqr(x);
    return x;
}
ZK_HD void tx_pow_x223(const Fr& a, Fr& x2, Fr& x22, Fr& x223) {
    x2 = spf_mul(spf_sqr(a), a);
    const Fr x3 = spf_mul(spf_sqr(x2), a);
    const Fr x6 = spf_mul(tx_sqr_n(x3, 3), x3);
    const Fr x9 = spf_mul(tx_sqr_n(x6, 3), x3);
    const Fr x11 = spf_mul(tx_sqr_n(x9, 2), x2);
    x22 = spf_mul(tx_sqr_n(x11, 11), x11);
    const Fr x44 = spf_mul(tx_sqr_n(x22, 22), x22);
    const Fr x88 = spf_mul(tx_sqr_n(x44, 44), x44);
    const Fr x176 = spf_mul(tx_sqr_n(x88, 88), x88);
    const Fr x220 = spf_mul(tx_sqr_n(x176, 44), x44);
    x223 = spf_mul(tx_sqr_n(x220, 3), x3);
}
// a^((P + 1) / 4): the square root of a when there is one (the caller squares it back)
ZK_NOINLINE Fr sp_sqrt_p(Fr a) {
    Fr x2, x22, x223;
    tx_pow_x223(a, x2, x22, x223);
    Fr t = spf_mul(tx_sqr_n(x223, 23), x22);
    t = spf_mul(tx_sqr_n(t, 6), x2);
    return tx_sqr_n(t, 2);
}
// a^(P - 2) = a^-1 mod P (0 -> 0)
ZK_NOINLINE Fr sp_inv_p(Fr a) {
    Fr x2, x22, x223;
    tx_pow_x223(a, x2, x22, x223);
    Fr t = spf_mul(tx_sqr_n(x223, 23), x22);
    t = spf_mul(tx_sqr_n(t, 5), a);
    t = spf_mul(tx_sqr_n(t, 3), x2);
    return spf_mul(tx_sqr_n(t, 2), a);
}

// What the recovery of a batch reads and writes: the Tx and the Sig assignment (sig_assign.hpp) differ only in where the words lie
struct SecpRecoverArgs {
    SecpLanes lanes;
    u64 n;
    const u64* vrs;     // signature i: v, r, s as three consecutive 256-bit words at vrs + i * vrs_stride
    u64 vrs_stride;
    Fr v_base;          // what v exceeds by the parity
    const u64* hash;    // the message hash of signature i: the 256-bit word at hash + i * hash_stride ...
    u64 hash_stride;
    u32 hash_bytes;     // ... 0: as an integer, 1: the word of its 32 bytes
    u64* pk;            // [n][8]: Q.x, Q.y (zero where the status is not)
    u32* status;        // [n]
};
SECP_HOST_DEVICE SecpRecoverArgs tx_recover_args(const TxAssignArgs& a) {  // (host code: the launcher's)
    SecpRecoverArgs q;
    q.lanes = a.lanes; q.n = a.n;
    q.vrs = a.fields + 20; q.vrs_stride = TX_NFIELDS * 4;
    const u64 lo = (a.chain_id << 1) + 35u, hi = (a.chain_id >> 63) + (lo < 35u ? 1u : 0u);  // 35 + 2 chain_id < 2^66
    for (int k = 0; k < 8; k++) q.v_base.v[k] = 0u;
    q.v_base.v[0] = (u32)lo; q.v_base.v[1] = (u32)(lo >> 32); q.v_base.v[2] = (u32)hi;
    q.hash = a.hash; q.hash_stride = 4; q.hash_bytes = 0;
    q.pk = a.pk; q.status = a.status;
    return q;
}
// Validation, the lift of R and the two scalars.  ECDSA_PENDING: `pr` is ready for ecdsa_partial / ecdsa_partial4 (R in pr.qx / qy,
// the GLV halves of u2 = s / r, the halves of u1 = -z / r); TX_RECOVER_EXACT: the plain chains over u1 / u2 (tx_recover_exact);
// anything else is the signature's status.
ZK_HD u32 tx_recover_prepare(const SecpRecoverArgs& q, u64 i, EcdsaPrep& pr, Fr& u1, Fr& u2) {
    const u64* f = q.vrs + i * q.vrs_stride;
    const Fr v = fr_load(f), r = fr_load(f + 4), s = fr_load(f + 8);
    Fr par;
    const u32 bw = u256_sub(par, v, q.v_base);
    if (bw || !fr_fits32(par) || par.v[0] > 1u) return TX_BAD_SIGNATURE;
    const Fr n = SecpN::mod();
    if (!fr_lt(r, n) || !fr_lt(s, n) || fr_is_zero(r) || fr_is_zero(s)) return TX_BAD_SIGNATURE;
    Fr seven = fr_zero();
    seven.v[0] = 7u;
    const Fr y2 = spf_add(spf_mul(spf_sqr(r), r), seven);  // r < N < P: a residue
    Fr y = sp_sqrt_p(y2);
    if (!fr_eq(spf_sqr(y), y2)) return TX_NO_CURVE_POINT;
    if ((y.v[0] & 1u) != par.v[0]) y = spf_sub(fr_zero(), y);  // (y != 0: the group order is odd)
    const Fr h = fr_load(q.hash + i * q.hash_stride);
    const Fr z = sp_reduce_once<SecpN>(q.hash_bytes ? tx_bswap256(h) : h);  // (the bytes read big-endian)
    const Fr rinvM = sp_to_mont<SecpN>(sp_inv_n_safegcd(r));
    u2 = sp_mont<SecpN>(s, rinvM);
    u1 = sp_sub<SecpN>(fr_zero(), sp_mont<SecpN>(z, rinvM));
    pr.r = r; pr.qx = r; pr.qy = y;
    if (sp_glv_split(u2, pr.kq[0], pr.neg[0], pr.kq[1], pr.neg[1])) {
        pr.kg[0] = fr_zero(); pr.kg[1] = fr_zero();
#pragma unroll
        for (int k = 0; k < 4; k++) { pr.kg[0].v[k] = u1.v[k]; pr.kg[1].v[k] = u1.v[4 + k]; }
        return ECDSA_PENDING;
    }
    return TX_RECOVER_EXACT;
}
// (the forms over the Tx block, which the host harness calls)
ZK_HD u32 tx_recover_prepare(const TxAssignArgs& a, u64 i, EcdsaPrep& pr, Fr& u1, Fr& u2) { return tx_recover_prepare(tx_recover_args(a), i, pr, u1, u2); }
ZK_HD SpPoint tx_recover_exact(const EcdsaPrep& pr, const Fr& u1, const Fr& u2) {
    SpPoint R;
    R.X = pr.qx; R.Y = pr.qy; R.Z = SecpP::one();
    SpPoint C = sp_scalar_mul_g(u1);
    sp_add_ip(C, sp_scalar_mul(R, u2));
    return C;
}
// Q (Jacobian) -> affine into out[8] (x, y); the signature's status
ZK_HD u32 tx_recover_finish_to(u64* out, const SpPoint& C) {
    if (fr_is_zero(C.Y) || fr_is_zero(C.Z)) {
#pragma unroll
        for (int q = 0; q < 8; q++) out[q] = 0;
        return TX_Q_INFINITY;
    }
    const Fr zi = sp_inv_p(C.Z), zi2 = spf_sqr(zi);
    const Fr x = spf_mul(C.X, zi2), y = spf_mul(C.Y, spf_mul(zi2, zi));
    kt_store(out, x);
    kt_store(out + 4, y);
    return 0;
}
ZK_HD u32 tx_recover_finish(const TxAssignArgs& a, u64 i, const SpPoint& C) { return tx_recover_finish_to(a.pk + i * 8, C); }
ZK_HD void tx_recover_fail_to(u64* out) {
#pragma unroll
    for (int q = 0; q < 8; q++) out[q] = 0;
}
ZK_HD void tx_recover_fail(const TxAssignArgs& a, u64 i) { tx_recover_fail_to(a.pk + i * 8); }

// ---- stage 3: rows, units, keccak rows -------------------------------------------------------------------------------------
ZK_HD void tx_put_row(u64* row, u64 tx_id, u64 tag, u64 index, const Fr& lo, const Fr& hi) {
    kt_store(row, fr_from_u64(tx_id));
    kt_store(row + 4, fr_from_u64(tag));
    kt_store(row + 8, fr_from_u64(index));
    kt_store(row + 12, lo);
    kt_store(row + 16, hi);
}
ZK_HD Fr tx_lo128(const Fr& x) { Fr r = x; r.v[4] = r.v[5] = r.v[6] = r.v[7] = 0u; return r; }
ZK_HD Fr tx_hi128(const Fr& x) {
    Fr r = fr_zero();
#pragma unroll
    for (int q = 0; q < 4; q++) r.v[q] = x.v[4 + q];
    return r;
}
// keccak-256 of the 64-byte key x || y (big-endian): one block
ZK_HD void tx_pk_digest(const Fr& x, const Fr& y, u64 h[4]) {
    u64 st[25];
#pragma unroll
    for (int k = 0; k < 25; k++) st[k] = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        st[q] = kt_bswap64(tx_limb64(x, 3 - q));
        st[4 + q] = kt_bswap64(tx_limb64(y, 3 - q));
    }
    st[8] ^= 1ull;
    st[16] ^= 0x80ull << 56;
    keccak_f1600_regs(st);
#pragma unroll
    for (int q = 0; q < 4; q++) h[q] = st[q];
}
// RLC(reversed(x || y), r) = sum of byte_k r^(63 - k) over the key's bytes (Horner front to back), lazily reduced as kt_chunk
ZK_HD Fr tx_pk_rlc(const Fr& x, const Fr& y, const u64* rpow) {
    u32 acc[9];
#pragma unroll
    for (int j = 0; j < 9; j++) acc[j] = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const u64 w = kt_bswap64(tx_limb64(q < 4 ? x : y, 3 - (q & 3)));  // message bytes 8q .. 8q + 7, first in the low byte
#pragma unroll
        for (u32 k = 0; k < 8; k++) {
            const u32 idx = 8u * (u32)q + k;
            const u32 byte = (u32)(w >> (8u * k)) & 0xffu;
            const Fr pw = fr_load(rpow + 4 * (63u - idx));
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
    Fr lo;
#pragma unroll
    for (int j = 0; j < 8; j++) lo.v[j] = acc[j];
    return fr_add(tx_mod_fr(lo), fr_mul(fr_from_u64(acc[8]), frm_one()));
}
ZK_HD void tx_store_bytes_row(uint8_t* row, u64 w0, u64 w1, u64 w2, u64 w3) {
    u64* p = (u64*)row;
    p[0] = w0; p[1] = w1; p[2] = w2; p[3] = w3;
}
ZK_HD void tx_store_bytes_fr(uint8_t* row, const Fr& x) { tx_store_bytes_row(row, tx_limb64(x, 0), tx_limb64(x, 1), tx_limb64(x, 2), tx_limb64(x, 3)); }

// tx slot i < max_txs: its 12 fixed rows, its SignVerify unit and (real txs) its keccak candidate row kcand[i + 1]
ZK_HD void tx_write_slot(const TxAssignArgs& a, u64 i) {
    u64* rows = a.tx_rows + i * (TX_FIXED_ROWS * TX_ROW_CELLS * 4);
    u32* flags = a.tx_flags + i * TX_FIXED_ROWS;
    uint8_t* ub = a.bytes + i * TX_UNIT_BYTES;
    const u64 tx_id = i + 1;
    const Fr z0 = fr_zero();
    Fr cell[TX_UNIT_CELLS];
#pragma unroll
    for (int c = 0; c < TX_UNIT_CELLS; c++) cell[c] = z0;
    if (i < a.n) {
        const u64* f = a.fields + i * (TX_NFIELDS * 4);
        const Fr nonce = fr_load(f), gas_price = fr_load(f + 4), gas = fr_load(f + 8), to = fr_load(f + 12), value = fr_load(f + 16);
        const Fr r = fr_load(f + 24), s = fr_load(f + 28);
        const Fr z = fr_load(a.hash + i * 4);
        const Fr x = fr_load(a.pk + i * 8), y = fr_load(a.pk + i * 8 + 4);
        const bool ok = a.status[i] == 0u;
        u64 h[4];
        tx_pk_digest(x, y, h);
        // CallerAddress: int.from_bytes(keccak(pk)[-20:], "big") = the low 160 bits of the digest read big-endian
        Fr addr = fr_zero();
        {
            const u64 l0 = kt_bswap64(h[3]), l1 = kt_bswap64(h[2]), l2 = kt_bswap64(h[1]);
            addr.v[0] = (u32)l0; addr.v[1] = (u32)(l0 >> 32); addr.v[2] = (u32)l1; addr.v[3] = (u32)(l1 >> 32); addr.v[4] = (u32)l2;
        }
        const u64 dlen = a.off[i + 1] - a.off[i];
        const bool none = a.to_none[i] != 0u;
        tx_put_row(rows + 0 * 20, tx_id, 1, 0, tx_mod_fr(nonce), z0);
        tx_put_row(rows + 1 * 20, tx_id, 2, 0, tx_mod_fr(gas), z0);
        tx_put_row(rows + 2 * 20, tx_id, 3, 0, tx_lo128(gas_price), tx_hi128(gas_price));
        tx_put_row(rows + 3 * 20, tx_id, 4, 0, addr, z0);
        tx_put_row(rows + 4 * 20, tx_id, 5, 0, none ? z0 : to, z0);
        tx_put_row(rows + 5 * 20, tx_id, 6, 0, fr_from_u64(none ? 1 : 0), z0);
        tx_put_row(rows + 6 * 20, tx_id, 7, 0, tx_lo128(value), tx_hi128(value));
        tx_put_row(rows + 7 * 20, tx_id, 8, 0, fr_from_u64(dlen), z0);
        tx_put_row(rows + 8 * 20, tx_id, 9, 0, fr_from_u64(a.gas_cost[i]), z0);
        tx_put_row(rows + 9 * 20, tx_id, 10, 0, z0, z0);
        tx_put_row(rows + 10 * 20, tx_id, 11, 0, z0, z0);
        tx_put_row(rows + 11 * 20, tx_id, 12, 0, tx_lo128(z), tx_hi128(z));
#pragma unroll
        for (int t = 0; t < TX_FIXED_ROWS; t++) flags[t] = (t == 2 || t == 6 || t == 11) ? 1u : 0u;
        // SignVerifyChip.assign (tx_circuit.py:190-203): pk_x, pk_y, the chip's pk_x, pk_y, msg_hash_bytes twice (little-endian),
        // pub_key_hash (the digest bytes), the chip's r, s (little-endian)
        tx_store_bytes_fr(ub + 0, x);
        tx_store_bytes_fr(ub + 32, y);
        tx_store_bytes_fr(ub + 64, x);
        tx_store_bytes_fr(ub + 96, y);
        tx_store_bytes_fr(ub + 128, z);
        tx_store_bytes_fr(ub + 160, z);
        tx_store_bytes_row(ub + 192, h[0], h[1], h[2], h[3]);
        tx_store_bytes_fr(ub + 224, r);
        tx_store_bytes_fr(ub + 256, s);
        cell[0] = addr;
        cell[1] = tx_lo128(z);
        cell[2] = tx_hi128(z);
        // KeccakTable.add(pk_bytes) (tx_circuit.py:48-58): (1, RLC(reversed(pk)), 64, Word(digest bytes))
        u64* kr = a.kcand + (i + 1) * (KT_NCELLS * 4);
        if (ok) {
            kt_store(kr, fr_from_u64(1));
            kt_store(kr + 4, tx_pk_rlc(x, y, a.rpow));
            kt_store(kr + 8, fr_from_u64(64));
            kr[12] = h[0]; kr[13] = h[1]; kr[14] = 0; kr[15] = 0;
            kr[16] = h[2]; kr[17] = h[3]; kr[18] = 0; kr[19] = 0;
        } else {  // no witness for this tx (the reference raises): the all-zero row, which the table holds anyway
#pragma unroll
            for (int q = 0; q < KT_NCELLS * 4; q++) kr[q] = 0;
        }
    } else {
        // padding_tx(i + 1) (tx_circuit.py:315-329): GasPrice / Value are Word(0), TxSignHash FQ(0)
#pragma unroll
        for (int t = 0; t < TX_FIXED_ROWS; t++) {
            tx_put_row(rows + t * 20, tx_id, (u64)t + 1, 0, z0, z0);
            flags[t] = (t == 2 || t == 6) ? 1u : 0u;
        }
        // the dummy chip (:461-478): DUMMY_PUBLIC_KEY, DUMMY_MSG_HASH = 1, DUMMY_SIGNATURE; pub_key_hash zero, address 0, Word(0)
        const u64 gx0 = 0x59F2815B16F81798ull, gx1 = 0x029BFCDB2DCE28D9ull, gx2 = 0x55A06295CE870B07ull, gx3 = 0x79BE667EF9DCBBACull;
        const u64 gy0 = 0x9C47D08FFB10D4B8ull, gy1 = 0xFD17B448A6855419ull, gy2 = 0x5DA4FBFC0E1108A8ull, gy3 = 0x483ADA7726A3C465ull;
        tx_store_bytes_row(ub + 0, gx0, gx1, gx2, gx3);
        tx_store_bytes_row(ub + 32, gy0, gy1, gy2, gy3);
        tx_store_bytes_row(ub + 64, gx0, gx1, gx2, gx3);
        tx_store_bytes_row(ub + 96, gy0, gy1, gy2, gy3);
        tx_store_bytes_row(ub + 128, 1, 0, 0, 0);
        tx_store_bytes_row(ub + 160, 1, 0, 0, 0);
        tx_store_bytes_row(ub + 192, 0, 0, 0, 0);
        tx_store_bytes_row(ub + 224, gx0, gx1, gx2, gx3);
        tx_store_bytes_row(ub + 256, gx0 + 1, gx1, gx2, gx3);
    }
#pragma unroll
    for (int c = 0; c < TX_UNIT_CELLS; c++) kt_store(a.cells + ((u64)c * a.max_txs + i) * 4, cell[c]);
    u32* m = a.meta + i * 4;
    m[0] = TX_META_PENDING; m[1] = 1u; m[2] = 0u; m[3] = 0u;
}
ZK_HD void tx_write_zero_candidate(const TxAssignArgs& a) {
#pragma unroll
    for (int q = 0; q < KT_NCELLS * 4; q++) a.kcand[q] = 0;
}
// CallData row j < max_calldata (rows after the fixed region): the byte's tx (a binary search over the offsets) or padding
ZK_HD void tx_write_calldata_row(const TxAssignArgs& a, u64 j) {
    u64* row = a.tx_rows + (a.max_txs * TX_FIXED_ROWS + j) * (TX_ROW_CELLS * 4);
    a.tx_flags[a.max_txs * TX_FIXED_ROWS + j] = 0u;
    const Fr z0 = fr_zero();
    if (j >= a.off[a.n]) {
        tx_put_row(row, 0, TX_TAG_CALLDATA, 0, z0, z0);
        return;
    }
    u64 lo = 0, hi = a.n;  // off[lo] <= j < off[hi]
    while (hi - lo > 1) {
        const u64 mid = (lo + hi) >> 1;
        if (a.off[mid] <= j) lo = mid; else hi = mid;
    }
    tx_put_row(row, lo + 1, TX_TAG_CALLDATA, j - a.off[lo], fr_from_u64(a.data[j]), z0);
}
// keccak rows compare as the tuples of their cells (is_enabled, input_rlc, input_len, output lo, hi): the cells' integer values,
// each four little-endian words
ZK_HD int tx_krow_cmp(const u64* x, const u64* y) {
    for (int c = 0; c < KT_NCELLS; c++)
        for (int q = 3; q >= 0; q--) {
            const u64 p = x[4 * c + q], r = y[4 * c + q];
            if (p != r) return p < r ? -1 : 1;
        }
    return 0;
}
