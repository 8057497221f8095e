// Withdrawal circuit: per-row constraint evaluation and witness assignment.
//
// Reference: src/zkevm_specs/withdrawal_circuit.py — `verify_circuit` :128-201 (row loop, id chain, keccak lookup, MPT lookup,
// final WithdrawalRoot block lookup); the assignment is the reference test's `withdrawals2witness` / `withdrawal2witness`
// (tests/test_withdrawal_circuit.py), the digest its eth_utils.keccak of the RLP.
//
// Row layout (row-major, 8 cells): id, validator_id, address, amount, hash lo, hi, root lo, hi.
// Assignment input (row-major, 5 cells): id, validator_id, address, amount, root (one 256-bit word, 4 x u64 LE, not reduced).
// Keccak table row (5 cells): is_enabled, input_rlc, input_len, output lo, hi (KeccakTable.table's tuples).
// MPT table row (12 cells): state_circuit.hpp's layout.   Block table row (4 cells): field_tag, block_number_or_zero, value lo, hi.
//
// Sites (low 24 bits of the status code), in the reference's order within a row:
//   0 rows[i] itself (IndexError: the witness holds fewer than MAX_WITHDRAWALS rows and none at all here)
//   1 id chain rows[i + 1].withdrawal_id == rows[i].withdrawal_id + 1 (AssertionError; IndexError when rows[i + 1] is missing)
//   2 keccak-table membership (AssertionError)
//   3 MPT lookup (LookupUnsatFailure / LookupAmbiguousFailure)
//   4 the WithdrawalRoot block lookup, on the row MAX_WITHDRAWALS - 1 only (Unsat / Ambiguous; IndexError for rows[-1] of no rows)
//   0xf0 a neighbour row the check needs lies outside the rows a sharded session holds (ZK_UNSUPPORTED: a halo too narrow)
// A row's first failing site is its status; the circuit's verdict is the lowest failing row's.  The type quirks of plain-int
// cells (Word(row.withdrawal_id.n) on an int, TableRow.match on an int address) are classified on the host by the mirror.
#pragma once
#include "row_circuits.hpp"
#include "state_circuit.hpp"
#include "keccak.hpp"

enum { WD_ID = 0, WD_VALIDATOR = 1, WD_ADDRESS = 2, WD_AMOUNT = 3, WD_HASH_LO = 4, WD_HASH_HI = 5, WD_ROOT_LO = 6, WD_ROOT_HI = 7,
       WD_NCELLS = 8 };
enum { WD_IN_NCELLS = 5, WD_BLOCK_NCELLS = 4 };
enum { WD_RLP_MAX = 134 };  // list header (2) + four items of at most 1 + 32 bytes
enum { WD_SITE_ROW = 0, WD_SITE_ID = 1, WD_SITE_KECCAK = 2, WD_SITE_MPT = 3, WD_SITE_BLOCK = 4, WD_SITE_HALO = 0xf0 };
// BlockContextFieldTag.WithdrawalRoot, MPTProofType.WithdrawalMod / NonExistingAccountProof (evm_circuit/table.py:128-144, 326-338)
enum { WD_TAG_WITHDRAWAL_ROOT = 9, WD_PROOF_WITHDRAWAL_MOD = 8, WD_PROOF_NON_EXISTING_ACCOUNT = 4 };

struct WithdrawalArgs {
    const u64* rows;    // [n_rows][8][4]
    u64 n_rows;         // rows held: the whole witness, or a shard with its halo
    u64 row_base;       // global index of rows[0]
    u64 total_rows;     // len(rows) of the whole witness
    u64 max_w;          // MAX_WITHDRAWALS
    ZkTable keccak;     // 5 cells, indexed on (rlc, len)
    ZkTable mpt;        // 12 cells, indexed on state_mpt_key_hash (plain row numbers in the slots)
    const u64* block;   // [n_block][4][4], scanned
    u64 n_block;
    Fr r;               // keccak randomness (canonical)
    // assignment (zk_withdrawal_assign)
    const u64* in;      // [n_in][5][4]
    u64 n_in;
    u64 n_out;          // rows written: max(n_in, max_w)
    u64* rows_out;      // [n_out][8][4]
    u64* keccak_out;    // [n_in][5][4] or nullptr
};

// Rows evaluated by a session over `a`: global rows [row_base, row_base + n) with n = max(1, min(MAX, len(rows))) - row_base, at most
// the rows held (MAX == 0 or no rows at all: one lane, which raises what the reference raises then).
#ifdef ZK_HOSTSIM
static inline
#else
__host__ __device__ inline  // (the library's open sizes the session with it too)
#endif
u64 wd_eval_rows(const WithdrawalArgs& a) {
    u64 n_eval = a.max_w < a.total_rows ? a.max_w : a.total_rows;
    if (n_eval == 0) n_eval = 1;
    if (a.row_base >= n_eval) return 0;
    const u64 n = n_eval - a.row_base;
    return a.n_rows == 0 ? 1 : (n < a.n_rows ? n : a.n_rows);
}

ZK_HD Fr wd_cell(const u64* rows, u64 j, int c) { return fr_load(rows + (j * WD_NCELLS + (u64)c) * 4); }

// ---- RLP of an integer field (rlp.encode of int(x): big-endian, no leading zeros; 0 -> 0x80, 1..127 -> the byte itself) ----
ZK_HD int wd_item_len(const Fr& x) {
    const int n = fr_byte_len(x);
    return (n == 1 && fr_byte(x, 0) < 0x80u) ? 1 : 1 + n;
}
ZK_HD int wd_payload_len(const Fr f[4]) { return wd_item_len(f[0]) + wd_item_len(f[1]) + wd_item_len(f[2]) + wd_item_len(f[3]); }
ZK_HD int wd_rlp_len(const Fr f[4]) {
    const int pl = wd_payload_len(f);
    return pl + (pl < 56 ? 1 : 2);
}
// RLP bytes into m (at least WD_RLP_MAX bytes: registers of the host, LDS on the device); returns the length
ZK_HD int wd_rlp_encode(const Fr f[4], uint8_t* m) {
    const int pl = wd_payload_len(f);
    int p = 0;
    if (pl < 56) m[p++] = (uint8_t)(0xc0 + pl);
    else { m[p++] = 0xf8; m[p++] = (uint8_t)pl; }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const Fr& x = f[i];
        const int n = fr_byte_len(x);
        if (n == 1 && fr_byte(x, 0) < 0x80u) { m[p++] = (uint8_t)fr_byte(x, 0); continue; }
        m[p++] = (uint8_t)(0x80 + n);
#pragma unroll
        for (int k = 31; k >= 0; k--)  // (constant limb indices, as in wd_rlc_item)
            if (k < n) m[p++] = (uint8_t)fr_byte(x, k);
    }
    return p;
}

// ---- RLC(bytes(reversed(data)), r, n_bytes=len).expr(): Horner over the RLP bytes in order, acc = acc * r + byte ----
// Streamed from the fields (no byte buffer): one Montgomery product per byte, acc in normal form (mont(acc, Mont(r)) = acc * r).
ZK_HD Fr wd_horner(const Fr& acc, const Fr& rM, u32 b) { return fr_add_u64(fr_mont(acc, rM), b); }
ZK_HD Fr wd_rlc_item(Fr acc, const Fr& x, const Fr& rM) {
    const int n = fr_byte_len(x);
    if (n == 1 && fr_byte(x, 0) < 0x80u) return wd_horner(acc, rM, fr_byte(x, 0));
    acc = wd_horner(acc, rM, 0x80u + (u32)n);
    // bytes n-1 .. 0, unrolled over all 32 so the limb index is a constant (a run-time index would put x on the stack)
#pragma unroll
    for (int k = 31; k >= 0; k--)
        if (k < n) acc = wd_horner(acc, rM, fr_byte(x, k));
    return acc;
}
ZK_HD Fr wd_rlp_rlc(const Fr f[4], const Fr& rM) {
    const int pl = wd_payload_len(f);
    Fr acc = fr_zero();
    if (pl < 56) acc = wd_horner(acc, rM, 0xc0u + (u32)pl);
    else { acc = wd_horner(acc, rM, 0xf8u); acc = wd_horner(acc, rM, (u32)pl); }
#pragma unroll
    for (int i = 0; i < 4; i++) acc = wd_rlc_item(acc, f[i], rM);
    return acc;
}

// ---- id chain: rows[i + 1].withdrawal_id == rows[i].withdrawal_id + 1 in Fr ----
ZK_HD bool wd_id_chain_ok(const Fr& id, const Fr& next_id) { return fr_eq(next_id, fr_add_u64(id, 1)); }

// ---- keccak digest of a padded single block: m holds the message, zero to byte 135, with the 0x01 / 0x80 padding applied ----
ZK_HD void wd_keccak_padded(const uint8_t* m, u64 out[4]) {
    u64 s[25];
#pragma unroll
    for (int k = 0; k < 25; k++) s[k] = 0;
#pragma unroll
    for (int w = 0; w < 17; w++) {
        u64 v = 0;
#pragma unroll
        for (int b = 0; b < 8; b++) v |= (u64)m[8 * w + b] << (8 * b);
        s[w] = v;
    }
    keccak_f1600(s);
    // Word(digest): lo = digest[0:16] little-endian, hi = digest[16:32]
    for (int k = 0; k < 4; k++) out[k] = s[k];
}

// ---- block lookup (field_tag = WithdrawalRoot, value = root): matching rows on (tag, lo, hi), identical rows counted once ----
ZK_HD u32 wd_block_lookup(const WithdrawalArgs& a, const Fr& root_lo, const Fr& root_hi) {
    const Fr tag = fr_from_u64(WD_TAG_WITHDRAWAL_ROOT);
    u64 first = ~0ull;
    bool ambiguous = false;
    for (u64 k = 0; k < a.n_block; k++) {
        const u64* p = a.block + k * WD_BLOCK_NCELLS * 4;
        if (!fr_eq(fr_load(p), tag) || !fr_eq(fr_load(p + 8), root_lo) || !fr_eq(fr_load(p + 12), root_hi)) continue;
        if (first == ~0ull) first = k;
        else if (!fr_eq(fr_load(p + 4), fr_load(a.block + first * WD_BLOCK_NCELLS * 4 + 4))) ambiguous = true;
    }
    if (first == ~0ull) return ZK_CODE(ZK_LOOKUP_UNSAT, WD_SITE_BLOCK);
    return ambiguous ? ZK_CODE(ZK_LOOKUP_AMBIGUOUS, WD_SITE_BLOCK) : 0u;
}

// ---- one row of verify_circuit's loop: held row j (global row row_base + j) ----
ZK_HD u32 wd_verify_row(const WithdrawalArgs& a, u64 j) {
    const u64 g = a.row_base + j;
    if (a.max_w == 0) {  // the loop does not run; the block lookup reads rows[-1]
        if (a.total_rows == 0) return ZK_CODE(ZK_INDEX_ERROR, WD_SITE_BLOCK);
        const u64 last = a.total_rows - 1;
        if (last < a.row_base || last - a.row_base >= a.n_rows) return ZK_CODE(ZK_UNSUPPORTED, WD_SITE_HALO);
        return wd_block_lookup(a, wd_cell(a.rows, last - a.row_base, WD_ROOT_LO), wd_cell(a.rows, last - a.row_base, WD_ROOT_HI));
    }
    if (g >= a.total_rows) return ZK_CODE(ZK_INDEX_ERROR, WD_SITE_ROW);
    const bool is_last = g == a.max_w - 1;
    const bool has_next = g + 1 < a.total_rows;
    // neighbours this row reads must be held (a shard's halo): checked before anything is read
    if (j >= a.n_rows || (!is_last && has_next && j + 1 >= a.n_rows) || (g != 0 && j == 0)) return ZK_CODE(ZK_UNSUPPORTED, WD_SITE_HALO);
    Fr f[4];
#pragma unroll
    for (int c = 0; c < 4; c++) f[c] = wd_cell(a.rows, j, c);
    // 1. id chain (every row but the last)
    if (!is_last) {
        if (!has_next) return ZK_CODE(ZK_INDEX_ERROR, WD_SITE_ID);
        if (!wd_id_chain_ok(f[WD_ID], wd_cell(a.rows, j + 1, WD_ID))) return ZK_CODE(ZK_ASSERT, WD_SITE_ID);
    }
    // 2. keccak lookup: (pad, pad * rlc, pad * len, hash.select(pad)) in the table
    const bool pad = !fr_is_zero(f[WD_AMOUNT]);  // is_not_padding
    const Fr hash_lo = wd_cell(a.rows, j, WD_HASH_LO), hash_hi = wd_cell(a.rows, j, WD_HASH_HI);
    {
        Fr q[KECCAK_NCELLS];
        q[0] = fr_from_u64(pad ? 1 : 0);
        q[1] = pad ? wd_rlp_rlc(f, fr_to_mont(a.r)) : fr_zero();
        q[2] = fr_from_u64(pad ? (u64)wd_rlp_len(f) : 0);
        q[3] = pad ? hash_lo : fr_zero();
        q[4] = pad ? hash_hi : fr_zero();
        if (!keccak_contains(a.keccak, q)) return ZK_CODE(ZK_ASSERT, WD_SITE_KECCAK);
    }
    // 3. MPT lookup with all seven fields (value = row.hash itself, not the selected one)
    const Fr root_lo = wd_cell(a.rows, j, WD_ROOT_LO), root_hi = wd_cell(a.rows, j, WD_ROOT_HI);
    {
        Fr q[MPT_NCELLS];
        q[0] = f[WD_ADDRESS];
        q[1] = fr_from_u64(pad ? WD_PROOF_WITHDRAWAL_MOD : WD_PROOF_NON_EXISTING_ACCOUNT);
        q[2] = fr_from_u128(fr_lo64(f[WD_ID]), fr_hi64of128(f[WD_ID]));  // Word(withdrawal_id.n): lo = low 128 bits
        q[3] = fr_zero();
#pragma unroll
        for (int k = 0; k < 4; k++) q[3].v[k] = f[WD_ID].v[4 + k];  // hi = id >> 128
        q[4] = root_lo;
        q[5] = root_hi;
        q[6] = g == 0 ? fr_zero() : wd_cell(a.rows, j - 1, WD_ROOT_LO);
        q[7] = g == 0 ? fr_zero() : wd_cell(a.rows, j - 1, WD_ROOT_HI);
        q[8] = hash_lo;
        q[9] = hash_hi;
        q[10] = fr_zero();
        q[11] = fr_zero();
        u32 kind;
        (void)table_probe_inline<MPT_NCELLS, 0xfffu>(a.mpt, state_mpt_hash_cells(q), q, kind);
        if (kind) return ZK_CODE(kind, WD_SITE_MPT);
    }
    // 4. after the loop: the final root in the block table (raised only if no row failed before: it rides on the last row)
    if (is_last) return wd_block_lookup(a, root_lo, root_hi);
    return 0u;
}

// ---- assignment: withdrawals2witness's rows (and the keccak rows KeccakTable.add makes) ----
// Row i < n_in: the withdrawal's fields, Word(keccak(rlp)), Word(root); i >= n_in: a padding row (0, 0, 0, 0, Word(0), last root).
// m: a scratch byte buffer of 136 bytes (LDS on the device).
ZK_HD void wd_store(u64* p, const Fr& x) {
    for (int k = 0; k < 4; k++) p[k] = (u64)x.v[2 * k] | ((u64)x.v[2 * k + 1] << 32);
}
ZK_HD void wd_assign_row(const WithdrawalArgs& a, u64 i, uint8_t* m) {
    u64* out = a.rows_out + i * WD_NCELLS * 4;
    if (i >= a.n_in) {
        for (int k = 0; k < WD_ROOT_LO * 4; k++) out[k] = 0;
        const u64* root = a.n_in ? a.in + ((a.n_in - 1) * WD_IN_NCELLS + 4) * 4 : nullptr;
        out[WD_ROOT_LO * 4 + 0] = root ? root[0] : 0;
        out[WD_ROOT_LO * 4 + 1] = root ? root[1] : 0;
        out[WD_ROOT_LO * 4 + 2] = 0;
        out[WD_ROOT_LO * 4 + 3] = 0;
        out[WD_ROOT_HI * 4 + 0] = root ? root[2] : 0;
        out[WD_ROOT_HI * 4 + 1] = root ? root[3] : 0;
        out[WD_ROOT_HI * 4 + 2] = 0;
        out[WD_ROOT_HI * 4 + 3] = 0;
        return;
    }
    const u64* in = a.in + i * WD_IN_NCELLS * 4;
    Fr f[4];
#pragma unroll
    for (int c = 0; c < 4; c++) f[c] = fr_load(in + 4 * c);
    for (int k = 0; k < 136; k++) m[k] = 0;
    const int len = wd_rlp_encode(f, m);
    m[len] ^= 0x01;   // pre-NIST keccak padding (len <= 134 < 135)
    m[135] ^= 0x80;
    u64 h[4];
    wd_keccak_padded(m, h);
#pragma unroll
    for (int c = 0; c < 4; c++) wd_store(out + 4 * c, f[c]);
    const u64 hw[8] = {h[0], h[1], 0, 0, h[2], h[3], 0, 0};
    const u64 rw[8] = {in[16], in[17], 0, 0, in[18], in[19], 0, 0};
#pragma unroll
    for (int k = 0; k < 8; k++) {
        out[WD_HASH_LO * 4 + k] = hw[k];
        out[WD_ROOT_LO * 4 + k] = rw[k];
    }
    if (a.keccak_out) {
        u64* kr = a.keccak_out + i * KECCAK_NCELLS * 4;
        wd_store(kr, fr_from_u64(1));
        wd_store(kr + 4, wd_rlp_rlc(f, fr_to_mont(a.r)));
        wd_store(kr + 8, fr_from_u64((u64)len));
#pragma unroll
        for (int k = 0; k < 8; k++) kr[12 + k] = hw[k];
    }
}

// the MPT table's index key (the rows' own cells through state_mpt_hash_cells)
ZK_HD u64 wd_mpt_key_hash(const ZkTable& t, u32 r) { return state_mpt_key_hash(t, r); }
