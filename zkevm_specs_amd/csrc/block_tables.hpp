// EVM circuit tx, block and withdrawal tables from raw block data (zk_evm_tables_from_block*).
//
// Replaces Transaction.table_assignments(), Block.table_assignments() and Withdrawal.table_assignments() (evm_circuit/typing.py:
// 209-281, 116-137, 306-314) followed by flatten_tx_table / flatten_block_table / flatten_withdrawal_table: the tables come out in the
// order of the reference's sets (ascending over the cells), which is closed-form once the ids are distinct and ascending (btb_plan
// checks that at open): per tx the rows of tags 1..12, then one CallData row per byte; the block table by tag, its HistoryHash rows by
// their number cell; the withdrawals by id.
//
//   btb_gas_chunk    non-zero bytes of one aligned 16-byte piece of the calldata (one aligned load; the ragged pieces at the two ends
//                    of the buffer byte by byte), btb_gas_block the sum over a block of BTB_GAS_BLOCK bytes
//   btb_gas_prefix   exclusive prefix of the blocks' counts (host form; k_block_tables.hip scans them in one workgroup)
//   btb_range_nonzero   non-zero bytes of calldata[o0, o1): whole blocks from the prefix, at most 2 BTB_GAS_BLOCK / 16 + 2 pieces beside
//                    them — no lane's work grows with a tx's length
//   btb_tx_of_row    the tx of a tx-table row by binary search over 12 i + offsets[i]; btb_tx_piece the 16-byte piece q (0..9) of the row
//   btb_tx_flag, btb_block_row, btb_wd_row
// The functions here define the results (CPU backend, tests/hostsim); k_block_tables.hip maps lanes onto them.
#pragma once
#include <stdio.h>
#include "fr.hpp"

enum { BTB_TX_NCELLS = 5, BTB_BLOCK_NCELLS = 4, BTB_WD_NCELLS = 4, BTB_NTX_FIELDS = 9, BTB_NBLOCK_FIELDS = 8, BTB_TX_FIXED = 12,
       BTB_TX_PIECES = 10,      // 16-byte pieces of a 160-byte tx-table row
       BTB_GAS_BLOCK = 256,     // bytes of calldata per partial count
       BTB_GAS_PIECES = BTB_GAS_BLOCK / 16,
       BTB_BLOCK_FIXED = 8, BTB_MAX_HISTORY = 256 };
// tx_fields[i][..]
enum { BTB_F_ID = 0, BTB_F_NONCE, BTB_F_GAS, BTB_F_GAS_PRICE, BTB_F_CALLER, BTB_F_CALLEE, BTB_F_VALUE, BTB_F_INVALID, BTB_F_SIGN_HASH };

struct BtbArgs {
    const u64* txf;            // [n_txs][9][4]
    const u32* to_none;        // [n_txs]
    const u32* access;         // [n_txs][2]
    const uint8_t* calldata;   // [n_bytes], any alignment
    const u64* offs;           // [n_txs + 1] the session's copy of the checked offsets
    const u64* ids;            // [n_txs][4] the session's copy of the checked tx ids
    const u64* block;          // [8][4] (n_block_rows > 0)
    const u64* hashes;         // [n_hist][4] oldest first
    const u64* wd;             // [n_wd][4][4]
    const u64* wd_ids;         // [n_wd][4] the session's copy of the checked withdrawal ids
    u64 n_txs, n_bytes, n_tx_rows, n_hist, n_block_rows, n_wd;
    u64 number[4];             // the block number as checked at open
    u32 mis;                   // address of calldata & 15: piece c of the aligned space holds calldata[16 c - mis ..]
    u32 hist_rot;              // HistoryHash row r holds history_hashes[(r + hist_rot) % n_hist] (non-zero only when number - n_hist + j crosses p)
    const u32* wave_tx;        // device sessions: [ceil(10 n_tx_rows / 64)] the tx of the first row of every 64 pieces of the tx table (btb_wave_index)
    u64 n_gas_blocks;          // ceil((mis + n_bytes) / BTB_GAS_BLOCK)
    u32* gas_part;             // [n_gas_blocks] non-zero bytes per block
    u32* gas_pre;              // [n_gas_blocks + 1] exclusive prefix of gas_part
    u64* tx;   u32* tx_flags;  // out [n_tx_rows][5][4], [n_tx_rows]
    u64* blk;  u32* blk_flags; // out [n_block_rows][4][4], [n_block_rows]
    u64* wdt;                  // out [n_wd][4][4]
};

// FQ(v) of a 256-bit word: 2^256 / p < 6, at most five subtractions
ZK_HD Fr btb_reduce(Fr v) {
    const Fr p = fr_modulus();
#pragma unroll
    for (int k = 0; k < 5; k++) {
        Fr t;
        const u32 bw = u256_sub(t, v, p);
        if (!bw) v = t;
    }
    return v;
}
ZK_HD u64 btb_limb(const Fr& v, int k) { return (u64)v.v[2 * k] | ((u64)v.v[2 * k + 1] << 32); }
ZK_HD void btb_store_cell(u64* p, const Fr& v) {
#pragma unroll
    for (int k = 0; k < 4; k++) p[k] = btb_limb(v, k);
}
ZK_HD void btb_store_small(u64* p, u64 x) { p[0] = x; p[1] = 0; p[2] = 0; p[3] = 0; }

// ---- calldata gas -----------------------------------------------------------------------------------------------------------------
ZK_HD u32 btb_nonzero_bytes(u64 x) {
    const u64 m = 0x7f7f7f7f7f7f7f7full;
    return (u32)__builtin_popcountll((((x & m) + m) | x) & ~m);
}
// the bytes [s, e) of a little-endian 8-byte word, 0 <= s, e <= 8
ZK_HD u64 btb_byte_mask(u32 s, u32 e) {
    if (s >= e) return 0;
    const u32 n = e - s;
    return (n >= 8u ? ~0ull : ((1ull << (8u * n)) - 1ull)) << (8u * s);
}
// non-zero bytes of piece c of the aligned space inside [lo, hi) (positions of the aligned space: calldata index + mis; the caller
// keeps [lo, hi) inside [mis, mis + n_bytes)).  A piece that lies inside the buffer is one aligned 16-byte load.
ZK_HD u32 btb_gas_chunk(const BtbArgs& a, u64 c, u64 lo, u64 hi) {
    const u64 c0 = 16 * c, c1 = c0 + 16;
    const u64 s = lo > c0 ? lo : c0, e = hi < c1 ? hi : c1;
    if (s >= e) return 0;
    if (c0 >= a.mis && c1 <= a.mis + a.n_bytes) {
        const uint4 v = *(const uint4*)(a.calldata + (c0 - a.mis));
        const u64 w0 = (u64)v.x | ((u64)v.y << 32), w1 = (u64)v.z | ((u64)v.w << 32);
        const u32 s0 = (u32)(s - c0), e0 = (u32)(e - c0);  // 0..16
        const u64 m0 = btb_byte_mask(s0 < 8u ? s0 : 8u, e0 < 8u ? e0 : 8u);
        const u64 m1 = btb_byte_mask(s0 > 8u ? s0 - 8u : 0u, e0 > 8u ? e0 - 8u : 0u);
        return btb_nonzero_bytes(w0 & m0) + btb_nonzero_bytes(w1 & m1);
    }
    u32 n = 0;
    for (u64 x = s; x < e; x++) n += a.calldata[x - a.mis] ? 1u : 0u;
    return n;
}
ZK_HD u32 btb_gas_block(const BtbArgs& a, u64 b) {
    const u64 lo = a.mis, hi = a.mis + a.n_bytes;
    u32 n = 0;
    for (u64 c = b * BTB_GAS_PIECES; c < (b + 1) * BTB_GAS_PIECES; c++) n += btb_gas_chunk(a, c, lo, hi);
    return n;
}
ZK_HD void btb_gas_prefix(const BtbArgs& a) {
    u32 run = 0;
    for (u64 b = 0; b < a.n_gas_blocks; b++) { a.gas_pre[b] = run; run += a.gas_part[b]; }
    a.gas_pre[a.n_gas_blocks] = run;
}
ZK_HD u64 btb_range_nonzero(const BtbArgs& a, u64 o0, u64 o1) {
    if (o0 >= o1) return 0;
    const u64 lo = o0 + a.mis, hi = o1 + a.mis;
    const u64 b0 = (lo + BTB_GAS_BLOCK - 1) / BTB_GAS_BLOCK, b1 = hi / BTB_GAS_BLOCK;  // the whole blocks are [b0, b1)
    u64 n = 0;
    if (b0 >= b1) {
        for (u64 c = lo / 16; c <= (hi - 1) / 16; c++) n += btb_gas_chunk(a, c, lo, hi);
        return n;
    }
    n = (u64)(a.gas_pre[b1] - a.gas_pre[b0]);
    const u64 h = b0 * BTB_GAS_BLOCK, t = b1 * BTB_GAS_BLOCK;
    if (lo < h)
        for (u64 c = lo / 16; c <= (h - 1) / 16; c++) n += btb_gas_chunk(a, c, lo, h);
    if (t < hi)
        for (u64 c = t / 16; c <= (hi - 1) / 16; c++) n += btb_gas_chunk(a, c, t, hi);
    return n;
}

// ---- the tx table -----------------------------------------------------------------------------------------------------------------
ZK_HD u64 btb_tx_row0(const BtbArgs& a, u64 i) { return (u64)BTB_TX_FIXED * i + a.offs[i]; }
// the tx that owns row `row` < n_tx_rows: the largest i in [from, n_txs) with row0(i) <= row (the caller knows row0(from) <= row)
ZK_HD u64 btb_tx_of_row(const BtbArgs& a, u64 row, u64 from) {
    u64 lo = from, hi = a.n_txs;
    while (hi - lo > 1) {
        const u64 mid = lo + ((hi - lo) >> 1);
        if (btb_tx_row0(a, mid) <= row) lo = mid;
        else hi = mid;
    }
    return lo;
}
// is_word of fixed row t (tag t + 1): GasPrice, CallerAddress, CalleeAddress, Value
ZK_HD bool btb_tx_is_word(u64 t) { return t == 2 || t == 3 || t == 4 || t == 6; }
// (o0, o1 below: offsets[i], offsets[i + 1] of the row's tx i = btb_tx_of_row(row), loaded by the caller)
ZK_HD u32 btb_tx_flag(u64 i, u64 o0, u64 row) { return btb_tx_is_word(row - ((u64)BTB_TX_FIXED * i + o0)) ? 1u : 0u; }
// The two 64-bit words of piece q (0..9) of row `row` of tx i: the row is (tx_id, tag, index, value lo, value hi), a cell is two pieces.
ZK_HD void btb_tx_piece(const BtbArgs& a, u64 i, u64 o0, u64 o1, u64 row, u32 q, u64& w0, u64& w1) {
    const u64 t = row - ((u64)BTB_TX_FIXED * i + o0);
    const u32 cell = q >> 1, half = q & 1u;
    w0 = 0;
    w1 = 0;
    if (cell == 0) { w0 = a.ids[4 * i + 2 * half]; w1 = a.ids[4 * i + 2 * half + 1]; return; }
    if (cell == 1) { if (!half) w0 = t < BTB_TX_FIXED ? t + 1 : 13; return; }
    if (cell == 2) { if (!half && t >= BTB_TX_FIXED) w0 = t - BTB_TX_FIXED; return; }
    if (t >= BTB_TX_FIXED) { if (q == 6) w0 = a.calldata[o0 + (t - BTB_TX_FIXED)]; return; }
    const u64* f = a.txf + i * (BTB_NTX_FIELDS * 4);
    int fld = -1;
    bool word = false;
    switch ((u32)t + 1u) {
    case 1: fld = BTB_F_NONCE; break;
    case 2: fld = BTB_F_GAS; break;
    case 3: fld = BTB_F_GAS_PRICE; word = true; break;
    case 4: fld = BTB_F_CALLER; word = true; break;
    case 5: fld = BTB_F_CALLEE; word = true; break;
    case 7: fld = BTB_F_VALUE; word = true; break;
    case 10: fld = BTB_F_INVALID; break;
    case 12: fld = BTB_F_SIGN_HASH; break;
    default: break;
    }
    if (word) {  // Word(w): lo = w mod 2^128, hi = w >> 128
        if (!half) { const u64* w = f + 4 * fld + (cell == 3 ? 0 : 2); w0 = w[0]; w1 = w[1]; }
        return;
    }
    if (cell != 3) return;  // a value's hi cell is 0
    if (fld >= 0) {         // FQ(v)
        const Fr v = btb_reduce(fr_load(f + 4 * fld));
        w0 = half ? btb_limb(v, 2) : btb_limb(v, 0);  // (constant limb indices: the value stays in registers)
        w1 = half ? btb_limb(v, 3) : btb_limb(v, 1);
        return;
    }
    if (half) return;  // the remaining values fit 64 bits
    const u64 len = o1 - o0;
    switch ((u32)t + 1u) {
    case 6: w0 = a.to_none[i] ? 1 : 0; break;
    case 8: w0 = len; break;
    case 9: w0 = 4 * len + 12 * btb_range_nonzero(a, o0, o0 + len); break;
    case 11: w0 = 2400ull * a.access[2 * i] + 1900ull * a.access[2 * i + 1]; break;
    default: break;
    }
}

// ---- the block and withdrawal tables ------------------------------------------------------------------------------------------------
ZK_HD void btb_block_row(const BtbArgs& a, u64 r) {
    u64* o = a.blk + r * (BTB_BLOCK_NCELLS * 4);
    const u64 last = a.n_block_rows - 1;
    u64 tag, src;  // src: the block field, or the history hash
    bool word, hist = false;
    Fr number = fr_zero();
    if (r < 7) { tag = r + 1; src = r; word = r == 0 || r == 4 || r == 5; }          // Coinbase, PrevRandao, BaseFee are Words
    else if (r == last) { tag = 9; src = 7; word = false; }                           // WithdrawalRoot
    else {
        const u64 j = (r - 7 + a.hist_rot) % a.n_hist;
        tag = 8; src = j; word = true; hist = true;
        Fr d;
        Fr num;  // (limb by limb: a.number sits in the kernel's argument block)
        num.v[0] = (u32)a.number[0]; num.v[1] = (u32)(a.number[0] >> 32); num.v[2] = (u32)a.number[1]; num.v[3] = (u32)(a.number[1] >> 32);
        num.v[4] = (u32)a.number[2]; num.v[5] = (u32)(a.number[2] >> 32); num.v[6] = (u32)a.number[3]; num.v[7] = (u32)(a.number[3] >> 32);
        u256_sub(d, num, fr_from_u64(a.n_hist - j));                                  // number - n_hist + j >= 0 (checked at open)
        number = btb_reduce(d);
    }
    const u64* w = (hist ? a.hashes : a.block) + 4 * src;
    btb_store_small(o, tag);
    btb_store_cell(o + 4, number);
    if (word) {
        o[8] = w[0]; o[9] = w[1]; o[10] = 0; o[11] = 0;
        o[12] = w[2]; o[13] = w[3]; o[14] = 0; o[15] = 0;
    } else {
        btb_store_cell(o + 8, btb_reduce(fr_load(w)));
        btb_store_small(o + 12, 0);
    }
    a.blk_flags[r] = word ? 1u : 0u;
}
ZK_HD void btb_wd_row(const BtbArgs& a, u64 r) {
    u64* o = a.wdt + r * (BTB_WD_NCELLS * 4);
    o[0] = a.wd_ids[4 * r]; o[1] = a.wd_ids[4 * r + 1]; o[2] = a.wd_ids[4 * r + 2]; o[3] = a.wd_ids[4 * r + 3];
    for (int c = 1; c < BTB_WD_NCELLS; c++) btb_store_cell(o + 4 * c, btb_reduce(fr_load(a.wd + (r * BTB_WD_NCELLS + c) * 4)));
}

// The tx of the first row of every 64 pieces (a wavefront's KiB) of the tx table, from the checked offsets: one walk on the host at open
// (the offsets are fixed for the session).  out: [ceil(10 n_tx_rows / 64)]; entry w = btb_tx_of_row(64 w / 10).
static inline void btb_wave_index(const u64* offs, u64 n_txs, u64 n_tx_rows, u32* out) {
    const u64 n_waves = (n_tx_rows * BTB_TX_PIECES + 63) / 64;
    u64 i = 0;
    for (u64 w = 0; w < n_waves; w++) {
        const u64 row = 64 * w / BTB_TX_PIECES;
        while (i + 1 < n_txs && (u64)BTB_TX_FIXED * (i + 1) + offs[i + 1] <= row) i++;
        out[w] = (u32)i;
    }
}

// ---- the open's checks, on the host (both backends; a device caller's fields are read back once) -----------------------------------
struct BtbPlan {
    u64 n_bytes, n_tx_rows, n_block_rows, n_gas_blocks;
    u32 hist_rot;
};
static const u64 BTB_P64[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};
static inline bool btbh_lt(const u64* x, const u64* y) {
    for (int k = 3; k >= 0; k--)
        if (x[k] != y[k]) return x[k] < y[k];
    return false;
}
static inline void btbh_sub(u64* r, const u64* x, const u64* y) {
    u64 bw = 0;
    for (int k = 0; k < 4; k++) {
        const u64 d = x[k] - y[k], d2 = d - bw;
        bw = (x[k] < y[k]) || (d < bw) ? 1 : 0;
        r[k] = d2;
    }
}
// ids: the first cell of every `stride`-word record, canonical and strictly ascending
static inline long long btbh_bad_id(const u64* recs, u64 n, u64 stride) {
    for (u64 i = 0; i < n; i++) {
        if (!btbh_lt(recs + i * stride, BTB_P64)) return (long long)i;
        if (i && !btbh_lt(recs + (i - 1) * stride, recs + i * stride)) return (long long)i;
    }
    return -1;
}
// the counts that need no array (the 2^31 limits come first: nothing is read or allocated for a table that large)
static inline int btb_plan_counts(u64 n_txs, u64 n_hist, u64 n_wd, bool has_block, char* msg, size_t msg_len) {
    if (n_txs >= (1ull << 31) / BTB_TX_FIXED || n_wd >= (1ull << 31)) {
        snprintf(msg, msg_len, "zk_evm_tables_from_block: %llu txs, %llu withdrawals (a table of 2^31 rows or more)", (unsigned long long)n_txs, (unsigned long long)n_wd);
        return -63;
    }
    if (n_hist > (has_block ? (u64)BTB_MAX_HISTORY : 0ull)) {
        snprintf(msg, msg_len, has_block ? "zk_evm_tables_from_block: %llu history hashes (more than min(256, number))"
                                         : "zk_evm_tables_from_block: %llu history hashes without a block (more than min(256, number))", (unsigned long long)n_hist);
        return -62;
    }
    return 0;
}
// txf / offs / block / wd: HOST copies.  0, or the error code with its text in msg.
static inline int btb_plan(const u64* txf, const u64* offs, u64 n_txs, const u64* block, u64 n_hist, const u64* wd, u64 n_wd, u32 mis,
                           BtbPlan& z, char* msg, size_t msg_len) {
    int rc = btb_plan_counts(n_txs, n_hist, n_wd, block != nullptr, msg, msg_len);
    if (rc) return rc;
    if (offs[0] != 0) { snprintf(msg, msg_len, "zk_evm_tables_from_block: calldata_offsets must start at 0"); return -61; }
    for (u64 i = 0; i < n_txs; i++)
        if (offs[i] > offs[i + 1]) {
            snprintf(msg, msg_len, "zk_evm_tables_from_block: calldata_offsets must be non-decreasing (tx %llu)", (unsigned long long)i);
            return -61;
        }
    z.n_bytes = offs[n_txs];
    if (z.n_bytes >= (1ull << 31) || BTB_TX_FIXED * n_txs + z.n_bytes >= (1ull << 31)) {
        snprintf(msg, msg_len, "zk_evm_tables_from_block: %llu txs with %llu calldata bytes (a tx table of 2^31 rows or more)", (unsigned long long)n_txs,
                 (unsigned long long)z.n_bytes);
        return -63;
    }
    z.n_tx_rows = BTB_TX_FIXED * n_txs + z.n_bytes;
    long long bad = btbh_bad_id(txf, n_txs, BTB_NTX_FIELDS * 4);
    if (bad >= 0) {
        snprintf(msg, msg_len, "zk_evm_tables_from_block: the id of tx %lld is no canonical cell or does not exceed the id before it (tx ids must be strictly ascending)", bad);
        return -60;
    }
    bad = btbh_bad_id(wd, n_wd, BTB_WD_NCELLS * 4);
    if (bad >= 0) {
        snprintf(msg, msg_len, "zk_evm_tables_from_block: the id of withdrawal %lld is no canonical cell or does not exceed the id before it (withdrawal ids must be strictly ascending)", bad);
        return -60;
    }
    z.n_block_rows = block ? BTB_BLOCK_FIXED + n_hist : 0;
    z.hist_rot = 0;
    if (n_hist) {
        const u64* number = block + 4 * 2;
        const u64 nh[4] = {n_hist, 0, 0, 0};
        if (btbh_lt(number, nh)) {
            snprintf(msg, msg_len, "zk_evm_tables_from_block: %llu history hashes (more than min(256, number))", (unsigned long long)n_hist);
            return -62;
        }
        // the number cells FQ(number - n_hist + j) ascend with j unless they cross a multiple of p: the rows from that j on come first
        u64 r0[4], d[4];
        btbh_sub(r0, number, nh);
        for (int k = 0; k < 5; k++)
            if (!btbh_lt(r0, BTB_P64)) btbh_sub(r0, r0, BTB_P64);
        btbh_sub(d, BTB_P64, r0);  // the first j whose cell is 0, when below n_hist
        if (btbh_lt(d, nh)) z.hist_rot = (u32)d[0];
    }
    z.n_gas_blocks = z.n_bytes ? (mis + z.n_bytes + BTB_GAS_BLOCK - 1) / BTB_GAS_BLOCK : 0;
    return 0;
}
