// PI-circuit witness assignment on the device.
//
// Replaces the reference's `public_data2witness(public_data, MAX_TXS, MAX_CALLDATA_BYTES, MAX_WITHDRAWALS)`
// (src/zkevm_specs/pi_circuit.py:839-1073): from a block header, its transactions and withdrawals to the 24-cell rows
// zk_pi_open takes, the calldata gas-cost table, the keccak table, the copy-constraint wire zk_pi_copy_open takes and the small
// tables of the Python Witness.
//
// The reference lists the raw public inputs as byte strings ("values", each at most 20 bytes), walks them last to first while
// walking each value's bytes first to last, and reverses the rows.  So row i holds byte i of the layout
//   [0] block table values (8,341 B) | block hash, state root, previous state root (96 B) | tx table: an empty row (17 B) and
//   336 B per tx slot | MAX_CALLDATA_BYTES calldata bytes | 56 B per withdrawal slot
// with the bytes of every value in REVERSE (row start + p of a value holds byte p of the value read as a little-endian integer),
// q_rpi_value_start on the value's last row, and two suffix recurrences over the rows: rpi_bytes_keccakrlc over all of them,
// rpi_value_lc restarted per value.  Independently of the byte it holds, row i also carries row i of the tx table
// (i < 10 MAX_TXS + 1 + MAX_CALLDATA_BYTES), then row i - that bound of the withdrawal table, and entry i < 268 of the block table:
// the reference's own alignment.
//
// Passes (one lane per item unless noted; k_pi_assign.hip on the device, plain loops in cpu_backend.cpp):
//   pia_check        open: a field wider than its to_bytes width, calldata offsets that decrease
//   gas scan         the calldata gas cost (4 / 16 per byte) as a prefix sum: per tile, then over the tile totals
//   pia_tx_inverse   value.lo^-1 of the 10 MAX_TXS fixed tx-table rows (Fermat); k^-1 for small k is a table built at open
//   pia_row_byte     the byte of row i into a buffer in the reference's generation order (rows n - 1 down to 0): the sponge's input
//   keccak           the existing long-message kernel over that buffer: digest, input RLC, length
//   suffix RLC       per slice of 8 rows and tile of 2,048 rows, then over the tile totals; the row lane finishes its own cell
//   pia_write_row    24 cells column-major, the row's table rows and the constraints / raw bytes of the value it belongs to
//   pia_patch        what depends on the digest: row 0's digest word, the keccak table, the public inputs, constraints 0 and 1
#pragma once
#include <stdio.h>
#include "common.hpp"
#include "exp_assign.hpp"
#include "keccak_table.hpp"
#include "pi_circuit.hpp"

enum { PIA_BLOCK_ENTRIES = 268, PIA_BLOCK_COLUMN = 265, PIA_BLOCK_BYTES = 8437, PIA_BLOCK_VALUES = 530, PIA_TX_LEN = 10, PIA_TX_BYTES = 336,
       PIA_TX_VALUES = 33, PIA_TX0_BYTES = 17, PIA_WD_BYTES = 56, PIA_CC_TX0 = 538, PIA_TAG_CALLDATA = 13, PIA_TAG_CDL = 8,
       PIA_SLICE = 8, PIA_TILE = 2048, PIA_GAS_LANE = 16, PIA_GAS_TILE = 4096, PIA_NBLOCK_FIELDS = 9, PIA_NTX_FIELDS = 7, PIA_NWD_FIELDS = 4 };
#define PIA_NO_REJECT (~0ull)

struct PiaArgs {
    // inputs (zk_pi_inputs)
    u64 chain_id;
    const u64* block;         // [9][4]  hash, coinbase, state_root, prev_randao, number, gas_limit, time, base_fee, withdrawals_root
    const u64* srp;           // [4]     state_root_prev
    const u64* hashes;        // [256][4]
    const u64* txf;           // [n_txs][7][4]  nonce, gas_price, gas, from_addr, to_addr, value, tx_sign_hash
    const u32* to_none;       // [n_txs]
    const uint8_t* calldata;  // [total_cd]
    const u64* offs;          // [n_txs + 1]
    const u64* wd;            // [n_wd][4][4]  id, validator_id, address, amount
    u64 n_txs, n_wd, max_txs, max_cd, max_wd, total_cd;
    // layout
    u64 n, tx_len, cd0, wd0, n_values, n_cc, n_tiles, n_gas_tiles, n_inv;
    Fr rand, base;            // keccak_rand, byte_pow_base (canonical; the lanes convert: one product)
    // work buffers
    u64* meta;                // [1]  min over rejected fields of their index, or PIA_NO_REJECT
    u32* gas_local;           // [total_cd]       inclusive prefix of the gas cost inside the byte's tile
    u64* gas_tile;            // [n_gas_tiles]    tile totals, then their exclusive prefix
    u64* inv_small;           // [n_inv][4]       k^-1, canonical (0 for k = 0)
    u64* inv_txlo;            // [10 max_txs][4]  value.lo^-1 of the fixed tx-table rows
    uint8_t* gen;             // [n]              the bytes in generation order: gen[n - 1 - i] = byte of row i
    u64* rpow;                // [PIA_TILE + 1][4]  keccak_rand^k in Montgomery form
    u64* slice_acc;           // [n_tiles * 256][4] suffix RLC of the slice's rows to the end of its tile
    u64* tile_acc;            // [n_tiles][4]       the same of the whole tile
    u64* carry;               // [n_tiles + 1][4]   rpi_bytes_keccakrlc of the tile's first row
    u64* krow;                // [5][4]             the keccak kernel's row: 2, input RLC, length, digest as a big-endian integer lo / hi
    // outputs (zk_pi_wire)
    u64* rows; u64* gas; u64* keccak;
    u64* cc_cells; uint8_t* cc_bytes; u32* cc_lens;
    u64* block_table; u32* block_flags;
    u64* tx_table; u32* tx_flags;
    u64* wd_table;
    u64* public_inputs;
    uint8_t* raw_bytes; u32* raw_lens;
};

// ---- host side of both backends: the layout's sizes from the three maxima
struct PiaSizes {
    u64 n, n_gas, n_cc, n_values, tx_table_rows;
};
// -> 0 or the error code of include/zkevm_hip.h with its text in `msg`
static inline int pia_sizes_of(u64 n_txs, u64 n_wd, u64 total_cd, u64 max_txs, u64 max_cd, u64 max_wd, PiaSizes& z, char* msg, size_t msg_len) {
    if (n_txs == 0 || n_txs > max_txs) {
        snprintf(msg, msg_len, "zk_pi_assign: %llu txs (at least one, at most MAX_TXS = %llu)", (unsigned long long)n_txs, (unsigned long long)max_txs);
        return -50;
    }
    if (n_wd == 0 || n_wd > max_wd) {
        snprintf(msg, msg_len, "zk_pi_assign: %llu withdrawals (at least one, at most MAX_WITHDRAWALS = %llu)", (unsigned long long)n_wd, (unsigned long long)max_wd);
        return -51;
    }
    if (total_cd > max_cd) {
        snprintf(msg, msg_len, "zk_pi_assign: %llu calldata bytes exceed MAX_CALLDATA_BYTES = %llu", (unsigned long long)total_cd, (unsigned long long)max_cd);
        return -52;
    }
    const u64 lim = 1ull << 31;
    if (max_txs >= lim / PIA_TX_BYTES || max_cd >= lim || max_wd >= lim / PIA_WD_BYTES) {
        snprintf(msg, msg_len, "zk_pi_assign: 2^31 rows or more");
        return -54;
    }
    z.tx_table_rows = PIA_TX_LEN * max_txs + 1 + max_cd;
    z.n = PIA_BLOCK_BYTES + PIA_TX0_BYTES + PIA_TX_BYTES * max_txs + max_cd + PIA_WD_BYTES * max_wd;
    z.n_gas = 1 + total_cd;
    z.n_values = PIA_BLOCK_VALUES + 3 + PIA_TX_VALUES * max_txs + max_cd + 5 * max_wd;
    z.n_cc = PIA_CC_TX0 + 4 * (PIA_TX_LEN * max_txs + 1) + 2 * max_cd + 5 * max_wd;
    if (z.n >= lim) {
        snprintf(msg, msg_len, "zk_pi_assign: %llu rows (2^31 or more)", (unsigned long long)z.n);
        return -54;
    }
    return 0;
}
static inline void pia_set_layout(PiaArgs& a, const PiaSizes& z) {
    a.n = z.n;
    a.tx_len = PIA_TX_LEN * a.max_txs + 1;
    a.cd0 = PIA_BLOCK_BYTES + PIA_TX0_BYTES + PIA_TX_BYTES * a.max_txs;
    a.wd0 = a.cd0 + a.max_cd;
    a.n_values = z.n_values;
    a.n_cc = z.n_cc;
    a.n_tiles = (z.n + PIA_TILE - 1) / PIA_TILE;
    a.n_gas_tiles = (a.total_cd + PIA_GAS_TILE - 1) / PIA_GAS_TILE;
    a.n_inv = (a.max_txs > 255 ? a.max_txs : 255) + 1;
}
static inline int pia_reject_text(u64 reject, char* msg, size_t msg_len) {
    snprintf(msg, msg_len, "zk_pi_assign: input field %llu is wider than the bytes the circuit gives it (block fields first, then 7 per tx, "
             "then 4 per withdrawal, then the calldata offsets)", (unsigned long long)reject);
    return -53;
}

ZK_HD void pia_store4(u64* out, u64 w0, u64 w1, u64 w2, u64 w3) {
    u64* o = (u64*)__builtin_assume_aligned(out, 32);
    o[0] = w0; o[1] = w1; o[2] = w2; o[3] = w3;
}
ZK_HD void pia_store_fr(u64* out, const Fr& x) {
    pia_store4(out, (u64)x.v[0] | ((u64)x.v[1] << 32), (u64)x.v[2] | ((u64)x.v[3] << 32), (u64)x.v[4] | ((u64)x.v[5] << 32), (u64)x.v[6] | ((u64)x.v[7] << 32));
}
ZK_HD Fr pia_fr(const u64 w[4]) {
    Fr r;
#pragma unroll
    for (int k = 0; k < 4; k++) { r.v[2 * k] = (u32)w[k]; r.v[2 * k + 1] = (u32)(w[k] >> 32); }
    return r;
}
// byte p (p < 24) of a little-endian integer held in registers: the limb is selected, never indexed
ZK_HD u32 pia_byte_of(const u64 w[4], u32 p) {
    const u32 k = p >> 3;
    const u64 x = k == 0 ? w[0] : (k == 1 ? w[1] : (k == 2 ? w[2] : w[3]));
    return (u32)(x >> (8u * (p & 7u))) & 0xffu;
}
// Mont(b^e) from Mont(b)
ZK_HD Fr pia_pow_mont(Fr bM, u64 e) {
    Fr acc = frm_one();
    while (e) {
        if (e & 1ull) acc = fr_mont(acc, bM);
        bM = fr_mont(bM, bM);
        e >>= 1;
    }
    return acc;
}

// ---- open: the domain of the inputs.  Item idx: 9 block fields, 7 per tx, 4 per withdrawal, then one per tx for its offsets.
ZK_HD bool pia_fits(const u64* w, u32 bits) {
    if (bits == 64u) return (w[1] | w[2] | w[3]) == 0ull;
    if (bits == 160u) return w[3] == 0ull && (w[2] >> 32) == 0ull;
    return true;
}
#define PIA_N_CHECKS(a) ((u64)PIA_NBLOCK_FIELDS + PIA_NTX_FIELDS * (a).n_txs + PIA_NWD_FIELDS * (a).n_wd + (a).n_txs)
ZK_HD bool pia_check(const PiaArgs& a, u64 idx) {
    if (idx < PIA_NBLOCK_FIELDS) {
        const u32 bits = idx == 1 ? 160u : ((idx == 4 || idx == 5 || idx == 6) ? 64u : 256u);
        return pia_fits(a.block + 4 * idx, bits);
    }
    idx -= PIA_NBLOCK_FIELDS;
    if (idx < PIA_NTX_FIELDS * a.n_txs) {
        const u32 f = (u32)(idx % PIA_NTX_FIELDS);
        const u32 bits = (f == 0 || f == 2) ? 64u : ((f == 3 || f == 4) ? 160u : 256u);
        return pia_fits(a.txf + 4 * idx, bits);
    }
    idx -= PIA_NTX_FIELDS * a.n_txs;
    if (idx < PIA_NWD_FIELDS * a.n_wd) {
        const u32 f = (u32)(idx % PIA_NWD_FIELDS);
        if (f == 0) return !fr_geq_p(fr_load(a.wd + 4 * idx));  // the table's FQ(withdrawal.id): a canonical cell
        return pia_fits(a.wd + 4 * idx, f == 2 ? 256u : 64u);
    }
    idx -= PIA_NWD_FIELDS * a.n_wd;
    return a.offs[idx] <= a.offs[idx + 1] && (idx != 0 || a.offs[0] == 0ull) && a.offs[idx + 1] <= a.total_cd;
}

// ---- calldata gas: G(c) = the cost of bytes [0, c)
ZK_HD u64 pia_gas_before(const PiaArgs& a, u64 c) { return c == 0 ? 0ull : a.gas_tile[(c - 1) / PIA_GAS_TILE] + a.gas_local[c - 1]; }
// the tx that owns calldata byte c < total_cd: the last one whose first byte is at or below c (a tx without data never is)
ZK_HD u64 pia_tx_of_byte(const PiaArgs& a, u64 c) {
    u64 lo = 0, hi = a.n_txs;
    while (hi - lo > 1) {
        const u64 mid = (lo + hi) >> 1;
        if (a.offs[mid] <= c) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- the values.  A value is an integer of `len` bytes; its row start + p holds byte p (little-endian).
// entry j of the block table's value column (the 265 of block_table_value_column, then block hash, state root, previous state root)
ZK_HD u32 pia_block_entry(const PiaArgs& a, u32 j, u64 w[4]) {  // -> bytes: 1, 8, 20 or 32 (a Word)
    const u64* src = nullptr;
    u32 len = 32;
    if (j >= 9u && j < (u32)PIA_BLOCK_COLUMN) src = a.hashes + 4 * (u64)(j - 9u);
    else if (j == 1u) { src = a.block + 4 * 1; len = 20; }
    else if (j == 2u) { src = a.block + 4 * 5; len = 8; }
    else if (j == 3u) { src = a.block + 4 * 4; len = 8; }
    else if (j == 4u) { src = a.block + 4 * 6; len = 8; }
    else if (j == 5u) src = a.block + 4 * 3;
    else if (j == 6u) src = a.block + 4 * 7;
    else if (j == 8u) src = a.block + 4 * 8;
    else if (j == 265u) src = a.block + 4 * 0;
    else if (j == 266u) src = a.block + 4 * 2;
    else if (j == 267u) src = a.srp;
    if (src) { w[0] = src[0]; w[1] = src[1]; w[2] = src[2]; w[3] = src[3]; return len; }
    w[0] = j == 7u ? a.chain_id : 0ull; w[1] = w[2] = w[3] = 0ull;
    return j == 7u ? 8u : 1u;
}
// field f (tag f + 1) of tx slot t: Nonce, Gas, GasPrice, CallerAddress, CalleeAddress, IsCreate, Value, CallDataLength, CallDataGasCost,
// TxSignHash; slots from n_txs on hold Transaction.default() (to_addr 0, not None)
ZK_HD u32 pia_tx_field(const PiaArgs& a, u64 t, u32 f, u64 w[4]) {  // -> bytes: 8, 20 or 32 (a Word)
    const u32 len = (f == 2u || f == 6u || f == 9u) ? 32u : ((f == 3u || f == 4u) ? 20u : 8u);
    w[0] = w[1] = w[2] = w[3] = 0ull;
    if (t >= a.n_txs) return len;
    const u64* tx = a.txf + t * PIA_NTX_FIELDS * 4;
    const bool none = a.to_none[t] != 0u;
    const u64* src = nullptr;
    if (f == 0u) src = tx + 0;
    else if (f == 1u) src = tx + 8;
    else if (f == 2u) src = tx + 4;
    else if (f == 3u) src = tx + 12;
    else if (f == 4u) src = none ? nullptr : tx + 16;
    else if (f == 6u) src = tx + 20;
    else if (f == 9u) src = tx + 24;
    if (src) { w[0] = src[0]; w[1] = src[1]; w[2] = src[2]; w[3] = src[3]; }
    else if (f == 5u) w[0] = none ? 1ull : 0ull;
    else if (f == 7u) w[0] = a.offs[t + 1] - a.offs[t];
    else if (f == 8u) w[0] = pia_gas_before(a, a.offs[t + 1]) - pia_gas_before(a, a.offs[t]);
    return len;
}

struct PiaValue {
    u64 start;     // its first row
    u32 len;       // bytes
    u32 empty_hi;  // the constraint behind its own is the (0, b"") of a value that is no Word
    u64 vidx;      // its index in copy_constrains
    u64 cc;        // the index of its constraint
    u64 w[4];      // the integer
    u64 cell[4];   // the table cell its constraint compares with (the integer itself but for the withdrawal id)
};
// lo / hi half of a Word at byte `at` of its 32
ZK_HD void pia_half(PiaValue& v, u32 hi) {
    if (hi) { v.w[0] = v.w[2]; v.w[1] = v.w[3]; }
    v.w[2] = v.w[3] = 0ull;
}
// one value of `vlen` bytes (a Word: two of 16) that starts at byte `at` of its group; u = the row's offset in the group
ZK_HD void pia_place(PiaValue& v, u64 group_start, u32 at, u32 vlen, u32 u, u64 vidx, u64 cc) {
    v.empty_hi = 0;
    if (vlen == 32u) {
        const u32 hi = u >= at + 16u ? 1u : 0u;
        pia_half(v, hi);
        v.start = group_start + at + 16u * hi; v.len = 16; v.vidx = vidx + hi; v.cc = cc + hi;
    } else {
        v.start = group_start + at; v.len = vlen; v.vidx = vidx; v.cc = cc; v.empty_hi = 1;
    }
}
ZK_HD void pia_value(const PiaArgs& a, u64 i, PiaValue& v) {
    if (i < (u64)PIA_BLOCK_BYTES) {
        const u32 o = (u32)i;
        u32 j, s0, vi;
        if (o >= 149u) { j = 9u + (o - 149u) / 32u; s0 = 149u + 32u * (j - 9u); vi = 12u + 2u * (j - 9u); }
        else if (o >= 117u) { j = 8; s0 = 117; vi = 10; }
        else if (o >= 109u) { j = 7; s0 = 109; vi = 9; }
        else if (o >= 77u) { j = 6; s0 = 77; vi = 7; }
        else if (o >= 45u) { j = 5; s0 = 45; vi = 5; }
        else if (o >= 37u) { j = 4; s0 = 37; vi = 4; }
        else if (o >= 29u) { j = 3; s0 = 29; vi = 3; }
        else if (o >= 21u) { j = 2; s0 = 21; vi = 2; }
        else if (o >= 1u) { j = 1; s0 = 1; vi = 1; }
        else { j = 0; s0 = 0; vi = 0; }
        const u32 len = pia_block_entry(a, j, v.w);
        pia_place(v, s0, 0, len, o - s0, vi, 2ull + 2ull * j);
    } else if (i < a.cd0) {
        const u64 o = i - PIA_BLOCK_BYTES;
        if (o < (u64)PIA_TX0_BYTES) {  // the tx table's empty row: id, index, value lo
            const u32 k = o < 8u ? 0u : (o < 16u ? 1u : 2u);
            v.w[0] = v.w[1] = v.w[2] = v.w[3] = 0ull;
            v.start = PIA_BLOCK_BYTES + 8u * k; v.len = k == 2u ? 1u : 8u; v.vidx = PIA_BLOCK_VALUES + k; v.cc = PIA_CC_TX0 + k; v.empty_hi = k == 2u;
        } else {
            const u64 t = (o - PIA_TX0_BYTES) / PIA_TX_BYTES;
            const u32 q = (u32)((o - PIA_TX0_BYTES) % PIA_TX_BYTES);
            // the ten fields: 16 bytes of (tx_id, index) and the value
            const u32 f = q >= 288u ? 9u : (q >= 264u ? 8u : (q >= 240u ? 7u : (q >= 192u ? 6u : (q >= 168u ? 5u : (q >= 132u ? 4u : (q >= 96u ? 3u : (q >= 48u ? 2u : (q >= 24u ? 1u : 0u))))))));
            const u32 foff = f == 9u ? 288u : (f == 8u ? 264u : (f == 7u ? 240u : (f == 6u ? 192u : (f == 5u ? 168u : (f == 4u ? 132u : (f == 3u ? 96u : (f == 2u ? 48u : (f == 1u ? 24u : 0u))))))));
            const u32 fv = f == 9u ? 29u : (f == 8u ? 26u : (f == 7u ? 23u : (f == 6u ? 19u : (f == 5u ? 16u : (f == 4u ? 13u : (f == 3u ? 10u : (f == 2u ? 6u : (f == 1u ? 3u : 0u))))))));
            const u32 u = q - foff;
            const u64 g0 = PIA_BLOCK_BYTES + PIA_TX0_BYTES + t * PIA_TX_BYTES + foff;
            const u64 vi = PIA_BLOCK_VALUES + 3 + t * PIA_TX_VALUES + fv, cc = PIA_CC_TX0 + 4ull * (1 + PIA_TX_LEN * t + f);
            if (u < 16u) {
                const u32 k = u >> 3;
                v.w[0] = k ? 0ull : t + 1; v.w[1] = v.w[2] = v.w[3] = 0ull;
                v.start = g0 + 8u * k; v.len = 8; v.vidx = vi + k; v.cc = cc + k; v.empty_hi = 0;
            } else {
                const u32 len = pia_tx_field(a, t, f, v.w);
                pia_place(v, g0, 16, len, u, vi + 2, cc + 2);
            }
        }
    } else if (i < a.wd0) {
        const u64 c = i - a.cd0;
        v.w[0] = c < a.total_cd ? (u64)a.calldata[c] : 0ull; v.w[1] = v.w[2] = v.w[3] = 0ull;
        v.start = i; v.len = 1; v.vidx = PIA_BLOCK_VALUES + 3 + PIA_TX_VALUES * a.max_txs + c; v.cc = PIA_CC_TX0 + 4 * a.tx_len + 2 * c; v.empty_hi = 1;
    } else {
        const u64 j = (i - a.wd0) / PIA_WD_BYTES;
        const u32 u = (u32)((i - a.wd0) % PIA_WD_BYTES);
        const u32 k = u >= 48u ? 4u : (u >= 32u ? 3u : (u >= 16u ? 2u : (u >= 8u ? 1u : 0u)));
        const u64* src = j < a.n_wd ? a.wd + j * PIA_NWD_FIELDS * 4 : nullptr;
        v.w[0] = v.w[1] = v.w[2] = v.w[3] = 0ull;
        if (k == 0u) v.w[0] = j;  // withdrawal_raw_bytes(i): the loop index, whatever withdrawal.id says
        else if (src && k == 1u) v.w[0] = src[4];
        else if (src && k == 2u) { v.w[0] = src[8]; v.w[1] = src[9]; }
        else if (src && k == 3u) { v.w[0] = src[10]; v.w[1] = src[11]; }
        else if (src && k == 4u) v.w[0] = src[12];
        v.start = a.wd0 + j * PIA_WD_BYTES + (k == 0u ? 0u : (k == 1u ? 8u : (k == 2u ? 16u : (k == 3u ? 32u : 48u))));
        v.len = (k == 2u || k == 3u) ? 16u : 8u;
        v.vidx = PIA_BLOCK_VALUES + 3 + PIA_TX_VALUES * a.max_txs + a.max_cd + 5 * j + k;
        v.cc = PIA_CC_TX0 + 4 * a.tx_len + 2 * a.max_cd + 5 * j + k;
        v.empty_hi = 0;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) v.cell[k] = v.w[k];
    if (i >= a.wd0) {
        const u64 j = (i - a.wd0) / PIA_WD_BYTES;
        if (v.start == a.wd0 + j * PIA_WD_BYTES) {  // the id: the table holds withdrawal.id
#pragma unroll
            for (int k = 0; k < 4; k++) v.cell[k] = j < a.n_wd ? a.wd[j * PIA_NWD_FIELDS * 4 + k] : 0ull;
        }
    }
}
// the byte of row i, also into the generation-order buffer
ZK_HD void pia_row_byte(const PiaArgs& a, u64 i) {
    PiaValue v;
    pia_value(a, i, v);
    a.gen[a.n - 1 - i] = (uint8_t)pia_byte_of(v.w, (u32)(i - v.start));
}
ZK_HD u32 pia_byte_at(const PiaArgs& a, u64 i) { return i < a.n ? (u32)a.gen[a.n - 1 - i] : 0u; }

// ---- inverses
ZK_HD void pia_small_inverse(const PiaArgs& a, u64 k) { pia_store_fr(a.inv_small + 4 * k, fr_inv(fr_from_u64(k))); }
// value.lo of the fixed tx-table row 1 + r
ZK_HD Fr pia_tx_value_lo(const PiaArgs& a, u64 r) {
    u64 w[4];
    const u32 len = pia_tx_field(a, r / PIA_TX_LEN, (u32)(r % PIA_TX_LEN), w);
    if (len == 32u) w[2] = w[3] = 0ull;
    return pia_fr(w);
}
ZK_HD void pia_tx_inverse(const PiaArgs& a, u64 r) { pia_store_fr(a.inv_txlo + 4 * r, fr_inv(pia_tx_value_lo(a, r))); }

// ---- suffix RLC.  sum of byte[k] * rand^(k - lo) over rows [lo, hi): Horner from the top
ZK_HD Fr pia_horner(const PiaArgs& a, u64 lo, u64 hi) {
    const Fr rand_m = fr_to_mont(a.rand);
    Fr h = fr_zero();
    for (u64 k = hi; k-- > lo;) h = fr_add_u64(fr_mulc(h, rand_m), pia_byte_at(a, k));
    return h;
}
// rpi_bytes_keccakrlc of row i from the slice / tile accumulators
ZK_HD Fr pia_rlc_at(const PiaArgs& a, u64 i) {
    const u64 s = i / PIA_SLICE, tile = i / PIA_TILE;
    const u64 slice_end = (s + 1) * PIA_SLICE, tile_end = (tile + 1) * PIA_TILE;
    Fr next = fr_mulc(fr_load(a.carry + 4 * (tile + 1)), fr_load(a.rpow + 4 * (tile_end - slice_end)));  // of the row behind the slice
    if (slice_end < tile_end) next = fr_add(next, fr_load(a.slice_acc + 4 * (s + 1)));
    return fr_add(pia_horner(a, i, slice_end), fr_mulc(next, fr_load(a.rpow + 4 * (slice_end - i))));
}

// ---- one output row
ZK_HD void pia_write_row(const PiaArgs& a, u64 i) {
    const u64 n = a.n;
    PiaValue v;
    pia_value(a, i, v);
    const u32 p = (u32)(i - v.start);
    const u32 byte = pia_byte_of(v.w, p);
    // rpi_value_lc: the value's bytes from its last row down to this one
    const Fr base_m = fr_to_mont(a.base);
    Fr lc = fr_zero();
    for (u32 q = v.len; q-- > p;) lc = fr_add_u64(fr_mulc(lc, base_m), pia_byte_of(v.w, q));
    const Fr rlc = pia_rlc_at(a, i);
    // the tx-table row, or the withdrawal-table row, that rides on row i
    const u64 txc_len = a.tx_len + a.max_cd;
    u64 tx_id = 0, tag = 0, index = 0, gas_cost = 0, is_final = 0, lo[4] = {0, 0, 0, 0}, hi[4] = {0, 0, 0, 0};
    u32 is_word = 0;
    Fr id_inv = fr_zero(), lo_inv = fr_zero(), diff_inv = fr_zero();
    const bool q_tx = i < a.tx_len, q_cd = !q_tx && i < txc_len, q_wd = i >= txc_len && i < txc_len + a.max_wd;
    if (q_tx && i > 0) {
        const u64 r = i - 1, t = r / PIA_TX_LEN;
        const u32 f = (u32)(r % PIA_TX_LEN);
        tx_id = t + 1; tag = f + 1;
        is_word = pia_tx_field(a, t, f, lo) == 32u;
        if (is_word) { hi[0] = lo[2]; hi[1] = lo[3]; lo[2] = lo[3] = 0ull; }
        lo_inv = fr_load(a.inv_txlo + 4 * r);
    }
    if (q_tx) {  // (tag - CallDataLength)^-1, tag 0 on the empty row
        const Fr inv = fr_load(a.inv_small + 4 * (tag >= (u64)PIA_TAG_CDL ? tag - PIA_TAG_CDL : PIA_TAG_CDL - tag));
        id_inv = tag >= (u64)PIA_TAG_CDL ? inv : fr_neg(inv);
    }
    if (q_cd) {
        const u64 c = i - a.tx_len;
        tag = PIA_TAG_CALLDATA;
        if (c < a.total_cd) {
            const u64 t = pia_tx_of_byte(a, c);
            tx_id = t + 1; index = c - a.offs[t]; lo[0] = a.calldata[c];
            is_final = c + 1 == a.offs[t + 1];
            gas_cost = pia_gas_before(a, c + 1) - pia_gas_before(a, a.offs[t]);
            id_inv = fr_load(a.inv_small + 4 * tx_id);
            lo_inv = fr_load(a.inv_small + 4 * lo[0]);
            if (c + 1 == a.total_cd) diff_inv = fr_neg(id_inv);               // tx_id_next = 0 behind the last byte
            else if (is_final) diff_inv = fr_load(a.inv_small + 4 * (pia_tx_of_byte(a, c + 1) - t));
        }
    }
    u64 wd_id[4] = {0, 0, 0, 0}, wd_amount = 0;
    if (q_wd) {
        const u64 j = i - txc_len;
        u64* t = a.wd_table + j * 5 * 4;
        const u64* src = a.wd + j * PIA_NWD_FIELDS * 4;
        if (j < a.n_wd) {
#pragma unroll
            for (int k = 0; k < 4; k++) wd_id[k] = src[k];
            wd_amount = src[12];
            pia_store4(t + 4, src[4], 0, 0, 0);
            pia_store4(t + 8, src[8], src[9], 0, 0);
            pia_store4(t + 12, src[10], src[11], 0, 0);
        } else {
            pia_store4(t + 4, 0, 0, 0, 0);
            pia_store4(t + 8, 0, 0, 0, 0);
            pia_store4(t + 12, 0, 0, 0, 0);
        }
        pia_store4(t + 0, wd_id[0], wd_id[1], wd_id[2], wd_id[3]);
        pia_store4(t + 16, wd_amount, 0, 0, 0);
    }
#define PIA_OUT(c) (a.rows + ((u64)(c) * n + i) * 4)
    pia_store4(PIA_OUT(PI_Q_BYTES_LAST), i + 1 == n, 0, 0, 0);
    pia_store4(PIA_OUT(PI_Q_TX_TABLE), q_tx, 0, 0, 0);
    pia_store4(PIA_OUT(PI_Q_TX_CALLDATA), q_cd, 0, 0, 0);
    pia_store4(PIA_OUT(PI_Q_TX_CALLDATA_START), i == a.tx_len && a.max_cd > 0, 0, 0, 0);
    pia_store4(PIA_OUT(PI_Q_KECCAK), i == 0, 0, 0, 0);
    pia_store4(PIA_OUT(PI_Q_VALUE_START), p + 1u == v.len, 0, 0, 0);
    pia_store_fr(PIA_OUT(PI_TX_ID_INV), id_inv);
    pia_store_fr(PIA_OUT(PI_TX_LO_INV), lo_inv);
    pia_store_fr(PIA_OUT(PI_TX_DIFF_INV), diff_inv);
    pia_store4(PIA_OUT(PI_GAS_COST), gas_cost, 0, 0, 0);
    pia_store4(PIA_OUT(PI_IS_FINAL), is_final, 0, 0, 0);
    pia_store4(PIA_OUT(PI_Q_WD), q_wd, 0, 0, 0);
    pia_store4(PIA_OUT(PI_RPI_BYTES), byte, 0, 0, 0);
    pia_store_fr(PIA_OUT(PI_RPI_RLC), rlc);
    pia_store_fr(PIA_OUT(PI_RPI_LC), lc);
    pia_store4(PIA_OUT(PI_DIGEST_LO), 0, 0, 0, 0);  // (row 0: pia_patch)
    pia_store4(PIA_OUT(PI_DIGEST_HI), 0, 0, 0, 0);
    pia_store4(PIA_OUT(PI_Q_BYTE_EN), 1, 0, 0, 0);
    pia_store4(PIA_OUT(PI_TX_ID), tx_id, 0, 0, 0);
    pia_store4(PIA_OUT(PI_TX_TAG), tag, 0, 0, 0);
    pia_store4(PIA_OUT(PI_TX_INDEX), index, 0, 0, 0);
    pia_store4(PIA_OUT(PI_TX_LO), lo[0], lo[1], lo[2], lo[3]);
    pia_store4(PIA_OUT(PI_WD_ID), wd_id[0], wd_id[1], wd_id[2], wd_id[3]);
    pia_store4(PIA_OUT(PI_WD_AMOUNT), wd_amount, 0, 0, 0);
#undef PIA_OUT
    if (i < txc_len) {
        u64* t = a.tx_table + i * 5 * 4;
        pia_store4(t + 0, tx_id, 0, 0, 0);
        pia_store4(t + 4, tag, 0, 0, 0);
        pia_store4(t + 8, index, 0, 0, 0);
        pia_store4(t + 12, lo[0], lo[1], lo[2], lo[3]);
        pia_store4(t + 16, hi[0], hi[1], 0, 0);
        a.tx_flags[i] = is_word;
    }
    if (q_cd && i - a.tx_len < a.total_cd) {
        u64* g = a.gas + (1 + i - a.tx_len) * PI_GAS_NCELLS * 4;
        pia_store4(g + 0, tx_id, 0, 0, 0);
        pia_store4(g + 4, is_final, 0, 0, 0);
        pia_store4(g + 8, gas_cost, 0, 0, 0);
    }
    if (i == 0) {  // the (0, 0, 0) row every padding row collapses into
        pia_store4(a.gas + 0, 0, 0, 0, 0);
        pia_store4(a.gas + 4, 0, 0, 0, 0);
        pia_store4(a.gas + 8, 0, 0, 0, 0);
    }
    if (i < (u64)PIA_BLOCK_ENTRIES) {
        u64 w[4];
        const bool word = pia_block_entry(a, (u32)i, w) == 32u;
        pia_store4(a.block_table + i * 8, w[0], w[1], word ? 0ull : w[2], word ? 0ull : w[3]);
        pia_store4(a.block_table + i * 8 + 4, word ? w[2] : 0ull, word ? w[3] : 0ull, 0, 0);
        a.block_flags[i] = word;
    }
    // what belongs to the value: its byte of copy_constrains from every row, its length and its constraint from its first row
    a.raw_bytes[v.start + (v.len - 1u - p)] = (uint8_t)byte;
    if (p == 0u) {
        a.raw_lens[v.vidx] = v.len;
        pia_store4(a.cc_cells + 4 * v.cc, v.cell[0], v.cell[1], v.cell[2], v.cell[3]);
        // the value big-endian, left-aligned in its 32-byte slot: the byte-swapped integer shifted to the top
        ExaU256 x;
        x.w[0] = v.w[0]; x.w[1] = v.w[1]; x.w[2] = v.w[2]; x.w[3] = v.w[3];
        x = exa_shl(x, 8u * (32u - v.len));
        pia_store4((u64*)(a.cc_bytes + 32 * v.cc), kt_bswap64(x.w[3]), kt_bswap64(x.w[2]), kt_bswap64(x.w[1]), kt_bswap64(x.w[0]));
        a.cc_lens[v.cc] = v.len;
        if (v.empty_hi) {
            pia_store4(a.cc_cells + 4 * (v.cc + 1), 0, 0, 0, 0);
            pia_store4((u64*)(a.cc_bytes + 32 * (v.cc + 1)), 0, 0, 0, 0);
            a.cc_lens[v.cc + 1] = 0;
        }
    }
}

// ---- behind the digest: row 0's digest word, the keccak table, the public inputs and the two constraints in front of all others
ZK_HD void pia_patch(const PiaArgs& a) {
    // krow holds Word(int.from_bytes(digest, "big")); the PI circuit's Word(digest) reads the 32 bytes little-endian
    const u64 d0 = kt_bswap64(a.krow[17]), d1 = kt_bswap64(a.krow[16]), d2 = kt_bswap64(a.krow[13]), d3 = kt_bswap64(a.krow[12]);
    pia_store4(a.rows + ((u64)PI_DIGEST_LO * a.n) * 4, d0, d1, 0, 0);
    pia_store4(a.rows + ((u64)PI_DIGEST_HI * a.n) * 4, d2, d3, 0, 0);
    for (int c = 0; c < 5; c++) pia_store4(a.keccak + 4 * c, 0, 0, 0, 0);
    pia_store4(a.keccak + 20, 1, 0, 0, 0);
    pia_store4(a.keccak + 24, a.krow[4], a.krow[5], a.krow[6], a.krow[7]);
    pia_store4(a.keccak + 28, a.n, 0, 0, 0);
    pia_store4(a.keccak + 32, d0, d1, 0, 0);
    pia_store4(a.keccak + 36, d2, d3, 0, 0);
    pia_store4(a.public_inputs + 0, d0, d1, 0, 0);
    pia_store4(a.public_inputs + 4, d2, d3, 0, 0);
    const u64* words[3] = {a.block + 0, a.block + 8, a.srp};
    for (int k = 0; k < 3; k++) {
        pia_store4(a.public_inputs + 8 * (k + 1), words[k][0], words[k][1], 0, 0);
        pia_store4(a.public_inputs + 8 * (k + 1) + 4, words[k][2], words[k][3], 0, 0);
    }
    pia_store4(a.cc_cells + 0, d0, d1, 0, 0);
    pia_store4(a.cc_cells + 4, d2, d3, 0, 0);
    pia_store4((u64*)a.cc_bytes, d0, d1, 0, 0);
    pia_store4((u64*)(a.cc_bytes + 32), d2, d3, 0, 0);
    a.cc_lens[0] = PI_COPY_CELL;
    a.cc_lens[1] = PI_COPY_CELL;
}
