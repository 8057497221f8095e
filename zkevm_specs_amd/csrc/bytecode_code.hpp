// Bytecode table, Bytecode-circuit witness and keccak rows from raw contract code (zk_bytecode_from_code*).
//
// Replaces, for a set of contracts, the reference's `Bytecode(code).table_assignments()` (evm_circuit/typing.py:317-324 init_is_code,
// :387-427): a Header row (hash, 1, 0, 0, len) and a Byte row (hash, 2, i, is_code_i, byte_i) per byte — the EVM circuit's bytecode table
// and the input of assign_bytecode_circuit (bytecode_circuit.py:104-167), whose 12-cell rows come out of the same pass, together with
// the keccak rows that circuit looks up (assign_keccak_table, :182-186).
//
// Input is the contracts' BYTES (one byte per byte of code, where bytecode_assign.hpp reads a 32-byte cell of a 192-byte row to learn
// it).  The two per-code recurrences — the push-data counter behind is_code and the running value_rlc — use bytecode_assign.hpp's
// decomposition, over chunks of 64 BYTES (a chunk never holds a Header row: BcaChunk::first = 0, chunk_m = count):
//   bcc_chunk        per chunk: Horner over its bytes from 0 (every byte's partial value is kept: 32 B per byte of scratch), and the
//                    33-entry map "counter after the chunk as a function of the counter before it"
//   bca_prefix_code  (bytecode_assign.hpp, unchanged) per code: value_rlc and counter entering every chunk
//   keccak_table_row (keccak_table.hpp, unchanged) per code: the keccak row, whose output word is the code hash
//   bcc_write_row    per OUTPUT row: the code of the row by binary search over the codes' first rows, the counter by walking the
//                    chunk's bytes from its entry state, then the 6-cell table row (row-major) and the 12-cell circuit row
//                    (column-major, padding rows included), full 32-byte cells
// The functions here define the results (CPU backend, tests/hostsim); k_bytecode_code.hip holds the wavefront form of bcc_chunk.
#pragma once
#include "bytecode_assign.hpp"
#include "keccak_table.hpp"

enum { BCC_TABLE_NCELLS = 6 };

struct BccArgs {
    const uint8_t* code;   // [n_bytes] the codes back to back
    const u64* offsets;    // [n_codes + 1] byte offsets
    const u32* row_off;    // [n_codes + 1] first table row of every code: offsets[j] + j (strictly increasing)
    u64 n_bytes, n_codes;
    u64 n_rows;            // table rows: n_bytes + n_codes
    u64 n_out;             // circuit rows: 2^k, or 0
    BcaArgs p;             // the chunk tables as bca_prefix_* take them: chunks (start = global byte offset, first = 0), code_chunk0,
                           // n_chunks, n_codes, rpow, chunk_acc / chunk_m / chunk_map (written by bcc_chunk), chunk_in / chunk_state
    u64* part;             // [n_bytes][4] Horner value of the chunk's bytes up to and including this one
    const u64* keccak;     // [n_codes][KT_NCELLS][4] the codes' keccak rows (cells 3, 4: hash lo, hi)
    u64* table;            // out [n_rows][6][4] row-major
    u64* rows;             // out [12][n_out][4] column-major (n_out > 0)
};

// get_push_size(byte): PUSH1..PUSH32 -> 1..32, anything else (PUSH0 = 0x5f included) -> 0
ZK_HD u32 bcc_push_size(u32 b) { return (b >= 0x60u && b <= 0x7fu) ? b - 0x5fu : 0u; }

// Chunk c (host form; bcc_chunk_wave_kernel is the device's): the reference's recurrence acc = acc * r + byte from 0, and the counter
// map by a backward pass over "counter after the chunk when position p is entered with 0" (as bca_chunk).
ZK_HD void bcc_chunk(const BccArgs& a, u64 c) {
    const BcaChunk ch = a.p.chunks[c];
    const Fr rM = fr_load(a.p.rpow + 4);
    Fr x = fr_zero();
    for (u32 t = 0; t < ch.count; t++) {
        x = fr_add(fr_mont(x, rM), fr_from_u64(a.code[(u64)ch.start + t]));
        bca_store(a.part + 4 * ((u64)ch.start + t), x);
    }
    bca_store(a.p.chunk_acc + 4 * c, x);
    a.p.chunk_m[c] = ch.count;
    uint8_t zero_out[BCA_CHUNK + 1];
    zero_out[ch.count] = 0;
    for (int p = (int)ch.count - 1; p >= 0; p--) {
        const u32 sz = bcc_push_size(a.code[(u64)ch.start + (u32)p]);
        if (sz == 0) zero_out[p] = zero_out[p + 1];
        else if ((u32)p + sz + 1u <= ch.count) zero_out[p] = zero_out[p + sz + 1];
        else zero_out[p] = (uint8_t)(sz - (ch.count - 1u - (u32)p));  // the push data runs past the chunk
    }
    uint8_t* map = a.p.chunk_map + c * BCA_MAP_STRIDE;
    for (u32 left = 0; left <= 32u; left++) map[left] = left <= ch.count ? zero_out[left] : (uint8_t)(left - ch.count);
}
// the code that owns table row i < n_rows: the largest j with row_off[j] <= i
ZK_HD u32 bcc_code_of_row(const BccArgs& a, u64 i) {
    u32 lo = 0, hi = (u32)a.n_codes;  // row_off[lo] <= i < row_off[hi]
    while (hi - lo > 1u) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if ((u64)a.row_off[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}
// Row i of both outputs: table row i (i < n_rows) and circuit row i (i < n_out; a padding row when i >= n_rows)
ZK_HD void bcc_write_row(const BccArgs& a, u64 i) {
    const u64 n = a.n_out;
#define BCC_OUT(c) (a.rows + ((u64)(c) * n + i) * 4)
    if (i < n) {
        bca_store(BCC_OUT(0), fr_from_u64(i == 0 ? 1 : 0));
        bca_store(BCC_OUT(1), fr_from_u64(i == n - 1 ? 1 : 0));
    }
    if (i >= a.n_rows) {  // padding (bytecode_circuit.py:150-165): Header rows of the empty bytecode
        if (i >= n) return;
        bca_store(BCC_OUT(2), fr_from_u128(0x7bfad8045d85a470ull, 0xe500b653ca82273bull));
        bca_store(BCC_OUT(3), fr_from_u128(0x927e7db2dcc703c0ull, 0xc5d2460186f7233cull));
        bca_store(BCC_OUT(4), fr_from_u64(1));
        for (int c = 5; c < BCA_OUT_NCELLS; c++) bca_store(BCC_OUT(c), fr_zero());
        return;
    }
    const u32 j = bcc_code_of_row(a, i);
    const u64 o0 = a.offsets[j], len = a.offsets[j + 1] - o0;
    const u32 t = (u32)(i - a.row_off[j]);  // 0: the Header row; else byte t - 1
    const Fr h_lo = fr_load(a.keccak + ((u64)j * KT_NCELLS + 3) * 4), h_hi = fr_load(a.keccak + ((u64)j * KT_NCELLS + 4) * 4);
    u32 left = 0, size = 0;
    u64 index = 0, value = len;
    Fr rlc = fr_zero();
    if (t) {
        const u64 b = (u64)t - 1u;
        const u64 c = (u64)a.p.code_chunk0[j] + b / BCA_CHUNK;
        const u32 q = (u32)(b % BCA_CHUNK);
        const uint8_t* bytes = a.code + o0 + (b - q);  // the chunk's bytes
        left = a.p.chunk_state[c];
        for (u32 s = 0; s < q; s++) left = left == 0u ? bcc_push_size(bytes[s]) : left - 1u;
        index = b;
        value = bytes[q];
        size = bcc_push_size((u32)value);
        rlc = fr_add(fr_mont(fr_load(a.p.chunk_in + 4 * c), fr_load(a.p.rpow + 4 * (u64)(q + 1u))), fr_load(a.part + 4 * (o0 + b)));
    }
    const Fr tag = fr_from_u64(t ? 2 : 1), idx = fr_from_u64(index), is_code = fr_from_u64((t && left == 0u) ? 1 : 0), val = fr_from_u64(value);
    u64* tr = a.table + i * (BCC_TABLE_NCELLS * 4);
    bca_store(tr + 0, h_lo);
    bca_store(tr + 4, h_hi);
    bca_store(tr + 8, tag);
    bca_store(tr + 12, idx);
    bca_store(tr + 16, is_code);
    bca_store(tr + 20, val);
    if (i < n) {  // bytecode_circuit.Row: q_first, q_last, hash lo, hi, tag, index, value, is_code, push_data_left, value_rlc, length, push_data_size
        bca_store(BCC_OUT(2), h_lo);
        bca_store(BCC_OUT(3), h_hi);
        bca_store(BCC_OUT(4), tag);
        bca_store(BCC_OUT(5), idx);
        bca_store(BCC_OUT(6), val);
        bca_store(BCC_OUT(7), is_code);
        bca_store(BCC_OUT(8), fr_from_u64(left));
        bca_store(BCC_OUT(9), rlc);
        bca_store(BCC_OUT(10), fr_from_u64(len));
        bca_store(BCC_OUT(11), fr_from_u64(size));
    }
#undef BCC_OUT
}
