// EVM circuit witness from compact trace records (zk_evm_witness_from_trace*): RW ops and step records to the wire rows zk_evm_tables takes.
//
// Replaces flatten_rw_table / flatten_steps over RWTableRow / StepState objects (evm_circuit/table.py:447-457, step.py:6-75) and the upload
// of their result (452 bytes per RW row, 416 per step).  An RW op is a head word, four 64-bit integers and the pool words its head names;
// a step is thirteen 64-bit words.  With strictly ascending rw_counters (checked at open) the RW table's set order is the input order and
// it holds no duplicate, so row i of the output is op i.
//
//   trw_head_bad / trw_head_words / trw_step_bad   the open's per-record checks and the pool words a head consumes
//   trw_rw_piece     the two 64-bit words of the 16-byte piece q (0..27) of RW row `row`;  trw_rw_flag its flag word
//   trw_step_piece   the same for piece q (0..25) of a step row
//   trw_verdict_*    the open's verdict block and the error it stands for (both backends format it here)
// The functions here define the results (CPU backend, tests/hostsim); k_trace_witness.hip maps lanes onto them.
#pragma once
#include <stdio.h>
#include "fr.hpp"
#include "block_tables.hpp"  // btb_reduce, btb_limb

enum { TRW_RW_NCELLS = 14, TRW_STEP_NCELLS = 13, TRW_STEP_WORDS = 13,
       TRW_RW_PIECES = 28,    // 16-byte pieces of a 448-byte RW row
       TRW_STEP_PIECES = 26,  // of a 416-byte step row
       // head bits
       TRW_H_WRITE = 1u << 0, TRW_H_TAG_SHIFT = 1, TRW_H_FIELD_SHIFT = 8, TRW_H_VALUE_WORD = 1u << 16, TRW_H_PREV_WORD = 1u << 17,
       TRW_H_ADDR_POOL = 1u << 20, TRW_H_KEY = 1u << 21, TRW_H_VALUE_POOL = 1u << 22, TRW_H_PREV_POOL = 1u << 23, TRW_H_AUX = 1u << 24,
       TRW_H_POOL_SHIFT = 20,
       TRW_HEAD_MASK = 0x1u | (0xfu << 1) | (0xffu << 8) | (0x3u << 16) | (0x1fu << 20),
       TRW_STEP_W0_MASK = 0x3ff,
       // verdict block (u64 words): the first offending RW op by head, by counter, the first offending step, the pool words consumed
       TRW_V_HEAD = 0, TRW_V_ORDER = 1, TRW_V_STEP = 2, TRW_V_POOL = 3, TRW_V_WORDS = 4 };
#define TRW_NONE (~0ull)

struct TrwArgs {
    const u32* head_in;     // [n_rw] the caller's heads: read at open only
    const u64* ctr_in;      // [n_rw] the caller's rw_counters (null: rw_base + i): read at open only
    const u64* id;          // [n_rw]
    const u64* addr;        // [n_rw]
    const u64* val;         // [n_rw]
    const u64* prev;        // [n_rw]
    const u64* pool;        // [n_pool][4]
    const u64* steps_in;    // [n_steps][13]
    u64 n_rw, n_pool, n_steps, rw_base;
    u32* head;              // [n_rw] the session's copy of the checked heads
    u64* ctr;               // [n_rw] the session's copy of the checked counters (null: rw_base + i)
    u64* off;               // [n_rw] the pool words consumed by the rows before row i (exclusive prefix of trw_head_words)
    u64* verdict;           // [TRW_V_WORDS]
    u64* rw;  u32* rw_flags;  // out [n_rw][14][4], [n_rw]
    u64* steps;               // out [n_steps][13][4]
};

// ---- the open's per-record checks (device at open; the host loop of trw_check_host for host callers' sizes) -------------------------
#if defined(ZK_HOSTSIM)
#define TRW_BOTH static inline
#else
#define TRW_BOTH __host__ __device__ __forceinline__
#endif
TRW_BOTH bool trw_head_bad(u32 h) { return (h & ~(u32)TRW_HEAD_MASK) != 0; }
TRW_BOTH u32 trw_head_words(u32 h) { return (u32)__builtin_popcount((h >> TRW_H_POOL_SHIFT) & 0x1fu); }
TRW_BOTH bool trw_step_bad(u64 w0) { return (w0 & ~(u64)TRW_STEP_W0_MASK) != 0; }
ZK_HD u32 trw_rw_flag(u32 h) { return (h >> 16) & 3u; }
ZK_HD u64 trw_counter(const TrwArgs& a, u64 row) { return a.ctr ? a.ctr[row] : a.rw_base + row; }

// ---- the rows ----------------------------------------------------------------------------------------------------------------------
// The two 64-bit words of piece q (0..27) of RW row `row`: cells rw_counter, is_write, tag, id, address, field_tag, storage_key lo / hi,
// value lo / hi, value_prev lo / hi, aux0 lo / hi; a cell is two pieces.  h / off: the session's head and pool offset of the row.
// The cell only selects WHAT to load — an immediate from the head, one 64-bit integer, 16 bytes of a pool word, or a whole pool word to
// reduce — and the loads themselves stand once behind the selection: the 28 lanes of a row take different cells, and a load inside
// each case would run the cases' memory latencies one after the other.
ZK_HD void trw_rw_piece(const TrwArgs& a, u64 row, u32 h, u64 off, u32 q, u64& w0, u64& w1) {
    const u32 cell = q >> 1, half = q & 1u;
    // the row's pool words in the order address, key, value, prev, aux
    const u64 p_key = off + ((h >> 20) & 1u), p_val = p_key + ((h >> 21) & 1u), p_prev = p_val + ((h >> 22) & 1u), p_aux = p_prev + ((h >> 23) & 1u);
    u64 imm = 0;               // the piece when nothing is loaded
    const u64* one = nullptr;  // w0 = *one
    const u64* two = nullptr;  // (w0, w1) = two[0..1]
    const u64* red = nullptr;  // the half `half` of FQ(red[0..3])
    switch (cell) {
    case 0: if (a.ctr) one = a.ctr + row; else imm = a.rw_base + row; break;
    case 1: imm = h & 1u; break;
    case 2: imm = (h >> TRW_H_TAG_SHIFT) & 0xfu; break;
    case 3: one = a.id + row; break;
    case 4: if (h & TRW_H_ADDR_POOL) red = a.pool + 4 * off; else one = a.addr + row; break;
    case 5: imm = (h >> TRW_H_FIELD_SHIFT) & 0xffu; break;
    case 6: case 7: if (h & TRW_H_KEY) two = a.pool + 4 * p_key + (cell == 7 ? 2 : 0); break;
    case 8: case 9: case 10: case 11: {
        const bool is_prev = cell >= 10, hi_cell = cell & 1u;
        const bool wide = (h & (is_prev ? TRW_H_PREV_POOL : TRW_H_VALUE_POOL)) != 0, word = (h & (is_prev ? TRW_H_PREV_WORD : TRW_H_VALUE_WORD)) != 0;
        const u64* w = a.pool + 4 * (is_prev ? p_prev : p_val);  // (dereferenced only when wide)
        if (!wide) { if (!hi_cell) one = (is_prev ? a.prev : a.val) + row; }  // a value below 2^64: (v, 0) with either flag
        else if (word) two = w + (hi_cell ? 2 : 0);                          // Word(w): lo = w mod 2^128, hi = w >> 128
        else if (!hi_cell) red = w;                                          // FQ(w), hi = 0
        break;
    }
    default: if (h & TRW_H_AUX) two = a.pool + 4 * p_aux + (cell == 13 ? 2 : 0); break;
    }
    w0 = imm;
    w1 = 0;
    if (red) {  // (before the half test: FQ(w) has a second half)
        const Fr v = btb_reduce(fr_load(red));
        w0 = half ? btb_limb(v, 2) : btb_limb(v, 0);  // (constant limb indices: the value stays in registers)
        w1 = half ? btb_limb(v, 3) : btb_limb(v, 1);
        return;
    }
    if (half) { w0 = 0; return; }  // everything else is below 2^128
    if (one) w0 = *one;
    if (two) { w0 = two[0]; w1 = two[1]; }
}
// Piece q (0..25) of step row `row`: cells execution_state, rw_counter, call_id, is_root, is_create, code_hash lo / hi, program_counter,
// stack_pointer, gas_left, memory_word_size, reversible_write_counter, log_id (flatten_steps' order) from the record's 13 words: the
// cell selects a word index, one load (two for a code-hash half) follows.
ZK_HD void trw_step_piece(const TrwArgs& a, u64 row, u32 q, u64& w0, u64& w1) {
    const u32 cell = q >> 1;
    w0 = 0;
    w1 = 0;
    if (q & 1u) return;  // every cell is below 2^128
    const u64* r = a.steps_in + row * TRW_STEP_WORDS;
    const bool hash = cell == 5 || cell == 6;
    const u32 at = cell >= 7 ? cell - 4 : hash ? 2 * cell - 1 : (cell == 1 || cell == 2) ? cell : 0;  // cells 7..12 are w3..w8, the hash w9..w12
    const u64 x = r[at];
    w0 = cell == 0 ? (x & 0xffu) : cell == 3 ? ((x >> 8) & 1u) : cell == 4 ? ((x >> 9) & 1u) : x;
    if (hash) w1 = r[at + 1];
}

// ---- the open's verdict (host side of both backends) ---------------------------------------------------------------------------------
// the counts that need no array: 0, or the error code with its text in msg
static inline int trw_plan_counts(u64 n_rw, u64 n_steps, u64 rw_base, bool has_ctr, char* msg, size_t msg_len) {
    if (n_rw >= (1ull << 31) || n_steps >= (1ull << 31)) {
        snprintf(msg, msg_len, "zk_evm_witness_from_trace: %llu RW ops, %llu steps (a table of 2^31 rows or more)", (unsigned long long)n_rw, (unsigned long long)n_steps);
        return -73;
    }
    const u64 end = rw_base + n_rw;
    if (!has_ctr && end < rw_base && end != 0) {  // rw_base + n_rw > 2^64: the last counter would wrap
        snprintf(msg, msg_len, "zk_evm_witness_from_trace: rw_base %llu + %llu RW ops passes 2^64", (unsigned long long)rw_base, (unsigned long long)n_rw);
        return -71;
    }
    return 0;
}
// v: the verdict block (HOST copy) after the checks ran over every record
static inline int trw_verdict_error(const u64* v, u64 n_pool, char* msg, size_t msg_len) {
    if (v[TRW_V_HEAD] != TRW_NONE) {
        snprintf(msg, msg_len, "zk_evm_witness_from_trace: the head of RW op %llu has a reserved bit set", (unsigned long long)v[TRW_V_HEAD]);
        return -70;
    }
    if (v[TRW_V_STEP] != TRW_NONE) {
        snprintf(msg, msg_len, "zk_evm_witness_from_trace: word 0 of step %llu has a reserved bit set", (unsigned long long)v[TRW_V_STEP]);
        return -70;
    }
    if (v[TRW_V_ORDER] != TRW_NONE) {
        snprintf(msg, msg_len, "zk_evm_witness_from_trace: the rw_counter of RW op %llu does not exceed the one before it (rw_counters must be strictly ascending)",
                 (unsigned long long)v[TRW_V_ORDER]);
        return -71;
    }
    if (v[TRW_V_POOL] != n_pool) {
        snprintf(msg, msg_len, "zk_evm_witness_from_trace: the heads consume %llu pool words, n_pool is %llu", (unsigned long long)v[TRW_V_POOL], (unsigned long long)n_pool);
        return -72;
    }
    return 0;
}
// The checks in a host loop (CPU backend, host callers' _sizes, hostsim): fills head / ctr / off when non-null, and the verdict
static inline void trw_check_host(const u32* head_in, const u64* ctr_in, u64 n_rw, const u64* steps_in, u64 n_steps, u32* head, u64* ctr, u64* off, u64* v) {
    v[TRW_V_HEAD] = v[TRW_V_ORDER] = v[TRW_V_STEP] = TRW_NONE;
    u64 run = 0;
    for (u64 i = 0; i < n_rw; i++) {
        const u32 h = head_in[i];
        if (trw_head_bad(h) && v[TRW_V_HEAD] == TRW_NONE) v[TRW_V_HEAD] = i;
        if (ctr_in && i && ctr_in[i] <= ctr_in[i - 1] && v[TRW_V_ORDER] == TRW_NONE) v[TRW_V_ORDER] = i;
        if (head) head[i] = h;
        if (ctr && ctr_in) ctr[i] = ctr_in[i];
        if (off) off[i] = run;
        run += trw_head_words(h);
    }
    for (u64 i = 0; i < n_steps; i++)
        if (trw_step_bad(steps_in[i * TRW_STEP_WORDS]) && v[TRW_V_STEP] == TRW_NONE) v[TRW_V_STEP] = i;
    v[TRW_V_POOL] = run;
}
