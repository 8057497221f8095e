// Exp-circuit witness assignment on the device.
//
// Replaces the reference's `ExpCircuit.add_event(base, exponent, identifier)` / `fill_dummy_events()`
// (src/zkevm_specs/evm_circuit/typing.py:868-994) and the exp-TABLE rows `Tables._convert_exp_circuit_to_table` derives
// (evm_circuit/table.py:654-671).  One event becomes bit_length(exponent) - 1 + popcount(exponent) - 1 step rows (none for an
// exponent of 0 or 1): the square-and-multiply chain of base^exponent mod 2^256 read from the full exponent down to base * base.
// Outputs: the 21-cell circuit rows column-major (exactly what zk_exp_open takes) and the 11-cell exp-table rows (what
// zk_evm_tables.exp takes).
//
// The reference recurses per event and threads the running exponent through the rows.  Here:
//   * exa_event_size:  one lane per event — domain checks and the step count from clz / popcount of the exponent;
//   * an exclusive scan of the counts gives each event's first row (exa_scan_block on the device, a loop on the host);
//   * exa_ident_check: identifiers of row-producing events strictly increase (one compare per event with the producer before it);
//   * exa_chain:       one lane per event — the power chain itself, sequential by nature: up to 255 squarings and 255 products
//     of 256-bit integers mod 2^256 on 32-bit limbs (truncated 8 x 8 products, no reduction).  It stores nothing but `d` of
//     every step (32 B) into a scratch array at the event's row positions, walking them backwards;
//   * exa_write_row:   one lane per OUTPUT row, coalesced — the row's exponent e_i in closed form from the event's exponent and
//     i, d_i and a_i = d_(i+1) from the scratch array, then 21 column-major cells and 11 row-major table cells.  The dummy
//     rows and the one dummy table row are lanes of the same loop.
#pragma once
#include <stdio.h>
#include "common.hpp"

enum { EXA_EV_NCELLS = 5, EXA_ROW_NCELLS = 21, EXA_TABLE_NCELLS = 11, EXA_OFFSET_INCREMENT = 7 };
enum { EXA_REJECT_CELL = 1, EXA_REJECT_ORDER = 2 };  // why an event was rejected (ZK_ERR_EXP_CELL / ZK_ERR_EXP_ORDER)
#define EXA_NO_REJECT (~0ull)

struct ExaArgs {
    const u64* events;  // [n_events][5][4]: identifier, base lo, base hi, exponent lo, exponent hi
    u64 n_events;
    u32* count;         // [n_events]      step rows per event
    u64* row0;          // [n_events + 1]  first row per event (exclusive scan of count), row0[n_events] = n_step
    u64* meta;          // [2]             min over rejected events of (event << 8 | reason) or EXA_NO_REJECT; n_step
    u64* d;             // [n_step][4]     base^(e_i) mod 2^256 of every step row
    u64 n_step, n_rows; // step rows; step rows + dummy rows
    u64* rows;          // out [21][n_rows][4]
    u64* table;         // out [n_step (+ 1 with dummy rows)][11][4]
};

struct ExaU256 {
    u64 w[4];
};
ZK_HD ExaU256 exa_word(const u64* lo, const u64* hi) {  // a Word from its lo / hi cells (halves below 2^128: exa_event_size checked)
    ExaU256 r;
    r.w[0] = lo[0]; r.w[1] = lo[1]; r.w[2] = hi[0]; r.w[3] = hi[1];
    return r;
}
ZK_HD u32 exa_bit_length(const ExaU256& x) {
    u32 n = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (x.w[k]) n = 64u * k + 64u - (u32)__builtin_clzll(x.w[k]);
    return n;
}
ZK_HD u32 exa_popcount(const ExaU256& x) {
    return (u32)(__builtin_popcountll(x.w[0]) + __builtin_popcountll(x.w[1]) + __builtin_popcountll(x.w[2]) + __builtin_popcountll(x.w[3]));
}
// x >> s, s in [0, 255]; the limbs are selected by comparisons, never indexed by a run-time value (they live in registers)
ZK_HD ExaU256 exa_shr(const ExaU256& x, u32 s) {
    const u32 ws = s >> 6, bs = s & 63u;
    u64 t[5];
    t[0] = ws == 0 ? x.w[0] : (ws == 1 ? x.w[1] : (ws == 2 ? x.w[2] : x.w[3]));
    t[1] = ws == 0 ? x.w[1] : (ws == 1 ? x.w[2] : (ws == 2 ? x.w[3] : 0ull));
    t[2] = ws == 0 ? x.w[2] : (ws == 1 ? x.w[3] : 0ull);
    t[3] = ws == 0 ? x.w[3] : 0ull;
    t[4] = 0ull;
    ExaU256 r;
#pragma unroll
    for (int k = 0; k < 4; k++) r.w[k] = bs ? ((t[k] >> bs) | (t[k + 1] << (64u - bs))) : t[k];
    return r;
}
ZK_HD ExaU256 exa_shl(const ExaU256& x, u32 s) {
    const u32 ws = s >> 6, bs = s & 63u;
    u64 t[5];
    t[4] = ws == 0 ? x.w[3] : (ws == 1 ? x.w[2] : (ws == 2 ? x.w[1] : x.w[0]));
    t[3] = ws == 0 ? x.w[2] : (ws == 1 ? x.w[1] : (ws == 2 ? x.w[0] : 0ull));
    t[2] = ws == 0 ? x.w[1] : (ws == 1 ? x.w[0] : 0ull);
    t[1] = ws == 0 ? x.w[0] : 0ull;
    t[0] = 0ull;
    ExaU256 r;
#pragma unroll
    for (int k = 0; k < 4; k++) r.w[k] = bs ? ((t[k + 1] << bs) | (t[k] >> (64u - bs))) : t[k + 1];
    return r;
}
// step rows of an exponent: bit_length - 1 squarings + popcount - 1 products (0 for exponents 0 and 1)
ZK_HD u32 exa_steps(const ExaU256& e) {
    const u32 bl = exa_bit_length(e);
    return bl < 2u ? 0u : bl - 1u + exa_popcount(e) - 1u;
}
// j + popcount(e mod 2^j): the rows it takes to consume the j low bits of e (a halving per bit, a decrement more per set bit)
ZK_HD u32 exa_cost(const ExaU256& e, u32 j) {
    u32 c = j;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const u32 base = 64u * k;
        if (j >= base + 64u) c += (u32)__builtin_popcountll(e.w[k]);
        else if (j > base) c += (u32)__builtin_popcountll(e.w[k] & ((1ull << (j - base)) - 1ull));
    }
    return c;
}
// the exponent of row i of an event (e_0 = exponent, e_(i + 1) = e_i / 2 when even, e_i - 1 when odd), i below exa_steps:
// j = the largest j with exa_cost(j) <= i low bits are gone, and one decrement more if a row is left over (exponent 5: 5, 4, 2)
ZK_HD ExaU256 exa_exponent_at(const ExaU256& e, u32 i) {
    u32 lo = 0, hi = 256;
    while (hi - lo > 1u) {
        const u32 mid = (lo + hi) >> 1;
        if (exa_cost(e, mid) <= i) lo = mid; else hi = mid;
    }
    ExaU256 r = exa_shr(e, lo);
    if (i != exa_cost(e, lo)) r.w[0] &= ~1ull;  // (bit `lo` of e is set then: the decrement of an odd value)
    return r;
}

// ---- 256-bit products mod 2^256 on 32-bit limbs (the chain lane): 36 multiply-adds, constant indices only
struct ExaLimbs {
    u32 v[8];
};
ZK_HD ExaLimbs exa_limbs(const ExaU256& x) {
    ExaLimbs r;
#pragma unroll
    for (int k = 0; k < 4; k++) { r.v[2 * k] = (u32)x.w[k]; r.v[2 * k + 1] = (u32)(x.w[k] >> 32); }
    return r;
}
ZK_HD ExaLimbs exa_mul_lo(const ExaLimbs& a, const ExaLimbs& b) {
    ExaLimbs t;
#pragma unroll
    for (int k = 0; k < 8; k++) t.v[k] = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        u64 c = 0;
#pragma unroll
        for (int j = 0; j < 8 - i; j++) {
            c += (u64)t.v[i + j] + (u64)a.v[i] * b.v[j];  // <= (2^32 - 1)^2 + 2 (2^32 - 1) = 2^64 - 1
            t.v[i + j] = (u32)c;
            c >>= 32;
        }
    }
    return t;
}
ZK_HD void exa_store_limbs(u64* out, const ExaLimbs& x) {
    u64* o = (u64*)__builtin_assume_aligned(out, 32);
#pragma unroll
    for (int k = 0; k < 4; k++) o[k] = (u64)x.v[2 * k] | ((u64)x.v[2 * k + 1] << 32);
}
ZK_HD void exa_store4(u64* out, u64 w0, u64 w1, u64 w2, u64 w3) {
    u64* o = (u64*)__builtin_assume_aligned(out, 32);
    o[0] = w0; o[1] = w1; o[2] = w2; o[3] = w3;
}

// One lane per event: its step count, or why it is rejected (a reason != 0; the count is 0 then)
ZK_HD u32 exa_event_size(const ExaArgs& a, u64 e) {
    const u64* c = a.events + e * EXA_EV_NCELLS * 4;
    bool ok = !fr_geq_p(fr_load(c));
#pragma unroll
    for (int k = 1; k < EXA_EV_NCELLS; k++) ok = ok && (c[4 * k + 2] | c[4 * k + 3]) == 0ull;
    a.count[e] = ok ? exa_steps(exa_word(c + 12, c + 16)) : 0u;
    return ok ? 0u : (u32)EXA_REJECT_CELL;
}
// the event that owns step row j: the last one whose first row is <= j (an event without rows never is)
ZK_HD u64 exa_event_of_row(const ExaArgs& a, u64 j) {
    u64 lo = 0, hi = a.n_events;
    while (hi - lo > 1) {
        const u64 mid = (lo + hi) >> 1;
        if (a.row0[mid] <= j) lo = mid; else hi = mid;
    }
    return lo;
}
// after the scan: a row-producing event's identifier must exceed that of the row-producing event before it
ZK_HD u32 exa_ident_check(const ExaArgs& a, u64 e) {
    if (a.count[e] == 0u || a.row0[e] == 0ull) return 0u;
    const u64 p = exa_event_of_row(a, a.row0[e] - 1);
    return fr_lt(fr_load(a.events + p * EXA_EV_NCELLS * 4), fr_load(a.events + e * EXA_EV_NCELLS * 4)) ? 0u : (u32)EXA_REJECT_ORDER;
}
ZK_HD u64 exa_reject_word(u64 e, u32 reason) { return (e << 8) | reason; }

// One lane per event: d of its rows, from the last row (base * base, exponent 2) up to the first (the full exponent)
ZK_HD void exa_chain(const ExaArgs& a, u64 e) {
    const u32 n = a.count[e];
    if (n == 0u) return;
    const u64* c = a.events + e * EXA_EV_NCELLS * 4;
    const ExaLimbs base = exa_limbs(exa_word(c + 4, c + 8));
    const ExaU256 ex = exa_word(c + 12, c + 16);
    const u32 bl = exa_bit_length(ex);
    ExaU256 bits = exa_shl(ex, 257u - bl);  // the second-highest bit of the exponent at bit 255 (bl >= 2)
    ExaLimbs x = base;
    u64 p = a.row0[e] + n;
    for (u32 k = bl - 1u; k > 0u; k--) {
        x = exa_mul_lo(x, x);
        exa_store_limbs(a.d + 4 * --p, x);
        if (bits.w[3] >> 63) {
            x = exa_mul_lo(x, base);
            exa_store_limbs(a.d + 4 * --p, x);
        }
        bits.w[3] = (bits.w[3] << 1) | (bits.w[2] >> 63);
        bits.w[2] = (bits.w[2] << 1) | (bits.w[1] >> 63);
        bits.w[1] = (bits.w[1] << 1) | (bits.w[0] >> 63);
        bits.w[0] <<= 1;
    }
}

// Output row j (ExpCircuitRow, table.py:519-535: q_usable, is_step, identifier, is_last, then base, exponent, exponentiation,
// a, b, c, d, q as lo / hi pairs, r) and its exp-table row (ExpTableRow :538-548).  Rows from n_step on are the dummy rows of
// fill_dummy_events (typing.py:941-962); the lane of the first one writes the single table row they all map to.
ZK_HD void exa_write_row(const ExaArgs& a, u64 j) {
    const u64 n = a.n_rows;
#define EXA_OUT(c) (a.rows + ((u64)(c) * n + j) * 4)
    if (j >= a.n_step) {
        exa_store4(EXA_OUT(0), 1, 0, 0, 0);
        exa_store4(EXA_OUT(1), 0, 0, 0, 0);
        exa_store4(EXA_OUT(2), 0, 0, 0, 0);
        exa_store4(EXA_OUT(3), 0, 0, 0, 0);
#pragma unroll
        for (int c = 4; c < 20; c++) exa_store4(EXA_OUT(c), (c % 2 == 0 && c != 14 && c != 18) ? 1 : 0, 0, 0, 0);  // Word(1) but c and q: Word(0)
        exa_store4(EXA_OUT(20), 1, 0, 0, 0);
        if (j == a.n_step) {
            u64* t = a.table + j * EXA_TABLE_NCELLS * 4;
            const u64 one[EXA_TABLE_NCELLS] = {1, 0, 0, 1, 0, 0, 0, 1, 0, 1, 0};
#pragma unroll
            for (int c = 0; c < EXA_TABLE_NCELLS; c++) exa_store4(t + 4 * c, one[c], 0, 0, 0);
        }
        return;
    }
    const u64 ei = exa_event_of_row(a, j);
    const u64* c = a.events + ei * EXA_EV_NCELLS * 4;
    const u32 i = (u32)(j - a.row0[ei]);
    const bool last = i + 1u == a.count[ei];
    const ExaU256 base = exa_word(c + 4, c + 8);
    const ExaU256 e = exa_exponent_at(exa_word(c + 12, c + 16), i);
    const bool odd = e.w[0] & 1ull;
    const u64* dp = a.d + 4 * j;
    ExaU256 d, x, y;  // d = a * b: x = the next row's d (the base itself on the last row), y = x (even) or the base (odd)
#pragma unroll
    for (int k = 0; k < 4; k++) d.w[k] = dp[k];
#pragma unroll
    for (int k = 0; k < 4; k++) x.w[k] = last ? base.w[k] : dp[4 + k];
    y = odd ? base : x;
    const ExaU256 q = exa_shr(e, 1);
    exa_store4(EXA_OUT(0), 1, 0, 0, 0);
    exa_store4(EXA_OUT(1), 1, 0, 0, 0);
    exa_store4(EXA_OUT(2), c[0], c[1], c[2], c[3]);
    exa_store4(EXA_OUT(3), last ? 1 : 0, 0, 0, 0);
    exa_store4(EXA_OUT(4), base.w[0], base.w[1], 0, 0);
    exa_store4(EXA_OUT(5), base.w[2], base.w[3], 0, 0);
    exa_store4(EXA_OUT(6), e.w[0], e.w[1], 0, 0);
    exa_store4(EXA_OUT(7), e.w[2], e.w[3], 0, 0);
    exa_store4(EXA_OUT(8), d.w[0], d.w[1], 0, 0);
    exa_store4(EXA_OUT(9), d.w[2], d.w[3], 0, 0);
    exa_store4(EXA_OUT(10), x.w[0], x.w[1], 0, 0);
    exa_store4(EXA_OUT(11), x.w[2], x.w[3], 0, 0);
    exa_store4(EXA_OUT(12), y.w[0], y.w[1], 0, 0);
    exa_store4(EXA_OUT(13), y.w[2], y.w[3], 0, 0);
    exa_store4(EXA_OUT(14), 0, 0, 0, 0);
    exa_store4(EXA_OUT(15), 0, 0, 0, 0);
    exa_store4(EXA_OUT(16), d.w[0], d.w[1], 0, 0);
    exa_store4(EXA_OUT(17), d.w[2], d.w[3], 0, 0);
    exa_store4(EXA_OUT(18), q.w[0], q.w[1], 0, 0);
    exa_store4(EXA_OUT(19), q.w[2], q.w[3], 0, 0);
    exa_store4(EXA_OUT(20), odd ? 1 : 0, 0, 0, 0);
#undef EXA_OUT
    u64* t = a.table + j * EXA_TABLE_NCELLS * 4;
    exa_store4(t + 0, 1, 0, 0, 0);
    exa_store4(t + 4, c[0], c[1], c[2], c[3]);
    exa_store4(t + 8, last ? 1 : 0, 0, 0, 0);
    exa_store4(t + 12, base.w[0], 0, 0, 0);
    exa_store4(t + 16, base.w[1], 0, 0, 0);
    exa_store4(t + 20, base.w[2], 0, 0, 0);
    exa_store4(t + 24, base.w[3], 0, 0, 0);
    exa_store4(t + 28, e.w[0], e.w[1], 0, 0);
    exa_store4(t + 32, e.w[2], e.w[3], 0, 0);
    exa_store4(t + 36, d.w[0], d.w[1], 0, 0);
    exa_store4(t + 40, d.w[2], d.w[3], 0, 0);
}

// ---- host side of both backends: what the open makes of the counts the size pass left
struct ExaSizes {
    u64 n_step, n_rows, n_table;
};
// -> 0, or the error code of include/zkevm_hip.h with its text in `msg` (reject: a.meta[0] as read back, n_step: a.meta[1])
static inline int exa_sizes_of(u64 reject, u64 n_step, u64 max_exp_steps, ExaSizes& z, char* msg, size_t msg_len) {
    if (reject != EXA_NO_REJECT) {
        const bool cell = (reject & 0xffull) == EXA_REJECT_CELL;
        snprintf(msg, msg_len, cell ? "zk_exp_assign: event %llu has a cell outside the wire's domain (identifier below the field modulus, lo / hi halves below 2^128)"
                                    : "zk_exp_assign: the identifier of event %llu does not exceed that of the row-producing event before it "
                                      "(identifiers must be strictly increasing: the reference's table is a set)",
                 (unsigned long long)(reject >> 8));
        return cell ? -40 : -41;
    }
    const u64 cap = max_exp_steps > (1ull << 31) ? (1ull << 34) : max_exp_steps * EXA_OFFSET_INCREMENT;
    z.n_step = n_step;
    z.n_rows = n_step < cap ? cap : n_step;
    z.n_table = n_step + (z.n_rows > n_step ? 1 : 0);
    if (z.n_rows >= (1ull << 31)) {
        snprintf(msg, msg_len, "zk_exp_assign: %llu rows (2^31 or more)", (unsigned long long)z.n_rows);
        return -42;
    }
    return 0;
}
