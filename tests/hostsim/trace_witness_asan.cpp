// Stand-alone host program (TEST INFRASTRUCTURE): the per-row functions of csrc/trace_witness.hpp over exactly-sized heap buffers, built
// with -fsanitize=address,undefined by tests/test_trace_witness_cpu.py and run as a child process.  Shapes: the directed sizes of the
// RW and step sets, every combination of the pool bits, all-wide and all-narrow rows at the ends and either side of every multiple of 16,
// pool words at the edges of p, 2^128 and 2^256, counters from rw_base (1 and 2^64 - n) and explicit.  Every row is compared with a
// cell-by-cell construction; exit status 0 = no mismatch (the sanitizers abort on their own findings).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../zkevm_specs_amd/csrc/trace_witness.hpp"

static u64 rnd_state = 0x9e3779b97f4a7c15ull;
static u64 rnd() {
    rnd_state ^= rnd_state << 13; rnd_state ^= rnd_state >> 7; rnd_state ^= rnd_state << 17;
    return rnd_state;
}
// v mod p by repeated subtraction on 64-bit limbs (independent of btb_reduce's 32-bit form)
static void mod_p(const u64* v, u64* out) {
    memcpy(out, v, 32);
    while (!btbh_lt(out, BTB_P64)) btbh_sub(out, out, BTB_P64);
}
static void edge_word(u64 k, u64* w) {
    const u64 one[4] = {1, 0, 0, 0};
    memset(w, 0, 32);
    switch (k % 12) {
    case 0: break;
    case 1: w[0] = 1; break;
    case 2: btbh_sub(w, BTB_P64, one); break;
    case 3: memcpy(w, BTB_P64, 32); break;
    case 4: memcpy(w, BTB_P64, 32); w[0] += 1; break;
    case 5: w[0] = w[1] = ~0ull; break;
    case 6: w[2] = 1; break;
    case 7: w[0] = w[1] = ~0ull; w[2] = 0xffffffffull; break;
    case 8: w[0] = w[1] = w[2] = w[3] = ~0ull; break;
    default: for (int j = 0; j < 4; j++) w[j] = rnd(); break;
    }
}
static bool cell_is(const u64* c, u64 a, u64 b, u64 d, u64 e) { return c[0] == a && c[1] == b && c[2] == d && c[3] == e; }

static int run_rw(u64 n, int variant, int mode) {
    // exactly-sized heap buffers: a read or a store one element past any of them is a finding
    std::vector<u32> head_in(n);
    std::vector<u64> id(n), addr(n), val(n), prev(n), ctr_in(mode == 2 ? n : 0), pool;
    u64 uses[5] = {0, 3, 6, 9, 1};
    for (u64 i = 0; i < n; i++) {
        const bool edge_row = i == 0 || i == n - 1 || i % 16 == 15 || i % 16 == 0;
        const u32 combo = edge_row ? (((i + variant) % 2 == 0) ? 31u : 0u) : (u32)((i * 7 + 3 + variant) % 32);
        head_in[i] = (u32)((i + variant) & 1) | (u32)((i % 16) << 1) | (u32)((rnd() & 0xff) << 8) | (u32)((rnd() & 3) << 16) | (combo << 20);
        id[i] = rnd(); addr[i] = rnd(); val[i] = i % 3 ? rnd() : ~0ull; prev[i] = i % 5 ? rnd() : 0;
        for (int s = 0; s < 5; s++)
            if ((combo >> s) & 1) { u64 w[4]; edge_word(uses[s]++, w); pool.insert(pool.end(), w, w + 4); }
        if (mode == 2) ctr_in[i] = (i ? ctr_in[i - 1] : rnd() >> 24) + 1 + rnd() % 1000;
    }
    const u64 rw_base = mode == 1 ? 0ull - n : 1ull, n_pool = pool.size() / 4;
    char msg[256];
    if (trw_plan_counts(n, 0, rw_base, mode == 2, msg, sizeof msg)) { fprintf(stderr, "trace_witness_asan: %s\n", msg); return 1; }
    std::vector<u32> head(n), flags(n);
    std::vector<u64> ctr(mode == 2 ? n : 0), off(n), out(n * TRW_RW_NCELLS * 4);
    u64 v[TRW_V_WORDS];
    trw_check_host(head_in.data(), mode == 2 ? ctr_in.data() : nullptr, n, nullptr, 0, head.data(), mode == 2 ? ctr.data() : nullptr, off.data(), v);
    if (trw_verdict_error(v, n_pool, msg, sizeof msg)) { fprintf(stderr, "trace_witness_asan: %s\n", msg); return 1; }
    TrwArgs a;
    memset(&a, 0, sizeof a);
    a.id = id.data(); a.addr = addr.data(); a.val = val.data(); a.prev = prev.data(); a.pool = n_pool ? pool.data() : nullptr;
    a.n_rw = n; a.n_pool = n_pool; a.rw_base = rw_base;
    a.head = head.data(); a.ctr = mode == 2 ? ctr.data() : nullptr; a.off = off.data(); a.rw = out.data(); a.rw_flags = flags.data();
    for (u64 row = 0; row < n; row++) {
        for (u32 q = 0; q < TRW_RW_PIECES; q++) trw_rw_piece(a, row, head[row], off[row], q, out[(row * TRW_RW_PIECES + q) * 2], out[(row * TRW_RW_PIECES + q) * 2 + 1]);
        flags[row] = trw_rw_flag(head[row]);
    }
    // the cell-by-cell construction
    int bad = 0;
    u64 at = 0;
    for (u64 i = 0; i < n; i++) {
        const u32 h = head_in[i];
        const u64* r = &out[i * TRW_RW_NCELLS * 4];
        const u64* w[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
        for (int s = 0; s < 5; s++)
            if ((h >> (20 + s)) & 1) w[s] = &pool[4 * at++];
        bad += !cell_is(r, mode == 2 ? ctr_in[i] : rw_base + i, 0, 0, 0) || !cell_is(r + 4, h & 1, 0, 0, 0) || !cell_is(r + 8, (h >> 1) & 15, 0, 0, 0);
        bad += !cell_is(r + 12, id[i], 0, 0, 0) || !cell_is(r + 20, (h >> 8) & 255, 0, 0, 0) || flags[i] != ((h >> 16) & 3);
        u64 m[4];
        if (w[0]) { mod_p(w[0], m); bad += memcmp(r + 16, m, 32) != 0; }
        else bad += !cell_is(r + 16, addr[i], 0, 0, 0);
        for (int s : {1, 4}) {
            const u64* lo = r + (s == 1 ? 24 : 48);
            bad += w[s] ? (!cell_is(lo, w[s][0], w[s][1], 0, 0) || !cell_is(lo + 4, w[s][2], w[s][3], 0, 0)) : (!cell_is(lo, 0, 0, 0, 0) || !cell_is(lo + 4, 0, 0, 0, 0));
        }
        for (int s : {2, 3}) {
            const u64* lo = r + (s == 2 ? 32 : 40);
            const bool word = (h >> (s == 2 ? 16 : 17)) & 1;
            if (!w[s]) bad += !cell_is(lo, s == 2 ? val[i] : prev[i], 0, 0, 0) || !cell_is(lo + 4, 0, 0, 0, 0);
            else if (word) bad += !cell_is(lo, w[s][0], w[s][1], 0, 0) || !cell_is(lo + 4, w[s][2], w[s][3], 0, 0);
            else { mod_p(w[s], m); bad += memcmp(lo, m, 32) != 0 || !cell_is(lo + 4, 0, 0, 0, 0); }
        }
    }
    bad += at != n_pool;
    if (bad) fprintf(stderr, "trace_witness_asan: %d RW mismatches (%llu rows, variant %d, mode %d)\n", bad, (unsigned long long)n, variant, mode);
    return bad;
}

static int run_steps(u64 n) {
    std::vector<u64> rec(n * TRW_STEP_WORDS), out(n * TRW_STEP_NCELLS * 4);
    for (u64 i = 0; i < n; i++) {
        u64* r = &rec[i * TRW_STEP_WORDS];
        r[0] = (i % 3 == 0 ? 0 : i % 3 == 1 ? 255 : rnd() & 255) | ((i / 3 % 4) << 8);
        for (int k = 1; k < 9; k++) r[k] = (i + k) % 3 == 0 ? 0 : (i + k) % 3 == 1 ? ~0ull : rnd();
        edge_word(i, r + 9);
    }
    u64 v[TRW_V_WORDS];
    char msg[256];
    trw_check_host(nullptr, nullptr, 0, rec.data(), n, nullptr, nullptr, nullptr, v);
    if (trw_verdict_error(v, 0, msg, sizeof msg)) { fprintf(stderr, "trace_witness_asan: %s\n", msg); return 1; }
    TrwArgs a;
    memset(&a, 0, sizeof a);
    a.steps_in = rec.data(); a.n_steps = n; a.steps = out.data();
    for (u64 row = 0; row < n; row++)
        for (u32 q = 0; q < TRW_STEP_PIECES; q++) trw_step_piece(a, row, q, out[(row * TRW_STEP_PIECES + q) * 2], out[(row * TRW_STEP_PIECES + q) * 2 + 1]);
    int bad = 0;
    for (u64 i = 0; i < n; i++) {
        const u64* r = &rec[i * TRW_STEP_WORDS];
        const u64* o = &out[i * TRW_STEP_NCELLS * 4];
        const u64 want[13][2] = {{r[0] & 255, 0}, {r[1], 0}, {r[2], 0}, {(r[0] >> 8) & 1, 0}, {(r[0] >> 9) & 1, 0}, {r[9], r[10]}, {r[11], r[12]},
                                 {r[3], 0}, {r[4], 0}, {r[5], 0}, {r[6], 0}, {r[7], 0}, {r[8], 0}};
        for (int c = 0; c < 13; c++) bad += !cell_is(o + 4 * c, want[c][0], want[c][1], 0, 0);
    }
    if (bad) fprintf(stderr, "trace_witness_asan: %d step mismatches (%llu rows)\n", bad, (unsigned long long)n);
    return bad;
}

// the open's checks reject what they must (no row function runs then)
static int run_rejections() {
    int bad = 0;
    char msg[256];
    u64 v[TRW_V_WORDS];
    std::vector<u32> head = {0, 1u << 20, 1u << 5};
    std::vector<u64> ctr = {5, 9, 9};
    trw_check_host(head.data(), ctr.data(), 3, nullptr, 0, nullptr, nullptr, nullptr, v);
    bad += v[TRW_V_HEAD] != 2 || v[TRW_V_ORDER] != 2 || v[TRW_V_POOL] != 1 || trw_verdict_error(v, 1, msg, sizeof msg) != -70;
    head[2] = 0;
    trw_check_host(head.data(), ctr.data(), 3, nullptr, 0, nullptr, nullptr, nullptr, v);
    bad += trw_verdict_error(v, 1, msg, sizeof msg) != -71;
    ctr[2] = 10;
    trw_check_host(head.data(), ctr.data(), 3, nullptr, 0, nullptr, nullptr, nullptr, v);
    bad += trw_verdict_error(v, 2, msg, sizeof msg) != -72 || trw_verdict_error(v, 1, msg, sizeof msg) != 0;
    std::vector<u64> step(13, 0);
    step[0] = 1u << 10;
    trw_check_host(nullptr, nullptr, 0, step.data(), 1, nullptr, nullptr, nullptr, v);
    bad += trw_verdict_error(v, 0, msg, sizeof msg) != -70;
    bad += trw_plan_counts(1ull << 31, 0, 1, false, msg, sizeof msg) != -73 || trw_plan_counts(0, 1ull << 31, 1, false, msg, sizeof msg) != -73;
    bad += trw_plan_counts(4, 0, 0ull - 3, false, msg, sizeof msg) != -71 || trw_plan_counts(4, 0, 0ull - 4, false, msg, sizeof msg) != 0;
    bad += trw_plan_counts(4, 0, 0ull - 3, true, msg, sizeof msg) != 0;
    if (bad) fprintf(stderr, "trace_witness_asan: %d rejection mismatches\n", bad);
    return bad;
}

int main() {
    int bad = 0, k = 0;
    for (u64 n : {1ull, 2ull, 3ull, 15ull, 16ull, 17ull, 63ull, 64ull, 65ull, 255ull, 256ull, 257ull, 1023ull, 1024ull, 1025ull, 4097ull})
        for (int variant = 0; variant < 2; variant++, k++) bad += run_rw(n, variant, k % 3);
    for (u64 n : {1ull, 2ull, 31ull, 32ull, 33ull, 64ull, 65ull, 1025ull}) bad += run_steps(n);
    bad += run_rw(0, 0, 0) + run_steps(0) + run_rejections();
    printf("trace_witness_asan: %s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
