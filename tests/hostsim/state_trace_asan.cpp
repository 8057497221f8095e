// Stand-alone host program (TEST INFRASTRUCTURE): the per-row functions of csrc/state_trace.hpp and the CPU backend's
// zk_state_verify_from_trace / zk_state_ops_from_trace over exactly-sized heap buffers, built with -fsanitize=address,undefined by
// tests/test_state_trace_cpu.py and run as a child process.  A few hundred seeded records per shape: every combination of the pool bits,
// all-wide and all-narrow rows at the ends, pool words at the edges of 2^128, 2^160, p and 2^256, counters from rw_base (1 and 2^64 - n)
// and explicit, prev null.  Every cell strc_cell / strc_row_cell give is compared with trw_rw_piece's; the sorted packed op stream is
// stored and loaded back; the entries' results are compared with the _from_rw entries' over the expanded rows.  Exit status 0 = no
// mismatch (the sanitizers abort on their own findings).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../zkevm_specs_amd/csrc/cpu_backend.cpp"

static u64 rnd_state = 0x2545f4914f6cdd1dull;
static u64 rnd() {
    rnd_state ^= rnd_state << 13; rnd_state ^= rnd_state >> 7; rnd_state ^= rnd_state << 17;
    return rnd_state;
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
    case 7: w[0] = w[1] = ~0ull; w[2] = 0xffffffffull; break;  // 2^160 - 1
    case 8: w[0] = w[1] = w[2] = w[3] = ~0ull; break;
    case 9: w[2] = 1ull << 32; break;                            // 2^160
    default: for (int j = 0; j < 4; j++) w[j] = rnd(); break;
    }
}

struct Records {
    std::vector<u32> head;
    std::vector<u64> id, addr, val, prev, ctr, pool;
    u64 rw_base = 1;
    zk_trace t;
};
// tame: only what leaves a witness (tags 1..11, small pool addresses, Account field tags 1..4) — the verdict entry returns a verdict
static void make(Records& r, u64 n, int variant, int mode, bool tame) {
    r.head.assign(n, 0);
    r.id.assign(n, 0); r.addr.assign(n, 0); r.val.assign(n, 0); r.prev.assign(n, 0);
    r.ctr.assign(mode == 2 ? n : 0, 0);
    r.pool.clear();
    u64 uses[5] = {0, 3, 6, 9, 1};
    for (u64 i = 0; i < n; i++) {
        const bool edge_row = i == 0 || i == n - 1 || i % 16 == 15 || i % 16 == 0;
        u32 combo = edge_row ? (((i + variant) % 2 == 0) ? 31u : 0u) : (u32)((i * 7 + 3 + variant) % 32);
        u32 tag = tame ? 1u + (u32)(i % 11) : (u32)(i % 16);
        u32 ft = tame ? (tag == 5u ? 1u + (u32)(i % 4) : (u32)(rnd() & 1)) : (u32)(rnd() & 0xff);
        r.head[i] = (u32)((i + variant) & 1) | (tag << 1) | (ft << 8) | (u32)((rnd() & 3) << 16) | (combo << 20);
        r.id[i] = rnd() % 7; r.addr[i] = tag == 7u ? rnd() % 30 : rnd() % 5; r.val[i] = i % 3 ? rnd() : ~0ull; r.prev[i] = i % 5 ? rnd() : 0;
        for (int s = 0; s < 5; s++)
            if ((combo >> s) & 1) {
                u64 w[4];
                edge_word(uses[s]++, w);
                if (s == 0 && tame) { w[2] &= 0xffffffffull; w[3] = 0; }  // an address below 2^160
                r.pool.insert(r.pool.end(), w, w + 4);
            }
        if (mode == 2) r.ctr[i] = (i ? r.ctr[i - 1] : rnd() >> 24) + 1 + rnd() % 1000;
    }
    r.rw_base = mode == 1 ? 0ull - n : 1ull;
    memset(&r.t, 0, sizeof r.t);
    r.t.head = r.head.data(); r.t.id = r.id.data(); r.t.addr = r.addr.data(); r.t.val = r.val.data();
    r.t.prev = variant ? nullptr : r.prev.data();  // (never read)
    r.t.rw_counter = mode == 2 ? r.ctr.data() : nullptr;
    r.t.rw_base = r.rw_base; r.t.n_rw = n;
    r.t.pool = r.pool.empty() ? nullptr : r.pool.data(); r.t.n_pool = r.pool.size() / 4;
}

static bool fr_is(const Fr& x, const u64* c) {
    for (int w = 0; w < 4; w++)
        if (((u64)x.v[2 * w] | ((u64)x.v[2 * w + 1] << 32)) != c[w]) return false;
    return true;
}

// the per-row functions against trw_rw_piece, the stream round trip
static int run_cells(u64 n, int variant, int mode) {
    Records r;
    make(r, n, variant, mode, false);
    std::vector<u32> head(n);
    std::vector<u64> ctr(mode == 2 ? n : 0), off(n), out(n * TRW_RW_NCELLS * 4), stream(n * STRC_STREAM_WORDS);
    u64 v[TRW_V_WORDS];
    char msg[256];
    trw_check_host(r.head.data(), r.t.rw_counter, n, nullptr, 0, head.data(), mode == 2 ? ctr.data() : nullptr, off.data(), v);
    if (trw_verdict_error(v, r.t.n_pool, msg, sizeof msg)) { fprintf(stderr, "state_trace_asan: %s\n", msg); return 1; }
    TrwArgs a;
    memset(&a, 0, sizeof a);
    a.id = r.id.data(); a.addr = r.addr.data(); a.val = r.val.data(); a.prev = r.prev.data(); a.pool = r.t.pool;
    a.n_rw = n; a.n_pool = r.t.n_pool; a.rw_base = r.rw_base;
    a.head = head.data(); a.ctr = mode == 2 ? ctr.data() : nullptr; a.off = off.data(); a.rw = out.data();
    StrcArgs c;
    memset(&c, 0, sizeof c);
    c.head = head.data(); c.ctr = a.ctr; c.id = a.id; c.addr = a.addr; c.val = a.val; c.off = off.data(); c.pool = a.pool; c.n = n; c.rw_base = r.rw_base;
    c.stream = stream.data();
    int bad = 0;
    for (u64 row = 0; row < n; row++) {
        for (u32 q = 0; q < TRW_RW_PIECES; q++) trw_rw_piece(a, row, head[row], off[row], q, out[(row * TRW_RW_PIECES + q) * 2], out[(row * TRW_RW_PIECES + q) * 2 + 1]);
        const StrcRec rec = strc_load(c, row);
        const StrcRow R = strc_widen(c.pool, rec);
        strc_stream_store(c.stream, row, rec);
        const StrcRow S = strc_stream_row(c, row);
        for (u32 k = 0; k < TRW_RW_NCELLS; k++) {
            if (k == 10 || k == 11) continue;
            const u64* want = &out[(row * TRW_RW_NCELLS + k) * 4];
            bad += !fr_is(strc_cell(c, row, head[row], off[row], k), want) || !fr_is(strc_row_cell(R, k), want) || !fr_is(strc_row_cell(S, k), want);
        }
        const u64* p = &out[row * TRW_RW_NCELLS * 4];
        const RwkKey k0 = rwk_key(p), k1 = strc_key(R);
        bad += k0.cls != k1.cls || k0.status != k1.status;
        for (int f = 0; f < RWK_NFIELDS; f++) bad += !fr_eq(k0.f[f], k1.f[f]);
        const RwkOp o0 = rwk_op(p, trw_rw_flag(head[row]), k0), o1 = strc_op(R, k1);
        bad += o0.flags != o1.flags || !fr_eq(o0.rw, o1.rw) || !fr_eq(o0.vlo, o1.vlo) || !fr_eq(o0.vhi, o1.vhi) || !fr_eq(o0.ilo, o1.ilo) || !fr_eq(o0.ihi, o1.ihi);
    }
    if (bad) fprintf(stderr, "state_trace_asan: %d cell mismatches (%llu rows, variant %d, mode %d)\n", bad, (unsigned long long)n, variant, mode);
    return bad;
}

// the CPU entries against the _from_rw entries over the expanded rows
static int run_entries(u64 n, int variant, int mode) {
    int bad = 0;
    for (int tame = 0; tame < 2; tame++) {
        Records r;
        make(r, n, variant, mode, tame != 0);
        std::vector<u64> rw(n * TRW_RW_NCELLS * 4), prev0(n, 0);
        std::vector<u32> fl(n);
        zk_trace full = r.t;
        full.prev = prev0.data();  // (the expansion reads prev; value_prev is not part of any State result)
        full.steps = nullptr; full.n_steps = 0;
        zk_trace_witness w = {rw.data(), fl.data(), nullptr};
        zk_result res, res2;
        if (zk_evm_witness_from_trace(&full, &w, 0, &res)) { fprintf(stderr, "state_trace_asan: %s\n", zk_last_error()); return 1; }
        u64 n_ops = 0, n_ops2 = 0;
        std::vector<u32> st(n), st2(n), of(n + 1), of2(n + 1);
        std::vector<u64> ops((n + 1) * 48), ops2((n + 1) * 48);
        const int rc = zk_state_ops_from_trace(&r.t, ops.data(), of.data(), &n_ops, 0, st.data(), &res);
        const int rc2 = zk_state_ops_from_rw(rw.data(), fl.data(), n, ops2.data(), of2.data(), &n_ops2, 0, st2.data(), &res2);
        bad += rc != 0 || rc2 != 0 || n_ops != n_ops2 || res.fail_count != res2.fail_count || st != st2;
        bad += memcmp(ops.data(), ops2.data(), n_ops * 48 * 8) != 0 || memcmp(of.data(), of2.data(), n_ops * 4) != 0;
        std::vector<u32> vs(n_ops), vs2(n_ops);  // exactly n_ops codes
        const int vrc = zk_state_verify_from_trace(&r.t, 0, vs.data(), &n_ops, &res);
        const int vrc2 = zk_state_verify_from_rw(rw.data(), fl.data(), n, 0, vs2.data(), &n_ops2, &res2);
        bad += vrc != vrc2 || (tame && vrc != 0);
        if (!vrc) bad += n_ops != n_ops2 || vs != vs2 || res.fail_count != res2.fail_count || res.first_fail_row != res2.first_fail_row || res.first_fail_code != res2.first_fail_code;
    }
    if (bad) fprintf(stderr, "state_trace_asan: %d entry mismatches (%llu rows, variant %d, mode %d)\n", bad, (unsigned long long)n, variant, mode);
    return bad;
}

int main() {
    int bad = 0, k = 0;
    for (u64 n : {1ull, 2ull, 15ull, 16ull, 17ull, 63ull, 64ull, 65ull, 255ull, 256ull, 257ull, 1025ull})
        for (int variant = 0; variant < 2; variant++, k++) bad += run_cells(n, variant, k % 3);
    for (u64 n : {1ull, 2ull, 63ull, 64ull, 65ull, 300ull})
        for (int variant = 0; variant < 2; variant++, k++) bad += run_entries(n, variant, k % 3);
    printf("state_trace_asan: %s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
