// Stand-alone host program (TEST INFRASTRUCTURE): the row writer's header functions (csrc/state_assign.hpp asg_row_cells_of /
// asg_write_row_of over csrc/state_trace.hpp's stream records) and the CPU backend's zk_state_assign_from_trace* over exactly-sized heap
// buffers, built with -fsanitize=address,undefined by tests/test_state_assign_trace_cpu.py and run as a child process.  Seeded tame record
// tables (every combination of the pool bits, pool words at the edges of 2^128, 2^160, p and 2^256, counters from rw_base and explicit, prev
// null).  Three results are compared for the 57-cell and the compact form: the session over the records, the from-RW session over the
// expanded rows, and the device's chain replayed on the host — the sorted packed op stream, the MPT passes by asg_insert_by /
// asg_find_first_by over strc_mpt_key, the root back-fill, asg_write_row_of over strc_row_slot — each into buffers of exactly n_ops rows.
// Exit status 0 = no mismatch (the sanitizers abort on their own findings).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../zkevm_specs_amd/csrc/cpu_backend.cpp"

static u64 rnd_state = 0x9e3779b97f4a7c15ull;
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
// tame rows only (tags 1..11, pool addresses below 2^160, Account field tags 1..4), few distinct keys so that key groups have several
// accesses; keyed: 0 = no Storage / Account row at all, 1 = mixed, 2 = the last op in State order is keyed (no tag above Account)
static void make(Records& r, u64 n, int variant, int mode, int keyed) {
    r.head.assign(n, 0);
    r.id.assign(n, 0); r.addr.assign(n, 0); r.val.assign(n, 0); r.prev.assign(n, 0);
    r.ctr.assign(mode == 2 ? n : 0, 0);
    r.pool.clear();
    u64 uses[5] = {0, 3, 6, 9, 1};
    for (u64 i = 0; i < n; i++) {
        const bool edge_row = i == 0 || i == n - 1 || i % 16 == 15 || i % 16 == 0;
        u32 combo = edge_row ? (((i + variant) % 2 == 0) ? 31u : 0u) : (u32)((i * 7 + 3 + variant) % 32);
        u32 tag = 1u + (u32)(i % 11);
        if (keyed == 0 && (tag == 5u || tag == 6u)) tag = 9u;
        if (keyed == 2 && (tag > 6u || (tag >= 2u && tag <= 4u))) tag = 5u + (u32)(i & 1);  // (Targets 2-4, 10, 11 sort behind Account)
        const u32 ft = tag == 5u ? 1u + (u32)(i % 4) : (u32)(rnd() & 1);
        r.head[i] = (u32)((i + variant) & 1) | (tag << 1) | (ft << 8) | (u32)((rnd() & 3) << 16) | (combo << 20);
        r.id[i] = rnd() % 3; r.addr[i] = tag == 7u ? rnd() % 25 : rnd() % 3; r.val[i] = i % 3 ? rnd() : ~0ull; r.prev[i] = i % 5 ? rnd() : 0;
        for (int s = 0; s < 5; s++)
            if ((combo >> s) & 1) {
                u64 w[4];
                edge_word(s == 1 ? uses[s]++ % 3 : uses[s]++, w);  // (three storage keys)
                if (s == 0) { w[1] = w[2] = w[3] = 0; w[0] %= 3; }  // three pool addresses
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

struct Witness {
    u64 n_ops = 0, n_mpt = 0;
    std::vector<u64> rows, mpt;
    std::vector<u32> flags, status;
    zk_result res;
};
static bool same(const Witness& a, const Witness& b) {
    return a.n_ops == b.n_ops && a.n_mpt == b.n_mpt && a.rows == b.rows && a.mpt == b.mpt && a.flags == b.flags && a.status == b.status &&
           a.res.fail_count == b.res.fail_count && a.res.first_fail_row == b.res.first_fail_row && a.res.first_fail_code == b.res.first_fail_code &&
           a.res.rows_evaluated == b.res.rows_evaluated;
}
// an opened assignment session run and read into buffers of exactly n_ops rows / n_mpt MPT rows
static int run_session(zk_session* s, u64 n_ops, bool compact, Witness& w) {
    w.n_ops = n_ops;
    int rc = zk_launch(s, nullptr);
    if (!rc) rc = zk_collect(s, &w.res);
    if (!rc) rc = zk_state_assign_read(s, nullptr, nullptr, nullptr, 0, &w.n_mpt);
    w.rows.assign(n_ops * (compact ? 15 : 57) * 4, 0); w.flags.assign(n_ops, 0); w.status.assign(n_ops, 0); w.mpt.assign(w.n_mpt * 48, 0);
    if (!rc) rc = zk_state_assign_read(s, w.rows.data(), w.flags.data(), w.mpt.data(), w.n_mpt, &w.n_mpt);
    if (!rc) rc = zk_read_status(s, w.status.data());
    zk_close(s);
    return rc;
}
// the device's chain on the host, from the records and the sorted order
static void replay(const Records& r, const std::vector<u64>& order_ctr, bool compact, Witness& w) {
    const u64 n = r.t.n_rw, n_ops = order_ctr.size();
    std::vector<u32> head(n);
    std::vector<u64> off(n), stream(n_ops * STRC_STREAM_WORDS);
    u64 v[TRW_V_WORDS];
    trw_check_host(r.head.data(), r.t.rw_counter, n, nullptr, 0, head.data(), nullptr, off.data(), v);
    StrcArgs c;
    memset(&c, 0, sizeof c);
    c.head = head.data(); c.ctr = r.t.rw_counter; c.id = r.t.id; c.addr = r.t.addr; c.val = r.t.val; c.off = off.data(); c.pool = r.t.pool;
    c.n = n; c.rw_base = r.rw_base; c.stream = stream.data();
    strc_stream_store(c.stream, 0, strc_stream_start());
    for (u64 j = 1; j < n_ops; j++) {  // op j is the record with op j's counter
        u64 row = order_ctr[j] - r.rw_base;
        if (r.t.rw_counter) { row = 0; while (r.ctr[row] != order_ctr[j]) row++; }
        strc_stream_store(c.stream, j, strc_load(c, row));
    }
    u32 cap = 16;
    while (cap < 2 * n_ops + 2) cap <<= 1;
    std::vector<u32> slots(cap, ZK_EMPTY_SLOT), first(n_ops, ASG_NONE), rank(n_ops, 0);
    w.n_ops = n_ops;
    w.rows.assign(n_ops * (compact ? 15 : 57) * 4, 0); w.flags.assign(n_ops, 0); w.status.assign(n_ops, 0);
    AssignArgs a;
    memset(&a, 0, sizeof a);
    a.n = n_ops; a.compact = compact; a.rows = w.rows.data(); a.row_flags = w.flags.data(); a.slots = slots.data(); a.mask = cap - 1;
    const auto key_of = [&c](u32 j) { return strc_mpt_key(c, j); };
    for (u64 j = 0; j < n_ops; j++)
        if (strc_stream_has_key(c, j)) asg_insert_by(a, (u32)j, key_of);
    u32 n_mpt = 0;
    for (u64 j = 0; j < n_ops; j++)
        if (strc_stream_has_key(c, j)) {
            first[j] = asg_find_first_by(a, (u32)j, key_of);
            if (first[j] == (u32)j) rank[j] = n_mpt++;
        }
    w.n_mpt = n_mpt;
    w.mpt.assign((u64)n_mpt * 48, 0);
    u32 next_rank = n_mpt;  // the rank of the first access of the next keyed op's key; behind the last keyed op: n_mpt
    w.res.fail_count = 0; w.res.first_fail_row = 0; w.res.first_fail_code = 0; w.res.rows_evaluated = n_ops;
    for (u64 j = n_ops; j-- > 0;) {
        const StrcRow row = strc_stream_row(c, j);
        const bool start = j == 0;
        const auto slot = [&row, start](u32 s) { return strc_row_slot(row, s, start); };
        w.status[j] = asg_write_row_of<true>(a, j, 3ull + 5ull * next_rank, first[j] == (u32)j, slot, strc_row_flags(row, start));
        if (first[j] == (u32)j) {
            Fr q[ASG_MPT_NCELLS];
            asg_mpt_cells_of(slot, strc_row_flags(row, start), rank[j], q);
            for (int x = 0; x < ASG_MPT_NCELLS; x++)
                for (int k = 0; k < 4; k++) w.mpt[((u64)rank[j] * 12 + x) * 4 + k] = (u64)q[x].v[2 * k] | ((u64)q[x].v[2 * k + 1] << 32);
        }
        if (first[j] != ASG_NONE) next_rank = rank[first[j]];
        if (w.status[j]) { w.res.fail_count++; w.res.first_fail_row = j; w.res.first_fail_code = w.status[j]; }
    }
}

static int run(u64 n, int variant, int mode, int keyed) {
    int bad = 0;
    Records r;
    make(r, n, variant, mode, keyed);
    std::vector<u64> rw(n * TRW_RW_NCELLS * 4), prev0(n, 0);
    std::vector<u32> fl(n);
    zk_trace full = r.t;
    full.prev = prev0.data();  // (the expansion reads prev; value_prev is not part of any State result)
    zk_trace_witness wire = {rw.data(), fl.data(), nullptr};
    zk_result res;
    if (zk_evm_witness_from_trace(&full, &wire, 0, &res)) { fprintf(stderr, "state_assign_trace_asan: %s\n", zk_last_error()); return 1; }
    for (int compact = 0; compact < 2; compact++) {
        const u32 opts = compact ? ZK_OPT_STATE_COMPACT : 0u;
        Witness got, want, host, shot;
        zk_session* s = nullptr;
        u64 n_ops = 0, n_ops2 = 0;
        if (zk_state_assign_from_trace_open(&r.t, nullptr, nullptr, nullptr, opts, &n_ops, &s) || run_session(s, n_ops, compact, got)) {
            fprintf(stderr, "state_assign_trace_asan: %s\n", zk_last_error());
            return 1;
        }
        if (zk_state_assign_from_rw_open(rw.data(), fl.data(), n, nullptr, nullptr, nullptr, opts, &n_ops2, &s) || run_session(s, n_ops2, compact, want)) {
            fprintf(stderr, "state_assign_trace_asan: %s\n", zk_last_error());
            return 1;
        }
        bad += !same(got, want);
        // the one-shot, into buffers of its documented capacity (n_rw + 1 rows), compared over n_ops rows
        shot.rows.assign((n + 1) * (compact ? 15 : 57) * 4, 0); shot.flags.assign(n + 1, 0); shot.status.assign(n + 1, 0); shot.mpt.assign((n + 1) * 48, 0);
        if (zk_state_assign_from_trace(&r.t, shot.rows.data(), shot.flags.data(), shot.mpt.data(), &shot.n_mpt, &shot.n_ops, opts, shot.status.data(), &shot.res)) {
            fprintf(stderr, "state_assign_trace_asan: %s\n", zk_last_error());
            return 1;
        }
        shot.rows.resize(got.rows.size()); shot.flags.resize(n_ops); shot.status.resize(n_ops); shot.mpt.resize(got.mpt.size());
        bad += !same(shot, got);
        std::vector<u64> order_ctr(n_ops, 0);  // the sorted order, read off the rows' rw_counter column
        for (u64 j = 0; j < n_ops; j++) order_ctr[j] = got.rows[j * 4];
        replay(r, order_ctr, compact != 0, host);
        if (host.res.fail_count == 0) host.res.first_fail_row = got.res.first_fail_row, host.res.first_fail_code = got.res.first_fail_code;
        bad += !same(host, got);
        bad += keyed == 0 && got.n_mpt != 0;
        bad += got.res.fail_count != 0;  // tame tables: every op is assigned
    }
    if (bad) fprintf(stderr, "state_assign_trace_asan: %d mismatches (%llu rows, variant %d, mode %d, keyed %d)\n", bad, (unsigned long long)n, variant, mode, keyed);
    return bad;
}

int main() {
    int bad = 0, k = 0;
    for (u64 n : {1ull, 2ull, 31ull, 63ull, 64ull, 255ull, 256ull, 257ull, 700ull})
        for (int variant = 0; variant < 2; variant++, k++) bad += run(n, variant, k % 3, k % 3 == 0 ? (k / 3) % 3 : 1);
    printf("state_assign_trace_asan: %s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
