// Stand-alone host program (TEST INFRASTRUCTURE): the functions of csrc/copy_sources.hpp and the CPU backend's zk_copy_assign_from_sources
// over exactly-sized heap buffers, built with -fsanitize=address,undefined by tests/test_copy_sources_cpu.py and run as a child process.
// Shaped events (lengths 0, 1, 63, 64, 65, 129, 1000; padding suffixes; every source and destination kind; dense and explicit counters;
// codes whose pushes cross chunk, segment and code ends, an empty code, an empty tx, calldata at an odd address) and the failing sites 1-6
// with the damaged byte first, at 63 / 64 and last.  The statuses are compared with what the events were built to give, the is_code bits
// with a per-byte recurrence written out here, the rows with zk_copy_assign over the gathered data.  Exit status 0 = no mismatch (the
// sanitizers abort on their own findings).
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
#define CHECK(cond, ...) do { if (!(cond)) { printf("copy_sources_asan: " __VA_ARGS__); printf("\n"); exit(1); } } while (0)

struct Op { u64 ctr; u32 head; u64 id, addr, val; bool dead; };
struct Block {
    std::vector<u64> cells;  // [n][12][4]
    std::vector<u32> flags, src_ref, dst_ref, want;
    std::vector<uint8_t> code, calldata;
    std::vector<u64> code_off{0}, cd_off{0};
    std::vector<Op> ops;
    u64 rwc = 7;
    u32 add_code(u64 n, u64 push_every) {
        for (u64 b = 0; b < n; b++) code.push_back(push_every && b % push_every == push_every - 1 ? 0x7f : (uint8_t)(rnd() % 0x60));
        code_off.push_back(code.size());
        return (u32)code_off.size() - 2;
    }
    u32 add_tx(u64 n) {
        for (u64 b = 0; b < n; b++) calldata.push_back((uint8_t)rnd());
        cd_off.push_back(calldata.size());
        return (u32)cd_off.size() - 2;
    }
    // -> index of the first op appended
    size_t copy(u32 st, u32 dt, u64 src_addr, u64 src_end, u64 dst_addr, u64 length, u32 sref, u32 dref, u32 site) {
        const u64 room = src_end > src_addr ? src_end - src_addr : 0, n_real = room < length ? room : length;
        const size_t op0 = ops.size();
        const u64 v[12] = {7, 0, st, 8, 0, dt, src_addr, src_end, dst_addr, length, 2, rwc};
        for (int k = 0; k < 12; k++) { cells.push_back(v[k]); cells.push_back(0); cells.push_back(0); cells.push_back(0); }
        flags.push_back(0); src_ref.push_back(sref); dst_ref.push_back(dref); want.push_back(site);
        const bool dst_rw = dt == CPA_MEMORY || dt == CPA_TX_LOG;
        for (u64 i = 0; i < length; i++) {
            if (st == CPA_MEMORY && i < n_real) ops.push_back(Op{rwc++, (u32)CPA_TARGET_MEMORY << 1, 7, src_addr + i, rnd() % 256, false});
            if (dst_rw) ops.push_back(Op{rwc++, ((u32)(dt == CPA_MEMORY ? CPA_TARGET_MEMORY : CPA_TARGET_TX_LOG) << 1) | 1u, 8, dst_addr + i, 0, false});
        }
        return op0;
    }
};

static void run(Block& b, bool explicit_ctr, const char* what) {
    std::vector<u32> head;
    std::vector<u64> id, addr, val, ctr;
    for (const Op& o : b.ops)
        if (!o.dead) { head.push_back(o.head); id.push_back(o.id); addr.push_back(o.addr); val.push_back(o.val); ctr.push_back(o.ctr); }
    const u64 n = b.flags.size();
    const u64 rand_cell[4] = {0x1234567812345678ull, 0x9abcdef09abcdef0ull, 0x1111, 0};
    // calldata at an odd address, every array exactly sized
    std::vector<uint8_t> cd(b.calldata.size() + 1);
    if (!b.calldata.empty()) memcpy(cd.data() + 1, b.calldata.data(), b.calldata.size());
    zk_copy_sources t;
    memset(&t, 0, sizeof t);
    t.events = b.cells.data(); t.flags = b.flags.data(); t.n_events = n; t.src_ref = b.src_ref.data(); t.dst_ref = b.dst_ref.data(); t.randomness = rand_cell;
    t.code = b.code.data(); t.n_code_bytes = b.code.size(); t.code_offsets = b.code_off.data(); t.n_codes = b.code_off.size() - 1;
    t.calldata = cd.data() + 1; t.calldata_offsets = b.cd_off.data(); t.n_txs = b.cd_off.size() - 1;
    t.trace.head = head.data(); t.trace.id = id.data(); t.trace.addr = addr.data(); t.trace.val = val.data();
    t.trace.rw_counter = explicit_ctr ? ctr.data() : nullptr; t.trace.rw_base = ctr.empty() ? 1 : ctr[0]; t.trace.n_rw = head.size();
    u64 n_rows = 0, n_table = 0, n_rw = 0, n_data = 0;
    CHECK(zk_copy_assign_from_sources_sizes(&t, 0, &n_rows, &n_table, &n_rw, &n_data) == 0, "%s: sizes: %s", what, zk_last_error());
    std::vector<u64> rows(n_rows * 20 * 4), table(n_table * 14 * 4), rw(n_rw * 14 * 4), offs(n + 1);
    std::vector<u32> rf(n_rows), rwf(n_rw), status(n);
    std::vector<uint16_t> data(n_data);
    zk_result res;
    CHECK(zk_copy_assign_from_sources(&t, rows.data(), rf.data(), table.data(), rw.data(), rwf.data(), data.data(), offs.data(), 0, status.data(), &res) == 0,
          "%s: %s", what, zk_last_error());
    u64 fails = 0;
    for (u64 e = 0; e < n; e++) {
        const u32 exp = b.want[e] ? ((u32)ZK_KIND_VALUE_ERROR << 24) | b.want[e] : 0u;
        CHECK(status[e] == exp, "%s: event %llu status 0x%08x, expected 0x%08x", what, (unsigned long long)e, status[e], exp);
        fails += exp != 0;
    }
    CHECK(res.fail_count == fails && res.rows_evaluated == n && offs[n] == n_data, "%s: tally", what);
    // is_code: the per-byte recurrence, per code
    for (u64 e = 0; e < n; e++) {
        const u64* c = b.cells.data() + e * 48;
        if (b.want[e] || (c[2 * 4] != CPA_BYTECODE && c[5 * 4] != CPA_BYTECODE)) continue;
        const u32 j = c[2 * 4] == CPA_BYTECODE ? b.src_ref[e] : b.dst_ref[e];
        const u64 base = c[2 * 4] == CPA_BYTECODE ? c[6 * 4] : c[8 * 4];
        std::vector<uint8_t> is_code;
        u32 left = 0;
        for (u64 p = b.code_off[j]; p < b.code_off[j + 1]; p++) {
            is_code.push_back(left == 0);
            left = left == 0 ? bcc_push_size(b.code[p]) : left - 1;
        }
        for (u64 i = 0; i < offs[e + 1] - offs[e]; i++)
            CHECK(((data[offs[e] + i] >> 8) & 1u) == is_code[base + i], "%s: event %llu byte %llu is_code", what, (unsigned long long)e, (unsigned long long)i);
    }
    // the composition: zk_copy_assign over the gathered data
    zk_copy_events ce;
    memset(&ce, 0, sizeof ce);
    ce.events = b.cells.data(); ce.flags = b.flags.data(); ce.n_events = n; ce.data = data.data(); ce.data_offsets = offs.data(); ce.randomness = rand_cell;
    std::vector<u64> rows2(rows.size()), table2(table.size()), rw2(rw.size());
    std::vector<u32> rf2(rf.size()), rwf2(rwf.size());
    zk_result res2;
    CHECK(zk_copy_assign(&ce, rows2.data(), rf2.data(), table2.data(), rw2.data(), rwf2.data(), 0, &res2) == 0, "%s: zk_copy_assign: %s", what, zk_last_error());
    CHECK(rows == rows2 && rf == rf2 && table == table2 && rw == rw2 && rwf == rwf2, "%s: rows differ from the composition", what);
}

int main() {
    const u64 lengths[] = {0, 1, 63, 64, 65, 129, 1000};
    for (int explicit_ctr = 0; explicit_ctr < 2; explicit_ctr++) {
        Block b;
        const u32 big = b.add_code(2300, 41), tail = b.add_code(70, 67), empty = b.add_code(0, 0), one = b.add_code(64, 64);
        const u32 t0 = b.add_tx(1100), t1 = b.add_tx(0), t2 = b.add_tx(129);
        (void)empty; (void)t1;
        for (u64 len : lengths) {
            b.copy(CPA_MEMORY, CPA_RLC_ACC, 10, 10 + len, 0, len, 0, 0, 0);
            b.copy(CPA_MEMORY, CPA_MEMORY, 5, 5 + len / 2, 100, len, 0, 0, 0);   // a padding suffix
            b.copy(CPA_MEMORY, CPA_TX_LOG, 0, len, 0, len, 0, 0, 0);
            b.copy(CPA_BYTECODE, CPA_MEMORY, 30, 2300, 0, len, big, 0, 0);
            b.copy(CPA_BYTECODE, CPA_RLC_ACC, 2300 - len / 3, 2300, 0, len, big, 0, 0);
            b.copy(CPA_TX_CALLDATA, CPA_MEMORY, 3, 1100, 0, len, t0, 0, 0);
            b.copy(CPA_MEMORY, CPA_BYTECODE, 0, len, 1, len, 0, big, 0);          // is_code from the destination
        }
        b.copy(CPA_BYTECODE, CPA_BYTECODE, 0, 64, 6, 64, one, tail, 0);
        b.copy(CPA_BYTECODE, CPA_MEMORY, 0, 70, 0, 80, tail, 0, 0);
        b.copy(CPA_BYTECODE, CPA_MEMORY, 0, 0, 0, 3, empty, 0, 0);
        b.copy(CPA_TX_CALLDATA, CPA_RLC_ACC, 0, 0, 0, 2, t1, 0, 0);
        b.copy(CPA_TX_CALLDATA, CPA_RLC_ACC, 0, 129, 0, 129, t2, 0, 0);
        run(b, explicit_ctr != 0, explicit_ctr ? "shaped, explicit counters" : "shaped, dense counters");
    }
    {   // the failing sites
        Block b;
        const u32 code = b.add_code(100, 9), tx = b.add_tx(50);
        b.copy(CPA_BYTECODE, CPA_MEMORY, 0, 10, 0, 10, 5, 0, CPS_SITE_REF);
        b.copy(CPA_TX_CALLDATA, CPA_MEMORY, 0, 10, 0, 10, 1, 0, CPS_SITE_REF);
        b.copy(CPA_MEMORY, CPA_BYTECODE, 0, 10, 0, 10, 0, 1, CPS_SITE_REF);
        b.copy(CPA_BYTECODE, CPA_MEMORY, 0, 101, 0, 101, code, 0, CPS_SITE_SRC_END);
        b.copy(CPA_TX_CALLDATA, CPA_RLC_ACC, 49, 51, 0, 2, tx, 0, CPS_SITE_SRC_END);
        b.copy(CPA_MEMORY, CPA_BYTECODE, 0, 10, 91, 10, 0, code, CPS_SITE_DST_END);
        b.copy(CPA_BYTECODE, CPA_MEMORY, 0, 100, 0, 100, code, 0, 0);
        const u64 n = 130, at[4] = {0, 63, 64, n - 1};
        for (u32 kind = 0; kind < 6; kind++)
            for (u64 i : at) {
                const u32 site = kind == 0 ? CPS_SITE_NO_OP : kind < 4 ? CPS_SITE_NOT_READ : CPS_SITE_NOT_BYTE;
                const size_t k = b.copy(CPA_MEMORY, kind % 2 ? CPA_MEMORY : CPA_RLC_ACC, 40, 40 + n, 0, n, 0, 0, site);
                Op& o = b.ops[k + (kind % 2 ? 2 * i : i)];
                switch (kind) {
                case 0: o.dead = true; break;
                case 1: o.head |= 1u; break;
                case 2: o.id = 9; break;
                case 3: o.addr += 1; break;
                case 4: o.val = 256; break;
                default: o.head |= TRW_H_VALUE_POOL; break;
                }
            }
        const size_t k = b.copy(CPA_MEMORY, CPA_RLC_ACC, 0, n, 0, n, 0, 0, CPS_SITE_NOT_BYTE);  // two sites: the lower byte wins
        b.ops[k + 20].val = 1000;
        b.ops[k + 90].dead = true;
        run(b, true, "failing sites");
    }
    printf("copy_sources_asan: ok\n");
    return 0;
}
