// Stand-alone host program (TEST INFRASTRUCTURE): the functions of csrc/trace_events.hpp and the CPU backend's zk_events_from_trace over
// exactly-sized heap buffers, built with -fsanitize=address,undefined by tests/test_events_from_trace_cpu.py and run as a child process.
// Traces of SHA3 / EXP / CODECOPY / EXTCODECOPY / LOG steps with narrow and pool-word operands, dense and explicit counters, steps whose
// ops are missing or past the end of the trace, hashes outside the set, a pc outside its code, an empty code set, no step at all, and
// ladders of 1 .. 1025 emitting steps.  Every event and status is compared with what the step was built to give.  Exit status 0 = no
// mismatch (the sanitizers abort on their own findings).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../zkevm_specs_amd/csrc/cpu_backend.cpp"

#define CHECK(cond, ...) do { if (!(cond)) { printf("events_from_trace_asan: " __VA_ARGS__); printf("\n"); exit(1); } } while (0)

struct W { u64 w[4]; };
static W word(u64 a, u64 b = 0, u64 c = 0, u64 d = 0) { return W{{a, b, c, d}}; }
static bool narrow(const W& x) { return (x.w[1] | x.w[2] | x.w[3]) == 0; }

struct Trace {
    std::vector<u32> head, want;
    std::vector<u64> id, addr, val, ctr, pool, steps;
    std::vector<uint8_t> code;
    std::vector<u64> code_off{0}, hashes;
    std::vector<u64> copy, exp;      // expected cells
    std::vector<u32> copy_flag, copy_ref, copy_step, exp_step;
    u64 rwc = 5;
    void add_code(const W& h, std::vector<uint8_t> bytes) {
        code.insert(code.end(), bytes.begin(), bytes.end());
        code_off.push_back(code.size());
        for (int k = 0; k < 4; k++) hashes.push_back(h.w[k]);
    }
    void op(u32 tag, u32 field, bool write, u64 id_, u64 addr_, const W& v) {
        u32 h = (write ? 1u : 0u) | (tag << 1) | (field << 8) | TRW_H_VALUE_WORD;
        if (!narrow(v)) { h |= TRW_H_VALUE_POOL; for (int k = 0; k < 4; k++) pool.push_back(v.w[k]); }
        head.push_back(h); id.push_back(id_); addr.push_back(addr_); val.push_back(narrow(v) ? v.w[0] : 0); ctr.push_back(rwc++);
    }
    u64 step(u32 state, u64 call_id, u64 pc, u64 sp, u64 log_id, const W& h, u32 status) {
        const u64 r[13] = {state, rwc, call_id, pc, sp, 1000, 0, 0, log_id, h.w[0], h.w[1], h.w[2], h.w[3]};
        steps.insert(steps.end(), r, r + 13);
        want.push_back(status);
        return want.size() - 1;
    }
    void expect_copy(u64 s, const W& src_id, u32 st, u64 dst_id, u32 dt, u64 a0, u64 a1, u64 d, u64 len, u64 log_id, u64 c, u32 flag, u32 ref) {
        const u64 v[12][2] = {{src_id.w[0], src_id.w[1]}, {src_id.w[2], src_id.w[3]}, {st, 0}, {dst_id, 0}, {0, 0}, {dt, 0}, {a0, 0}, {a1, 0}, {d, 0}, {len, 0}, {log_id, 0}, {c, 0}};
        for (int k = 0; k < 12; k++) { copy.push_back(v[k][0]); copy.push_back(v[k][1]); copy.push_back(0); copy.push_back(0); }
        copy_flag.push_back(flag); copy_ref.push_back(ref); copy_step.push_back((u32)s);
    }
    void sha3(u64 offset, u64 size, u64 call_id, u32 status = 0) {
        const u64 c0 = rwc, s = step(ES_SHA3, call_id, 0, 900, 0, word(1), status);
        op(TG_Stack, 0, false, call_id, 900, word(offset)); op(TG_Stack, 0, false, call_id, 901, word(size)); op(TG_Stack, 0, true, call_id, 901, word(77, 1));
        if (size && !status) expect_copy(s, word(call_id), TEV_TAG_MEMORY, call_id, TEV_TAG_RLC_ACC, offset, offset + size, 0, size, 0, c0 + 3, 0, 0);
    }
    void exp_step_(const W& base, const W& e, u32 status = 0) {
        const u64 c0 = rwc, s = step(ES_EXP, 3, 0, 900, 0, word(1), status);
        op(TG_Stack, 0, false, 3, 900, base); op(TG_Stack, 0, false, 3, 901, e); op(TG_Stack, 0, true, 3, 901, word(1));
        if (!status && !(narrow(e) && e.w[0] <= 1)) {
            const u64 v[5][2] = {{c0 + 3, 0}, {base.w[0], base.w[1]}, {base.w[2], base.w[3]}, {e.w[0], e.w[1]}, {e.w[2], e.w[3]}};
            for (int k = 0; k < 5; k++) { exp.push_back(v[k][0]); exp.push_back(v[k][1]); exp.push_back(0); exp.push_back(0); }
            exp_step.push_back((u32)s);
        }
    }
    void codecopy(u64 mem, u64 coff, u64 size, const W& h, u32 ref, u64 len, u32 status = 0) {
        const u64 c0 = rwc, s = step(ES_CODECOPY, 4, 0, 900, 0, h, status);
        op(TG_Stack, 0, false, 4, 900, word(mem)); op(TG_Stack, 0, false, 4, 901, word(coff)); op(TG_Stack, 0, false, 4, 902, word(size));
        if (size && !status) expect_copy(s, h, TEV_TAG_BYTECODE, 4, TEV_TAG_MEMORY, coff, len, mem, size, 0, c0 + 3, 1, ref);
    }
    void extcodecopy(u64 mem, u64 coff, u64 size, const W& h, u32 ref, u64 len, u32 status = 0) {
        const u64 c0 = rwc, s = step(ES_EXTCODECOPY, 4, 0, 900, 0, word(1), status);
        op(TG_Stack, 0, false, 4, 900, word(9, 9)); op(TG_Stack, 0, false, 4, 901, word(mem)); op(TG_Stack, 0, false, 4, 902, word(coff));
        op(TG_Stack, 0, false, 4, 903, word(size));
        op(TG_CallContext, 0, false, 4, CC_TxId, word(1)); op(TG_CallContext, 0, false, 4, CC_RwCounterEndOfReversion, word(0));
        op(TG_CallContext, 0, false, 4, CC_IsPersistent, word(1)); op(TG_TxAccessListAccount, 0, true, 1, 0, word(1));
        op(TG_Account, ACC_CodeHash, false, 0, 0, h);
        if (size && !status) expect_copy(s, h, TEV_TAG_BYTECODE, 4, TEV_TAG_MEMORY, coff, len, mem, size, 0, c0 + 9, 1, ref);
    }
    void log(u64 mstart, u64 msize, u64 topics, u64 pc, const W& h, u64 log_id, u32 status = 0) {
        const u64 c0 = rwc, s = step(ES_LOG, 6, pc, 900, log_id, h, status);
        op(TG_Stack, 0, false, 6, 900, word(mstart)); op(TG_Stack, 0, false, 6, 901, word(msize));
        op(TG_CallContext, 0, false, 6, CC_TxId, word(2)); op(TG_CallContext, 0, false, 6, CC_IsStatic, word(0));
        op(TG_CallContext, 0, false, 6, CC_CalleeAddress, word(5, 5)); op(TG_CallContext, 0, false, 6, CC_IsPersistent, word(1));
        for (u64 t = 0; t < 1 + 2 * topics; t++) op(TG_TxLog, 0, true, 2, t, word(t));
        if (msize && !status) expect_copy(s, word(6), TEV_TAG_MEMORY, 2, TEV_TAG_TX_LOG, mstart, mstart + msize, 0, msize, log_id + 1, c0 + 7 + 2 * topics, 0, 0);
    }
};

static void run(Trace& t, bool explicit_ctr, const char* what) {
    const u64 ns = t.want.size();
    zk_trace_sources in;
    memset(&in, 0, sizeof in);
    in.trace.head = t.head.data(); in.trace.id = t.id.data(); in.trace.addr = t.addr.data(); in.trace.val = t.val.data();
    in.trace.rw_counter = explicit_ctr ? t.ctr.data() : nullptr; in.trace.rw_base = t.ctr.empty() ? 1 : t.ctr[0]; in.trace.n_rw = t.head.size();
    in.trace.pool = t.pool.data(); in.trace.n_pool = t.pool.size() / 4; in.trace.steps = t.steps.data(); in.trace.n_steps = ns;
    in.code = t.code.data(); in.n_code_bytes = t.code.size(); in.code_offsets = t.code_off.data(); in.n_codes = t.code_off.size() - 1;
    in.code_hashes = t.hashes.data();
    u64 cap = ~0ull;
    CHECK(zk_events_from_trace_sizes(&in, 0, &cap) == 0 && cap == ns, "%s: sizes: %s", what, zk_last_error());
    // every output exactly at its capacity
    std::vector<u64> copy(ns * 48), exp(ns * 20);
    std::vector<u32> flag(ns), ref(ns), cstep(ns), estep(ns), status(ns);
    zk_trace_events out{copy.data(), flag.data(), ref.data(), cstep.data(), exp.data(), estep.data()};
    u64 n_copy = ~0ull, n_exp = ~0ull;
    zk_result res;
    CHECK(zk_events_from_trace(&in, &out, 0, status.data(), &n_copy, &n_exp, &res) == 0, "%s: %s", what, zk_last_error());
    u64 fails = 0;
    for (u64 s = 0; s < ns; s++) {
        CHECK(status[s] == t.want[s], "%s: step %llu status 0x%08x, expected 0x%08x", what, (unsigned long long)s, status[s], t.want[s]);
        fails += t.want[s] != 0;
    }
    CHECK(res.fail_count == fails && res.rows_evaluated == ns, "%s: tally", what);
    CHECK(n_copy == t.copy_step.size() && n_exp == t.exp_step.size(), "%s: %llu copy / %llu EXP events, expected %zu / %zu", what,
          (unsigned long long)n_copy, (unsigned long long)n_exp, t.copy_step.size(), t.exp_step.size());
    copy.resize(n_copy * 48); exp.resize(n_exp * 20); flag.resize(n_copy); ref.resize(n_copy); cstep.resize(n_copy); estep.resize(n_exp);
    CHECK(copy == t.copy && flag == t.copy_flag && ref == t.copy_ref && cstep == t.copy_step, "%s: the copy events differ", what);
    CHECK(exp == t.exp && estep == t.exp_step, "%s: the EXP events differ", what);
}

int main() {
    const u32 S1 = ((u32)ZK_KIND_VALUE_ERROR << 24) | 1, S2 = S1 + 1, S3 = S1 + 2, S4 = S1 + 3;
    const W hA = word(7, 0, 0, 0x1111), hB = word(9, 0, 0x2222), hC = word(5), hX = word(1, 2, 3, 4), big = word(12345, 0, 0xabc, 1ull << 63);
    const std::vector<uint8_t> codeA = {0x60, 0x01, 0xA0, 0xA1, 0xA2, 0xA3, 0xA4, 0x00};
    for (int explicit_ctr = 0; explicit_ctr < 2; explicit_ctr++) {
        Trace t;
        t.add_code(hA, codeA); t.add_code(hB, std::vector<uint8_t>(23, 0x5b)); t.add_code(hA, std::vector<uint8_t>(40, 0)); t.add_code(hC, {});
        t.sha3(64, 32, 1); t.sha3(0, 0, 1); t.sha3(1ull << 62, 1, 1, S3); t.sha3((1ull << 62) - 1, 1, 2, S3);
        t.exp_step_(word(3), word(200)); t.exp_step_(big, big); t.exp_step_(big, word(1)); t.exp_step_(word(2), word(0));
        t.codecopy(0, 2, 5, hA, 0, codeA.size()); t.codecopy(1, 2, 3, hB, 1, 23); t.codecopy(1, 0, 3, hC, 3, 0); t.codecopy(1, 2, 0, hX, 0, 0);
        t.codecopy(1, 2, 3, hX, 0, 0, S4);
        t.extcodecopy(1, 2, 3, hB, 1, 23); t.extcodecopy(1, 2, 3, word(0), 0, 0); t.extcodecopy(1, 2, 3, hX, 0, 0, S4);
        for (u64 topics = 0; topics < 5; topics++) t.log(10, 4 + topics, topics, 2 + topics, hA, topics);
        t.log(10, 4, 0, codeA.size(), hA, 0, S4);   // pc one past the code's last byte
        t.log(10, 4, 0, 1, hA, 0, S4);              // not a LOG opcode
        t.log(10, 4, 0, 2, hX, 0, S4);
        t.log(10, 0, 3, 99, hX, 0);
        // a step whose counters nobody holds (site 1; with dense counters the ops there are another call's: site 2), one whose second op
        // is a write (site 2)
        t.step(ES_SHA3, 1, 0, 900, 0, word(1), explicit_ctr ? S1 : S2);
        t.rwc += explicit_ctr ? 3 : 0;
        t.step(ES_EXP, 3, 0, 900, 0, word(1), S2);
        t.sha3(5, 6, 8);
        {
            const u64 s = t.step(ES_SHA3, 1, 0, 900, 0, word(1), S2);
            (void)s;
            t.op(TG_Stack, 0, false, 1, 900, word(1)); t.op(TG_Stack, 0, true, 1, 901, word(2));
        }
        t.step(ES_CALL_OP, 1, 0, 900, 0, word(1), ((u32)ZK_KIND_UNSUPPORTED << 24) | 1);
        t.step(ES_LOG, 6, 0, 900, 0, hA, S1);       // the trace's last step: every op it reads is past the end
        run(t, explicit_ctr != 0, explicit_ctr ? "kinds, explicit counters" : "kinds, dense counters");
    }
    for (u64 n : {1ull, 63ull, 64ull, 65ull, 255ull, 256ull, 257ull, 1025ull}) {
        Trace t;
        for (u64 i = 0; i < n; i++) {
            if (i % 3 == 0) t.exp_step_(word(3 + i), word(2 + i));
            else if (i % 2) t.sha3(i, 1 + i % 40, 1 + i % 5);
            else t.sha3(i, 0, 1);
        }
        run(t, n % 2 == 1, "ladder");
    }
    {   // no code set, and no step at all
        Trace t;
        t.sha3(1, 2, 1); t.codecopy(1, 2, 3, hA, 0, 0, S4); t.log(1, 2, 0, 0, hA, 0, S4);
        run(t, false, "no codes");
        Trace none;
        run(none, false, "no steps");
    }
    printf("events_from_trace_asan: ok\n");
    return 0;
}
