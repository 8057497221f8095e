// Stand-alone host program (TEST INFRASTRUCTURE): the CPU backend's zk_events_from_trace_ext over exactly-sized heap buffers, built with
// -fsanitize=address,undefined by tests/test_events_from_trace_ext_cpu.py and run as a child process.  Traces of RETURN / DATACOPY /
// BeginTx steps in every form (a deployment, a return to a caller, a root return, two-event steps, the create path told from the
// successor) beside SHA3 and EXP steps, with dense and explicit counters, pool-word operands and hashes, steps whose ops are missing or
// past the end of the trace, a last step that needs a successor, hashes outside the set, no code set, no step at all, a table of
// DATACOPY steps alone (the copy capacity exactly) and ladders of 1 .. 1025 steps.  Every event, ref and status is compared with what the
// step was built to give.  Exit status 0 = no mismatch (the sanitizers abort on their own findings).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../zkevm_specs_amd/csrc/cpu_backend.cpp"

#define CHECK(cond, ...) do { if (!(cond)) { printf("events_from_trace_ext_asan: " __VA_ARGS__); printf("\n"); exit(1); } } while (0)

struct W { u64 w[4]; };
static W word(u64 a, u64 b = 0, u64 c = 0, u64 d = 0) { return W{{a, b, c, d}}; }
static bool narrow(const W& x) { return (x.w[1] | x.w[2] | x.w[3]) == 0; }

struct Trace {
    std::vector<u32> head, want;
    std::vector<u64> id, addr, val, ctr, pool, steps;
    std::vector<uint8_t> code;
    std::vector<u64> code_off{0}, hashes;
    std::vector<u64> copy, exp;      // expected cells
    std::vector<u32> copy_flag, copy_ref, copy_dst, copy_step, exp_step;
    u64 rwc = 5, pairs = 0;
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
    void ctx(u64 call_id, u32 field, const W& v) { op(TG_CallContext, 0, false, call_id, field, v); }
    u64 step(u32 state, bool root, bool create, u64 call_id, u64 sp, u32 status) {
        const u64 r[13] = {state | ((u64)root << 8) | ((u64)create << 9), rwc, call_id, 0, sp, 1000, 0, 0, 0, 1, 0, 0, 0};
        steps.insert(steps.end(), r, r + 13);
        want.push_back(status);
        pairs += state == ES_BeginTx || state == ES_DATACOPY;
        return want.size() - 1;
    }
    void expect_copy(u64 s, const W& src_id, u32 st, const W& dst_id, u32 dt, u64 a0, u64 a1, u64 d, u64 len, u64 c, u32 flag, u32 ref, u32 dst) {
        const u64 v[12][2] = {{src_id.w[0], src_id.w[1]}, {src_id.w[2], src_id.w[3]}, {st, 0}, {dst_id.w[0], dst_id.w[1]}, {dst_id.w[2], dst_id.w[3]},
                              {dt, 0}, {a0, 0}, {a1, 0}, {d, 0}, {len, 0}, {0, 0}, {c, 0}};
        for (int k = 0; k < 12; k++) { copy.push_back(v[k][0]); copy.push_back(v[k][1]); copy.push_back(0); copy.push_back(0); }
        copy_flag.push_back(flag); copy_ref.push_back(ref); copy_dst.push_back(dst); copy_step.push_back((u32)s);
    }
    void sha3(u64 offset, u64 size, u64 call_id) {
        const u64 c0 = rwc, s = step(ES_SHA3, false, false, call_id, 900, 0);
        op(TG_Stack, 0, false, call_id, 900, word(offset)); op(TG_Stack, 0, false, call_id, 901, word(size)); op(TG_Stack, 0, true, call_id, 901, word(77, 1));
        if (size) expect_copy(s, word(call_id), TEV_TAG_MEMORY, word(call_id), TEV_TAG_RLC_ACC, offset, offset + size, 0, size, c0 + 3, 0, 0, 0);
    }
    void exp_step_(const W& base, const W& e) {
        const u64 c0 = rwc, s = step(ES_EXP, false, false, 3, 900, 0);
        op(TG_Stack, 0, false, 3, 900, base); op(TG_Stack, 0, false, 3, 901, e); op(TG_Stack, 0, true, 3, 901, word(1));
        if (!(narrow(e) && e.w[0] <= 1)) {
            const u64 v[5][2] = {{c0 + 3, 0}, {base.w[0], base.w[1]}, {base.w[2], base.w[3]}, {e.w[0], e.w[1]}, {e.w[2], e.w[3]}};
            for (int k = 0; k < 5; k++) { exp.push_back(v[k][0]); exp.push_back(v[k][1]); exp.push_back(0); exp.push_back(0); }
            exp_step.push_back((u32)s);
        }
    }
    // a deployment: the Account write of the code hash h, whose index in the set is `dst`
    void ret_create(const W& off, u64 len, const W& h, u32 dst, u32 status = 0, bool write = true) {
        const u64 c0 = rwc, s = step(ES_RETURN, true, true, 4, 900, status);
        ctx(4, CC_IsSuccess, word(1)); op(TG_Stack, 0, false, 4, 900, off); op(TG_Stack, 0, false, 4, 901, word(len));
        ctx(4, CC_CalleeAddress, word(5, 5, 5)); op(TG_Account, ACC_CodeHash, write, 0, 0, h);
        if (len && !status) expect_copy(s, word(4), TEV_TAG_MEMORY, h, TEV_TAG_BYTECODE, off.w[0], off.w[0] + len, 0, len, c0 + 5, 2, 0, dst);
    }
    // a return to a caller; the caller's id is the next step's call id
    void ret_caller(u64 off, u64 len, u64 ro, u64 rl, u64 next_call, u32 status = 0) {
        const u64 c0 = rwc, s = step(ES_RETURN, false, false, 4, 900, status);
        ctx(4, CC_IsSuccess, word(1)); op(TG_Stack, 0, false, 4, 900, word(off)); op(TG_Stack, 0, false, 4, 901, word(len));
        ctx(4, CC_ReturnDataOffset, word(ro)); ctx(4, CC_ReturnDataLength, word(rl));
        if (!status) expect_copy(s, word(4), TEV_TAG_MEMORY, word(next_call), TEV_TAG_MEMORY, off, off + len, ro, len < rl ? len : rl, c0 + 5, 0, 0, 0);
    }
    void ret_root() {
        step(ES_RETURN, true, false, 4, 900, 0);
        ctx(4, CC_IsSuccess, word(1));
    }
    void datacopy(u64 c, u64 cdo, u64 cdl, u64 rdo, u64 rdl, u64 call_id, u32 status = 0) {
        const u64 c0 = rwc, s = step(ES_DATACOPY, false, false, call_id, 900, status);
        ctx(call_id, CC_CalleeAddress, word(4, 0, 1)); ctx(call_id, CC_CallerId, word(c)); ctx(call_id, CC_CallDataOffset, word(cdo));
        ctx(call_id, CC_CallDataLength, word(cdl)); ctx(call_id, CC_ReturnDataOffset, word(rdo)); ctx(call_id, CC_ReturnDataLength, word(rdl));
        if (status) return;
        const u64 l0 = rdo + rdl, inc = l0 + (l0 < cdl ? l0 : cdl);
        expect_copy(s, word(c), TEV_TAG_MEMORY, word(c), TEV_TAG_MEMORY, cdo, cdo + cdl, rdo, l0, c0 + 6, 0, 0, 0);
        expect_copy(s, word(c), TEV_TAG_MEMORY, word(call_id), TEV_TAG_MEMORY, cdo, cdo + cdl, 0, rdl, c0 + 6 + inc, 0, 0, 0);
    }
    // BeginTx with `n_ops` ops (23: the create path) and the step behind it; emits when the successor is a create step at rwc + 23
    void begin_tx(u64 tx, u64 n, const W& h, u32 dst, u64 n_ops, bool next_create, u32 next_state, u32 status = 0, bool emits = true) {
        const u64 c0 = rwc, s = step(ES_BeginTx, false, false, 0, 900, status);
        for (u64 k = 0; k < n_ops; k++) {
            if (k == 0) ctx(c0, CC_TxId, word(tx));
            else if (k == 14) ctx(c0, CC_CallDataLength, word(n));
            else if (k == 22) ctx(c0, CC_CodeHash, h);
            else if (k >= 4 && k < 10) op(TG_Account, 1, true, 0, 0, word(k, k));
            else ctx(c0, CC_IsStatic, word(0));
        }
        step(next_state, true, next_create, c0, 900, 0);
        if (status || !emits) return;
        expect_copy(s, word(tx), TEV_TAG_TX_CALLDATA, word(c0), TEV_TAG_RLC_ACC, 0, n, 0, n, c0 + 10, 0, (u32)(tx - 1), 0);
        expect_copy(s, word(tx), TEV_TAG_TX_CALLDATA, h, TEV_TAG_BYTECODE, 0, n, 0, n, c0 + 10, 2, (u32)(tx - 1), dst);
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
    u64 cap = ~0ull, cap_exp = ~0ull;
    CHECK(zk_events_from_trace_ext_sizes(&in, 0, &cap, &cap_exp) == 0 && cap == ns + t.pairs && cap_exp == ns, "%s: sizes: %s", what, zk_last_error());
    // every output exactly at its capacity
    std::vector<u64> copy(cap * 48), exp(ns * 20);
    std::vector<u32> flag(cap), ref(cap), dst(cap), cstep(cap), estep(ns), status(ns);
    zk_trace_events_ext out{copy.data(), flag.data(), ref.data(), dst.data(), cstep.data(), exp.data(), estep.data()};
    u64 n_copy = ~0ull, n_exp = ~0ull;
    zk_result res;
    CHECK(zk_events_from_trace_ext(&in, &out, 0, status.data(), &n_copy, &n_exp, &res) == 0, "%s: %s", what, zk_last_error());
    u64 fails = 0;
    for (u64 s = 0; s < ns; s++) {
        CHECK(status[s] == t.want[s], "%s: step %llu status 0x%08x, expected 0x%08x", what, (unsigned long long)s, status[s], t.want[s]);
        fails += t.want[s] != 0;
    }
    CHECK(res.fail_count == fails && res.rows_evaluated == ns, "%s: tally", what);
    CHECK(n_copy == t.copy_step.size() && n_exp == t.exp_step.size(), "%s: %llu copy / %llu EXP events, expected %zu / %zu", what,
          (unsigned long long)n_copy, (unsigned long long)n_exp, t.copy_step.size(), t.exp_step.size());
    copy.resize(n_copy * 48); exp.resize(n_exp * 20); flag.resize(n_copy); ref.resize(n_copy); dst.resize(n_copy); cstep.resize(n_copy); estep.resize(n_exp);
    CHECK(copy == t.copy && flag == t.copy_flag && ref == t.copy_ref && dst == t.copy_dst && cstep == t.copy_step, "%s: the copy events differ", what);
    CHECK(exp == t.exp && estep == t.exp_step, "%s: the EXP events differ", what);
    // a session with two passes gives the same counts
    zk_session* s = nullptr;
    CHECK(zk_events_from_trace_ext_open(&in, nullptr, 0, &s) == 0, "%s: open: %s", what, zk_last_error());
    for (int pass = 0; pass < 2; pass++) {
        u64 a = ~0ull, b = ~0ull;
        CHECK(zk_launch(s, nullptr) == 0 && zk_collect(s, &res) == 0 && zk_events_from_trace_ext_counts(s, &a, &b) == 0 && a == n_copy && b == n_exp,
              "%s: session pass %d", what, pass);
    }
    zk_close(s);
}

int main() {
    const u32 S1 = ((u32)ZK_KIND_VALUE_ERROR << 24) | 1, S2 = S1 + 1, S3 = S1 + 2, S4 = S1 + 3, S5 = S1 + 4;
    const W hA = word(7, 0, 0, 0x1111), hB = word(9, 0, 0x2222), hC = word(5), hX = word(1, 2, 3, 4), big = word(12345, 0, 0xabc, 1ull << 63);
    for (int explicit_ctr = 0; explicit_ctr < 2; explicit_ctr++) {
        Trace t;
        t.add_code(hA, std::vector<uint8_t>(12, 0x60)); t.add_code(hB, std::vector<uint8_t>(23, 0x5b)); t.add_code(hA, std::vector<uint8_t>(40, 0)); t.add_code(hC, {});
        t.sha3(64, 32, 1);
        t.ret_create(word(0), 12, hA, 0); t.ret_create(word(3), 20, hB, 1); t.ret_create(word(3), 0, hX, 0); t.ret_create(big, 0, hC, 3);
        t.ret_create(word(3), 5, hX, 0, S4); t.ret_create(word(1ull << 62), 5, hX, 0, S3); t.ret_create(word(3), 5, hB, 1, S2, false);
        t.ret_caller(32, 8, 100, 20, 9); t.sha3(1, 1, 9);
        t.ret_caller(32, 20, 100, 20, 3); t.exp_step_(word(3), word(200));
        t.ret_caller(32, 50, 7, 20, 3); t.exp_step_(big, big);
        t.ret_caller(32, 0, 7, 20, 1); t.sha3(0, 0, 1);
        t.ret_caller((1ull << 62) - 1, 1, 7, 20, 1, S3); t.sha3(0, 0, 1);
        t.ret_root();
        t.datacopy(6, 10, 7, 3, 5, 11); t.datacopy(6, 0, 32, 0, 32, 11); t.datacopy(6, 0, 2, 4, 9, 12); t.datacopy(6, 5, 0, 0, 0, 12);
        t.datacopy(6, 1ull << 61, 1ull << 61, 0, 0, 12, S3); t.datacopy(6, 0, 1, 1ull << 61, 1ull << 61, 12, S3);
        t.begin_tx(1, 37, hB, 1, 23, true, ES_ADD); t.begin_tx(3, 5, hA, 0, 23, true, ES_EndTx);
        t.begin_tx(1, 37, hB, 1, 10, true, ES_EndTx, 0, false); t.begin_tx(1, 37, hB, 1, 24, false, ES_ADD, 0, false);
        t.begin_tx(1, 37, hX, 0, 23, false, ES_ADD, 0, false);
        t.begin_tx(1, 37, hX, 0, 23, true, ES_ADD, S4); t.begin_tx(0, 37, hB, 1, 23, true, ES_ADD, S3); t.begin_tx(1ull << 33, 37, hB, 1, 23, true, ES_ADD, S3);
        t.begin_tx(1, 0, hB, 1, 23, true, ES_ADD, S5);
        // steps whose counters nobody holds (site 1; with dense counters the ops there are another step's: site 2)
        t.step(ES_DATACOPY, false, false, 1, 900, explicit_ctr ? S1 : S2);
        t.rwc += explicit_ctr ? 7 : 0;
        t.step(ES_RETURN, false, false, 1, 900, explicit_ctr ? S1 : S2);
        t.rwc += explicit_ctr ? 7 : 0;
        t.sha3(5, 6, 8);
        t.step(ES_CALL_OP, false, false, 1, 900, ((u32)ZK_KIND_UNSUPPORTED << 24) | 1);
        t.step(ES_CREATE, false, false, 1, 900, ((u32)ZK_KIND_UNSUPPORTED << 24) | 1);
        t.step(ES_CREATE2, false, false, 1, 900, ((u32)ZK_KIND_UNSUPPORTED << 24) | 1);
        t.step(ES_DATACOPY, false, false, 6, 900, S1);  // every op it reads is past the end
        t.step(ES_BeginTx, false, false, 0, 900, S5);   // the trace's last step: no successor
        run(t, explicit_ctr != 0, explicit_ctr ? "forms, explicit counters" : "forms, dense counters");
    }
    {   // last steps: a return to a caller needs a successor, a deployment and a DATACOPY do not
        Trace a; a.add_code(hA, {1, 2, 3});
        a.sha3(1, 2, 1); a.step(ES_RETURN, false, false, 4, 900, S5);
        run(a, false, "last: return to a caller");
        Trace b; b.add_code(hA, {1, 2, 3});
        b.sha3(1, 2, 1); b.ret_create(word(0), 3, hA, 0);
        run(b, true, "last: deployment");
        Trace c;
        c.datacopy(6, 10, 7, 3, 5, 11);
        run(c, false, "last: datacopy");
    }
    {   // DATACOPY steps alone: 2 n events, the copy capacity exactly
        Trace t;
        for (u64 i = 0; i < 257; i++) t.datacopy(6 + i % 3, i, 1 + i % 5, i % 4, i % 7, 20 + i % 2);
        run(t, false, "pairs");
    }
    for (u64 n : {1ull, 63ull, 64ull, 65ull, 255ull, 256ull, 257ull, 1025ull}) {
        Trace t;
        t.add_code(hB, {1});
        while (t.want.size() < n) {
            const u64 i = t.want.size();
            if (i % 4 == 0) t.datacopy(6, i, 1 + i % 5, i % 3, i % 4, 11);
            else if (i % 4 == 1 && i + 1 < n) { t.ret_caller(i, 1 + i % 9, i % 5, 4, 3); }  // (the next step is an EXP step of call 3)
            else if (i % 4 == 2 || i % 4 == 1) t.exp_step_(word(3 + i), word(2 + i));
            else t.sha3(i, i % 2 ? 1 + i % 40 : 0, 1 + i % 5);
        }
        run(t, n % 2 == 1, "ladder");
    }
    {   // no code set, and no step at all
        Trace t;
        t.sha3(1, 2, 1); t.ret_create(word(0), 3, hA, 0, S4); t.begin_tx(1, 37, hB, 0, 23, true, ES_ADD, S4); t.datacopy(6, 10, 7, 3, 5, 11);
        run(t, false, "no codes");
        Trace none;
        run(none, false, "no steps");
    }
    printf("events_from_trace_ext_asan: ok\n");
    return 0;
}
