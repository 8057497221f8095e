// libzkevm_cpu.so — the C ABI of include/zkevm_hip.h evaluated on the host cores (SURVEY.md §2 native piece vi, §8b
// `backend` selector, §8d "C++ CPU backend on 1 and all cores").
//
// The per-row / per-step device functions of csrc/*.hpp are plain C++ when compiled without hipcc (the ZK_HOSTSIM switch of
// fr.hpp selects the host flavour of the ZK_HD / ZK_NOINLINE macros); this file puts the same session protocol around them
// that zkevm_hip.hip puts around the kernels: open = copy the caller's arrays and build the indices, launch = one pass over the
// rows with an OpenMP parallel-for, collect = the tally, read_status = the per-row codes.  What it is for:
//   * BASELINE configs[0] ("Bytecode circuit ... pure CPU path (plumbing, no GPU)") through the real boundary;
//   * the fair optimised-CPU line next to the GPU numbers (bench.py cpu_baseline legs `cpu_backend_1core` / `_allcores`).
// It is selected explicitly (ZK_BACKEND=cpu -> zkevm_specs_amd/_lib.py loads this library instead of libzkevm_hip.so); nothing
// falls back to it, and it shares no code with oracle/ (the Python restatement used as the test oracle).
// Not implemented here (they return an error that says so): the device-side witness assignments (zk_state_assign*,
// zk_bytecode_assign*, zk_copy_assign*), ZK_OPT_DEVICE_PTRS, zk_session_set_stream.
#include <stdio.h>
#include <string.h>
#include <chrono>
#include <functional>
#include <string>
#include <vector>

#include "../../include/zkevm_hip.h"
#include "dist_tally.hpp"
#include "state_circuit.hpp"
#include "evm_circuit.hpp"
#include "host_index.hpp"
#include "row_circuits.hpp"
#include "copy_circuit.hpp"
#include "sign_circuit.hpp"
#include "keccak_table.hpp"
#include "secp256k1.hpp"
#include "pi_circuit.hpp"
#include "state_assign.hpp"
#include "bytecode_assign.hpp"
#include "bytecode_code.hpp"
#include "block_tables.hpp"
#include "trace_witness.hpp"
#include "state_rekey.hpp"
#include "ecc_circuit.hpp"
#include "ecc_calls.hpp"
#include "withdrawal_circuit.hpp"
#include "tx_assign.hpp"
#include "sig_assign.hpp"
#include "exp_assign.hpp"
#include "pi_assign.hpp"

static thread_local std::string g_err;
#define ARG_TRY(cond, msg) do { if (!(cond)) { g_err = msg; return -1; } } while (0)
#include "copy_assign_plan.hpp"  // (uses ARG_TRY)
#include "copy_sources_plan.hpp"
#include "trace_events_plan.hpp"
#include "trace_sha3.hpp"

extern "C" const char* zk_last_error(void) { return g_err.c_str(); }
extern "C" int zk_init(int) { return 0; }
extern "C" void zk_shutdown(void) {}
extern "C" int zk_set_stream(void*) { return 0; }

// ---------------------------------------------------------------------------------------
// tables: a private copy of the caller's rows + the open-addressing index
// ---------------------------------------------------------------------------------------
struct CpuTable {
    ZkTable t;
    std::vector<u64> cells;
    std::vector<u32> flags, slots;
};
static void cpu_table(CpuTable& h, const u64* cells, const u32* flags, u64 n, u32 ncells, u64 (*hash_of)(const ZkTable&, u32)) {
    static const u64 zero_row[64] = {0};
    static const u32 zero_flag[1] = {0};
    if (n) h.cells.assign(cells, cells + n * ncells * 4);
    if (n && flags) h.flags.assign(flags, flags + n);
    h.t.cells = n ? h.cells.data() : zero_row;  // empty table: one readable zero row (as in the HIP library)
    h.t.flags = n ? (flags ? h.flags.data() : nullptr) : zero_flag;
    h.t.n = (u32)n;
    h.t.ncells = ncells;
    u32 cap = 16;
    while (cap < 2 * n + 2) cap <<= 1;
    h.slots.assign(cap, ZK_EMPTY_SLOT);
    h.t.slots = h.slots.data();
    h.t.mask = cap - 1;
    if (hash_of)
        for (u32 r = 0; r < (u32)n; r++) {
            u32 s = (u32)hash_of(h.t, r) & h.t.mask;
            while (h.slots[s] != ZK_EMPTY_SLOT) s = (s + 1) & h.t.mask;
            h.slots[s] = r;
        }
}
static Fr cell_of(const u64* p) { return fr_load(p); }

// ---------------------------------------------------------------------------------------
// sessions
// ---------------------------------------------------------------------------------------
struct zk_session {
    u64 n = 0, lo = 0, hi = 0;            // rows; evaluated range
    std::function<u32(u64)> row;          // status code of row i
    std::function<void(u64, u64)> before_rows;  // work of a pass over [lo, hi) that its rows share (ECC: stage 1 over the range's pairs)
    std::vector<u32> status;
    u32 launches = 0;
    double ms = 0;
    u64 fail_count = 0, first_row = ~0ull;
    u32 first_code = 0;
    bool range_ok = false;                // zk_set_range applies (row circuits)
    bool range_may_be_empty = false;      // ... and takes lo == hi (ECC sessions)
    // owned inputs (kept alive for `row`)
    std::vector<u64> a64[4];
    std::vector<u32> a32[4];
    std::vector<uint8_t> a8, a8b;
    std::vector<uint16_t> a16;
    std::vector<u64> w64[4];              // assignment sessions: work / output buffers
    std::vector<u32> out32;
    void (*pass)(zk_session*) = nullptr;  // assignment sessions: one pass computes the outputs and fills `status`
    int assign_kind = 0;                  // 1 state, 2 bytecode, 3 copy, 4 RW -> State ops, 5 tx, 6 exp, 7 PI, 8 ECC, 9 sig, 10 bytecode from code, 11 tables from block, 12 witness from trace, 13 ECC precompile calls, 14 copy from sources, 15 events from trace, 16 SHA3 from trace, 17 events from trace (ext)
    u64 n_ops = 0;                        // RW -> State ops: 1 + kept rows
    std::vector<u32> rekey_plan;          // RW -> State ops: the RwkHostPlan's plan (as words) ...
    std::vector<u32> rekey_jobs;          // ... and its rank jobs (cls, field, base, count)
    u64 n_mpt = 0;
    CpuTable tab[12];
    std::vector<u64> keccak_rows;         // keccak sessions: the table
    // per-circuit argument blocks (one is used)
    StateArgs state;
    EvmArgs evm;
    BytecodeArgs bytecode;
    ExpArgs exp;
    CopyArgs copy;
    SignArgs sign;
    PiArgs pi;
    PiCopyArgs picopy;
    AssignArgs assign;
    BcaArgs bca;
    std::vector<BcaChunk> bca_chunks;
    std::vector<uint8_t> bca_map;
    BccArgs bcc;                    // Bytecode table / rows / keccak rows from raw code (its chunk tables live in bca_chunks, bca_map)
    KeccakGenArgs bcc_kgen;
    std::vector<u64> bcc64[8];      // offsets, rpow, chunk_acc, chunk_in, part, table, rows, keccak rpow
    std::vector<u32> bcc32[4];      // row_off, code_chunk0, chunk_m, chunk_state
    BtbArgs btb;                    // EVM tx / block / withdrawal tables from raw block data
    std::vector<u64> btb64[10];     // tx_fields, offsets, ids, block, hashes, withdrawals, withdrawal ids, tx, block table, withdrawal table
    std::vector<u32> btb32[6];      // to_is_none, access_list, gas_part, gas_pre, tx_flags, block_flags
    TrwArgs trw;                    // EVM witness from compact trace records
    std::vector<u64> trw64[4];      // counters, offsets, rw, steps
    std::vector<u32> trw32[2];      // heads, rw_flags
    CpaArgs cpa;
    CpaPlan cpa_plan;
    CpsArgs cps;                    // Copy assignment from raw sources: the gather in front of `cpa` (its plan: cps_plan.cpa)
    CpsPlan cps_plan;
    std::vector<u64> cps64[4];      // is_code mask, counters, code offsets, per-event failing byte
    std::vector<u32> cps32[1];      // heads
    TevArgs tev;                    // Copy and EXP events from compact trace records
    TevPlan tev_plan;               // ... the sorted hash directory
    std::vector<u64> tev64[6];      // counters, pool offsets, code offsets, copy events, EXP events, counts
    std::vector<u32> tev32[5];      // heads, copy flags, copy refs, copy steps, EXP steps
    TevxArgs tevx;                  // ... the wider entry (zk_events_from_trace_ext*): its TevArgs in tevx.t, the buffers above
    std::vector<u32> tevx_dst;      // ... its copy dst refs
    Ts3Args ts3;                    // SHA3 inputs and keccak rows from compact trace records
    KeccakGenArgs ts3_kgen;         // ... the keccak table over the gathered bytes
    std::vector<u64> ts364[8];      // counters, pool offsets, sizes, session offsets, fail words, rows, out offsets, powers of the randomness
    std::vector<u32> ts332[3];      // heads, open-time statuses, steps
    std::vector<Ts3Msg> ts3_msg;
    std::vector<uint8_t> ts3_data;
    EcdsaArgs ecdsa;
    KeccakGenArgs kgen;
    TxAssignArgs txa;
    SigAssignArgs sga;
    std::vector<u64> sga64[8];      // Sig assignment: fields, addr, rpow, pk, cells, keccak candidates / table, sig candidates / table, aux
    std::vector<u32> sga32[3];      // expect_valid, meta, the signatures' status
    u64 n_sig_rows = 0;
    ExaArgs exa;
    ExaSizes exa_sizes;
    PiaArgs pia;
    PiaSizes pia_sizes;
    KeccakGenArgs pia_kgen;
    EccArgs ecc_assign;             // ECC assignment session (the verify session's args live in its `row` closure)
    EccCallArgs ecl;                // ECC precompile calls
    std::vector<u64> ecl64[10];     // [3..8]: points, pair_out, rows, table candidates, table, aux
    std::vector<u32> ecl32[4];      // pair_off, aux_kind, tdup, pair_flags
    std::vector<bn::Fq12> ecl_f;    // the pairs' Miller values
    std::vector<u32> ecc_pair_flags;     // ECC verification session: stage 1's per-pair records
    std::vector<bn::Fq12> ecc_pair_f;
    u64 n_ecl_table = 0;
    std::vector<u64> pia64[20];     // PI assignment: inputs, work buffers and outputs of 64-bit words
    std::vector<u32> pia32[6];
    std::vector<uint8_t> pia8[4];
    std::vector<u64> txa_out64[4];  // Tx assignment outputs: tx_rows, cells, keccak candidates, keccak
    std::vector<u32> txa_out32[3];  // tx_flags, meta, the txs' status
    u64 n_keccak = 0;
    ZkRwMeta rw_meta;
    HostCodeDir dir;
    std::vector<u64> aux64;
    bool status_external = false;  // the last pass wrote to the caller's buffer (zk_read_status refuses then, like the HIP library)
};

static void run_pass(zk_session* s, u32* status_out) {
    const auto t0 = std::chrono::steady_clock::now();
    u32* st = status_out ? status_out : s->status.data();
    const long long lo = (long long)s->lo, hi = (long long)s->hi;
    if (s->pass) {  // witness assignment: sequential host loops over the device functions
        s->pass(s);
        if (status_out) memcpy(status_out, s->status.data(), s->n * sizeof(u32));
    } else {
        if (s->before_rows) s->before_rows(s->lo, s->hi);
#pragma omp parallel for schedule(dynamic, 256)
        for (long long i = lo; i < hi; i++) st[i] = s->row((u64)i);
    }
    u64 fails = 0, first = ~0ull;
    for (long long i = lo; i < hi; i++)
        if (st[i]) {
            if (!fails) first = (u64)i;
            fails++;
        }
    s->fail_count = fails;
    s->first_row = first;
    s->first_code = fails ? st[first] : 0u;
    s->ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    s->launches++;
}
extern "C" int zk_launch(zk_session* s, uint32_t* status_dev) {
    ARG_TRY(s, "zk_launch: null session");
    s->status_external = status_dev != nullptr;
    run_pass(s, status_dev);
    return 0;
}
extern "C" int zk_collect(zk_session* s, zk_result* r) {
    ARG_TRY(s && r, "zk_collect: bad arguments");
    r->fail_count = s->fail_count;
    r->first_fail_row = s->first_row == ~0ull ? UINT64_MAX : s->first_row;
    r->first_fail_code = s->first_code;
    r->launches = s->launches;
    r->rows_evaluated = s->hi - s->lo;
    r->kernel_ms = s->launches ? s->ms / s->launches : 0.0;
    s->launches = 0;
    s->ms = 0;
    return 0;
}
extern "C" int zk_read_status(zk_session* s, uint32_t* status_host) {
    ARG_TRY(s && status_host, "zk_read_status: bad arguments");
    // same contract as the HIP library: the last pass's codes are the caller's when it handed over its own buffer
    ARG_TRY(!s->status_external, "zk_read_status: the last pass wrote its statuses to the caller's status_dev buffer, not the session's");
    memcpy(status_host, s->status.data(), s->n * sizeof(u32));
    return 0;
}
extern "C" int zk_close(zk_session* s) {
    delete s;
    return 0;
}
extern "C" int zk_session_set_stream(zk_session*, void*) { return 0; }
// device-side event spans: nothing to measure on the host (callers read -1 = not measured)
extern "C" int zk_session_timing(zk_session*, double* open_ms, double* span_ms) {
    if (open_ms) *open_ms = -1.0;
    if (span_ms) *span_ms = -1.0;
    return 0;
}
// Multi-GPU tally.  World 1 is the identity with the row offset applied.  World > 1 goes through the same collective binding as
// the HIP library (dist_tally.hpp) with HOST buffers — which RCCL itself does not accept, so it needs ZK_RCCL_LIB to name a
// collective library that does (tests/fakerccl: an all-gather over a shared-memory file); without one, ranks of a CPU job
// exchange their tallies on the host (zkevm_specs_amd.distributed.reduce_tally over gloo).
struct zk_comm {
    int rank = 0, world = 1;
    void* nccl = nullptr;
    std::vector<uint64_t> buf;  // TALLY_WORDS of this rank | TALLY_WORDS * world gathered
};
#define RCCL_TRY(expr, what)                                                                                                                   \
    do {                                                                                                                                       \
        const int r_ = (expr);                                                                                                                 \
        if (r_ != 0) {                                                                                                                         \
            char buf_[256];                                                                                                                    \
            snprintf(buf_, sizeof buf_, "%s: RCCL error %d (%s)", what, r_, zkdist::rccl().GetErrorString ? zkdist::rccl().GetErrorString(r_) : "?"); \
            g_err = buf_;                                                                                                                      \
            return -3;                                                                                                                         \
        }                                                                                                                                      \
    } while (0)
// a collective library that takes HOST buffers: it has to say so itself (`zk_collective_buffers() == 0`, dist_tally.hpp) — ZK_RCCL_LIB
// may just as well name the integrator's own build of RCCL, whose ncclAllGather must never see host pointers
static bool host_collective() { return getenv("ZK_RCCL_LIB") && zkdist::rccl().ok && zkdist::rccl().named_by_env && zkdist::rccl().buffers == 0; }
extern "C" int zk_dist_unique_id(uint8_t* id) {
    ARG_TRY(id, "zk_dist_unique_id: id is null");
    memset(id, 0, ZK_DIST_ID_BYTES);
    if (host_collective()) {
        zkdist::RcclId u;
        RCCL_TRY(zkdist::rccl().GetUniqueId(&u), "ncclGetUniqueId");
        memcpy(id, u.internal, ZK_DIST_ID_BYTES);
    }
    return 0;
}
extern "C" int zk_dist_close(zk_comm* c) {
    if (c && c->nccl) (void)zkdist::rccl().CommDestroy(c->nccl);
    delete c;
    return 0;
}
extern "C" int zk_dist_init(const uint8_t* id, int rank, int world, zk_comm** out) {
    ARG_TRY(id && out && world >= 1 && rank >= 0 && rank < world, "zk_dist_init: bad arguments");
    ARG_TRY(world == 1 || host_collective(),
            "zk_dist_init: the CPU backend has no collective of its own (world must be 1, or ZK_RCCL_LIB must name a library that gathers host buffers); reduce on the host");
    zk_comm* c = new zk_comm();
    c->rank = rank;
    c->world = world;
    c->buf.assign((size_t)(world + 1) * zkdist::TALLY_WORDS, 0);
    if (world > 1) {
        zkdist::RcclId u;
        memcpy(u.internal, id, ZK_DIST_ID_BYTES);
        if (int r = zkdist::rccl().CommInitRank(&c->nccl, world, u, rank)) {
            char buf[256];
            snprintf(buf, sizeof buf, "ncclCommInitRank: RCCL error %d", r);
            g_err = buf;
            c->nccl = nullptr;
            zk_dist_close(c);
            return -3;
        }
    }
    *out = c;
    return 0;
}
extern "C" int zk_dist_tally(zk_comm* c, const zk_result* local, uint64_t row_offset, zk_result* global) {
    ARG_TRY(c && local && global, "zk_dist_tally: bad arguments");
    uint64_t* mine = c->buf.data();
    uint64_t* all = mine + zkdist::TALLY_WORDS;
    zkdist::tally_pack(mine, local, row_offset);
    if (c->world == 1) memcpy(all, mine, zkdist::TALLY_WORDS * sizeof(uint64_t));
    else RCCL_TRY(zkdist::rccl().AllGather(mine, all, zkdist::TALLY_WORDS, zkdist::RCCL_UINT64, c->nccl, nullptr), "ncclAllGather");
    zkdist::tally_reduce(all, c->world, local, global);
    return 0;
}
extern "C" int zk_last_host_phases(double* us4) {
    if (us4) for (int k = 0; k < 4; k++) us4[k] = -1.0;
    return 0;
}
extern "C" int zk_timing_sums(double* sums_ms, uint64_t* count, int) {  // (no device spans on this backend)
    if (sums_ms) for (int k = 0; k < 3; k++) sums_ms[k] = -1.0;
    if (count) *count = 0;
    return 0;
}
extern "C" int zk_last_timing(double* open_ms, double* pass_ms, double* span_ms) {
    if (open_ms) *open_ms = -1.0;
    if (pass_ms) *pass_ms = -1.0;
    if (span_ms) *span_ms = -1.0;
    return 0;
}
extern "C" int zk_set_range(zk_session* s, uint64_t row_lo, uint64_t row_hi) {
    ARG_TRY(s && s->range_ok, "zk_set_range: not a row-circuit session");
    ARG_TRY((row_lo < row_hi || (s->range_may_be_empty && row_lo == row_hi)) && row_hi <= s->n, "zk_set_range: bad range");
    s->lo = row_lo;
    s->hi = row_hi;
    std::fill(s->status.begin(), s->status.end(), 0u);
    return 0;
}
extern "C" int zk_state_set_range(zk_session* s, uint64_t row_lo, uint64_t row_hi) { return zk_set_range(s, row_lo, row_hi); }

static zk_session* new_session(u64 n, bool range_ok) {
    zk_session* s = new zk_session();
    s->n = n;
    s->lo = 0;
    s->hi = n;
    s->status.assign(n ? n : 1, 0u);
    s->range_ok = range_ok;
    return s;
}
static int one_shot(zk_session* s, uint32_t* status_out, zk_result* result) {
    int rc = zk_launch(s, nullptr);
    if (!rc) rc = zk_collect(s, result);
    if (!rc && status_out) rc = zk_read_status(s, status_out);
    zk_close(s);
    return rc;
}
#define NO_DEVICE_PTRS(opts, name) ARG_TRY(!((opts) & ZK_OPT_DEVICE_PTRS), name ": ZK_OPT_DEVICE_PTRS has no meaning on the CPU backend")
#ifndef ZK_OPT_STATE_COMPACT
#define ZK_OPT_STATE_COMPACT 32u
#endif

// ---- Fr vector ops ------------------------------------------------------------------------------------------------------
extern "C" int zk_fr_op(int op, const uint64_t* a, const uint64_t* b, uint64_t* out, uint64_t n, uint32_t opts) {
    NO_DEVICE_PTRS(opts, "zk_fr_op");
    ARG_TRY(a && b && out, "zk_fr_op: null pointer");
    ARG_TRY(op < 19 || op > 25 || n % 12 == 0, "zk_fr_op 19..25: n must be a multiple of 12");
#pragma omp parallel for
    for (long long i = 0; i < (long long)n; i++) {
        const Fr x = fr_load(a + 4 * i), y = fr_load(b + 4 * i);
        Fr r;
        switch (op) {
        case 0: r = fr_add(x, y); break;
        case 1: r = fr_sub(x, y); break;
        case 2: r = fr_mul(x, y); break;
        case 3: r = fr_mont(x, y); break;
        case 4: r = fr_neg(x); break;
        case 5: r = fr_inv(x); break;
        case 6: r = fr_div(x, y); break;
        case 18: r = ecc_fq_mul_hook(x, y); break;
        case 26: r = sp_sqrt_p(x); break;
        case 27: r = sp_inv_p(x); break;
        case 19: case 20: case 21: case 22: case 23: case 24: case 25:
            if (i % 12 == 0 && i + 12 <= (long long)n) ecc_fq12_op_hook(op, a + 4 * i, b + 4 * i, out + 4 * i);
            continue;
        default: r = fr_zero();
        }
        for (int k = 0; k < 4; k++) out[4 * i + k] = (u64)r.v[2 * k] | ((u64)r.v[2 * k + 1] << 32);
    }
    return 0;
}

// ---- State circuit ------------------------------------------------------------------------------------------------------
extern "C" int zk_state_open(const uint64_t* rows, const uint32_t* flags, uint64_t n, const uint64_t* mpt, uint64_t n_mpt,
                             uint32_t opts, zk_session** out) {
    NO_DEVICE_PTRS(opts, "zk_state_open");
    ARG_TRY(out && rows && n > 0 && n < (1ull << 32) && n_mpt < (1ull << 31), "zk_state_open: bad arguments");
    zk_session* s = new_session(n, true);
    const bool compact = opts & ZK_OPT_STATE_COMPACT;  // 15-cell rows, limb / byte decompositions derived (include/zkevm_hip.h)
    s->a64[0].assign(rows, rows + n * (compact ? 15 : ST_NCELLS) * 4);
    s->state.rows.skip = compact ? 42u : 0u;
    if (flags) s->a32[0].assign(flags, flags + n);
    else s->a32[0].assign(n, 0u);
    cpu_table(s->tab[0], mpt, nullptr, n_mpt, MPT_NCELLS, nullptr);
    {  // the MPT index carries a hash fingerprint in each slot (state_mpt_slot_value)
        CpuTable& h = s->tab[0];
        for (u32 r = 0; r < (u32)n_mpt; r++) {
            const u64 hv = state_mpt_key_hash(h.t, r);
            u32 k = (u32)hv & h.t.mask;
            while (h.slots[k] != ZK_EMPTY_SLOT) k = (k + 1) & h.t.mask;
            h.slots[k] = state_mpt_slot_value(h.t, r, hv);
        }
    }
    s->state.rows.cells = s->a64[0].data();
    s->state.rows.flags = s->a32[0].data();
    s->state.rows.n = n;
    s->state.mpt = s->tab[0].t;
    s->state.eval_lo = 0;
    s->state.eval_hi = n;
    s->row = [s](u64 i) { return state_check_row(s->state, i); };
    *out = s;
    return 0;
}
extern "C" int zk_state_verify(const uint64_t* rows, const uint32_t* flags, uint64_t n, const uint64_t* mpt, uint64_t n_mpt,
                               uint32_t opts, uint32_t* status_out, zk_result* result) {
    ARG_TRY(result, "zk_state_verify: result is null");
    zk_session* s = nullptr;
    const int rc = zk_state_open(rows, flags, n, mpt, n_mpt, opts, &s);
    return rc ? rc : one_shot(s, status_out, result);
}

// ---- EVM circuit --------------------------------------------------------------------------------------------------------
extern "C" int zk_evm_open(const zk_evm_tables* t, uint32_t opts, zk_session** out) {
    NO_DEVICE_PTRS(opts, "zk_evm_open");
    ARG_TRY(t && out && t->steps && t->n_steps >= 2 && t->n_steps < (1ull << 32), "zk_evm_open: bad arguments");
    ARG_TRY(t->aux_cells == 0 || (t->aux_cells >= 2 && t->aux_cells <= 64), "zk_evm_open: aux_cells must be 0 (= 2) or 2..64");
    zk_session* s = new_session(t->n_steps - 1, false);
    EvmArgs& a = s->evm;
    s->a64[0].assign(t->steps, t->steps + t->n_steps * STEP_NCELLS * 4);
    a.dyn = nullptr;
    a.step_recs = nullptr;
    a.defer_list = nullptr;
    a.defer_count = nullptr;
    a.steps = s->a64[0].data();
    a.n_steps = t->n_steps;
    cpu_table(s->tab[0], t->rw, t->rw_flags, t->n_rw, RW_NCELLS, rw_key_hash);
    cpu_table(s->tab[1], t->bytecode, nullptr, t->n_bytecode, BYTECODE_NCELLS, bc_key_hash);
    cpu_table(s->tab[2], t->tx, t->tx_flags, t->n_tx, TX_NCELLS, tx_key_hash);
    cpu_table(s->tab[3], t->block, t->block_flags, t->n_block, BLOCK_NCELLS, blk_key_hash);
    cpu_table(s->tab[4], t->copy, nullptr, t->n_copy, COPY_T_NCELLS, copy_key_hash);
    cpu_table(s->tab[5], t->keccak, nullptr, t->n_keccak, KECCAK_NCELLS, keccak_key_hash);
    cpu_table(s->tab[6], t->exp, nullptr, t->n_exp, EXP_T_NCELLS, expt_key_hash);
    cpu_table(s->tab[7], t->sig, nullptr, t->n_sig, SIG_T_NCELLS, sig_key_hash);
    cpu_table(s->tab[8], t->ecc, nullptr, t->n_ecc, ECC_T_NCELLS, ecc_key_hash);
    cpu_table(s->tab[9], t->withdrawals, nullptr, t->n_withdrawals, 4, nullptr);  // walked in order: no index
    a.rw = s->tab[0].t; a.bytecode = s->tab[1].t; a.tx = s->tab[2].t; a.block = s->tab[3].t; a.copy = s->tab[4].t;
    a.keccak = s->tab[5].t; a.exp = s->tab[6].t; a.sig = s->tab[7].t; a.ecc = s->tab[8].t; a.withdrawals = s->tab[9].t;
    {
        const HostEvmAgg g = evm_aggregates_host(t->tx, t->tx_flags, t->n_tx, t->withdrawals, t->n_withdrawals);
        a.agg_max_txs = g.max_txs; a.agg_total_txs = g.total_txs; a.agg_invalid_txs = g.invalid_txs;
        a.agg_bad_invalid_rows = g.bad_invalid_rows; a.agg_total_wds = g.total_wds;
        a.agg_rw_dups = rw_duplicate_rows_host(t->rw, t->n_rw);
    }
    a.aux = nullptr;
    a.aux_kind = nullptr;
    a.aux_cells = t->aux_cells ? t->aux_cells : 2u;
    if (t->aux && t->aux_kind) {
        s->aux64.assign(t->aux, t->aux + t->n_steps * a.aux_cells * 4);
        s->a32[1].assign(t->aux_kind, t->aux_kind + t->n_steps);
        a.aux = s->aux64.data();
        a.aux_kind = s->a32[1].data();
    }
    a.perm = nullptr;
    a.prof = nullptr;
    a.n_pairs = (u32)(t->n_steps - 1);
    a.opts = (t->begin_with_first_step ? 1u : 0u) | (t->end_with_last_step ? 2u : 0u);
    a.rw_dense = 0;
    a.rw_base = 0;
    a.rw_keys = nullptr;
    a.codes.n = 0;
    a.codes.mask = 0;
    a.codes.packed = nullptr;
    a.codes.entries = nullptr;
    a.codes.slots = nullptr;
    if (!(opts & ZK_OPT_GENERIC_INDEX)) {
        s->rw_meta = rw_dense_meta_host(s->tab[0].t.n ? s->tab[0].cells.data() : nullptr, t->n_rw);
        a.rw_dense = s->rw_meta.dense;
        a.rw_base = s->rw_meta.base;
        if (s->rw_meta.dense) {  // packed key records, as the device open builds them
            s->a64[1].resize((size_t)t->n_rw * 4);
            for (u64 r = 0; r < t->n_rw; r++) {
                const RwKey k = rw_pack_row(a.rw, (u32)r);
                for (int j = 0; j < 4; j++) s->a64[1][4 * r + j] = k.w[j];
            }
            a.rw_keys = s->a64[1].data();
        }
        if (t->n_bytecode) {
            build_code_dir(s->tab[1].cells.data(), t->n_bytecode, s->dir);
            a.codes.entries = s->dir.entries.data();
            a.codes.slots = s->dir.slots.data();
            a.codes.mask = s->dir.mask;
            a.codes.n = (u32)s->dir.entries.size();
            a.codes.packed = s->dir.packed.data();
        }
    }
    s->row = [s](u64 i) {  // as on the device: the hot and the cold instantiation split the states
        u32 c = evm_check_step<EVM_GROUP_ALL>(s->evm, i);
        if (c == ZK_NOT_MINE) c = evm_check_step<EVM_GROUP_WARM>(s->evm, i);
        if (c == ZK_NOT_MINE) c = evm_check_step<EVM_GROUP_COLD>(s->evm, i);
        return c;
    };
    *out = s;
    return 0;
}
extern "C" int zk_evm_verify(const zk_evm_tables* t, uint32_t opts, uint32_t* status_out, zk_result* result) {
    ARG_TRY(result, "zk_evm_verify: result is null");
    zk_session* s = nullptr;
    const int rc = zk_evm_open(t, opts, &s);
    return rc ? rc : one_shot(s, status_out, result);
}

extern "C" int zk_evm_verify_batch(const zk_evm_tables* const* t, uint64_t n, uint32_t opts, zk_result* results) {
    ARG_TRY((t && results) || n == 0, "zk_evm_verify_batch: bad arguments");
    for (uint64_t i = 0; i < n; i++) ARG_TRY(t[i], "zk_evm_verify_batch: null witness");
    for (uint64_t i = 0; i < n; i++) {  // nothing to pipeline on the host: one witness after the other
        const int rc = zk_evm_verify(t[i], opts, nullptr, &results[i]);
        if (rc) return rc;
    }
    return 0;
}

// ---- Bytecode / Exp circuits --------------------------------------------------------------------------------------------
extern "C" int zk_bytecode_open(const uint64_t* rows, uint64_t n, const uint64_t* keccak, uint64_t n_keccak, const uint64_t* randomness,
                                uint32_t opts, zk_session** out) {
    NO_DEVICE_PTRS(opts, "zk_bytecode_open");
    ARG_TRY(out && rows && randomness && n > 0 && n < (1ull << 32) && n_keccak < (1ull << 31), "zk_bytecode_open: bad arguments");
    zk_session* s = new_session(n, true);
    s->a64[0].assign(rows, rows + n * BC_NCELLS * 4);
    cpu_table(s->tab[0], keccak, nullptr, n_keccak, KECCAK_NCELLS, keccak_key_hash);
    s->bytecode.rows.cells = s->a64[0].data();
    s->bytecode.rows.flags = nullptr;
    s->bytecode.rows.n = n;
    s->bytecode.keccak = s->tab[0].t;
    s->bytecode.r = cell_of(randomness);
    s->bytecode.r_mont = nullptr;
    s->row = [s](u64 i) { return bytecode_check_row(s->bytecode, i); };
    *out = s;
    return 0;
}
extern "C" int zk_bytecode_verify(const uint64_t* rows, uint64_t n, const uint64_t* keccak, uint64_t n_keccak, const uint64_t* randomness,
                                  uint32_t opts, uint32_t* status_out, zk_result* result) {
    ARG_TRY(result, "zk_bytecode_verify: result is null");
    zk_session* s = nullptr;
    const int rc = zk_bytecode_open(rows, n, keccak, n_keccak, randomness, opts, &s);
    return rc ? rc : one_shot(s, status_out, result);
}
extern "C" int zk_exp_open(const uint64_t* rows, uint64_t n, uint32_t opts, zk_session** out) {
    NO_DEVICE_PTRS(opts, "zk_exp_open");
    ARG_TRY(out && rows && n > 0 && n < (1ull << 32), "zk_exp_open: bad arguments");
    zk_session* s = new_session(n, true);
    s->a64[0].assign(rows, rows + n * EX_NCELLS * 4);
    s->exp.rows.cells = s->a64[0].data();
    s->exp.rows.flags = nullptr;
    s->exp.rows.n = n;
    s->row = [s](u64 i) { return exp_check_row(s->exp, i); };
    *out = s;
    return 0;
}
extern "C" int zk_exp_verify(const uint64_t* rows, uint64_t n, uint32_t opts, uint32_t* status_out, zk_result* result) {
    ARG_TRY(result, "zk_exp_verify: result is null");
    zk_session* s = nullptr;
    const int rc = zk_exp_open(rows, n, opts, &s);
    return rc ? rc : one_shot(s, status_out, result);
}

// ---- Copy circuit -------------------------------------------------------------------------------------------------------
extern "C" int zk_copy_open(const zk_copy_tables* t, uint32_t opts, zk_session** out) {
    NO_DEVICE_PTRS(opts, "zk_copy_open");
    ARG_TRY(t && out && t->rows && t->randomness && t->n_rows > 0 && t->n_rows < (1ull << 32), "zk_copy_open: bad arguments");
    zk_session* s = new_session(t->n_rows, true);
    s->a64[0].assign(t->rows, t->rows + t->n_rows * CP_NCELLS * 4);
    if (t->row_flags) s->a32[0].assign(t->row_flags, t->row_flags + t->n_rows);
    cpu_table(s->tab[0], t->rw, t->rw_flags, t->n_rw, RW_NCELLS, rw_key_hash);
    cpu_table(s->tab[1], t->bytecode, nullptr, t->n_bytecode, BYTECODE_NCELLS, bc_key_hash);
    cpu_table(s->tab[2], t->tx, t->tx_flags, t->n_tx, TX_NCELLS, tx_key_hash);
    s->copy.rows.cells = s->a64[0].data();
    s->copy.rows.flags = t->row_flags ? s->a32[0].data() : nullptr;
    s->copy.rows.n = t->n_rows;
    s->copy.rw = s->tab[0].t;
    s->copy.bytecode = s->tab[1].t;
    s->copy.tx = s->tab[2].t;
    s->rw_meta = rw_dense_meta_host(t->n_rw ? s->tab[0].cells.data() : nullptr, t->n_rw);
    s->copy.rw_meta = (opts & ZK_OPT_GENERIC_INDEX) ? nullptr : &s->rw_meta;
    s->copy.r = cell_of(t->randomness);
    s->row = [s](u64 i) { return copy_check_row(s->copy, i); };
    *out = s;
    return 0;
}
extern "C" int zk_copy_verify(const zk_copy_tables* t, uint32_t opts, uint32_t* status_out, zk_result* result) {
    ARG_TRY(result, "zk_copy_verify: result is null");
    zk_session* s = nullptr;
    const int rc = zk_copy_open(t, opts, &s);
    return rc ? rc : one_shot(s, status_out, result);
}

// ---- Tx / Sig circuits --------------------------------------------------------------------------------------------------
extern "C" int zk_sign_open(const zk_sign_units* t, uint32_t opts, zk_session** out) {
    NO_DEVICE_PTRS(opts, "zk_sign_open");
    ARG_TRY(t && out && t->bytes && t->cells && t->meta && t->randomness && t->n_units > 0 && t->n_units < (1ull << 32), "zk_sign_open: bad arguments");
    const u64 n = t->n_units;
    zk_session* s = new_session(n, true);
    s->a8.assign(t->bytes, t->bytes + n * SG_NBYTES_ROWS * 32);
    s->a64[0].assign(t->cells, t->cells + n * SG_NCELLS * 4);
    s->a32[0].assign(t->meta, t->meta + n * 4);
    cpu_table(s->tab[0], t->keccak, nullptr, t->n_keccak, KECCAK_NCELLS, keccak_key_hash);
    cpu_table(s->tab[1], t->tx_rows, t->tx_flags, t->n_tx_rows, TX_NCELLS, nullptr);
    SignArgs& a = s->sign;
    a.bytes = s->a8.data();
    a.cells.cells = s->a64[0].data();
    a.cells.flags = nullptr;
    a.cells.n = n;
    a.meta = s->a32[0].data();
    a.keccak = s->tab[0].t;
    a.tx_rows = s->tab[1].t;
    a.tx_rows.n = (u32)t->n_tx_rows;
    a.r = cell_of(t->randomness);
    s->a64[1].resize(64 * 4);
    sign_fill_rpow(a.r, s->a64[1].data());
    a.rpow = s->a64[1].data();
    a.is_sig = t->is_sig ? 1u : 0u;
    s->row = [s](u64 i) { return sign_check_unit(s->sign, i); };
    *out = s;
    return 0;
}
extern "C" int zk_sign_verify(const zk_sign_units* t, uint32_t opts, uint32_t* status_out, zk_result* result) {
    ARG_TRY(result, "zk_sign_verify: result is null");
    zk_session* s = nullptr;
    const int rc = zk_sign_open(t, opts, &s);
    return rc ? rc : one_shot(s, status_out, result);
}

// ---- PI circuit ---------------------------------------------------------------------------------------------------------
extern "C" int zk_pi_open(const uint64_t* rows, uint64_t n, const uint64_t* keccak, uint64_t n_keccak, const uint64_t* gas, uint64_t n_gas,
                          uint64_t circuit_len, const uint64_t* keccak_rand, const uint64_t* byte_pow_base, uint32_t opts, zk_session** out) {
    NO_DEVICE_PTRS(opts, "zk_pi_open");
    ARG_TRY(out && rows && keccak_rand && byte_pow_base && n > 0 && n < (1ull << 32), "zk_pi_open: bad arguments");
    zk_session* s = new_session(n, true);
    s->a64[0].assign(rows, rows + n * 24 * 4);
    cpu_table(s->tab[0], keccak, nullptr, n_keccak, KECCAK_NCELLS, keccak_key_hash);
    cpu_table(s->tab[1], gas, nullptr, n_gas, PI_GAS_NCELLS, pi_gas_key_hash);
    PiArgs& a = s->pi;
    a.rows.cells = s->a64[0].data();
    a.rows.flags = nullptr;
    a.rows.n = n;
    a.keccak = s->tab[0].t;
    a.gas = s->tab[1].t;
    a.keccak_rand_m = fr_to_mont(cell_of(keccak_rand));
    a.byte_pow_base_m = fr_to_mont(cell_of(byte_pow_base));
    a.circuit_len = fr_from_u64(circuit_len);
    s->row = [s](u64 i) { return pi_check_row(s->pi, i); };
    *out = s;
    return 0;
}
extern "C" int zk_pi_verify(const uint64_t* rows, uint64_t n, const uint64_t* keccak, uint64_t n_keccak, const uint64_t* gas, uint64_t n_gas,
                            uint64_t circuit_len, const uint64_t* keccak_rand, const uint64_t* byte_pow_base, uint32_t opts,
                            uint32_t* status_out, zk_result* result) {
    ARG_TRY(result, "zk_pi_verify: result is null");
    zk_session* s = nullptr;
    const int rc = zk_pi_open(rows, n, keccak, n_keccak, gas, n_gas, circuit_len, keccak_rand, byte_pow_base, opts, &s);
    return rc ? rc : one_shot(s, status_out, result);
}

extern "C" int zk_pi_copy_open(const uint64_t* cells, const uint8_t* bytes, const uint32_t* lens, uint64_t n, uint32_t opts, zk_session** out) {
    NO_DEVICE_PTRS(opts, "zk_pi_copy_open");
    ARG_TRY(out && cells && bytes && lens && n > 0 && n < (1ull << 32), "zk_pi_copy_open: bad arguments");
    zk_session* s = new_session(n, false);
    s->a64[0].assign(cells, cells + n * 4);
    s->a8.assign(bytes, bytes + n * 32);
    s->a32[0].assign(lens, lens + n);
    s->picopy.cells = s->a64[0].data();
    s->picopy.bytes = s->a8.data();
    s->picopy.lens = s->a32[0].data();
    s->picopy.n = n;
    s->row = [s](u64 i) { return pi_copy_check(s->picopy, i); };
    *out = s;
    return 0;
}
extern "C" int zk_pi_copy_verify(const uint64_t* cells, const uint8_t* bytes, const uint32_t* lens, uint64_t n, uint32_t opts, uint32_t* status_out,
                                 zk_result* result) {
    ARG_TRY(result, "zk_pi_copy_verify: result is null");
    zk_session* s = nullptr;
    const int rc = zk_pi_copy_open(cells, bytes, lens, n, opts, &s);
    return rc ? rc : one_shot(s, status_out, result);
}

// ---- Keccak table generation --------------------------------------------------------------------------------------------
extern "C" int zk_keccak_open(const uint8_t* data, uint64_t n_bytes, const uint64_t* offsets, uint64_t n_msgs, const uint64_t* randomness,
                              uint32_t mode, uint64_t* rows_dev, uint32_t opts, zk_session** out) {
    NO_DEVICE_PTRS(opts, "zk_keccak_open");
    ARG_TRY(out && offsets && randomness && n_msgs > 0 && n_msgs < (1ull << 32) && (data || n_bytes == 0) && mode <= 1u && !rows_dev,
            "zk_keccak_open: bad arguments");
    for (u64 k = 0; k < n_msgs; k++) ARG_TRY(offsets[k] <= offsets[k + 1], "zk_keccak_open: offsets must be non-decreasing");
    ARG_TRY(offsets[n_msgs] <= n_bytes, "zk_keccak_open: offsets exceed the data buffer");
    zk_session* s = new_session(n_msgs, false);
    s->a8.assign(data, data + n_bytes);
    s->a64[0].assign(offsets, offsets + n_msgs + 1);
    s->a64[1].resize(KT_RPOW_ROWS * 4);
    kt_fill_rpow(cell_of(randomness), s->a64[1].data());
    s->keccak_rows.assign(n_msgs * KT_NCELLS * 4, 0);
    KeccakGenArgs& g = s->kgen;
    g.data = s->a8.data();
    g.offsets = s->a64[0].data();
    g.n = n_msgs;
    g.rpow = s->a64[1].data();
    g.rows = s->keccak_rows.data();
    g.mode = mode;
    g.long_list = nullptr;
    g.long_count = nullptr;
    s->row = [s](u64 i) { return keccak_table_row(s->kgen, i); };
    *out = s;
    return 0;
}
extern "C" int zk_keccak_read_rows(zk_session* s, uint64_t* rows_host) {
    ARG_TRY(s && rows_host && !s->keccak_rows.empty(), "zk_keccak_read_rows: bad arguments");
    memcpy(rows_host, s->keccak_rows.data(), s->keccak_rows.size() * 8);
    return 0;
}
extern "C" int zk_keccak_table(const uint8_t* data, uint64_t n_bytes, const uint64_t* offsets, uint64_t n_msgs, const uint64_t* randomness,
                               uint32_t mode, uint64_t* rows_out, uint32_t opts, uint32_t* status_out, zk_result* result) {
    ARG_TRY(result && rows_out, "zk_keccak_table: null output");
    zk_session* s = nullptr;
    int rc = zk_keccak_open(data, n_bytes, offsets, n_msgs, randomness, mode, nullptr, opts, &s);
    if (rc) return rc;
    rc = zk_launch(s, nullptr);
    if (!rc) rc = zk_collect(s, result);
    if (!rc) rc = zk_keccak_read_rows(s, rows_out);
    if (!rc && status_out) rc = zk_read_status(s, status_out);
    zk_close(s);
    return rc;
}

// ---- secp256k1 ECDSA verification ---------------------------------------------------------------------------------------
extern "C" int zk_ecdsa_open_batches(const zk_ecdsa_batch* bt, uint32_t n_batches, uint32_t opts, zk_session** out) {
    NO_DEVICE_PTRS(opts, "zk_ecdsa_open_batches");
    ARG_TRY(out && bt && (n_batches == 1 || n_batches == 2), "zk_ecdsa_open_batches: one or two batches");
    u64 n = 0;
    for (u32 k = 0; k < n_batches; k++) {
        ARG_TRY(bt[k].bytes && bt[k].n > 0 && bt[k].n < (1ull << 31) && bt[k].layout <= 2u && (!bt[k].v || bt[k].v_stride >= 1) && !bt[k].out_dev,
                "zk_ecdsa_open: bad arguments");
        n += bt[k].n;
    }
    static const u32 OFF[2][5] = {{0, 32, 64, 96, 128}, {64, 96, 160, 224, 256}};
    zk_session* s = new_session(n, false);
    EcdsaArgs& a = s->ecdsa;
    a.n = n;
    ecdsa_single_batch(a);
    a.n0 = bt[0].n;
    for (u32 k = 0; k < n_batches; k++) {
        const u64 stride = bt[k].layout ? 288 : 160;
        std::vector<uint8_t>& hb = k == 0 ? s->a8 : s->a8b;
        std::vector<u32>& hv = s->a32[k];
        hb.assign(bt[k].bytes, bt[k].bytes + bt[k].n * stride);
        if (bt[k].v) hv.assign(bt[k].v, bt[k].v + bt[k].n * bt[k].v_stride);
        if (k == 0) {
            a.stride = stride; a.bytes = hb.data(); a.v = bt[k].v ? hv.data() : nullptr; a.v_stride = bt[k].v_stride; a.msg_be = bt[k].layout != 1u;
            for (int c = 0; c < 5; c++) a.off[c] = OFF[bt[k].layout ? 1 : 0][c];
        } else {
            a.stride1 = stride; a.bytes1 = hb.data(); a.v1 = bt[k].v ? hv.data() : nullptr; a.v_stride1 = bt[k].v_stride; a.msg_be1 = bt[k].layout != 1u;
            for (int c = 0; c < 5; c++) a.off1[c] = OFF[bt[k].layout ? 1 : 0][c];
        }
    }
    a.out = nullptr;
    a.out_stride = 0;
    a.lanes = SecpLanes{nullptr, 1, 1, nullptr, 0};
    s->row = [s](u64 i) {
        u32 tab[15 * 24];  // the key's multiples: per call on the CPU
        return ecdsa_verify_one(s->ecdsa, i, tab, 1);
    };
    *out = s;
    return 0;
}
extern "C" int zk_ecdsa_open(const uint8_t* bytes, uint32_t layout, const uint32_t* v, uint32_t v_stride, uint64_t n, uint32_t* out_dev,
                             uint32_t out_stride, uint32_t opts, zk_session** out) {
    zk_ecdsa_batch b;
    b.bytes = bytes; b.layout = layout; b.v = v; b.v_stride = v_stride; b.n = n; b.out_dev = out_dev; b.out_stride = out_stride;
    return zk_ecdsa_open_batches(&b, 1, opts, out);
}
extern "C" int zk_ecdsa_verify(const uint8_t* bytes, uint32_t layout, const uint32_t* v, uint32_t v_stride, uint64_t n, uint32_t opts,
                               uint32_t* status_out, zk_result* result) {
    ARG_TRY(result, "zk_ecdsa_verify: result is null");
    zk_session* s = nullptr;
    const int rc = zk_ecdsa_open(bytes, layout, v, v_stride, n, nullptr, 0, opts, &s);
    return rc ? rc : one_shot(s, status_out, result);
}

// ---- witness assignment (state_circuit.py:827-934, bytecode_circuit.py:104-167, evm_circuit/typing.py CopyCircuit.copy): the device
// functions of csrc/state_assign.hpp / bytecode_assign.hpp / copy_assign.hpp in plain host loops.  A pass (zk_launch) computes the
// outputs into session-owned buffers; zk_*_assign_read copies them out.  Output pointers at open need ZK_OPT_DEVICE_PTRS, which
// has no meaning here.
static void state_assign_pass(zk_session* s) {
    AssignArgs& a = s->assign;
    const u64 n = a.n;
    std::fill(s->a32[1].begin(), s->a32[1].end(), ZK_EMPTY_SLOT);  // slots
    std::fill(s->a32[2].begin(), s->a32[2].end(), ASG_NONE);       // first
    // ops are inserted in REVERSE order so that the "smallest index wins" rule is what makes the result right
    for (u64 i = n; i-- > 0;)
        if (asg_has_key(asg_slot(a, ASG_TAG, i))) asg_insert(a, (u32)i);
    u32 r = 0;
    u32* first = s->a32[2].data();
    u32* rank = s->a32[3].data();
    for (u64 i = 0; i < n; i++) {
        if (!asg_has_key(asg_slot(a, ASG_TAG, i))) continue;
        first[i] = asg_find_first(a, (u32)i);
        if (first[i] == (u32)i) { rank[i] = r; asg_write_mpt(a, i, r); r++; }
    }
    s->n_mpt = r;
    u32 nxt = ASG_NONE;
    for (u64 i = n; i-- > 0;) {
        const u64 root = 3ull + 5ull * (nxt == ASG_NONE ? r : rank[first[nxt]]);
        s->status[i] = asg_write_row(a, i, root, first[i] == (u32)i);
        if (first[i] != ASG_NONE) nxt = (u32)i;
    }
}
extern "C" int zk_state_assign_open(const uint64_t* ops, const uint32_t* op_flags, uint64_t n, uint64_t* rows_dev, uint32_t* row_flags_dev,
                                    uint64_t* mpt_dev, uint32_t opts, zk_session** out) {
    NO_DEVICE_PTRS(opts, "zk_state_assign_open");
    ARG_TRY(out && ops && op_flags && n > 0 && n < (1ull << 31) && !rows_dev && !row_flags_dev && !mpt_dev, "zk_state_assign_open: bad arguments");
    zk_session* s = new_session(n, false);
    s->a64[0].assign(ops, ops + n * ASG_NSLOTS * 4);
    s->a32[0].assign(op_flags, op_flags + n);
    const bool compact = opts & ZK_OPT_STATE_COMPACT;
    s->a64[1].assign(n * (compact ? 15 : ASG_ROW_NCELLS) * 4, 0);  // rows
    s->a64[2].assign(n * ASG_MPT_NCELLS * 4, 0);  // mpt
    s->out32.assign(n, 0);                        // row flags
    u32 cap = 16;
    while (cap < 2 * n + 2) cap <<= 1;
    s->a32[1].assign(cap, ZK_EMPTY_SLOT);
    s->a32[2].assign(n, ASG_NONE);
    s->a32[3].assign(n, 0);
    AssignArgs& a = s->assign;
    a.ops = s->a64[0].data(); a.op_flags = s->a32[0].data(); a.n = n;
    a.rows = s->a64[1].data(); a.row_flags = s->out32.data(); a.mpt = s->a64[2].data();
    a.slots = s->a32[1].data(); a.mask = cap - 1; a.first = s->a32[2].data(); a.rank = s->a32[3].data();
    a.nb = 0; a.blk_cnt = nullptr; a.blk_next = nullptr;
    a.compact = compact ? 1u : 0u;
    s->pass = state_assign_pass;
    s->assign_kind = 1;
    *out = s;
    return 0;
}
extern "C" int zk_state_assign_read(zk_session* s, uint64_t* rows_host, uint32_t* row_flags_host, uint64_t* mpt_host, uint64_t mpt_capacity_rows,
                                    uint64_t* n_mpt_out) {
    ARG_TRY(s && s->assign_kind == 1, "zk_state_assign_read: bad arguments");
    if (n_mpt_out) *n_mpt_out = s->n_mpt;
    if (rows_host) memcpy(rows_host, s->a64[1].data(), s->a64[1].size() * 8);
    if (row_flags_host) memcpy(row_flags_host, s->out32.data(), s->out32.size() * 4);
    if (mpt_host) {
        ARG_TRY(mpt_capacity_rows >= s->n_mpt, "zk_state_assign_read: mpt buffer too small");
        memcpy(mpt_host, s->a64[2].data(), (size_t)s->n_mpt * ASG_MPT_NCELLS * 32);
    }
    return 0;
}
extern "C" int zk_state_assign(const uint64_t* ops, const uint32_t* op_flags, uint64_t n, uint64_t* rows_out, uint32_t* row_flags_out,
                               uint64_t* mpt_out, uint64_t* n_mpt_out, uint32_t opts, uint32_t* status_out, zk_result* result) {
    ARG_TRY(result && n_mpt_out, "zk_state_assign: null output");
    zk_session* s = nullptr;
    int rc = zk_state_assign_open(ops, op_flags, n, nullptr, nullptr, nullptr, opts, &s);
    if (rc) return rc;
    rc = zk_launch(s, nullptr);
    if (!rc) rc = zk_collect(s, result);
    if (!rc) rc = zk_state_assign_read(s, rows_out, row_flags_out, mpt_out, n, n_mpt_out);
    if (!rc && status_out) rc = zk_read_status(s, status_out);
    zk_close(s);
    return rc;
}

// ---- RW table -> State-circuit operations (state_rekey.hpp): the device's per-row functions and its compact-key plan, the sort
// itself a std::stable_sort over the compact keys (the device sorts the same keys with LSD radix passes).
#include "state_rekey_plan.hpp"
#include <algorithm>
static void rekey_scan_host(const u64* rw, u64 n, std::vector<u32>& masks) {
    masks.assign(2 * RWK_MASK_WORDS_H + RWK_NCLASSES, 0u);
    for (u64 i = 0; i < n; i++) {
        const RwkKey k = rwk_key(rw + i * (RWK_RW_NCELLS * 4));
        masks[2 * RWK_MASK_WORDS_H + k.cls]++;
        if (k.cls == RWK_CLASS_DROPPED) continue;
        for (int f = 0; f < RWK_NFIELDS; f++)
            for (int w = 0; w < 8; w++) {
                const u32 slot = (k.cls * RWK_NFIELDS + f) * 8 + w;
                masks[slot] |= k.f[f].v[w];
                masks[RWK_MASK_WORDS_H + slot] |= ~k.f[f].v[w];
            }
    }
}
static void state_rekey_pass(zk_session* s) {
    const u64 n = s->n;
    const u64* rw = s->a64[0].data();
    const u32* fl = s->a32[0].data();
    RwkPlan plan;
    memcpy(&plan, s->rekey_plan.data(), sizeof(plan));
    // ranks of the plan's wide fields: rank = number of class members with a smaller value
    std::vector<u32> ranks[RWK_NFIELDS];
    for (size_t j = 0; j + 3 < s->rekey_jobs.size(); j += 4) {
        const u32 cls = s->rekey_jobs[j], field = s->rekey_jobs[j + 1];
        if (ranks[field].empty()) ranks[field].assign(n, 0u);
        std::vector<std::pair<Fr, u32>> mem;
        for (u64 i = 0; i < n; i++) {
            const RwkKey k = rwk_key(rw + i * (RWK_RW_NCELLS * 4));
            if (k.cls == cls) mem.push_back({k.f[field], (u32)i});
        }
        std::sort(mem.begin(), mem.end(), [](const std::pair<Fr, u32>& x, const std::pair<Fr, u32>& y) { return fr_lt(x.first, y.first); });
        u32 r = 0;
        for (size_t q = 0; q < mem.size(); q++) {
            if (q && fr_lt(mem[q - 1].first, mem[q].first)) r = (u32)q;
            ranks[field][mem[q].second] = r;
        }
    }
    const u32 kw = plan.key_words;
    std::vector<u32> keys((size_t)kw * n);
    for (u64 i = 0; i < n; i++) {
        const RwkKey k = rwk_key(rw + i * (RWK_RW_NCELLS * 4));
        u32 rk[RWK_NFIELDS];
        for (int f = 0; f < RWK_NFIELDS; f++) rk[f] = ranks[f].empty() ? 0u : ranks[f][i];
        rwk_pack(plan, plan.cls[k.cls], k, rk, keys.data() + i, n);
        s->status[i] = k.status;
    }
    std::vector<u32> order(n);
    for (u64 i = 0; i < n; i++) order[i] = (u32)i;
    std::stable_sort(order.begin(), order.end(), [&](u32 x, u32 y) {
        for (u32 w = 0; w < kw; w++) {
            const u32 a = keys[(size_t)w * n + x], b = keys[(size_t)w * n + y];
            if (a != b) return a < b;
        }
        return false;
    });
    u64* ops = s->a64[1].data();
    u32* of = s->out32.data();
    rwk_emit_start(ops, of, s->n_ops);
    for (u64 j = 1; j < s->n_ops; j++) {
        const u64* p = rw + (u64)order[j - 1] * (RWK_RW_NCELLS * 4);
        const RwkKey k = rwk_key(p);
        rwk_emit(ops, of, s->n_ops, j, k, rwk_op(p, fl[order[j - 1]], k));
    }
}
extern "C" int zk_state_ops_from_rw_open(const uint64_t* rw, const uint32_t* rw_flags, uint64_t n, uint64_t* ops_dev, uint32_t* op_flags_dev,
                                         uint32_t opts, uint64_t* n_ops_out, zk_session** out) {
    NO_DEVICE_PTRS(opts, "zk_state_ops_from_rw_open");
    ARG_TRY(out && rw && n > 0 && n < (1ull << 31) && !ops_dev && !op_flags_dev, "zk_state_ops_from_rw_open: bad arguments");
    zk_session* s = new_session(n, false);
    s->a64[0].assign(rw, rw + n * RWK_RW_NCELLS * 4);
    if (rw_flags) s->a32[0].assign(rw_flags, rw_flags + n);
    else s->a32[0].assign(n, 0u);
    std::vector<u32> masks;
    rekey_scan_host(s->a64[0].data(), n, masks);
    RwkHostPlan hp;
    const char* e = getenv("ZK_REKEY_NO_RANKS");
    rwk_build_plan(masks.data(), !(e && e[0] == '1'), hp);
    s->rekey_plan.assign((sizeof(RwkPlan) + 3) / 4, 0u);
    memcpy(s->rekey_plan.data(), &hp.plan, sizeof(RwkPlan));
    for (const RwkRankJob& j : hp.jobs) { s->rekey_jobs.push_back(j.cls); s->rekey_jobs.push_back(j.field); s->rekey_jobs.push_back(j.base); s->rekey_jobs.push_back(j.count); }
    s->n_ops = 1 + hp.n_kept;
    s->a64[1].assign(s->n_ops * RWK_NSLOTS * 4, 0);
    s->out32.assign(s->n_ops, 0);
    s->pass = state_rekey_pass;
    s->assign_kind = 4;
    if (n_ops_out) *n_ops_out = s->n_ops;
    *out = s;
    return 0;
}
extern "C" int zk_state_ops_from_rw_read(zk_session* s, uint64_t* ops_host, uint32_t* op_flags_host, uint64_t* n_ops_out) {
    ARG_TRY(s && s->assign_kind == 4, "zk_state_ops_from_rw_read: bad arguments");
    if (n_ops_out) *n_ops_out = s->n_ops;
    if (ops_host) memcpy(ops_host, s->a64[1].data(), s->a64[1].size() * 8);
    if (op_flags_host) memcpy(op_flags_host, s->out32.data(), s->out32.size() * 4);
    return 0;
}
extern "C" int zk_state_ops_from_rw(const uint64_t* rw, const uint32_t* rw_flags, uint64_t n, uint64_t* ops_out, uint32_t* op_flags_out,
                                    uint64_t* n_ops_out, uint32_t opts, uint32_t* status_out, zk_result* result) {
    ARG_TRY(result && n_ops_out, "zk_state_ops_from_rw: null output");
    zk_session* s = nullptr;
    int rc = zk_state_ops_from_rw_open(rw, rw_flags, n, nullptr, nullptr, opts, n_ops_out, &s);
    if (rc) return rc;
    rc = zk_launch(s, nullptr);
    if (!rc) rc = zk_collect(s, result);
    if (!rc) rc = zk_state_ops_from_rw_read(s, ops_out, op_flags_out, n_ops_out);
    if (!rc && status_out) rc = zk_read_status(s, status_out);
    zk_close(s);
    return rc;
}

// RW table -> State rows in one session: here simply the two host passes back to back (the device reads its ops straight from
// the RW rows; the results are the same by construction of asg_slot_rw, which tests/test_state_rekey.py checks on the device).
extern "C" int zk_state_assign_from_rw_open(const uint64_t* rw, const uint32_t* rw_flags, uint64_t n_rw, uint64_t* rows_dev,
                                            uint32_t* row_flags_dev, uint64_t* mpt_dev, uint32_t opts, uint64_t* n_ops_out, zk_session** out) {
    NO_DEVICE_PTRS(opts, "zk_state_assign_from_rw_open");
    ARG_TRY(out && rw && n_rw > 0 && !rows_dev && !row_flags_dev && !mpt_dev, "zk_state_assign_from_rw_open: bad arguments");
    zk_session* r = nullptr;
    uint64_t n_ops = 0;
    int rc = zk_state_ops_from_rw_open(rw, rw_flags, n_rw, nullptr, nullptr, opts, &n_ops, &r);
    if (rc) return rc;
    run_pass(r, nullptr);
    if (r->fail_count) {
        g_err = "zk_state_assign_from_rw_open: the RW table has rows the re-keying rejects (zk_state_ops_from_rw reports them)";
        zk_close(r);
        return -1;
    }
    rc = zk_state_assign_open(r->a64[1].data(), r->out32.data(), n_ops, nullptr, nullptr, nullptr, opts, out);
    zk_close(r);
    if (!rc && n_ops_out) *n_ops_out = n_ops;
    return rc;
}

// RW table -> State verdict: the device evaluates the rows where it computes them (state_fused.hpp); here the three host passes back
// to back — re-keying, assignment (15-cell rows), State circuit — with the errors of the first two reported by the open.
extern "C" int zk_state_verify_from_rw_open(const uint64_t* rw, const uint32_t* rw_flags, uint64_t n_rw, uint32_t opts, uint64_t* n_ops_out,
                                            zk_session** out) {
    NO_DEVICE_PTRS(opts, "zk_state_verify_from_rw_open");
    ARG_TRY(out && rw && n_rw > 0, "zk_state_verify_from_rw_open: bad arguments");
    zk_session* a = nullptr;
    uint64_t n_ops = 0;
    int rc = zk_state_assign_from_rw_open(rw, rw_flags, n_rw, nullptr, nullptr, nullptr, opts | ZK_OPT_STATE_COMPACT, &n_ops, &a);
    if (rc) return rc;
    run_pass(a, nullptr);
    if (a->fail_count) {
        char msg[200];
        snprintf(msg, sizeof msg, "zk_state_verify_from_rw: the State witness assignment failed for %llu ops (first: %llu, code 0x%08x; zk_state_assign_from_rw reports each)",
                 (unsigned long long)a->fail_count, (unsigned long long)a->first_row, (unsigned)a->first_code);
        g_err = msg;
        zk_close(a);
        return -1;
    }
    rc = zk_state_open(a->a64[1].data(), a->out32.data(), n_ops, a->a64[2].data(), a->n_mpt, opts | ZK_OPT_STATE_COMPACT, out);
    zk_close(a);
    if (!rc && n_ops_out) *n_ops_out = n_ops;
    return rc;
}
extern "C" int zk_state_verify_from_rw(const uint64_t* rw, const uint32_t* rw_flags, uint64_t n, uint32_t opts, uint32_t* status_out,
                                       uint64_t* n_ops_out, zk_result* result) {
    ARG_TRY(result, "zk_state_verify_from_rw: result is null");
    zk_session* s = nullptr;
    int rc = zk_state_verify_from_rw_open(rw, rw_flags, n, opts, n_ops_out, &s);
    if (rc) return rc;
    rc = zk_launch(s, nullptr);
    if (!rc) rc = zk_collect(s, result);
    if (!rc && status_out) rc = zk_read_status(s, status_out);
    zk_close(s);
    return rc;
}

// the block one-shot is four chains on four device streams: there is nothing to overlap on the host — callers of the CPU backend use the
// per-circuit entries (zkevm_specs_amd/super_circuit.py does, on host arrays)
extern "C" int zk_block_verify(const zk_block*, uint32_t, zk_result*, double*) {
    g_err = "zk_block_verify: not available on the CPU backend (it needs ZK_OPT_DEVICE_PTRS); use the per-circuit entries";
    return -1;
}

static void bytecode_assign_pass(zk_session* s) {
    BcaArgs& a = s->bca;
    for (u64 c = 0; c < a.n_chunks; c++) bca_chunk(a, c);
    for (u64 j = 0; j < a.n_codes; j++) bca_prefix_code(a, j);
    for (u64 c = 0; c < a.n_chunks; c++) bca_rlc_chunk(a, c);
    for (u64 i = 0; i < a.n_out; i++) bca_write_row(a, i);
}
extern "C" int zk_bytecode_assign_open(const uint64_t* in_rows, uint64_t n_rows, const uint64_t* offsets, const uint64_t* lengths, uint64_t n_codes,
                                       uint32_t k, const uint64_t* randomness, uint64_t* rows_dev, uint32_t opts, zk_session** out) {
    NO_DEVICE_PTRS(opts, "zk_bytecode_assign_open");
    ARG_TRY(out && offsets && (lengths || n_codes == 0) && randomness && k >= 1 && k <= 30 && n_rows < (1ull << 31) && n_codes < (1ull << 31) && (in_rows || n_rows == 0) &&
            !rows_dev, "zk_bytecode_assign_open: bad arguments");
    ARG_TRY(offsets[0] == 0 && offsets[n_codes] == n_rows, "zk_bytecode_assign_open: offsets must span the rows");
    for (u64 j = 0; j < n_codes; j++) ARG_TRY(offsets[j] <= offsets[j + 1], "zk_bytecode_assign_open: offsets must be non-decreasing");
    zk_session* s = new_session(1ull << k, false);
    s->a64[0].assign(in_rows, in_rows + n_rows * 6 * 4);
    s->a64[1].assign(offsets, offsets + n_codes + 1);
    s->a64[2].assign(lengths, lengths + n_codes);
    std::vector<BcaChunk>& chunks = s->bca_chunks;
    s->a32[0].assign(n_codes + 1, 0);  // code_chunk0
    for (u64 j = 0; j < n_codes; j++) {
        s->a32[0][j] = (u32)chunks.size();
        for (u64 g = offsets[j]; g < offsets[j + 1]; g += BCA_CHUNK) {
            BcaChunk c;
            c.code = (u32)j; c.start = (u32)g;
            c.count = (u32)((offsets[j + 1] - g < BCA_CHUNK) ? offsets[j + 1] - g : BCA_CHUNK);
            c.first = g == offsets[j] ? 1u : 0u;
            chunks.push_back(c);
        }
    }
    s->a32[0][n_codes] = (u32)chunks.size();
    s->a64[3].assign(BCA_RPOW_ROWS * 4, 0);
    bca_fill_rpow(cell_of(randomness), s->a64[3].data());
    s->w64[0].assign(chunks.size() * 4 + 4, 0);  // chunk_acc
    s->w64[1].assign(chunks.size() * 4 + 4, 0);  // chunk_in
    s->w64[2].assign(n_rows * 4 + 4, 0);         // rlc
    s->w64[3].assign((size_t)(1ull << k) * 12 * 4, 0);  // output rows
    s->a32[1].assign(chunks.size() + 1, 0);      // chunk_m
    s->a32[2].assign(n_rows + 1, 0);             // row_code
    s->a32[3].assign(chunks.size() + 1, 0);      // chunk_state
    s->bca_map.assign((chunks.size() + 1) * BCA_MAP_STRIDE, 0);
    s->a8.assign(2 * n_rows + 2, 0);             // track
    BcaArgs& a = s->bca;
    a.in_rows = s->a64[0].data(); a.offsets = s->a64[1].data(); a.lengths = s->a64[2].data(); a.n_in = n_rows; a.n_codes = n_codes; a.n_out = 1ull << k;
    a.rpow = s->a64[3].data(); a.chunks = chunks.data(); a.code_chunk0 = s->a32[0].data(); a.n_chunks = chunks.size();
    a.track = s->a8.data(); a.chunk_acc = s->w64[0].data(); a.chunk_m = s->a32[1].data(); a.chunk_in = s->w64[1].data(); a.rlc = s->w64[2].data();
    a.row_code = s->a32[2].data(); a.rows = s->w64[3].data();
    a.chunk_map = s->bca_map.data(); a.chunk_state = s->a32[3].data();
    s->pass = bytecode_assign_pass;
    s->assign_kind = 2;
    *out = s;
    return 0;
}
extern "C" int zk_bytecode_assign_read(zk_session* s, uint64_t* rows_host) {
    ARG_TRY(s && rows_host && s->assign_kind == 2, "zk_bytecode_assign_read: bad arguments");
    memcpy(rows_host, s->w64[3].data(), s->w64[3].size() * 8);
    return 0;
}
extern "C" int zk_bytecode_assign(const uint64_t* in_rows, uint64_t n_rows, const uint64_t* offsets, const uint64_t* lengths, uint64_t n_codes, uint32_t k,
                                  const uint64_t* randomness, uint64_t* rows_out, uint32_t opts, zk_result* result) {
    ARG_TRY(result && rows_out, "zk_bytecode_assign: null output");
    zk_session* s = nullptr;
    int rc = zk_bytecode_assign_open(in_rows, n_rows, offsets, lengths, n_codes, k, randomness, nullptr, opts, &s);
    if (rc) return rc;
    rc = zk_launch(s, nullptr);
    if (!rc) rc = zk_collect(s, result);
    if (!rc) rc = zk_bytecode_assign_read(s, rows_out);
    zk_close(s);
    return rc;
}

// ---- Bytecode table + Bytecode-circuit witness + keccak rows from raw contract code (bytecode_code.hpp): the device functions in host loops
static void bytecode_from_code_pass(zk_session* s) {
    BccArgs& a = s->bcc;
    for (u64 c = 0; c < a.p.n_chunks; c++) bcc_chunk(a, c);
    for (u64 j = 0; j < a.n_codes; j++) bca_prefix_code(a.p, j);
    for (u64 j = 0; j < a.n_codes; j++) keccak_table_row(s->bcc_kgen, j);
    const u64 n_lanes = a.n_rows > a.n_out ? a.n_rows : a.n_out;
    for (u64 i = 0; i < n_lanes; i++) bcc_write_row(a, i);
}
extern "C" int zk_bytecode_from_code_open(const zk_code_set* in, const zk_code_wire* out_dev, uint32_t opts, zk_session** out) {
    NO_DEVICE_PTRS(opts, "zk_bytecode_from_code_open");
    ARG_TRY(in && out && in->randomness && in->offsets && (in->code || in->n_bytes == 0) && !out_dev, "zk_bytecode_from_code_open: bad arguments");
    ARG_TRY(in->k <= 28, "zk_bytecode_from_code_open: k must be at most 28");
    ARG_TRY(in->n_bytes < (1ull << 31) && in->n_codes < (1ull << 31) && in->n_bytes + in->n_codes < (1ull << 31),
            "zk_bytecode_from_code_open: n_bytes + n_codes must be below 2^31");
    const u64 n_codes = in->n_codes, n_bytes = in->n_bytes, n_rows = n_bytes + n_codes, n_out = in->k ? 1ull << in->k : 0;
    const u64* off = in->offsets;
    ARG_TRY(off[0] == 0, "zk_bytecode_from_code_open: offsets must start at 0");
    for (u64 j = 0; j < n_codes; j++) ARG_TRY(off[j] <= off[j + 1], "zk_bytecode_from_code_open: offsets must be non-decreasing");
    ARG_TRY(off[n_codes] == n_bytes, "zk_bytecode_from_code_open: offsets must end at n_bytes");
    zk_session* s = new_session(n_rows, false);
    s->a8.assign((n_bytes + 15) & ~7ull, 0);  // (the sponge reads whole aligned words)
    if (n_bytes) memcpy(s->a8.data(), in->code, n_bytes);
    s->bcc64[0].assign(off, off + n_codes + 1);
    std::vector<BcaChunk>& chunks = s->bca_chunks;
    s->bcc32[0].assign(n_codes + 1, 0);  // row_off
    s->bcc32[1].assign(n_codes + 1, 0);  // code_chunk0
    for (u64 j = 0; j < n_codes; j++) {
        s->bcc32[0][j] = (u32)(off[j] + j);
        s->bcc32[1][j] = (u32)chunks.size();
        for (u64 b = off[j]; b < off[j + 1]; b += BCA_CHUNK) {
            BcaChunk c;
            c.code = (u32)j; c.start = (u32)b;
            c.count = (u32)((off[j + 1] - b < BCA_CHUNK) ? off[j + 1] - b : BCA_CHUNK);
            c.first = 0;
            chunks.push_back(c);
        }
    }
    s->bcc32[0][n_codes] = (u32)n_rows;
    s->bcc32[1][n_codes] = (u32)chunks.size();
    s->bcc64[1].assign(BCA_RPOW_ROWS * 4, 0);
    bca_fill_rpow(cell_of(in->randomness), s->bcc64[1].data());
    s->bcc64[2].assign(chunks.size() * 4 + 4, 0);  // chunk_acc
    s->bcc64[3].assign(chunks.size() * 4 + 4, 0);  // chunk_in
    s->bcc64[4].assign(n_bytes * 4 + 4, 0);        // part
    s->bcc64[5].assign(n_rows * BCC_TABLE_NCELLS * 4 + 4, 0);  // table
    s->bcc64[6].assign(n_out * BCA_OUT_NCELLS * 4 + 4, 0);     // rows
    s->bcc64[7].assign(KT_RPOW_ROWS * 4, 0);
    kt_fill_rpow(cell_of(in->randomness), s->bcc64[7].data());
    s->bcc32[2].assign(chunks.size() + 1, 0);      // chunk_m
    s->bcc32[3].assign(chunks.size() + 1, 0);      // chunk_state
    s->bca_map.assign((chunks.size() + 1) * BCA_MAP_STRIDE, 0);
    s->keccak_rows.assign(n_codes * KT_NCELLS * 4 + 4, 0);
    KeccakGenArgs& g = s->bcc_kgen;
    g.data = s->a8.data(); g.offsets = s->bcc64[0].data(); g.n = n_codes; g.rpow = s->bcc64[7].data(); g.rows = s->keccak_rows.data();
    g.mode = KT_MODE_CIRCUIT; g.long_list = nullptr; g.long_count = nullptr;
    BccArgs& a = s->bcc;
    memset(&a, 0, sizeof(a));
    a.code = s->a8.data(); a.offsets = s->bcc64[0].data(); a.row_off = s->bcc32[0].data();
    a.n_bytes = n_bytes; a.n_codes = n_codes; a.n_rows = n_rows; a.n_out = n_out;
    a.p.chunks = chunks.data(); a.p.code_chunk0 = s->bcc32[1].data(); a.p.n_chunks = chunks.size(); a.p.n_codes = n_codes;
    a.p.rpow = s->bcc64[1].data(); a.p.chunk_acc = s->bcc64[2].data(); a.p.chunk_in = s->bcc64[3].data(); a.p.chunk_m = s->bcc32[2].data();
    a.p.chunk_state = s->bcc32[3].data(); a.p.chunk_map = s->bca_map.data();
    a.part = s->bcc64[4].data(); a.keccak = g.rows; a.table = s->bcc64[5].data(); a.rows = s->bcc64[6].data();
    s->pass = bytecode_from_code_pass;
    s->assign_kind = 10;
    *out = s;
    return 0;
}
extern "C" int zk_bytecode_from_code_read(zk_session* s, const zk_code_wire* host) {
    ARG_TRY(s && s->assign_kind == 10, "zk_bytecode_from_code_read: bad arguments");
    const BccArgs& a = s->bcc;
    ARG_TRY(!(host && host->rows) || a.n_out, "zk_bytecode_from_code_read: rows asked for with k == 0");
    if (host) {
        if (host->table) memcpy(host->table, a.table, a.n_rows * BCC_TABLE_NCELLS * 32);
        if (host->rows) memcpy(host->rows, a.rows, a.n_out * BCA_OUT_NCELLS * 32);
        if (host->keccak) memcpy(host->keccak, a.keccak, a.n_codes * KT_NCELLS * 32);
    }
    return 0;
}
extern "C" int zk_bytecode_from_code(const zk_code_set* in, const zk_code_wire* out, uint32_t opts, zk_result* result) {
    ARG_TRY(result && out && in, "zk_bytecode_from_code: null argument");
    ARG_TRY(in->k > 0 || !out->rows, "zk_bytecode_from_code: rows asked for with k == 0");
    zk_session* s = nullptr;
    int rc = zk_bytecode_from_code_open(in, nullptr, opts, &s);
    if (rc) return rc;
    rc = zk_launch(s, nullptr);
    if (!rc) rc = zk_collect(s, result);
    if (!rc) rc = zk_bytecode_from_code_read(s, out);
    zk_close(s);
    return rc;
}

// ---- EVM circuit tx / block / withdrawal tables from raw block data (block_tables.hpp): the device functions in host loops
static void tables_from_block_pass(zk_session* s) {
    BtbArgs& a = s->btb;
    for (u64 b = 0; b < a.n_gas_blocks; b++) a.gas_part[b] = btb_gas_block(a, b);
    btb_gas_prefix(a);
    for (u64 row = 0; row < a.n_tx_rows; row++) {
        const u64 i = btb_tx_of_row(a, row, 0);
        const u64 o0 = a.offs[i], o1 = a.offs[i + 1];
        for (u32 q = 0; q < BTB_TX_PIECES; q++) btb_tx_piece(a, i, o0, o1, row, q, a.tx[(row * BTB_TX_PIECES + q) * 2], a.tx[(row * BTB_TX_PIECES + q) * 2 + 1]);
        a.tx_flags[row] = btb_tx_flag(i, o0, row);
    }
    for (u64 r = 0; r < a.n_block_rows; r++) btb_block_row(a, r);
    for (u64 r = 0; r < a.n_wd; r++) btb_wd_row(a, r);
}
#define BTB_ARGS_OK(t) ((t) && (t)->calldata_offsets && ((t)->n_txs == 0 || ((t)->tx_fields && (t)->to_is_none && (t)->access_list)) && \
                        ((t)->n_history == 0 || (t)->history_hashes) && ((t)->n_withdrawals == 0 || (t)->withdrawals))
static int btb_prepare(const zk_block_data* t, BtbPlan& z) {
    char msg[256];
    int rc = btb_plan_counts(t->n_txs, t->n_history, t->n_withdrawals, t->block != nullptr, msg, sizeof msg);  // (before any array is read)
    if (!rc) rc = btb_plan(t->tx_fields, t->calldata_offsets, t->n_txs, t->block, t->n_history, t->withdrawals, t->n_withdrawals, 0, z, msg, sizeof msg);
    if (rc) { g_err = msg; return rc; }
    if (z.n_bytes && !t->calldata) { g_err = "zk_evm_tables_from_block: calldata is null"; return -1; }
    return 0;
}
extern "C" int zk_evm_tables_from_block_sizes(const zk_block_data* t, uint32_t opts, uint64_t* n_tx_rows, uint64_t* n_block_rows, uint64_t* n_withdrawal_rows) {
    NO_DEVICE_PTRS(opts, "zk_evm_tables_from_block_sizes");
    ARG_TRY(BTB_ARGS_OK(t), "zk_evm_tables_from_block_sizes: bad arguments");
    BtbPlan z;
    const int rc = btb_prepare(t, z);
    if (rc) return rc;
    if (n_tx_rows) *n_tx_rows = z.n_tx_rows;
    if (n_block_rows) *n_block_rows = z.n_block_rows;
    if (n_withdrawal_rows) *n_withdrawal_rows = t->n_withdrawals;
    return 0;
}
extern "C" int zk_evm_tables_from_block_open(const zk_block_data* t, const zk_block_tables* out_dev, uint32_t opts, zk_session** out) {
    NO_DEVICE_PTRS(opts, "zk_evm_tables_from_block_open");
    ARG_TRY(BTB_ARGS_OK(t) && out, "zk_evm_tables_from_block_open: bad arguments");
    ARG_TRY(!out_dev, "zk_evm_tables_from_block_open: out_dev needs ZK_OPT_DEVICE_PTRS");
    BtbPlan z;
    int rc = btb_prepare(t, z);
    if (rc) return rc;
    const u64 n = t->n_txs, nw = t->n_withdrawals, nh = t->n_history;
    zk_session* s = new_session(z.n_tx_rows, false);
    BtbArgs& a = s->btb;
    memset(&a, 0, sizeof(a));
    s->btb64[0].assign(t->tx_fields, t->tx_fields + n * BTB_NTX_FIELDS * 4);
    s->btb64[1].assign(t->calldata_offsets, t->calldata_offsets + n + 1);
    s->btb64[2].assign(n * 4 + 4, 0);
    for (u64 i = 0; i < n; i++) memcpy(s->btb64[2].data() + 4 * i, t->tx_fields + i * BTB_NTX_FIELDS * 4, 32);
    if (t->block) s->btb64[3].assign(t->block, t->block + BTB_NBLOCK_FIELDS * 4);
    s->btb64[4].assign(t->history_hashes, t->history_hashes + nh * 4);
    s->btb64[5].assign(t->withdrawals, t->withdrawals + nw * BTB_WD_NCELLS * 4);
    s->btb64[6].assign(nw * 4 + 4, 0);
    for (u64 i = 0; i < nw; i++) memcpy(s->btb64[6].data() + 4 * i, t->withdrawals + i * BTB_WD_NCELLS * 4, 32);
    s->btb64[7].assign(z.n_tx_rows * BTB_TX_NCELLS * 4 + 4, 0);
    s->btb64[8].assign(z.n_block_rows * BTB_BLOCK_NCELLS * 4 + 4, 0);
    s->btb64[9].assign(nw * BTB_WD_NCELLS * 4 + 4, 0);
    s->btb32[0].assign(t->to_is_none, t->to_is_none + n);
    s->btb32[1].assign(t->access_list, t->access_list + 2 * n);
    s->a8.assign(z.n_bytes + 16, 0);
    if (z.n_bytes) memcpy(s->a8.data(), t->calldata, z.n_bytes);
    a.txf = s->btb64[0].data(); a.offs = s->btb64[1].data(); a.ids = s->btb64[2].data(); a.block = s->btb64[3].data();
    a.hashes = s->btb64[4].data(); a.wd = s->btb64[5].data(); a.wd_ids = s->btb64[6].data();
    a.to_none = s->btb32[0].data(); a.access = s->btb32[1].data(); a.calldata = s->a8.data();
    a.n_txs = n; a.n_bytes = z.n_bytes; a.n_tx_rows = z.n_tx_rows; a.n_hist = nh; a.n_block_rows = z.n_block_rows; a.n_wd = nw;
    if (t->block) memcpy(a.number, t->block + 4 * 2, 32);
    a.mis = (u32)((uintptr_t)a.calldata & 15u);
    a.hist_rot = z.hist_rot;
    a.n_gas_blocks = z.n_bytes ? (a.mis + z.n_bytes + BTB_GAS_BLOCK - 1) / BTB_GAS_BLOCK : 0;
    s->btb32[2].assign(a.n_gas_blocks + 1, 0);
    s->btb32[3].assign(a.n_gas_blocks + 1, 0);
    s->btb32[4].assign(z.n_tx_rows + 1, 0);
    s->btb32[5].assign(z.n_block_rows + 1, 0);
    a.gas_part = s->btb32[2].data(); a.gas_pre = s->btb32[3].data();
    a.tx = s->btb64[7].data(); a.tx_flags = s->btb32[4].data(); a.blk = s->btb64[8].data(); a.blk_flags = s->btb32[5].data(); a.wdt = s->btb64[9].data();
    s->pass = tables_from_block_pass;
    s->assign_kind = 11;
    *out = s;
    return 0;
}
extern "C" int zk_evm_tables_from_block_read(zk_session* s, const zk_block_tables* host) {
    ARG_TRY(s && s->assign_kind == 11, "zk_evm_tables_from_block_read: bad arguments");
    const BtbArgs& a = s->btb;
    if (host) {
        if (host->tx) memcpy(host->tx, a.tx, a.n_tx_rows * BTB_TX_NCELLS * 32);
        if (host->tx_flags) memcpy(host->tx_flags, a.tx_flags, a.n_tx_rows * 4);
        if (host->block) memcpy(host->block, a.blk, a.n_block_rows * BTB_BLOCK_NCELLS * 32);
        if (host->block_flags) memcpy(host->block_flags, a.blk_flags, a.n_block_rows * 4);
        if (host->withdrawals) memcpy(host->withdrawals, a.wdt, a.n_wd * BTB_WD_NCELLS * 32);
    }
    return 0;
}
extern "C" int zk_evm_tables_from_block(const zk_block_data* t, const zk_block_tables* out_wire, uint32_t opts, zk_result* result) {
    ARG_TRY(result && out_wire && t, "zk_evm_tables_from_block: null argument");
    zk_session* s = nullptr;
    int rc = zk_evm_tables_from_block_open(t, nullptr, opts, &s);
    if (rc) return rc;
    rc = zk_launch(s, nullptr);
    if (!rc) rc = zk_collect(s, result);
    if (!rc) rc = zk_evm_tables_from_block_read(s, out_wire);
    zk_close(s);
    return rc;
}

// ---- EVM circuit witness from compact trace records (trace_witness.hpp): the device functions in host loops.  The session keeps its
//      own heads, counters and pool offsets; id / addr / val / prev / pool / steps stay the caller's arrays and every pass reads them.
static void witness_from_trace_pass(zk_session* s) {
    TrwArgs& a = s->trw;
    for (u64 row = 0; row < a.n_rw; row++) {
        const u32 h = a.head[row];
        const u64 off = a.off[row];
        for (u32 q = 0; q < TRW_RW_PIECES; q++) trw_rw_piece(a, row, h, off, q, a.rw[(row * TRW_RW_PIECES + q) * 2], a.rw[(row * TRW_RW_PIECES + q) * 2 + 1]);
        a.rw_flags[row] = trw_rw_flag(h);
    }
    for (u64 row = 0; row < a.n_steps; row++)
        for (u32 q = 0; q < TRW_STEP_PIECES; q++) trw_step_piece(a, row, q, a.steps[(row * TRW_STEP_PIECES + q) * 2], a.steps[(row * TRW_STEP_PIECES + q) * 2 + 1]);
}
#define TRW_ARGS_OK(t) ((t) && ((t)->n_rw == 0 || ((t)->head && (t)->id && (t)->addr && (t)->val && (t)->prev)) && ((t)->n_pool == 0 || (t)->pool) && \
                        ((t)->n_steps == 0 || (t)->steps))
// the open's checks; head / ctr / off (nullable) receive the session's copies
static int trw_prepare(const zk_trace* t, u32* head, u64* ctr, u64* off) {
    char msg[256];
    int rc = trw_plan_counts(t->n_rw, t->n_steps, t->rw_base, t->rw_counter != nullptr, msg, sizeof msg);  // (before any array is read)
    if (rc) { g_err = msg; return rc; }
    u64 v[TRW_V_WORDS];
    trw_check_host(t->head, t->rw_counter, t->n_rw, t->steps, t->n_steps, head, ctr, off, v);
    rc = trw_verdict_error(v, t->n_pool, msg, sizeof msg);
    if (rc) g_err = msg;
    return rc;
}
extern "C" int zk_evm_witness_from_trace_sizes(const zk_trace* t, uint32_t opts, uint64_t* n_rw_rows, uint64_t* n_step_rows) {
    NO_DEVICE_PTRS(opts, "zk_evm_witness_from_trace_sizes");
    ARG_TRY(TRW_ARGS_OK(t), "zk_evm_witness_from_trace_sizes: bad arguments");
    const int rc = trw_prepare(t, nullptr, nullptr, nullptr);
    if (rc) return rc;
    if (n_rw_rows) *n_rw_rows = t->n_rw;
    if (n_step_rows) *n_step_rows = t->n_steps;
    return 0;
}
extern "C" int zk_evm_witness_from_trace_open(const zk_trace* t, const zk_trace_witness* out_dev, uint32_t opts, zk_session** out) {
    NO_DEVICE_PTRS(opts, "zk_evm_witness_from_trace_open");
    ARG_TRY(TRW_ARGS_OK(t) && out, "zk_evm_witness_from_trace_open: bad arguments");
    ARG_TRY(!out_dev, "zk_evm_witness_from_trace_open: out_dev needs ZK_OPT_DEVICE_PTRS");
    char msg[256];
    if (int rc = trw_plan_counts(t->n_rw, t->n_steps, t->rw_base, t->rw_counter != nullptr, msg, sizeof msg)) { g_err = msg; return rc; }  // (before anything is allocated)
    std::vector<u32> head(t->n_rw + 1, 0);
    std::vector<u64> ctr(t->rw_counter ? t->n_rw + 1 : 0, 0), off(t->n_rw + 1, 0);
    const int rc = trw_prepare(t, head.data(), t->rw_counter ? ctr.data() : nullptr, off.data());
    if (rc) return rc;
    zk_session* s = new_session(t->n_rw, false);
    TrwArgs& a = s->trw;
    memset(&a, 0, sizeof(a));
    s->trw32[0].swap(head);
    s->trw64[0].swap(ctr);
    s->trw64[1].swap(off);
    s->trw64[2].assign(t->n_rw * TRW_RW_NCELLS * 4 + 4, 0);
    s->trw64[3].assign(t->n_steps * TRW_STEP_NCELLS * 4 + 4, 0);
    s->trw32[1].assign(t->n_rw + 1, 0);
    a.id = t->id; a.addr = t->addr; a.val = t->val; a.prev = t->prev; a.pool = t->pool; a.steps_in = t->steps;
    a.n_rw = t->n_rw; a.n_pool = t->n_pool; a.n_steps = t->n_steps; a.rw_base = t->rw_base;
    a.head = s->trw32[0].data(); a.ctr = t->rw_counter ? s->trw64[0].data() : nullptr; a.off = s->trw64[1].data();
    a.rw = s->trw64[2].data(); a.rw_flags = s->trw32[1].data(); a.steps = s->trw64[3].data();
    s->pass = witness_from_trace_pass;
    s->assign_kind = 12;
    *out = s;
    return 0;
}
extern "C" int zk_evm_witness_from_trace_read(zk_session* s, const zk_trace_witness* host) {
    ARG_TRY(s && s->assign_kind == 12, "zk_evm_witness_from_trace_read: bad arguments");
    const TrwArgs& a = s->trw;
    if (host) {
        if (host->rw) memcpy(host->rw, a.rw, a.n_rw * TRW_RW_NCELLS * 32);
        if (host->rw_flags) memcpy(host->rw_flags, a.rw_flags, a.n_rw * 4);
        if (host->steps) memcpy(host->steps, a.steps, a.n_steps * TRW_STEP_NCELLS * 32);
    }
    return 0;
}
extern "C" int zk_evm_witness_from_trace(const zk_trace* t, const zk_trace_witness* out_wire, uint32_t opts, zk_result* result) {
    ARG_TRY(result && out_wire && t, "zk_evm_witness_from_trace: null argument");
    zk_session* s = nullptr;
    int rc = zk_evm_witness_from_trace_open(t, nullptr, opts, &s);
    if (rc) return rc;
    rc = zk_launch(s, nullptr);
    if (!rc) rc = zk_collect(s, result);
    if (!rc) rc = zk_evm_witness_from_trace_read(s, out_wire);
    zk_close(s);
    return rc;
}

// ---- State circuit from compact trace records (state_trace.hpp).  The device reads the records where its from-RW kernels read wire rows;
//      here the record's cells (strc_cell, one at a time: the definition) are laid out as the rows the host passes of the _from_rw entries
//      take, which copy what they keep at open.  Errors carry those entries' texts under this entry's name.
#include "state_trace.hpp"
static void strc_retitle(const char* name) {
    const std::string cur = g_err;
    const size_t c = cur.find(':');
    g_err = std::string(name) + (c == std::string::npos ? ": " + cur : cur.substr(c));
}
#define STRC_ARGS_OK(t) ((t) && (t)->n_rw > 0 && (t)->head && (t)->id && (t)->addr && (t)->val && ((t)->n_pool == 0 || (t)->pool))
static int strc_rows(const zk_trace* t, const char* name, std::vector<u64>& rw, std::vector<u32>& fl) {
    char msg[256];
    int rc = trw_plan_counts(t->n_rw, 0, t->rw_base, t->rw_counter != nullptr, msg, sizeof msg);  // (before any array is read)
    if (!rc) {
        std::vector<u32> head(t->n_rw);
        std::vector<u64> off(t->n_rw);
        u64 v[TRW_V_WORDS];
        trw_check_host(t->head, t->rw_counter, t->n_rw, nullptr, 0, head.data(), nullptr, off.data(), v);
        rc = trw_verdict_error(v, t->n_pool, msg, sizeof msg);
        if (!rc) {
            StrcArgs c;
            memset(&c, 0, sizeof(c));
            c.head = head.data(); c.ctr = t->rw_counter; c.id = t->id; c.addr = t->addr; c.val = t->val; c.off = off.data(); c.pool = t->pool;
            c.n = t->n_rw; c.rw_base = t->rw_base;
            rw.assign(t->n_rw * RWK_RW_NCELLS * 4, 0);
            fl.assign(t->n_rw, 0);
            for (u64 row = 0; row < t->n_rw; row++) {
                for (u32 k = 0; k < RWK_RW_NCELLS; k++) {
                    if (k == 10 || k == 11) continue;  // value_prev: not read by the State circuit
                    const Fr x = strc_cell(c, row, head[row], off[row], k);
                    for (int w = 0; w < 4; w++) rw[(row * RWK_RW_NCELLS + k) * 4 + w] = (u64)x.v[2 * w] | ((u64)x.v[2 * w + 1] << 32);
                }
                fl[row] = trw_rw_flag(head[row]);
            }
            return 0;
        }
    }
    g_err = msg;
    strc_retitle(name);
    return rc;
}
extern "C" int zk_state_ops_from_trace_open(const zk_trace* t, uint64_t* ops_dev, uint32_t* op_flags_dev, uint32_t opts, uint64_t* n_ops_out,
                                            zk_session** out) {
    NO_DEVICE_PTRS(opts, "zk_state_ops_from_trace_open");
    ARG_TRY(out && STRC_ARGS_OK(t) && !ops_dev && !op_flags_dev, "zk_state_ops_from_trace_open: bad arguments");
    std::vector<u64> rw;
    std::vector<u32> fl;
    int rc = strc_rows(t, "zk_state_ops_from_trace", rw, fl);
    if (rc) return rc;
    rc = zk_state_ops_from_rw_open(rw.data(), fl.data(), t->n_rw, nullptr, nullptr, opts, n_ops_out, out);
    if (rc) strc_retitle("zk_state_ops_from_trace_open");
    return rc;
}
extern "C" int zk_state_ops_from_trace_read(zk_session* s, uint64_t* ops_host, uint32_t* op_flags_host, uint64_t* n_ops_out) {
    ARG_TRY(s && s->assign_kind == 4, "zk_state_ops_from_trace_read: bad arguments");
    return zk_state_ops_from_rw_read(s, ops_host, op_flags_host, n_ops_out);
}
extern "C" int zk_state_ops_from_trace(const zk_trace* t, uint64_t* ops_out, uint32_t* op_flags_out, uint64_t* n_ops_out, uint32_t opts,
                                       uint32_t* status_out, zk_result* result) {
    ARG_TRY(result && n_ops_out, "zk_state_ops_from_trace: null output");
    zk_session* s = nullptr;
    int rc = zk_state_ops_from_trace_open(t, nullptr, nullptr, opts, n_ops_out, &s);
    if (rc) return rc;
    rc = zk_launch(s, nullptr);
    if (!rc) rc = zk_collect(s, result);
    if (!rc) rc = zk_state_ops_from_trace_read(s, ops_out, op_flags_out, n_ops_out);
    if (!rc && status_out) rc = zk_read_status(s, status_out);
    zk_close(s);
    return rc;
}
extern "C" int zk_state_verify_from_trace_open(const zk_trace* t, uint32_t opts, uint64_t* n_ops_out, zk_session** out) {
    NO_DEVICE_PTRS(opts, "zk_state_verify_from_trace_open");
    ARG_TRY(out && STRC_ARGS_OK(t), "zk_state_verify_from_trace_open: bad arguments");
    std::vector<u64> rw;
    std::vector<u32> fl;
    int rc = strc_rows(t, "zk_state_verify_from_trace", rw, fl);
    if (rc) return rc;
    rc = zk_state_verify_from_rw_open(rw.data(), fl.data(), t->n_rw, opts, n_ops_out, out);
    if (rc) strc_retitle("zk_state_verify_from_trace");
    return rc;
}
extern "C" int zk_state_verify_from_trace(const zk_trace* t, uint32_t opts, uint32_t* status_out, uint64_t* n_ops_out, zk_result* result) {
    ARG_TRY(result, "zk_state_verify_from_trace: result is null");
    zk_session* s = nullptr;
    int rc = zk_state_verify_from_trace_open(t, opts, n_ops_out, &s);
    if (rc) return rc;
    rc = zk_launch(s, nullptr);
    if (!rc) rc = zk_collect(s, result);
    if (!rc && status_out) rc = zk_read_status(s, status_out);
    zk_close(s);
    return rc;
}
// Records -> State witness: the record's cells laid out as wire rows, then the from-RW twin's host passes (which copy what they keep).
extern "C" int zk_state_assign_from_trace_open(const zk_trace* t, uint64_t* rows_dev, uint32_t* row_flags_dev, uint64_t* mpt_dev,
                                               uint32_t opts, uint64_t* n_ops_out, zk_session** out) {
    NO_DEVICE_PTRS(opts, "zk_state_assign_from_trace_open");
    ARG_TRY(out && STRC_ARGS_OK(t) && !rows_dev && !row_flags_dev && !mpt_dev, "zk_state_assign_from_trace_open: bad arguments");
    std::vector<u64> rw;
    std::vector<u32> fl;
    int rc = strc_rows(t, "zk_state_assign_from_trace", rw, fl);
    if (rc) return rc;
    rc = zk_state_assign_from_rw_open(rw.data(), fl.data(), t->n_rw, nullptr, nullptr, nullptr, opts, n_ops_out, out);
    if (rc) strc_retitle("zk_state_assign_from_trace_open");
    return rc;
}
extern "C" int zk_state_assign_from_trace(const zk_trace* t, uint64_t* rows_out, uint32_t* row_flags_out, uint64_t* mpt_out,
                                          uint64_t* n_mpt_out, uint64_t* n_ops_out, uint32_t opts, uint32_t* status_out, zk_result* result) {
    ARG_TRY(result && n_mpt_out && n_ops_out, "zk_state_assign_from_trace: null output");
    zk_session* s = nullptr;
    int rc = zk_state_assign_from_trace_open(t, nullptr, nullptr, nullptr, opts, n_ops_out, &s);
    if (rc) return rc;
    rc = zk_launch(s, nullptr);
    if (!rc) rc = zk_collect(s, result);
    if (!rc) rc = zk_state_assign_read(s, rows_out, row_flags_out, mpt_out, *n_ops_out, n_mpt_out);
    if (!rc && status_out) rc = zk_read_status(s, status_out);
    zk_close(s);
    return rc;
}

static void copy_assign_pass(zk_session* s) {
    CpaArgs& a = s->cpa;
    for (u64 c = 0; c < a.n_chunks; c++) cpa_chunk(a, c);
    for (u64 e = 0; e < a.n_events; e++) cpa_prefix_event(a, e);
    for (u64 j = 0; j < a.n_rows; j++) cpa_write_row(a, j);
}
extern "C" int zk_copy_assign_sizes(const zk_copy_events* t, uint32_t opts, uint64_t* n_rows, uint64_t* n_table, uint64_t* n_rw) {
    NO_DEVICE_PTRS(opts, "zk_copy_assign_sizes");
    ARG_TRY(t && t->n_events > 0 && t->events && t->data_offsets, "zk_copy_assign_sizes: bad arguments");
    CpaPlan pl;
    const int rc = cpa_plan(t->events, t->flags, t->data_offsets, t->n_events, pl);
    if (rc) return rc;
    if (n_rows) *n_rows = pl.n_rows;
    if (n_table) *n_table = pl.n_table;
    if (n_rw) *n_rw = pl.n_rw;
    return 0;
}
// the session's buffers and the Copy assignment's arguments over a plan the session owns and its source data (s->a16)
static void cpa_session_setup(zk_session* s, CpaPlan& pl, const u64* events, u64 n_events, const u64* randomness) {
    s->a64[0].assign(events, events + n_events * CPA_EV_NCELLS * 4);
    s->a64[1].assign(CPA_RPOW_ROWS * 4, 0);
    cpa_fill_rpow(cell_of(randomness), s->a64[1].data());
    s->w64[0].assign(pl.chunks.size() * 4 + 4, 0);  // chunk_acc
    s->w64[1].assign(pl.chunks.size() * 4 + 4, 0);  // chunk_in
    s->w64[2].assign(n_events * 4 + 4, 0);          // ev_rlc
    s->w64[3].assign(pl.n_rlc * 4 + 4, 0);          // rlc
    s->a64[2].assign(pl.n_rows * CPA_ROW_NCELLS * 4 + 4, 0);   // rows
    s->a64[3].assign(pl.n_table * CPA_TABLE_NCELLS * 4 + 4, 0);  // table
    s->keccak_rows.assign(pl.n_rw * CPA_RW_NCELLS * 4 + 4, 0);  // rw rows
    s->out32.assign(pl.n_rows + 1, 0);              // row flags
    s->a32[0].assign(pl.n_rw + 1, 0);               // rw flags
    CpaArgs& a = s->cpa;
    a.events = s->a64[0].data(); a.ev = pl.ev.data(); a.row0 = pl.row0.data(); a.n_events = n_events; a.n_rows = pl.n_rows; a.data = s->a16.data();
    a.rpow = s->a64[1].data(); a.chunks = pl.chunks.data(); a.n_chunks = pl.chunks.size(); a.chunk_acc = s->w64[0].data(); a.chunk_in = s->w64[1].data();
    a.ev_rlc = s->w64[2].data(); a.rlc = s->w64[3].data(); a.rows = s->a64[2].data(); a.row_flags = s->out32.data(); a.table = s->a64[3].data();
    a.rw = s->keccak_rows.data(); a.rw_flags = s->a32[0].data();
}
static void cpa_read_copy(const zk_session* s, const CpaPlan& pl, uint64_t* rows_host, uint32_t* row_flags_host, uint64_t* table_host, uint64_t* rw_host,
                          uint32_t* rw_flags_host) {
    if (rows_host) memcpy(rows_host, s->a64[2].data(), (size_t)pl.n_rows * CPA_ROW_NCELLS * 32);
    if (row_flags_host) memcpy(row_flags_host, s->out32.data(), (size_t)pl.n_rows * 4);
    if (table_host && pl.n_table) memcpy(table_host, s->a64[3].data(), (size_t)pl.n_table * CPA_TABLE_NCELLS * 32);
    if (rw_host && pl.n_rw) memcpy(rw_host, s->keccak_rows.data(), (size_t)pl.n_rw * CPA_RW_NCELLS * 32);
    if (rw_flags_host && pl.n_rw) memcpy(rw_flags_host, s->a32[0].data(), (size_t)pl.n_rw * 4);
}
extern "C" int zk_copy_assign_open(const zk_copy_events* t, uint64_t* rows_dev, uint32_t* row_flags_dev, uint64_t* table_dev, uint64_t* rw_dev,
                                   uint32_t* rw_flags_dev, uint32_t opts, zk_session** out) {
    NO_DEVICE_PTRS(opts, "zk_copy_assign_open");
    ARG_TRY(t && out && t->n_events > 0 && t->n_events < (1ull << 31) && t->events && t->data_offsets && t->randomness, "zk_copy_assign_open: bad arguments");
    ARG_TRY(!rows_dev && !row_flags_dev && !table_dev && !rw_dev && !rw_flags_dev, "zk_copy_assign_open: output buffers need ZK_OPT_DEVICE_PTRS");
    zk_session* s = new_session(1, false);
    CpaPlan& pl = s->cpa_plan;
    const int rc = cpa_plan(t->events, t->flags, t->data_offsets, t->n_events, pl);
    if (rc) { delete s; return rc; }
    s->n = s->hi = pl.n_rows;
    s->status.assign(pl.n_rows ? pl.n_rows : 1, 0u);
    s->a16.assign(t->data, t->data + pl.n_data);
    cpa_session_setup(s, pl, t->events, t->n_events, t->randomness);
    s->pass = copy_assign_pass;
    s->assign_kind = 3;
    *out = s;
    return 0;
}
extern "C" int zk_copy_assign_read(zk_session* s, uint64_t* rows_host, uint32_t* row_flags_host, uint64_t* table_host, uint64_t* rw_host,
                                   uint32_t* rw_flags_host) {
    ARG_TRY(s && s->assign_kind == 3, "zk_copy_assign_read: bad arguments");
    cpa_read_copy(s, s->cpa_plan, rows_host, row_flags_host, table_host, rw_host, rw_flags_host);
    return 0;
}
extern "C" int zk_copy_assign(const zk_copy_events* t, uint64_t* rows_out, uint32_t* row_flags_out, uint64_t* table_out, uint64_t* rw_out,
                              uint32_t* rw_flags_out, uint32_t opts, zk_result* result) {
    ARG_TRY(result && rows_out && row_flags_out, "zk_copy_assign: null output");
    zk_session* s = nullptr;
    int rc = zk_copy_assign_open(t, nullptr, nullptr, nullptr, nullptr, nullptr, opts, &s);
    if (rc) return rc;
    rc = zk_launch(s, nullptr);
    if (!rc) rc = zk_collect(s, result);
    if (!rc) rc = zk_copy_assign_read(s, rows_out, row_flags_out, table_out, rw_out, rw_flags_out);
    zk_close(s);
    return rc;
}

// ---- Copy-circuit witness assignment from raw sources (copy_sources.hpp): the gather's per-byte function in host loops, the is_code bits by
//      the reference's recurrence, then the pass above.  The session keeps its plan (the events' integers, the refs' resolution, the offsets)
//      and its own heads and counters; code, calldata, id / addr / val stay the caller's arrays and every pass reads them.
static void copy_sources_pass(zk_session* s) {
    CpsArgs& g = s->cps;
    const CpsPlan& pl = s->cps_plan;
    if (pl.any_code) cps_code_mask_host(g.code, s->cps64[2].data(), pl.chunk0.data(), pl.chunk0.size() - 1, s->cps64[0].data());
    for (u64 e = 0; e < g.n_events; e++) {
        cps_gather_event(g, e);
        s->status[e] = cps_status(g.sev[e], g.ev_fail[e]);
    }
    copy_assign_pass(s);
}
#define CPS_ARGS_OK(t) ((t) && (t)->n_events > 0 && (t)->n_events < (1ull << 31) && (t)->events && (t)->src_ref &&                                  \
                        ((t)->n_codes == 0 || (t)->code_offsets) && ((t)->n_code_bytes == 0 || (t)->code) && ((t)->n_txs == 0 || (t)->calldata_offsets) && \
                        ((t)->trace.n_rw == 0 || ((t)->trace.head && (t)->trace.id && (t)->trace.addr && (t)->trace.val)))
// the domain checks and the plan; head / ctr (nullable) receive the session's copies of the trace's heads and counters
static int cps_prepare(const zk_copy_sources* t, CpsPlan& pl, u32* head, u64* ctr) {
    const char* const name = "zk_copy_assign_from_sources";
    const zk_trace& tr = t->trace;
    char msg[256];
    int rc = trw_plan_counts(tr.n_rw, 0, tr.rw_base, tr.rw_counter != nullptr, msg, sizeof msg);  // (before any array is read)
    if (rc) { g_err = msg; cps_retitle(name); return rc; }
    if ((rc = cps_plan(t->events, t->flags, t->src_ref, t->dst_ref, t->n_events, t->code_offsets, t->n_codes, t->n_code_bytes, t->calldata_offsets,
                       t->n_txs, pl)))
        return rc;
    ARG_TRY(!t->n_txs || t->calldata_offsets[t->n_txs] == 0 || t->calldata, "zk_copy_assign_from_sources: calldata is null");
    u64 v[TRW_V_WORDS];
    trw_check_host(tr.head, tr.rw_counter, tr.n_rw, nullptr, 0, head, ctr, nullptr, v);
    if ((rc = trw_verdict_error(v, v[TRW_V_POOL], msg, sizeof msg))) { g_err = msg; cps_retitle(name); }  // (the pool is not read: its count is not checked)
    return rc;
}
extern "C" int zk_copy_assign_from_sources_sizes(const zk_copy_sources* t, uint32_t opts, uint64_t* n_rows, uint64_t* n_table, uint64_t* n_rw,
                                                 uint64_t* n_data) {
    NO_DEVICE_PTRS(opts, "zk_copy_assign_from_sources_sizes");
    ARG_TRY(CPS_ARGS_OK(t), "zk_copy_assign_from_sources_sizes: bad arguments");
    CpsPlan pl;
    const int rc = cps_prepare(t, pl, nullptr, nullptr);
    if (rc) return rc;
    if (n_rows) *n_rows = pl.cpa.n_rows;
    if (n_table) *n_table = pl.cpa.n_table;
    if (n_rw) *n_rw = pl.cpa.n_rw;
    if (n_data) *n_data = pl.data0[t->n_events];
    return 0;
}
extern "C" int zk_copy_assign_from_sources_open(const zk_copy_sources* t, uint64_t* rows_dev, uint32_t* row_flags_dev, uint64_t* table_dev,
                                                uint64_t* rw_dev, uint32_t* rw_flags_dev, uint16_t* data_dev, uint32_t opts, zk_session** out) {
    NO_DEVICE_PTRS(opts, "zk_copy_assign_from_sources_open");
    ARG_TRY(CPS_ARGS_OK(t) && out && t->randomness, "zk_copy_assign_from_sources_open: bad arguments");
    ARG_TRY(!rows_dev && !row_flags_dev && !table_dev && !rw_dev && !rw_flags_dev && !data_dev, "zk_copy_assign_from_sources_open: output buffers need ZK_OPT_DEVICE_PTRS");
    const zk_trace& tr = t->trace;
    zk_session* s = new_session(t->n_events, false);
    CpsPlan& pl = s->cps_plan;
    s->cps32[0].assign(tr.n_rw + 1, 0);                         // heads
    s->cps64[1].assign(tr.rw_counter ? tr.n_rw + 1 : 0, 0);     // counters
    const int rc = cps_prepare(t, pl, s->cps32[0].data(), tr.rw_counter ? s->cps64[1].data() : nullptr);
    if (rc) { delete s; return rc; }
    const u64 n_data = pl.data0[t->n_events];
    s->status.assign(t->n_events, 0u);
    s->a16.assign(n_data + 1, 0);
    cpa_session_setup(s, pl.cpa, t->events, t->n_events, t->randomness);
    s->cps64[0].assign(pl.n_chunks + 1, 0);                     // is_code mask
    s->cps64[2].assign(t->code_offsets, t->code_offsets + (t->n_codes ? t->n_codes + 1 : 0));  // the session's copy of the code offsets
    s->cps64[3].assign(t->n_events, CPS_NO_FAIL);               // per-event failing byte
    CpsArgs& g = s->cps;
    memset(&g, 0, sizeof(g));
    g.events = s->cpa.events; g.ev = pl.cpa.ev.data(); g.sev = pl.sev.data(); g.data0 = pl.data0.data(); g.n_events = t->n_events; g.n_data = n_data;
    g.code = t->code; g.code_mask = s->cps64[0].data(); g.calldata = t->calldata;
    g.head = s->cps32[0].data(); g.ctr = tr.rw_counter ? s->cps64[1].data() : nullptr; g.id = tr.id; g.addr = tr.addr; g.val = tr.val;
    g.n_rw = tr.n_rw; g.rw_base = tr.rw_base;
    g.data = s->a16.data();
    g.ev_fail = (unsigned long long*)s->cps64[3].data();
    s->pass = copy_sources_pass;
    s->assign_kind = 14;
    *out = s;
    return 0;
}
extern "C" int zk_copy_assign_from_sources_read(zk_session* s, uint64_t* rows_host, uint32_t* row_flags_host, uint64_t* table_host,
                                                uint64_t* rw_host, uint32_t* rw_flags_host, uint16_t* data_host, uint64_t* data_offsets_host) {
    ARG_TRY(s && s->assign_kind == 14, "zk_copy_assign_from_sources_read: bad arguments");
    const CpsPlan& pl = s->cps_plan;
    cpa_read_copy(s, pl.cpa, rows_host, row_flags_host, table_host, rw_host, rw_flags_host);
    if (data_host && s->cps.n_data) memcpy(data_host, s->cps.data, (size_t)s->cps.n_data * 2);
    if (data_offsets_host) memcpy(data_offsets_host, pl.data0.data(), pl.data0.size() * 8);
    return 0;
}
extern "C" int zk_copy_assign_from_sources(const zk_copy_sources* t, uint64_t* rows_out, uint32_t* row_flags_out, uint64_t* table_out,
                                           uint64_t* rw_out, uint32_t* rw_flags_out, uint16_t* data_out, uint64_t* data_offsets_out,
                                           uint32_t opts, uint32_t* status_out, zk_result* result) {
    ARG_TRY(result && rows_out && row_flags_out, "zk_copy_assign_from_sources: null output");
    zk_session* s = nullptr;
    int rc = zk_copy_assign_from_sources_open(t, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, opts, &s);
    if (rc) return rc;
    rc = zk_launch(s, nullptr);
    if (!rc) rc = zk_collect(s, result);
    if (!rc && status_out) rc = zk_read_status(s, status_out);
    if (!rc) rc = zk_copy_assign_from_sources_read(s, rows_out, row_flags_out, table_out, rw_out, rw_flags_out, data_out, data_offsets_out);
    zk_close(s);
    return rc;
}

// ---- Copy and EXP events from compact trace records (trace_events.hpp): the per-step function in a host loop.  The session keeps its own
//      heads, counters, pool offsets, code offsets and hash directory; id / addr / val / pool / steps / code stay the caller's arrays and
//      every pass reads them.
static void events_from_trace_pass(zk_session* s) { tev_pass_host(s->tev, s->status.data()); }
#define TEV_ARGS_OK(t) ((t) && ((t)->trace.n_rw == 0 || ((t)->trace.head && (t)->trace.id && (t)->trace.addr && (t)->trace.val)) &&                        \
                        ((t)->trace.n_pool == 0 || (t)->trace.pool) && ((t)->trace.n_steps == 0 || (t)->trace.steps) &&                                      \
                        ((t)->n_codes == 0 || ((t)->code_offsets && (t)->code_hashes)) && ((t)->n_code_bytes == 0 || (t)->code))
// the domain checks; head / ctr / off (nullable) receive the session's copies
static int tev_prepare(const zk_trace_sources* t, u32* head, u64* ctr, u64* off) {
    const char* const name = "zk_events_from_trace";
    const zk_trace& tr = t->trace;
    char msg[256];
    int rc = tev_counts_check(tr.n_steps, t->n_code_bytes, t->n_codes);  // (before any array is read)
    if (rc) return rc;
    if ((rc = trw_plan_counts(tr.n_rw, tr.n_steps, tr.rw_base, tr.rw_counter != nullptr, msg, sizeof msg))) { g_err = msg; cps_retitle(name); return rc; }
    if ((rc = tev_offsets_check(t->code_offsets, t->n_codes, t->n_code_bytes))) return rc;
    u64 v[TRW_V_WORDS];
    trw_check_host(tr.head, tr.rw_counter, tr.n_rw, tr.steps, tr.n_steps, head, ctr, off, v);
    if ((rc = trw_verdict_error(v, tr.n_pool, msg, sizeof msg))) { g_err = msg; cps_retitle(name); }
    return rc;
}
extern "C" int zk_events_from_trace_sizes(const zk_trace_sources* t, uint32_t opts, uint64_t* capacity) {
    NO_DEVICE_PTRS(opts, "zk_events_from_trace_sizes");
    ARG_TRY(TEV_ARGS_OK(t), "zk_events_from_trace_sizes: bad arguments");
    const int rc = tev_prepare(t, nullptr, nullptr, nullptr);
    if (rc) return rc;
    if (capacity) *capacity = t->trace.n_steps;
    return 0;
}
extern "C" int zk_events_from_trace_open(const zk_trace_sources* t, const zk_trace_events* out_dev, uint32_t opts, zk_session** out) {
    NO_DEVICE_PTRS(opts, "zk_events_from_trace_open");
    ARG_TRY(TEV_ARGS_OK(t) && out, "zk_events_from_trace_open: bad arguments");
    ARG_TRY(!out_dev, "zk_events_from_trace_open: out_dev needs ZK_OPT_DEVICE_PTRS");
    const zk_trace& tr = t->trace;
    int rc = tev_counts_check(tr.n_steps, t->n_code_bytes, t->n_codes);  // (before anything is allocated)
    if (rc) return rc;
    char msg[256];
    if ((rc = trw_plan_counts(tr.n_rw, tr.n_steps, tr.rw_base, tr.rw_counter != nullptr, msg, sizeof msg))) { g_err = msg; cps_retitle("zk_events_from_trace"); return rc; }
    const u64 n = tr.n_rw, ns = tr.n_steps, nc = t->n_codes;
    zk_session* s = new_session(ns, false);
    s->tev32[0].assign(n + 1, 0);                        // heads
    s->tev64[0].assign(tr.rw_counter ? n + 1 : 0, 0);    // counters
    s->tev64[1].assign(n + 1, 0);                        // pool offsets
    if ((rc = tev_prepare(t, s->tev32[0].data(), tr.rw_counter ? s->tev64[0].data() : nullptr, s->tev64[1].data()))) { delete s; return rc; }
    s->tev64[2].assign(t->code_offsets, t->code_offsets + (nc ? nc + 1 : 0));  // the session's copy of the code offsets
    s->tev64[2].push_back(0);
    tev_dir_build(t->code_hashes, nc, s->tev_plan);
    s->tev64[3].assign(ns * TEV_COPY_NCELLS * 4 + 4, 0);  // copy events
    s->tev64[4].assign(ns * TEV_EXP_NCELLS * 4 + 4, 0);   // EXP events
    s->tev64[5].assign(2, 0);                             // counts
    for (int k = 1; k < 5; k++) s->tev32[k].assign(ns + 1, 0);  // copy flags, refs, steps; EXP steps
    TevArgs& a = s->tev;
    memset(&a, 0, sizeof(a));
    a.head = s->tev32[0].data(); a.ctr = tr.rw_counter ? s->tev64[0].data() : nullptr; a.off = s->tev64[1].data();
    a.id = tr.id; a.addr = tr.addr; a.val = tr.val; a.pool = tr.pool; a.steps = tr.steps;
    a.n_rw = n; a.n_pool = tr.n_pool; a.n_steps = ns; a.rw_base = tr.rw_base;
    a.code = t->code; a.code_off = s->tev64[2].data(); a.dir_hash = s->tev_plan.dir_hash.data(); a.dir_idx = s->tev_plan.dir_idx.data(); a.n_codes = (u32)nc;
    a.counts = s->tev64[5].data();
    a.copy_events = s->tev64[3].data(); a.copy_flags = s->tev32[1].data(); a.copy_src_ref = s->tev32[2].data(); a.copy_step = s->tev32[3].data();
    a.exp_events = s->tev64[4].data(); a.exp_step = s->tev32[4].data();
    s->pass = events_from_trace_pass;
    s->assign_kind = 15;
    *out = s;
    return 0;
}
extern "C" int zk_events_from_trace_read(zk_session* s, const zk_trace_events* host, uint64_t* n_copy, uint64_t* n_exp) {
    ARG_TRY(s && s->assign_kind == 15, "zk_events_from_trace_read: bad arguments");
    const TevArgs& a = s->tev;
    const u64 nc = a.counts[0], ne = a.counts[1];
    if (host) {
        if (host->copy_events && nc) memcpy(host->copy_events, a.copy_events, nc * TEV_COPY_NCELLS * 32);
        if (host->copy_flags && nc) memcpy(host->copy_flags, a.copy_flags, nc * 4);
        if (host->copy_src_ref && nc) memcpy(host->copy_src_ref, a.copy_src_ref, nc * 4);
        if (host->copy_step && nc) memcpy(host->copy_step, a.copy_step, nc * 4);
        if (host->exp_events && ne) memcpy(host->exp_events, a.exp_events, ne * TEV_EXP_NCELLS * 32);
        if (host->exp_step && ne) memcpy(host->exp_step, a.exp_step, ne * 4);
    }
    if (n_copy) *n_copy = nc;
    if (n_exp) *n_exp = ne;
    return 0;
}
extern "C" int zk_events_from_trace_counts(zk_session* s, uint64_t* n_copy, uint64_t* n_exp) {
    ARG_TRY(s && s->assign_kind == 15, "zk_events_from_trace_counts: bad arguments");
    return zk_events_from_trace_read(s, nullptr, n_copy, n_exp);
}
extern "C" int zk_events_from_trace(const zk_trace_sources* t, const zk_trace_events* out_wire, uint32_t opts, uint32_t* status_out,
                                    uint64_t* n_copy, uint64_t* n_exp, zk_result* result) {
    ARG_TRY(result && out_wire && t, "zk_events_from_trace: null argument");
    zk_session* s = nullptr;
    int rc = zk_events_from_trace_open(t, nullptr, opts, &s);
    if (rc) return rc;
    rc = zk_launch(s, nullptr);
    if (!rc) rc = zk_collect(s, result);
    if (!rc && status_out) rc = zk_read_status(s, status_out);
    if (!rc) rc = zk_events_from_trace_read(s, out_wire, n_copy, n_exp);
    zk_close(s);
    return rc;
}
// zk_events_from_trace_ext*: the same checks under that entry's name, the wider per-step function, the copy capacity of the two-event
// states (counted over the steps' word 0) and the dst refs
static void events_from_trace_ext_pass(zk_session* s) { tevx_pass_host(s->tevx, s->status.data()); }
static int tevx_prepare(const zk_trace_sources* t, u32* head, u64* ctr, u64* off, u64* cap_copy) {
    const int rc = tev_prepare(t, head, ctr, off);
    if (rc) { cps_retitle("zk_events_from_trace_ext"); return rc; }
    u64 pairs = 0;
    for (u64 s = 0; s < t->trace.n_steps; s++) pairs += tevx_is_pair_state(t->trace.steps[s * TRW_STEP_WORDS]);
    *cap_copy = t->trace.n_steps + pairs;
    return 0;
}
extern "C" int zk_events_from_trace_ext_sizes(const zk_trace_sources* t, uint32_t opts, uint64_t* copy_capacity, uint64_t* exp_capacity) {
    NO_DEVICE_PTRS(opts, "zk_events_from_trace_ext_sizes");
    ARG_TRY(TEV_ARGS_OK(t), "zk_events_from_trace_ext_sizes: bad arguments");
    u64 cap = 0;
    const int rc = tevx_prepare(t, nullptr, nullptr, nullptr, &cap);
    if (rc) return rc;
    if (copy_capacity) *copy_capacity = cap;
    if (exp_capacity) *exp_capacity = t->trace.n_steps;
    return 0;
}
extern "C" int zk_events_from_trace_ext_open(const zk_trace_sources* t, const zk_trace_events_ext* out_dev, uint32_t opts, zk_session** out) {
    NO_DEVICE_PTRS(opts, "zk_events_from_trace_ext_open");
    ARG_TRY(TEV_ARGS_OK(t) && out, "zk_events_from_trace_ext_open: bad arguments");
    ARG_TRY(!out_dev, "zk_events_from_trace_ext_open: out_dev needs ZK_OPT_DEVICE_PTRS");
    const zk_trace& tr = t->trace;
    int rc = tev_counts_check(tr.n_steps, t->n_code_bytes, t->n_codes);  // (before anything is allocated)
    char msg[256];
    if (!rc && (rc = trw_plan_counts(tr.n_rw, tr.n_steps, tr.rw_base, tr.rw_counter != nullptr, msg, sizeof msg))) g_err = msg;
    if (rc) { cps_retitle("zk_events_from_trace_ext"); return rc; }
    const u64 n = tr.n_rw, ns = tr.n_steps, nc = t->n_codes;
    zk_session* s = new_session(ns, false);
    s->tev32[0].assign(n + 1, 0);                        // heads
    s->tev64[0].assign(tr.rw_counter ? n + 1 : 0, 0);    // counters
    s->tev64[1].assign(n + 1, 0);                        // pool offsets
    u64 cap = 0;
    if ((rc = tevx_prepare(t, s->tev32[0].data(), tr.rw_counter ? s->tev64[0].data() : nullptr, s->tev64[1].data(), &cap))) { delete s; return rc; }
    s->tev64[2].assign(t->code_offsets, t->code_offsets + (nc ? nc + 1 : 0));  // the session's copy of the code offsets
    s->tev64[2].push_back(0);
    tev_dir_build(t->code_hashes, nc, s->tev_plan);
    s->tev64[3].assign(cap * TEV_COPY_NCELLS * 4 + 4, 0);  // copy events
    s->tev64[4].assign(ns * TEV_EXP_NCELLS * 4 + 4, 0);    // EXP events
    s->tev64[5].assign(2, 0);                              // counts
    for (int k = 1; k < 4; k++) s->tev32[k].assign(cap + 1, 0);  // copy flags, refs, steps
    s->tev32[4].assign(ns + 1, 0);                               // EXP steps
    s->tevx_dst.assign(cap + 1, 0);
    TevxArgs& ax = s->tevx;
    memset(&ax, 0, sizeof(ax));
    TevArgs& a = ax.t;
    a.head = s->tev32[0].data(); a.ctr = tr.rw_counter ? s->tev64[0].data() : nullptr; a.off = s->tev64[1].data();
    a.id = tr.id; a.addr = tr.addr; a.val = tr.val; a.pool = tr.pool; a.steps = tr.steps;
    a.n_rw = n; a.n_pool = tr.n_pool; a.n_steps = ns; a.rw_base = tr.rw_base;
    a.code = t->code; a.code_off = s->tev64[2].data(); a.dir_hash = s->tev_plan.dir_hash.data(); a.dir_idx = s->tev_plan.dir_idx.data(); a.n_codes = (u32)nc;
    a.counts = s->tev64[5].data();
    a.copy_events = s->tev64[3].data(); a.copy_flags = s->tev32[1].data(); a.copy_src_ref = s->tev32[2].data(); a.copy_step = s->tev32[3].data();
    a.exp_events = s->tev64[4].data(); a.exp_step = s->tev32[4].data();
    ax.copy_dst_ref = s->tevx_dst.data();
    ax.cap_copy = cap;
    s->pass = events_from_trace_ext_pass;
    s->assign_kind = 17;
    *out = s;
    return 0;
}
extern "C" int zk_events_from_trace_ext_read(zk_session* s, const zk_trace_events_ext* host, uint64_t* n_copy, uint64_t* n_exp) {
    ARG_TRY(s && s->assign_kind == 17, "zk_events_from_trace_ext_read: bad arguments");
    const TevArgs& a = s->tevx.t;
    const u64 nc = a.counts[0], ne = a.counts[1];
    if (host) {
        if (host->copy_events && nc) memcpy(host->copy_events, a.copy_events, nc * TEV_COPY_NCELLS * 32);
        if (host->copy_flags && nc) memcpy(host->copy_flags, a.copy_flags, nc * 4);
        if (host->copy_src_ref && nc) memcpy(host->copy_src_ref, a.copy_src_ref, nc * 4);
        if (host->copy_dst_ref && nc) memcpy(host->copy_dst_ref, s->tevx.copy_dst_ref, nc * 4);
        if (host->copy_step && nc) memcpy(host->copy_step, a.copy_step, nc * 4);
        if (host->exp_events && ne) memcpy(host->exp_events, a.exp_events, ne * TEV_EXP_NCELLS * 32);
        if (host->exp_step && ne) memcpy(host->exp_step, a.exp_step, ne * 4);
    }
    if (n_copy) *n_copy = nc;
    if (n_exp) *n_exp = ne;
    return 0;
}
extern "C" int zk_events_from_trace_ext_counts(zk_session* s, uint64_t* n_copy, uint64_t* n_exp) {
    ARG_TRY(s && s->assign_kind == 17, "zk_events_from_trace_ext_counts: bad arguments");
    return zk_events_from_trace_ext_read(s, nullptr, n_copy, n_exp);
}
extern "C" int zk_events_from_trace_ext(const zk_trace_sources* t, const zk_trace_events_ext* out_wire, uint32_t opts, uint32_t* status_out,
                                        uint64_t* n_copy, uint64_t* n_exp, zk_result* result) {
    ARG_TRY(result && out_wire && t, "zk_events_from_trace_ext: null argument");
    zk_session* s = nullptr;
    int rc = zk_events_from_trace_ext_open(t, nullptr, opts, &s);
    if (rc) return rc;
    rc = zk_launch(s, nullptr);
    if (!rc) rc = zk_collect(s, result);
    if (!rc && status_out) rc = zk_read_status(s, status_out);
    if (!rc) rc = zk_events_from_trace_ext_read(s, out_wire, n_copy, n_exp);
    zk_close(s);
    return rc;
}

// ---- SHA3 inputs and keccak rows from compact trace records (trace_sha3.hpp): the per-step and per-byte functions in host loops.  The
//      session keeps its own heads, counters, pool offsets, sizes, records and data offsets; id / addr / val / pool stay the caller's
//      arrays and every pass reads them.
static void sha3_from_trace_pass(zk_session* s) { ts3_pass_host(s->ts3, s->ts3_kgen, s->status.data()); }
#define TS3_ARGS_OK(t) ((t) && ((t)->n_rw == 0 || ((t)->head && (t)->id && (t)->addr && (t)->val)) && ((t)->n_pool == 0 || (t)->pool) &&                  \
                        ((t)->n_steps == 0 || (t)->steps))
// The open: the counts, the trace checks, every step's open-time status and size, the verdict.  check_only: no session is left.
static int ts3_open_host(const zk_trace* tr, const uint64_t* randomness, bool check_only, uint64_t* n_msgs, uint64_t* n_bytes, zk_session** out) {
    const char* const name = "zk_sha3_from_trace";
    char msg[256];
    int rc = ts3_counts_check(tr->n_rw, tr->n_steps, msg, sizeof msg);  // (before any array is read or anything allocated)
    if (rc) { g_err = msg; return rc; }
    if ((rc = trw_plan_counts(tr->n_rw, tr->n_steps, tr->rw_base, tr->rw_counter != nullptr, msg, sizeof msg))) { g_err = msg; cps_retitle(name); return rc; }
    const u64 n = tr->n_rw, ns = tr->n_steps;
    zk_session* s = new_session(ns, false);
    s->ts332[0].assign(n + 1, 0);                         // heads
    s->ts364[0].assign(tr->rw_counter ? n + 1 : 0, 0);    // counters
    s->ts364[1].assign(n + 1, 0);                         // pool offsets
    u64 v[TRW_V_WORDS];
    trw_check_host(tr->head, tr->rw_counter, n, tr->steps, ns, s->ts332[0].data(), tr->rw_counter ? s->ts364[0].data() : nullptr, s->ts364[1].data(), v);
    if ((rc = trw_verdict_error(v, tr->n_pool, msg, sizeof msg))) { g_err = msg; cps_retitle(name); delete s; return rc; }
    Ts3Args& a = s->ts3;
    memset(&a, 0, sizeof(a));
    TevArgs& t = a.t;
    t.head = s->ts332[0].data(); t.ctr = tr->rw_counter ? s->ts364[0].data() : nullptr; t.off = s->ts364[1].data();
    t.id = tr->id; t.addr = tr->addr; t.val = tr->val; t.pool = tr->pool; t.steps = tr->steps;
    t.n_rw = n; t.n_pool = tr->n_pool; t.n_steps = ns; t.rw_base = tr->rw_base;
    s->ts332[1].assign(ns + 1, 0);                        // open-time statuses
    s->ts364[2].assign(ns + 1, 0);                        // sizes
    u64 c[TS3_V_WORDS];
    a.st_open = s->ts332[1].data(); a.sz = s->ts364[2].data(); a.verdict = c;
    ts3_count_host(a);
    a.verdict = nullptr;
    if (c[TS3_V_BYTES] >= TS3_BYTES_LIMIT) { rc = ts3_bytes_error(c[TS3_V_CROSS], msg, sizeof msg); g_err = msg; delete s; return rc; }
    if (n_msgs) *n_msgs = c[TS3_V_MSGS];
    if (n_bytes) *n_bytes = c[TS3_V_BYTES];
    if (check_only) { delete s; return 0; }
    const u64 nm = a.n_msgs = c[TS3_V_MSGS], nby = a.n_bytes = c[TS3_V_BYTES];
    s->ts3_msg.assign(nm + 1, Ts3Msg{0, 0, 0, 0, 0, 0});
    s->ts364[3].assign(nm + 1, 0);                        // the session's offsets
    s->ts364[4].assign(nm + 1, 0);                        // fail words
    s->ts364[5].assign(nm * KT_NCELLS * 4 + 4, 0);        // rows
    s->ts364[6].assign(nm + 1, 0);                        // out offsets
    s->ts364[7].assign(KT_RPOW_ROWS * 4, 0);
    s->ts332[2].assign(nm + 1, 0);                        // steps
    s->ts3_data.assign((size_t)((nby + 15) & ~7ull), 0);  // (the sponge reads whole aligned words)
    a.msg = s->ts3_msg.data(); a.data_off = s->ts364[3].data(); a.fail = (unsigned long long*)s->ts364[4].data();
    a.rows = s->ts364[5].data(); a.data_offsets = s->ts364[6].data(); a.step = s->ts332[2].data(); a.data = s->ts3_data.data();
    ts3_write_host(a);
    kt_fill_rpow(cell_of(randomness), s->ts364[7].data());
    KeccakGenArgs& g = s->ts3_kgen;
    g.data = a.data; g.offsets = a.data_off; g.n = nm; g.rpow = s->ts364[7].data(); g.rows = a.rows; g.mode = KT_MODE_CIRCUIT;
    g.long_list = nullptr; g.long_count = nullptr;
    s->pass = sha3_from_trace_pass;
    s->assign_kind = 16;
    *out = s;
    return 0;
}
extern "C" int zk_sha3_from_trace_sizes(const zk_trace* t, uint32_t opts, uint64_t* n_msgs, uint64_t* n_bytes) {
    NO_DEVICE_PTRS(opts, "zk_sha3_from_trace_sizes");
    ARG_TRY(TS3_ARGS_OK(t), "zk_sha3_from_trace_sizes: bad arguments");
    return ts3_open_host(t, nullptr, true, n_msgs, n_bytes, nullptr);
}
extern "C" int zk_sha3_from_trace_open(const zk_trace* t, const uint64_t* randomness, const zk_trace_sha3* out_dev, uint32_t opts, zk_session** out) {
    NO_DEVICE_PTRS(opts, "zk_sha3_from_trace_open");
    ARG_TRY(TS3_ARGS_OK(t) && randomness && out, "zk_sha3_from_trace_open: bad arguments");
    ARG_TRY(!out_dev, "zk_sha3_from_trace_open: out_dev needs ZK_OPT_DEVICE_PTRS");
    return ts3_open_host(t, randomness, false, nullptr, nullptr, out);
}
extern "C" int zk_sha3_from_trace_read(zk_session* s, const zk_trace_sha3* host, uint64_t* n_msgs, uint64_t* n_bytes) {
    ARG_TRY(s && s->assign_kind == 16, "zk_sha3_from_trace_read: bad arguments");
    const Ts3Args& a = s->ts3;
    if (host) {
        if (host->rows && a.n_msgs) memcpy(host->rows, a.rows, a.n_msgs * KT_NCELLS * 32);
        if (host->step && a.n_msgs) memcpy(host->step, a.step, a.n_msgs * 4);
        if (host->data && a.n_bytes) memcpy(host->data, a.data, a.n_bytes);
        if (host->data_offsets) memcpy(host->data_offsets, a.data_offsets, (a.n_msgs + 1) * 8);
    }
    if (n_msgs) *n_msgs = a.n_msgs;
    if (n_bytes) *n_bytes = a.n_bytes;
    return 0;
}
extern "C" int zk_sha3_from_trace(const zk_trace* t, const uint64_t* randomness, const zk_trace_sha3* out_wire, uint32_t opts, uint32_t* status_out,
                                  uint64_t* n_msgs, uint64_t* n_bytes, zk_result* result) {
    ARG_TRY(result && out_wire && t, "zk_sha3_from_trace: null argument");
    zk_session* s = nullptr;
    int rc = zk_sha3_from_trace_open(t, randomness, nullptr, opts, &s);
    if (rc) return rc;
    rc = zk_launch(s, nullptr);
    if (!rc) rc = zk_collect(s, result);
    if (!rc && status_out) rc = zk_read_status(s, status_out);
    if (!rc) rc = zk_sha3_from_trace_read(s, out_wire, n_msgs, n_bytes);
    zk_close(s);
    return rc;
}

// ---- Exp-circuit witness assignment: the per-event / per-row functions of csrc/exp_assign.hpp in plain loops
static void exp_assign_pass(zk_session* s) {
    ExaArgs& a = s->exa;
    for (u64 e = 0; e < a.n_events; e++) exa_chain(a, e);
    for (u64 j = 0; j < a.n_rows; j++) exa_write_row(a, j);
}
// the size pass of an open: counts, first rows, the first rejected event (buffers owned by `s`)
static int exa_size_pass(const zk_exp_events* t, zk_session* s, ExaSizes& z) {
    ExaArgs& a = s->exa;
    s->a64[0].assign(t->events, t->events + t->n_events * EXA_EV_NCELLS * 4);
    s->a32[0].assign(t->n_events + 1, 0);
    s->a64[1].assign(t->n_events + 1, 0);
    a.events = s->a64[0].data(); a.n_events = t->n_events; a.count = s->a32[0].data(); a.row0 = s->a64[1].data();
    u64 reject = EXA_NO_REJECT, run = 0;
    for (u64 e = 0; e < a.n_events; e++) {
        const u32 reason = exa_event_size(a, e);
        if (reason && reject == EXA_NO_REJECT) reject = exa_reject_word(e, reason);
        a.row0[e] = run;
        run += a.count[e];
    }
    a.row0[a.n_events] = run;
    for (u64 e = 0; e < a.n_events; e++) {
        const u32 reason = exa_ident_check(a, e);
        if (reason && exa_reject_word(e, reason) < reject) reject = exa_reject_word(e, reason);
    }
    char msg[256];
    const int rc = exa_sizes_of(reject, run, t->max_exp_steps, z, msg, sizeof msg);
    if (rc) { g_err = msg; return rc; }
    a.n_step = z.n_step;
    a.n_rows = z.n_rows;
    return 0;
}
extern "C" int zk_exp_assign_sizes(const zk_exp_events* t, uint32_t opts, uint64_t* n_rows, uint64_t* n_step_rows, uint64_t* n_table) {
    NO_DEVICE_PTRS(opts, "zk_exp_assign_sizes");
    ARG_TRY(t && (t->events || t->n_events == 0) && t->n_events < (1ull << 31), "zk_exp_assign_sizes: bad arguments");
    zk_session* s = new_session(1, false);
    ExaSizes z;
    const int rc = exa_size_pass(t, s, z);
    delete s;
    if (rc) return rc;
    if (n_rows) *n_rows = z.n_rows;
    if (n_step_rows) *n_step_rows = z.n_step;
    if (n_table) *n_table = z.n_table;
    return 0;
}
extern "C" int zk_exp_assign_open(const zk_exp_events* t, uint64_t* rows_dev, uint64_t* table_dev, uint32_t opts, zk_session** out) {
    NO_DEVICE_PTRS(opts, "zk_exp_assign_open");
    ARG_TRY(t && out && (t->events || t->n_events == 0) && t->n_events < (1ull << 31), "zk_exp_assign_open: bad arguments");
    ARG_TRY(!rows_dev && !table_dev, "zk_exp_assign_open: output buffers need ZK_OPT_DEVICE_PTRS");
    zk_session* s = new_session(1, false);
    ExaSizes& z = s->exa_sizes;
    const int rc = exa_size_pass(t, s, z);
    if (rc) { delete s; return rc; }
    if (z.n_rows == 0) { delete s; g_err = "zk_exp_assign_open: no rows (every exponent is 0 or 1 and max_exp_steps is 0)"; return -1; }
    s->n = s->hi = z.n_rows;
    s->status.assign(z.n_rows, 0u);
    s->w64[0].assign((z.n_step + 1) * 4, 0);                     // d
    s->w64[1].assign(z.n_rows * EXA_ROW_NCELLS * 4 + 4, 0);      // rows
    s->w64[2].assign(z.n_table * EXA_TABLE_NCELLS * 4 + 4, 0);   // table
    s->exa.d = s->w64[0].data(); s->exa.rows = s->w64[1].data(); s->exa.table = s->w64[2].data();
    s->pass = exp_assign_pass;
    s->assign_kind = 6;
    *out = s;
    return 0;
}
extern "C" int zk_exp_assign_counts(zk_session* s, uint64_t* n_rows, uint64_t* n_step_rows, uint64_t* n_table) {
    ARG_TRY(s && s->assign_kind == 6, "zk_exp_assign_counts: bad arguments");
    if (n_rows) *n_rows = s->exa_sizes.n_rows;
    if (n_step_rows) *n_step_rows = s->exa_sizes.n_step;
    if (n_table) *n_table = s->exa_sizes.n_table;
    return 0;
}
extern "C" int zk_exp_assign_read(zk_session* s, uint64_t* rows_host, uint64_t* table_host) {
    ARG_TRY(s && s->assign_kind == 6, "zk_exp_assign_read: bad arguments");
    const ExaSizes& z = s->exa_sizes;
    if (rows_host) memcpy(rows_host, s->w64[1].data(), (size_t)z.n_rows * EXA_ROW_NCELLS * 32);
    if (table_host && z.n_table) memcpy(table_host, s->w64[2].data(), (size_t)z.n_table * EXA_TABLE_NCELLS * 32);
    return 0;
}
extern "C" int zk_exp_assign(const zk_exp_events* t, uint64_t* rows_out, uint64_t* table_out, uint32_t opts, zk_result* result) {
    ARG_TRY(result && rows_out, "zk_exp_assign: null output");
    zk_session* s = nullptr;
    int rc = zk_exp_assign_open(t, nullptr, nullptr, opts, &s);
    if (rc) return rc;
    rc = zk_launch(s, nullptr);
    if (!rc) rc = zk_collect(s, result);
    if (!rc) rc = zk_exp_assign_read(s, rows_out, table_out);
    zk_close(s);
    return rc;
}

// ---- PI-circuit witness assignment: the per-row functions of csrc/pi_assign.hpp in plain loops
static void pi_assign_pass(zk_session* s) {
    PiaArgs& a = s->pia;
    {   // calldata gas: the prefix inside each tile, the tile bases
        u64 base = 0;
        u32 run = 0;
        for (u64 c = 0; c < a.total_cd; c++) {
            if (c % PIA_GAS_TILE == 0) { base += run; run = 0; a.gas_tile[c / PIA_GAS_TILE] = base; }
            run += a.calldata[c] ? 16u : 4u;
            a.gas_local[c] = run;
        }
    }
    for (u64 r = 0; r < PIA_TX_LEN * a.max_txs; r++) {  // (one Fermat chain per distinct value: the padding slots share theirs)
        const Fr lo = pia_tx_value_lo(a, r);
        if (fr_is_zero(lo)) pia_store_fr(a.inv_txlo + 4 * r, lo); else pia_tx_inverse(a, r);
    }
#pragma omp parallel for schedule(static)
    for (long long i = 0; i < (long long)a.n; i++) pia_row_byte(a, (u64)i);
    keccak_table_row(s->pia_kgen, 0);
    {   // suffix RLC: one walk from the last row of the last tile, keeping the tile's own sum beside the whole one
        const Fr rand_m = fr_to_mont(a.rand);
        Fr all = fr_zero(), tile = fr_zero();
        pia_store_fr(a.carry + 4 * a.n_tiles, all);
        for (u64 i = a.n_tiles * PIA_TILE; i-- > 0;) {
            const u32 b = pia_byte_at(a, i);
            all = fr_add_u64(fr_mulc(all, rand_m), b);
            tile = fr_add_u64(fr_mulc(tile, rand_m), b);
            if (i % PIA_SLICE == 0) pia_store_fr(a.slice_acc + 4 * (i / PIA_SLICE), tile);
            if (i % PIA_TILE == 0) {
                pia_store_fr(a.tile_acc + 4 * (i / PIA_TILE), tile);
                pia_store_fr(a.carry + 4 * (i / PIA_TILE), all);
                tile = fr_zero();
            }
        }
    }
#pragma omp parallel for schedule(static)
    for (long long i = 0; i < (long long)a.n; i++) pia_write_row(a, (u64)i);
    pia_patch(a);
}
static int pia_prepare(const zk_pi_inputs* t, zk_session* s, PiaSizes& z) {
    PiaArgs& a = s->pia;
    char msg[256];
    const u64 total = t->calldata_offsets[t->n_txs];
    int rc = pia_sizes_of(t->n_txs, t->n_withdrawals, total, t->max_txs, t->max_calldata_bytes, t->max_withdrawals, z, msg, sizeof msg);
    if (rc) { g_err = msg; return rc; }
    s->pia64[0].assign(t->block, t->block + PIA_NBLOCK_FIELDS * 4);
    s->pia64[1].assign(t->state_root_prev, t->state_root_prev + 4);
    s->pia64[2].assign(t->block_hashes, t->block_hashes + 256 * 4);
    s->pia64[3].assign(t->tx_fields, t->tx_fields + t->n_txs * PIA_NTX_FIELDS * 4);
    s->pia64[4].assign(t->calldata_offsets, t->calldata_offsets + t->n_txs + 1);
    s->pia64[5].assign(t->withdrawals, t->withdrawals + t->n_withdrawals * PIA_NWD_FIELDS * 4);
    s->pia32[0].assign(t->to_is_none, t->to_is_none + t->n_txs);
    s->pia8[0].assign(t->calldata, t->calldata + total);
    s->pia8[0].push_back(0);
    a.chain_id = t->chain_id;
    a.block = s->pia64[0].data(); a.srp = s->pia64[1].data(); a.hashes = s->pia64[2].data(); a.txf = s->pia64[3].data();
    a.offs = s->pia64[4].data(); a.wd = s->pia64[5].data(); a.to_none = s->pia32[0].data(); a.calldata = s->pia8[0].data();
    a.n_txs = t->n_txs; a.n_wd = t->n_withdrawals; a.max_txs = t->max_txs; a.max_cd = t->max_calldata_bytes; a.max_wd = t->max_withdrawals;
    a.total_cd = total;
    pia_set_layout(a, z);
    a.rand = cell_of(t->keccak_rand);
    a.base = cell_of(t->byte_pow_base);
    for (u64 k = 0; k < PIA_N_CHECKS(a); k++)
        if (!pia_check(a, k)) { rc = pia_reject_text(k, msg, sizeof msg); g_err = msg; return rc; }
    return 0;
}
#define PIA_ARGS_OK(t) ((t) && (t)->block && (t)->state_root_prev && (t)->block_hashes && (t)->calldata_offsets && (t)->keccak_rand && (t)->byte_pow_base && \
                        ((t)->n_txs == 0 || ((t)->tx_fields && (t)->to_is_none)) && ((t)->n_withdrawals == 0 || (t)->withdrawals) && (t)->n_txs < (1ull << 31) && \
                        (t)->n_withdrawals < (1ull << 31) && ((t)->calldata || (t)->calldata_offsets[(t)->n_txs] == 0))
extern "C" int zk_pi_assign_sizes(const zk_pi_inputs* t, uint32_t opts, uint64_t* circuit_len, uint64_t* n_gas, uint64_t* n_constraints) {
    NO_DEVICE_PTRS(opts, "zk_pi_assign_sizes");
    ARG_TRY(PIA_ARGS_OK(t), "zk_pi_assign_sizes: bad arguments");
    zk_session* s = new_session(1, false);
    PiaSizes z;
    const int rc = pia_prepare(t, s, z);
    delete s;
    if (rc) return rc;
    if (circuit_len) *circuit_len = z.n;
    if (n_gas) *n_gas = z.n_gas;
    if (n_constraints) *n_constraints = z.n_cc;
    return 0;
}
extern "C" int zk_pi_assign_open(const zk_pi_inputs* t, const zk_pi_wire* out_dev, uint32_t opts, zk_session** out) {
    NO_DEVICE_PTRS(opts, "zk_pi_assign_open");
    ARG_TRY(PIA_ARGS_OK(t) && out, "zk_pi_assign_open: bad arguments");
    ARG_TRY(!out_dev, "zk_pi_assign_open: output buffers need ZK_OPT_DEVICE_PTRS");
    zk_session* s = new_session(1, false);
    PiaSizes& z = s->pia_sizes;
    const int rc = pia_prepare(t, s, z);
    if (rc) { delete s; return rc; }
    PiaArgs& a = s->pia;
    s->n = s->hi = z.n;
    s->status.assign(z.n, 0u);
    s->pia32[1].assign(a.total_cd + 1, 0);                         a.gas_local = s->pia32[1].data();
    s->pia64[6].assign(a.n_gas_tiles + 1, 0);                      a.gas_tile = s->pia64[6].data();
    s->pia64[7].assign(a.n_inv * 4, 0);                            a.inv_small = s->pia64[7].data();
    s->pia64[8].assign(PIA_TX_LEN * a.max_txs * 4 + 4, 0);         a.inv_txlo = s->pia64[8].data();
    s->pia8[1].assign(z.n, 0);                                     a.gen = s->pia8[1].data();
    s->pia64[9].assign(((size_t)PIA_TILE + 1) * 4, 0);             a.rpow = s->pia64[9].data();
    s->pia64[10].assign(a.n_tiles * 256 * 4, 0);                   a.slice_acc = s->pia64[10].data();
    s->pia64[11].assign((a.n_tiles + 1) * 4, 0);                   a.tile_acc = s->pia64[11].data();
    s->pia64[12].assign((a.n_tiles + 1) * 4, 0);                   a.carry = s->pia64[12].data();
    s->pia64[13].assign(KT_NCELLS * 4 + (size_t)KT_RPOW_ROWS * 4 + 2, 0);  a.krow = s->pia64[13].data();
    s->pia64[14].assign(z.n * PI_NCELLS * 4, 0);                   a.rows = s->pia64[14].data();
    s->pia64[15].assign(z.n_gas * PI_GAS_NCELLS * 4, 0);           a.gas = s->pia64[15].data();
    s->pia64[16].assign(2 * 5 * 4 + 4 * 2 * 4, 0);                 a.keccak = s->pia64[16].data(); a.public_inputs = a.keccak + 2 * 5 * 4;
    s->pia64[17].assign(z.n_cc * 4, 0);                            a.cc_cells = s->pia64[17].data();
    s->pia8[2].assign(z.n_cc * 32, 0);                             a.cc_bytes = s->pia8[2].data();
    s->pia32[2].assign(z.n_cc, 0);                                 a.cc_lens = s->pia32[2].data();
    s->pia64[18].assign((size_t)PIA_BLOCK_ENTRIES * 2 * 4, 0);     a.block_table = s->pia64[18].data();
    s->pia32[3].assign(PIA_BLOCK_ENTRIES, 0);                      a.block_flags = s->pia32[3].data();
    s->pia64[19].assign(z.tx_table_rows * 5 * 4 + a.max_wd * 5 * 4, 0);  a.tx_table = s->pia64[19].data(); a.wd_table = a.tx_table + z.tx_table_rows * 5 * 4;
    s->pia32[4].assign(z.tx_table_rows, 0);                        a.tx_flags = s->pia32[4].data();
    s->pia8[3].assign(z.n, 0);                                     a.raw_bytes = s->pia8[3].data();
    s->pia32[5].assign(z.n_values, 0);                             a.raw_lens = s->pia32[5].data();
    for (u64 k = 0; k <= (u64)PIA_TILE; k++) pia_store_fr(a.rpow + 4 * k, pia_pow_mont(fr_to_mont(a.rand), k));
    {   // k^-1 from one Fermat chain: the inverse of (n_inv - 1)!, walked down
        std::vector<Fr> fact(a.n_inv, fr_from_u64(1));
        for (u64 k = 2; k < a.n_inv; k++) fact[k] = fr_mul(fact[k - 1], fr_from_u64(k));
        Fr finv = fr_inv(fact[a.n_inv - 1]);  // 1 / (n_inv - 1)!
        for (u64 k = a.n_inv; k-- > 1;) {
            pia_store_fr(a.inv_small + 4 * k, fr_mul(finv, fact[k - 1]));  // (k - 1)! / k!
            finv = fr_mul(finv, fr_from_u64(k));
        }
    }
    KeccakGenArgs& g = s->pia_kgen;
    u64* offs = a.krow + KT_NCELLS * 4 + (size_t)KT_RPOW_ROWS * 4;
    offs[0] = 0; offs[1] = z.n;
    kt_fill_rpow(cell_of(t->keccak_rand), a.krow + KT_NCELLS * 4);
    g.data = a.gen; g.offsets = offs; g.n = 1; g.rpow = a.krow + KT_NCELLS * 4; g.rows = a.krow; g.mode = KT_MODE_CIRCUIT; g.long_list = nullptr; g.long_count = nullptr;
    s->pass = pi_assign_pass;
    s->assign_kind = 7;
    *out = s;
    return 0;
}
#define PIA_COPY(dst, src, bytes) do { if (dst) memcpy(dst, src, bytes); } while (0)
extern "C" int zk_pi_assign_read(zk_session* s, const zk_pi_wire* h) {
    ARG_TRY(s && h && s->assign_kind == 7, "zk_pi_assign_read: bad arguments");
    const PiaArgs& a = s->pia;
    const PiaSizes& z = s->pia_sizes;
    PIA_COPY(h->rows, a.rows, (size_t)z.n * PI_NCELLS * 32);
    PIA_COPY(h->gas, a.gas, (size_t)z.n_gas * PI_GAS_NCELLS * 32);
    PIA_COPY(h->keccak, a.keccak, 2 * 5 * 32);
    PIA_COPY(h->cc_cells, a.cc_cells, (size_t)z.n_cc * 32);
    PIA_COPY(h->cc_bytes, a.cc_bytes, (size_t)z.n_cc * 32);
    PIA_COPY(h->cc_lens, a.cc_lens, (size_t)z.n_cc * 4);
    PIA_COPY(h->block_table, a.block_table, (size_t)PIA_BLOCK_ENTRIES * 2 * 32);
    PIA_COPY(h->block_flags, a.block_flags, (size_t)PIA_BLOCK_ENTRIES * 4);
    PIA_COPY(h->tx_table, a.tx_table, (size_t)z.tx_table_rows * 5 * 32);
    PIA_COPY(h->tx_flags, a.tx_flags, (size_t)z.tx_table_rows * 4);
    PIA_COPY(h->wd_table, a.wd_table, (size_t)a.max_wd * 5 * 32);
    PIA_COPY(h->public_inputs, a.public_inputs, 4 * 2 * 32);
    PIA_COPY(h->raw_bytes, a.raw_bytes, (size_t)z.n);
    PIA_COPY(h->raw_lens, a.raw_lens, (size_t)z.n_values * 4);
    return 0;
}
extern "C" int zk_pi_assign(const zk_pi_inputs* t, const zk_pi_wire* out_wire, uint32_t opts, zk_result* result) {
    ARG_TRY(result && out_wire && out_wire->rows, "zk_pi_assign: null output");
    zk_session* s = nullptr;
    int rc = zk_pi_assign_open(t, nullptr, opts, &s);
    if (rc) return rc;
    rc = zk_launch(s, nullptr);
    if (!rc) rc = zk_collect(s, result);
    if (!rc) rc = zk_pi_assign_read(s, out_wire);
    zk_close(s);
    return rc;
}

// ---- ECC circuit ------------------------------------------------------------------------------------------------------
extern "C" int zk_ecc_assign(const zk_ecc_ops* ops, uint32_t opts, uint64_t* rows_out) {
    NO_DEVICE_PTRS(opts, "zk_ecc_assign");
    EccArgs a;
    const char* err = ecc_args_from_ops(ops, a);
    ARG_TRY(!err, err ? (std::string("zk_ecc_assign: ") + err).c_str() : "");
    ARG_TRY(rows_out, "zk_ecc_assign: rows_out is null");
    const u64 np = a.n_add + a.n_mul, n = np + a.n_pairing;
#pragma omp parallel for schedule(dynamic, 16)
    for (long long i = 0; i < (long long)n; i++) {
        u64* row = rows_out + (u64)i * ECC_NCELLS * 4;
        if ((u64)i < np) ecc_assign_point_row(a, (u64)i, row);
        else ecc_assign_pairing_row(a, (u64)i - np, row);
    }
    return 0;
}
extern "C" int zk_ecc_verify(const zk_ecc_ops* ops, const uint64_t* rows, uint32_t opts, uint32_t* status_out, zk_result* result) {
    NO_DEVICE_PTRS(opts, "zk_ecc_verify");
    ARG_TRY(result && rows, "zk_ecc_verify: rows / result is null");
    EccArgs a;
    const char* err = ecc_args_from_ops(ops, a);
    ARG_TRY(!err, err ? (std::string("zk_ecc_verify: ") + err).c_str() : "");
    a.rows = rows;
    zk_session* s = new_session(a.n_add + a.n_mul + a.n_pairing, true);
    s->row = [a](u64 i) { return ecc_verify_row(a, i); };
    return one_shot(s, status_out, result);
}

// ECC sessions: a private copy of the ops (and rows).  A verification pass over [lo, hi) takes the HIP session's form: the point rows
// by ecc_verify_point_row, ecc_pair_stage1 once per pair of the pairing ops in range (pairs pair_off[k_lo] .. pair_off[k_hi]), then
// ecc_pair_stage2 per pairing row over the records; the one-shot zk_ecc_verify keeps the one-call form ecc_verify_row
static int ecc_session_ops(zk_session* s, const zk_ecc_ops* ops, EccArgs& a, const char* name) {
    const char* err = ecc_args_from_ops(ops, a);
    if (err) { g_err = std::string(name) + ": " + err; return -1; }
    const u64 np = a.n_add + a.n_mul, n_pp = a.n_pairing ? a.pair_off[a.n_pairing] : 0;
    if (np) s->a64[0].assign(a.pts, a.pts + np * 24);
    if (n_pp) s->a64[1].assign(a.pair_pts, a.pair_pts + n_pp * 24);
    if (a.n_pairing) s->a64[2].assign(a.pair_out, a.pair_out + a.n_pairing * 4);
    s->a32[0].assign(a.n_pairing + 1, 0u);
    if (a.n_pairing) memcpy(s->a32[0].data(), a.pair_off, (a.n_pairing + 1) * 4);
    a.pts = s->a64[0].data(); a.pair_pts = s->a64[1].data(); a.pair_out = s->a64[2].data(); a.pair_off = s->a32[0].data();
    return 0;
}
extern "C" int zk_ecc_open(const zk_ecc_ops* ops, const uint64_t* rows, uint32_t opts, zk_session** out) {
    NO_DEVICE_PTRS(opts, "zk_ecc_open");
    ARG_TRY(out, "zk_ecc_open: out is null");
    ARG_TRY(rows, "zk_ecc_open: rows is null");
    zk_session* s = new zk_session();
    EccArgs a;
    if (int rc = ecc_session_ops(s, ops, a, "zk_ecc_open")) { delete s; return rc; }
    const u64 n = a.n_add + a.n_mul + a.n_pairing;
    s->n = n; s->lo = 0; s->hi = n;
    s->status.assign(n, 0u);
    s->range_ok = s->range_may_be_empty = true;
    s->a64[3].assign(rows, rows + n * ECC_NCELLS * 4);
    a.rows = s->a64[3].data();
    const u64 np = a.n_add + a.n_mul;
    s->ecc_pair_flags.assign(a.n_pairing ? a.pair_off[a.n_pairing] : 0, 0u);
    s->ecc_pair_f.resize(s->ecc_pair_flags.size());
    const EccPairArgs pr = {a, s->ecc_pair_flags.data(), s->ecc_pair_f.data()};
    s->before_rows = [pr, np](u64 lo, u64 hi) {
        const u64 k_lo = (lo > np ? lo : np) - np, k_hi = (hi > np ? hi : np) - np;
        if (k_hi <= k_lo) return;
        const long long t_lo = pr.a.pair_off[k_lo], t_hi = pr.a.pair_off[k_hi];
#pragma omp parallel for schedule(dynamic, 1)
        for (long long t = t_lo; t < t_hi; t++) ecc_pair_stage1(pr, (u32)t);
    };
    s->row = [pr, np](u64 i) { return i < np ? ecc_verify_point_row(pr.a, i) : ecc_pair_stage2(pr, i); };
    *out = s;
    return 0;
}
static void ecc_assign_pass(zk_session* s) {
    const EccArgs a = s->ecc_assign;
    const u64 np = a.n_add + a.n_mul;
#pragma omp parallel for schedule(dynamic, 16)
    for (long long i = 0; i < (long long)s->n; i++) {
        u64* row = a.rows_out + (u64)i * ECC_NCELLS * 4;
        if ((u64)i < np) ecc_assign_point_row(a, (u64)i, row);
        else ecc_assign_pairing_row(a, (u64)i - np, row);
    }
}
extern "C" int zk_ecc_assign_open(const zk_ecc_ops* ops, uint64_t* rows_dev, uint32_t opts, zk_session** out) {
    NO_DEVICE_PTRS(opts, "zk_ecc_assign_open");
    ARG_TRY(out && !rows_dev, "zk_ecc_assign_open: bad arguments (rows_dev needs ZK_OPT_DEVICE_PTRS)");
    zk_session* s = new zk_session();
    EccArgs& a = s->ecc_assign;
    if (int rc = ecc_session_ops(s, ops, a, "zk_ecc_assign_open")) { delete s; return rc; }
    const u64 n = a.n_add + a.n_mul + a.n_pairing;
    s->n = n; s->lo = 0; s->hi = n;
    s->status.assign(n, 0u);
    s->w64[0].assign(n * ECC_NCELLS * 4, 0);
    a.rows_out = s->w64[0].data();
    s->pass = ecc_assign_pass;
    s->assign_kind = 8;
    *out = s;
    return 0;
}
extern "C" int zk_ecc_assign_read(zk_session* s, uint64_t* rows_host) {
    ARG_TRY(s && rows_host && s->assign_kind == 8, "zk_ecc_assign_read: bad arguments");
    memcpy(rows_host, s->w64[0].data(), s->w64[0].size() * 8);
    return 0;
}

// ---- Withdrawal circuit -----------------------------------------------------------------------------------------------
extern "C" int zk_withdrawal_open(const zk_withdrawal_witness* w, uint32_t opts, zk_session** out) {
    NO_DEVICE_PTRS(opts, "zk_withdrawal_open");
    ARG_TRY(w && out && w->randomness && (w->rows || w->n_rows == 0), "zk_withdrawal_open: bad arguments");
    ARG_TRY(w->n_rows < (1ull << 32) && w->n_mpt < (1ull << 31) && w->n_keccak < (1ull << 31) && w->n_block < (1ull << 31),
            "zk_withdrawal_open: table too large");
    ARG_TRY(w->row_base + w->n_rows <= w->total_rows || (w->n_rows == 0 && w->row_base == 0), "zk_withdrawal_open: rows beyond total_rows");
    WithdrawalArgs a = {};
    a.n_rows = w->n_rows;
    a.row_base = w->row_base;
    a.total_rows = w->total_rows;
    a.max_w = w->max_withdrawals;
    const u64 n = wd_eval_rows(a);
    ARG_TRY(n > 0, "zk_withdrawal_open: row_base lies beyond the evaluated rows");
    zk_session* s = new_session(n, true);
    s->a64[0].assign(w->rows, w->rows + w->n_rows * WD_NCELLS * 4);
    s->a64[1].assign(w->block, w->block + w->n_block * WD_BLOCK_NCELLS * 4);
    cpu_table(s->tab[0], w->keccak, nullptr, w->n_keccak, KECCAK_NCELLS, keccak_key_hash);
    cpu_table(s->tab[1], w->mpt, nullptr, w->n_mpt, MPT_NCELLS, wd_mpt_key_hash);
    a.rows = s->a64[0].data();
    a.block = s->a64[1].data();
    a.n_block = w->n_block;
    a.keccak = s->tab[0].t;
    a.mpt = s->tab[1].t;
    a.r = cell_of(w->randomness);
    s->row = [s, a](u64 j) { (void)s; return wd_verify_row(a, j); };
    *out = s;
    return 0;
}
extern "C" int zk_withdrawal_verify(const zk_withdrawal_witness* w, uint32_t opts, uint32_t* status_out, zk_result* result) {
    ARG_TRY(result, "zk_withdrawal_verify: result is null");
    zk_session* s = nullptr;
    const int rc = zk_withdrawal_open(w, opts, &s);
    return rc ? rc : one_shot(s, status_out, result);
}
extern "C" int zk_withdrawal_assign(const uint64_t* withdrawals, uint64_t n, uint64_t max_withdrawals, const uint64_t* randomness,
                                    uint32_t opts, uint64_t* rows_out, uint64_t* keccak_out) {
    NO_DEVICE_PTRS(opts, "zk_withdrawal_assign");
    ARG_TRY(randomness && (rows_out || (n == 0 && max_withdrawals == 0)) && (withdrawals || n == 0), "zk_withdrawal_assign: bad arguments");
    ARG_TRY(n < (1ull << 32) && max_withdrawals < (1ull << 32), "zk_withdrawal_assign: too many rows");
    WithdrawalArgs a = {};
    a.in = withdrawals;
    a.n_in = n;
    a.n_out = n > max_withdrawals ? n : max_withdrawals;
    a.rows_out = rows_out;
    a.keccak_out = keccak_out;
    a.r = cell_of(randomness);
#pragma omp parallel for schedule(dynamic, 256)
    for (long long i = 0; i < (long long)a.n_out; i++) {
        uint8_t m[136];
        wd_assign_row(a, (u64)i, m);
    }
    return 0;
}

// ---- what the Tx and the Sig witness assignment share
// signature i of a recovery batch in the one-lane form: its key and its status
static void secp_recover_one(const SecpRecoverArgs& q, u64 i) {
    u32 tab[15 * 24];
    EcdsaPrep pr;
    Fr u1, u2;
    const u32 st = tx_recover_prepare(q, i, pr, u1, u2);
    u32 code;
    if (st == ECDSA_PENDING) code = tx_recover_finish_to(q.pk + i * 8, ecdsa_partial(pr, 0, 1, tab, 1, nullptr));
    else if (st == TX_RECOVER_EXACT) code = tx_recover_finish_to(q.pk + i * 8, tx_recover_exact(pr, u1, u2));
    else { code = st; tx_recover_fail_to(q.pk + i * 8); }
    q.status[i] = code;
}
// the m keccak candidates as a sorted set in `keccak`; returns its size
static u64 keccak_sorted_set(const u64* kc, u64 m, u64* keccak) {
    std::vector<u64> idx((size_t)m);
    for (u64 k = 0; k < m; k++) idx[k] = k;
    std::sort(idx.begin(), idx.end(), [kc](u64 x, u64 y) { return tx_krow_cmp(kc + x * 20, kc + y * 20) < 0; });
    u64 cnt = 0;
    for (u64 k = 0; k < m; k++) {
        if (cnt && tx_krow_cmp(keccak + (cnt - 1) * 20, kc + idx[k] * 20) == 0) continue;
        memcpy(keccak + cnt * 20, kc + idx[k] * 20, 160);
        cnt++;
    }
    return cnt;
}

// ---- Tx circuit witness assignment (tx_assign.hpp): the device functions in host loops; recovery in the one-lane form
static void tx_assign_pass(zk_session* s) {
    TxAssignArgs& a = s->txa;
    const SecpRecoverArgs q = tx_recover_args(a);
    const long long n = (long long)a.n;
#pragma omp parallel for schedule(dynamic, 16)
    for (long long i = 0; i < n; i++) {
        tx_sign_hash(a, (u64)i);
        secp_recover_one(q, (u64)i);
    }
    memcpy(s->status.data(), a.status, (size_t)a.n * sizeof(u32));
#pragma omp parallel for schedule(dynamic, 64)
    for (long long i = 0; i < (long long)a.max_txs; i++) tx_write_slot(a, (u64)i);
    tx_write_zero_candidate(a);
#pragma omp parallel for schedule(static)
    for (long long j = 0; j < (long long)a.max_calldata; j++) tx_write_calldata_row(a, (u64)j);
    s->n_keccak = keccak_sorted_set(a.kcand, a.n + 1, a.keccak);
}
extern "C" int zk_tx_assign_open(const zk_tx_inputs* in, const zk_tx_wire* out_dev, uint32_t opts, zk_session** out) {
    NO_DEVICE_PTRS(opts, "zk_tx_assign_open");
    ARG_TRY(in && out && !out_dev && in->randomness && in->calldata_offsets && (in->n_txs == 0 || (in->fields && in->to_is_none)) &&
            in->n_txs <= in->max_txs && in->max_txs < (1ull << 31) && in->max_calldata_bytes < (1ull << 34),
            "zk_tx_assign_open: bad arguments");
    const u64 n = in->n_txs, mt = in->max_txs, mc = in->max_calldata_bytes;
    const u64* off = in->calldata_offsets;
    ARG_TRY(off[0] == 0, "zk_tx_assign_open: calldata offsets must start at 0");
    for (u64 j = 0; j < n; j++) ARG_TRY(off[j] <= off[j + 1], "zk_tx_assign_open: calldata offsets must be non-decreasing");
    ARG_TRY(off[n] <= mc, "zk_tx_assign_open: more calldata bytes than max_calldata_bytes");
    ARG_TRY(!off[n] || in->calldata, "zk_tx_assign_open: calldata is null");
    zk_session* s = new_session(n, false);
    s->a64[0].assign(in->fields, in->fields + n * TX_NFIELDS * 4);
    s->a32[0].assign(in->to_is_none, in->to_is_none + n);
    s->a64[1].assign(off, off + n + 1);
    s->a8.assign((size_t)((off[n] + 15) & ~7ull), 0);  // whole aligned words for the sponge's reads
    if (off[n]) memcpy(s->a8.data(), in->calldata, (size_t)off[n]);
    s->a64[2].assign(KT_RPOW_ROWS * 4, 0);
    kt_fill_rpow(cell_of(in->randomness), s->a64[2].data());
    s->a64[3].assign((size_t)(n + 1) * 4, 0);   // hash
    s->w64[0].assign((size_t)n + 1, 0);         // gas cost
    s->w64[1].assign((size_t)(n + 1) * 8, 0);   // pk
    s->txa_out32[2].assign((size_t)n + 1, 0);   // status
    const u64 rows = mt * TX_FIXED_ROWS + mc;
    s->txa_out64[0].assign((size_t)rows * TX_ROW_CELLS * 4 + 4, 0);
    s->txa_out32[0].assign((size_t)rows + 1, 0);
    s->a8b.assign((size_t)mt * TX_UNIT_BYTES + 32, 0);
    s->txa_out64[1].assign((size_t)mt * TX_UNIT_CELLS * 4 + 4, 0);
    s->txa_out32[1].assign((size_t)mt * 4 + 4, 0);
    s->txa_out64[2].assign((size_t)(n + 1) * KT_NCELLS * 4, 0);
    s->txa_out64[3].assign((size_t)(n + 1) * KT_NCELLS * 4, 0);
    TxAssignArgs& a = s->txa;
    memset(&a, 0, sizeof(a));
    a.fields = s->a64[0].data(); a.to_none = s->a32[0].data(); a.data = s->a8.data(); a.off = s->a64[1].data();
    a.n = n; a.max_txs = mt; a.max_calldata = mc; a.chain_id = in->chain_id; a.rpow = s->a64[2].data();
    a.hash = s->a64[3].data(); a.gas_cost = s->w64[0].data(); a.pk = s->w64[1].data(); a.status = s->txa_out32[2].data();
    a.tx_rows = s->txa_out64[0].data(); a.tx_flags = s->txa_out32[0].data(); a.bytes = s->a8b.data(); a.cells = s->txa_out64[1].data();
    a.meta = s->txa_out32[1].data(); a.kcand = s->txa_out64[2].data(); a.keccak = s->txa_out64[3].data();
    a.lanes.lanes_per_sig = 1;
    s->pass = tx_assign_pass;
    s->assign_kind = 5;
    *out = s;
    return 0;
}
extern "C" int zk_tx_assign_read(zk_session* s, const zk_tx_wire* host, uint64_t* n_keccak_out) {
    ARG_TRY(s && s->assign_kind == 5, "zk_tx_assign_read: bad arguments");
    const TxAssignArgs& a = s->txa;
    const u64 rows = a.max_txs * TX_FIXED_ROWS + a.max_calldata;
    if (host) {
        if (host->tx_rows) memcpy(host->tx_rows, a.tx_rows, (size_t)rows * TX_ROW_CELLS * 32);
        if (host->tx_flags) memcpy(host->tx_flags, a.tx_flags, (size_t)rows * 4);
        if (host->bytes) memcpy(host->bytes, a.bytes, (size_t)a.max_txs * TX_UNIT_BYTES);
        if (host->cells) memcpy(host->cells, a.cells, (size_t)a.max_txs * TX_UNIT_CELLS * 32);
        if (host->meta) memcpy(host->meta, a.meta, (size_t)a.max_txs * 16);
        if (host->keccak) memcpy(host->keccak, a.keccak, (size_t)s->n_keccak * KT_NCELLS * 32);
    }
    if (n_keccak_out) *n_keccak_out = s->n_keccak;
    return 0;
}
extern "C" int zk_tx_assign(const zk_tx_inputs* in, const zk_tx_wire* out, uint32_t opts, uint32_t* status_out, uint64_t* n_keccak_out,
                            zk_result* result) {
    ARG_TRY(result && out, "zk_tx_assign: null output");
    zk_session* s = nullptr;
    int rc = zk_tx_assign_open(in, nullptr, opts, &s);
    if (rc) return rc;
    rc = zk_launch(s, nullptr);
    if (!rc) rc = zk_collect(s, result);
    if (!rc && status_out) rc = zk_read_status(s, status_out);
    if (!rc) rc = zk_tx_assign_read(s, out, n_keccak_out);
    zk_close(s);
    return rc;
}

// ---- Sig circuit witness assignment (sig_assign.hpp): the device functions in host loops; recovery in the one-lane form
static void sig_assign_pass(zk_session* s) {
    SigAssignArgs& a = s->sga;
    const SecpRecoverArgs q = sig_recover_args(a);
    const long long n = (long long)a.n;
#pragma omp parallel for schedule(dynamic, 16)
    for (long long i = 0; i < n; i++) secp_recover_one(q, (u64)i);
    memcpy(s->status.data(), a.status, (size_t)a.n * sizeof(u32));
#pragma omp parallel for schedule(dynamic, 64)
    for (long long i = 0; i < n; i++) sig_write_unit(a, (u64)i);
    sig_write_zero_candidate(a);
    s->n_keccak = keccak_sorted_set(a.kcand, a.n + 1, a.keccak);
    // the sig table: first occurrences in input order (equal rows are adjacent once sorted by (row, index))
    const u64* sc = a.scand;
    std::vector<u64> idx((size_t)a.n);
    for (u64 k = 0; k < a.n; k++) idx[k] = k;
    std::sort(idx.begin(), idx.end(), [sc](u64 x, u64 y) {
        const int c = memcmp(sc + x * SIG_TABLE_WORDS, sc + y * SIG_TABLE_WORDS, SIG_TABLE_WORDS * 8);
        return c ? c < 0 : x < y;
    });
    for (u64 k = 0; k < a.n; k++) a.sdup[idx[k]] = k && sig_row_eq(sc + idx[k - 1] * SIG_TABLE_WORDS, sc + idx[k] * SIG_TABLE_WORDS);
    u64 m = 0;
    for (u64 k = 0; k < a.n; k++)
        if (!a.sdup[k]) memcpy(a.sig_table + m++ * SIG_TABLE_WORDS, sc + k * SIG_TABLE_WORDS, SIG_TABLE_WORDS * 8);
    s->n_sig_rows = m;
}
extern "C" int zk_sig_assign_open(const zk_sig_inputs* in, const zk_sig_wire* out_dev, uint32_t opts, zk_session** out) {
    NO_DEVICE_PTRS(opts, "zk_sig_assign_open");
    ARG_TRY(in && out && !out_dev && in->randomness && (in->n == 0 || in->fields) && in->n < (1ull << 31), "zk_sig_assign_open: bad arguments");
    const u64 n = in->n;
    zk_session* s = new_session(n, false);
    if (n) s->sga64[0].assign(in->fields, in->fields + n * SIG_NFIELDS * 4);
    if (n && in->addr) s->sga64[1].assign(in->addr, in->addr + n * 4);
    if (n && in->expect_valid) s->sga32[0].assign(in->expect_valid, in->expect_valid + n);
    s->sga64[2].assign(KT_RPOW_ROWS * 4, 0);
    kt_fill_rpow(cell_of(in->randomness), s->sga64[2].data());
    s->sga64[3].assign((size_t)(n + 1) * 8, 0);                                        // pk
    s->sga32[2].assign((size_t)n + 1, 0);                                              // status
    s->a8b.assign((size_t)n * TX_UNIT_BYTES + 32, 0);
    s->sga64[4].assign((size_t)n * TX_UNIT_CELLS * 4 + 4, 0);
    s->sga32[1].assign((size_t)n * 4 + 4, 0);
    s->sga64[5].assign((size_t)(n + 1) * KT_NCELLS * 4 * 2, 0);                        // keccak candidates, then the table
    s->sga64[6].assign((size_t)(n + 1) * SIG_TABLE_WORDS * 2, 0);                      // sig candidates, then the table
    s->sga64[7].assign((size_t)n * SIG_AUX_CELLS * 4 + 4, 0);
    s->a32[0].assign((size_t)n + 1, 0);                                                // sdup
    SigAssignArgs& a = s->sga;
    memset(&a, 0, sizeof(a));
    a.fields = s->sga64[0].data();
    a.addr = (n && in->addr) ? s->sga64[1].data() : nullptr;
    a.expect_valid = (n && in->expect_valid) ? s->sga32[0].data() : nullptr;
    a.n = n; a.v_offset = in->v_offset;
    memcpy(a.rand, in->randomness, 32);
    a.rpow = s->sga64[2].data(); a.pk = s->sga64[3].data(); a.status = s->sga32[2].data();
    a.bytes = s->a8b.data(); a.cells = s->sga64[4].data(); a.meta = s->sga32[1].data();
    a.kcand = s->sga64[5].data(); a.keccak = a.kcand + (n + 1) * KT_NCELLS * 4;
    a.scand = s->sga64[6].data(); a.sig_table = a.scand + (n + 1) * SIG_TABLE_WORDS; a.sdup = s->a32[0].data();
    a.aux = s->sga64[7].data();
    a.lanes.lanes_per_sig = 1;
    s->pass = sig_assign_pass;
    s->assign_kind = 9;
    *out = s;
    return 0;
}
extern "C" int zk_sig_assign_read(zk_session* s, const zk_sig_wire* host, uint64_t* n_keccak_out, uint64_t* n_sig_rows_out) {
    ARG_TRY(s && s->assign_kind == 9, "zk_sig_assign_read: bad arguments");
    const SigAssignArgs& a = s->sga;
    if (host) {
        if (host->bytes) memcpy(host->bytes, a.bytes, (size_t)a.n * TX_UNIT_BYTES);
        if (host->cells) memcpy(host->cells, a.cells, (size_t)a.n * TX_UNIT_CELLS * 32);
        if (host->meta) memcpy(host->meta, a.meta, (size_t)a.n * 16);
        if (host->keccak) memcpy(host->keccak, a.keccak, (size_t)s->n_keccak * KT_NCELLS * 32);
        if (host->sig_table) memcpy(host->sig_table, a.sig_table, (size_t)s->n_sig_rows * SIG_TABLE_CELLS * 32);
        if (host->aux) memcpy(host->aux, a.aux, (size_t)a.n * SIG_AUX_CELLS * 32);
    }
    if (n_keccak_out) *n_keccak_out = s->n_keccak;
    if (n_sig_rows_out) *n_sig_rows_out = s->n_sig_rows;
    return 0;
}
extern "C" int zk_sig_assign(const zk_sig_inputs* in, const zk_sig_wire* out, uint32_t opts, uint32_t* status_out, uint64_t* n_keccak_out,
                             uint64_t* n_sig_rows_out, zk_result* result) {
    ARG_TRY(result && out, "zk_sig_assign: null output");
    zk_session* s = nullptr;
    int rc = zk_sig_assign_open(in, nullptr, opts, &s);
    if (rc) return rc;
    rc = zk_launch(s, nullptr);
    if (!rc) rc = zk_collect(s, result);
    if (!rc && status_out) rc = zk_read_status(s, status_out);
    if (!rc) rc = zk_sig_assign_read(s, out, n_keccak_out, n_sig_rows_out);
    zk_close(s);
    return rc;
}

// ---- ECC precompile calls (ecc_calls.hpp): the device functions in host loops
static void ecc_calls_pass(zk_session* s) {
    const EccCallArgs& a = s->ecl;
    const long long np = (long long)(a.n_add + a.n_mul), n = np + (long long)a.n_pairing;
    const long long n_pp = a.n_pairing ? (long long)a.pair_off[a.n_pairing] : 0;
#pragma omp parallel for schedule(dynamic, 16)
    for (long long i = 0; i < np; i++) ecc_call_point(a, (u64)i);
    EccPairArgs pr{};
    pr.a.pair_pts = a.pair_pts;
    pr.pair_flags = a.pair_flags;
    pr.pair_f = a.pair_f;
#pragma omp parallel for schedule(dynamic, 1)
    for (long long t = 0; t < n_pp; t++) ecc_pair_stage1(pr, (u32)t);
#pragma omp parallel for schedule(dynamic, 1)
    for (long long k = 0; k < (long long)a.n_pairing; k++) ecc_call_pairing(a, (u64)k);
    // the ecc table: first occurrences in input order (equal rows are adjacent once sorted by (row, index))
    const u64* tc = a.tcand;
    std::vector<u64> idx((size_t)n);
    for (long long k = 0; k < n; k++) idx[k] = (u64)k;
    std::sort(idx.begin(), idx.end(), [tc](u64 x, u64 y) {
        const int c = memcmp(tc + x * ECL_ROW_WORDS, tc + y * ECL_ROW_WORDS, ECL_ROW_WORDS * 8);
        return c ? c < 0 : x < y;
    });
    for (long long k = 0; k < n; k++) a.tdup[idx[k]] = k && ecl_row_eq(tc + idx[k - 1] * ECL_ROW_WORDS, tc + idx[k] * ECL_ROW_WORDS);
    u64 m = 0;
    for (long long k = 0; k < n; k++)
        if (!a.tdup[k]) memcpy(a.ecc_table + m++ * ECL_ROW_WORDS, tc + (u64)k * ECL_ROW_WORDS, ECL_ROW_WORDS * 8);
    s->n_ecl_table = m;
    std::fill(s->status.begin(), s->status.end(), 0u);
}
extern "C" int zk_ecc_from_calls_open(const zk_ecc_calls* in, const zk_ecc_call_wire* out_dev, uint32_t opts, zk_session** out) {
    NO_DEVICE_PTRS(opts, "zk_ecc_from_calls_open");
    ARG_TRY(in && out && !out_dev, "zk_ecc_from_calls_open: bad arguments (out_dev needs ZK_OPT_DEVICE_PTRS)");
    EccCallArgs a;
    memset(&a, 0, sizeof(a));
    const char* err = nullptr;
    if (int rc = ecc_calls_check(in, a, &err)) { g_err = std::string("zk_ecc_from_calls_open: ") + err; return rc; }
    const u64 np = a.n_add + a.n_mul, n = np + a.n_pairing, n_pp = a.n_pairing ? in->pair_off[a.n_pairing] : 0;
    zk_session* s = new_session(n, false);
    // (the call words are read in place by every pass: the caller's arrays are this backend's resident memory; pair_off is copied)
    s->ecl32[0].assign(a.n_pairing + 1, 0u);
    if (a.n_pairing) memcpy(s->ecl32[0].data(), in->pair_off, (a.n_pairing + 1) * 4);
    s->ecl64[3].assign(np * 24 + 4, 0);
    s->ecl64[4].assign(a.n_pairing * 4 + 4, 0);
    s->ecl64[5].assign(n * ECL_ROW_WORDS, 0);
    s->ecl64[6].assign(n * ECL_ROW_WORDS, 0);
    s->ecl64[7].assign(n * ECL_ROW_WORDS, 0);
    s->ecl64[8].assign(n * ECL_AUX_CELLS * 4, 0);
    s->ecl32[1].assign(n, 0u);
    s->ecl32[2].assign(n, 0u);
    s->ecl32[3].assign(n_pp + 1, 0u);
    s->ecl_f.resize(n_pp + 1);
    a.add_in = in->add_in; a.mul_in = in->mul_in; a.pair_pts = in->pair_pts; a.pair_off = s->ecl32[0].data();
    a.points = s->ecl64[3].data(); a.pair_out = s->ecl64[4].data(); a.rows = s->ecl64[5].data(); a.tcand = s->ecl64[6].data();
    a.ecc_table = s->ecl64[7].data(); a.aux = s->ecl64[8].data(); a.aux_kind = s->ecl32[1].data(); a.tdup = s->ecl32[2].data();
    a.pair_flags = s->ecl32[3].data(); a.pair_f = s->ecl_f.data();
    s->ecl = a;
    s->pass = ecc_calls_pass;
    s->assign_kind = 13;
    *out = s;
    return 0;
}
extern "C" int zk_ecc_from_calls_read(zk_session* s, const zk_ecc_call_wire* host, uint64_t* n_table_rows_out) {
    ARG_TRY(s && s->assign_kind == 13, "zk_ecc_from_calls_read: bad arguments");
    const EccCallArgs& a = s->ecl;
    const u64 np = a.n_add + a.n_mul, n = np + a.n_pairing;
    if (host) {
        if (host->points) memcpy(host->points, a.points, (size_t)np * 192);
        if (host->pair_out) memcpy(host->pair_out, a.pair_out, (size_t)a.n_pairing * 32);
        if (host->rows) memcpy(host->rows, a.rows, (size_t)n * ECL_ROW_WORDS * 8);
        if (host->ecc_table) memcpy(host->ecc_table, a.ecc_table, (size_t)s->n_ecl_table * ECL_ROW_WORDS * 8);
        if (host->aux) memcpy(host->aux, a.aux, (size_t)n * ECL_AUX_CELLS * 32);
        if (host->aux_kind) memcpy(host->aux_kind, a.aux_kind, (size_t)n * 4);
    }
    if (n_table_rows_out) *n_table_rows_out = s->n_ecl_table;
    return 0;
}
extern "C" int zk_ecc_from_calls(const zk_ecc_calls* in, const zk_ecc_call_wire* out, uint32_t opts, uint32_t* status_out,
                                 uint64_t* n_table_rows_out, zk_result* result) {
    ARG_TRY(result && out, "zk_ecc_from_calls: null output");
    zk_session* s = nullptr;
    int rc = zk_ecc_from_calls_open(in, nullptr, opts, &s);
    if (rc) return rc;
    rc = zk_launch(s, nullptr);
    if (!rc) rc = zk_collect(s, result);
    if (!rc && status_out) rc = zk_read_status(s, status_out);
    if (!rc) rc = zk_ecc_from_calls_read(s, out, n_table_rows_out);
    zk_close(s);
    return rc;
}
