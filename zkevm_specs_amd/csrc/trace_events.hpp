// Copy and EXP events derived from compact trace records (zk_events_from_trace*).
//
// The event lists zk_copy_assign_from_sources / zk_copy_assign / zk_exp_assign take are the arguments of the copy_lookup / exp_lookup
// calls of the reference's gadgets (execution/sha3.py:20, calldatacopy.py:41, codecopy.py:26, extcodecopy.py:39, returndatacopy.py:36,
// log.py:65, exp.py:31).  Every argument is in the trace already: the step record, and the RW ops at fixed offsets behind
// step.rw_counter.  Here a step's event is computed where the records are.
//
//   tev_find_op    index of the RW op with a given counter (dense: counter - rw_base; else binary search), as cps_find_op
//   tev_read       one op a step reads: the checks of sites 1 and 2 and the op's value as a 256-bit integer
//   tev_code_of    a code hash in the session's sorted directory -> the lowest index of that hash in the code set
//   tev_step       a step's status, and its event when it emits one
//   tev_store_*    an event's cells in zk_copy_sources' / zk_exp_events' layout
// The functions here define the results (CPU backend, tests/hostsim); k_trace_events.hip maps lanes onto them.
#pragma once
#include "trace_witness.hpp"
#include "evm_tables.h"

enum { TEV_COPY_NCELLS = 12, TEV_EXP_NCELLS = 5,
       TEV_KIND_VALUE_ERROR = 9, TEV_KIND_UNSUPPORTED = 15,  // ZK_KIND_* (include/zkevm_hip.h)
       TEV_SITE_NO_OP = 1, TEV_SITE_NOT_THE_OP = 2, TEV_SITE_DOMAIN = 3, TEV_SITE_CODE = 4,
       TEV_NONE = 0, TEV_COPY = 1, TEV_EXP = 2,                // what a step emits
       TEV_TAG_BYTECODE = 1, TEV_TAG_MEMORY = 2, TEV_TAG_TX_CALLDATA = 3, TEV_TAG_TX_LOG = 4, TEV_TAG_RLC_ACC = 5,  // CopyDataTypeTag
       TEV_READS = 6,                                          // ops a step reads, at most
       TEV_WANT_STACK = 1, TEV_WANT_CONTEXT = 2, TEV_WANT_ACCOUNT = 3 };
#define TEV_LIMIT (1ull << 62)  // the domain of zk_copy_assign's integer cells
#define TEV_NO_CODE (~0u)
// one op a step reads: k (its counter is step.rw_counter + k) | kind << 4 | field tag << 8; 0: no op.  A stack read's position is k.
#define TEV_RD(k, kind, field) ((uint16_t)((k) | ((kind) << 4) | ((field) << 8)))

struct TevArgs {
    const u32* head;        // [n_rw] the session's copy of the checked heads
    const u64* ctr;         // [n_rw] ... of the checked counters (null: rw_base + i)
    const u64* off;         // [n_rw] ... the pool words consumed by the ops before op i
    const u64 *id, *addr, *val;  // [n_rw] the caller's
    const u64* pool;        // [n_pool][4] the caller's
    const u64* steps;       // [n_steps][13] the caller's
    u64 n_rw, n_pool, n_steps, rw_base;
    const uint8_t* code;    // the caller's code bytes (read for LOG steps: the opcode at pc)
    const u64* code_off;    // [n_codes + 1] the session's copy
    const u64* dir_hash;    // [n_codes][4] the code hashes, ascending as 256-bit integers (equal hashes by ascending index)
    const u32* dir_idx;     // [n_codes] the index in the code set of each entry
    u32 n_codes;
    uint8_t* kind;          // [n_steps] scratch: what each step emits
    u32* blk;               // [2 * blocks of 256 steps] scratch: copy / EXP events per block, then the events in front of the block
    u64* counts;            // [2] n_copy, n_exp of the pass
    u64* copy_events;       // out [n_copy][12][4] (capacity n_steps, like every output)
    u32 *copy_flags, *copy_src_ref, *copy_step;
    u64* exp_events;        // out [n_exp][5][4]
    u32* exp_step;
};
struct TevWord { u64 w[4]; };  // a 256-bit integer, little-endian
struct TevEvent {
    u32 kind;               // TEV_NONE / TEV_COPY / TEV_EXP
    u32 flag, src_ref;      // copy: zk_copy_sources' flags / src_ref
    u32 src_tag, dst_tag;
    TevWord src_id;         // copy: the source id (a code hash, or an integer); EXP: the base
    TevWord exponent;
    u64 dst_id, src_addr, src_end, dst_addr, length, log_id, rwc;  // rwc: the copy event's rw_counter, the EXP event's identifier
};

ZK_HD bool tev_is_zero(const TevWord& x) { return (x.w[0] | x.w[1] | x.w[2] | x.w[3]) == 0; }
ZK_HD bool tev_fits(const TevWord& x) { return (x.w[1] | x.w[2] | x.w[3]) == 0 && x.w[0] < TEV_LIMIT; }
// index of the trace op with rw_counter `c`, or n_rw
ZK_HD u64 tev_find_op(const TevArgs& a, u64 c) {
    if (!a.ctr) return (c >= a.rw_base && c - a.rw_base < a.n_rw) ? c - a.rw_base : a.n_rw;
    u64 lo = 0, hi = a.n_rw;  // first op whose counter is >= c (strictly ascending counters)
    while (lo < hi) {
        const u64 mid = lo + ((hi - lo) >> 1);
        if (a.ctr[mid] < c) lo = mid + 1; else hi = mid;
    }
    return (lo < a.n_rw && a.ctr[lo] == c) ? lo : a.n_rw;
}
// The op described by d (TEV_RD) of a step with counter rwc: 0 and its value, or site 1 / 2.  The loads of an op stand together, the
// checks follow them; the ops of a step do not depend on each other, so their loads overlap.
ZK_HD u32 tev_read(const TevArgs& a, u64 rwc, u32 d, u64 call_id, u64 sp, TevWord& v) {
    v.w[0] = v.w[1] = v.w[2] = v.w[3] = 0;
    const u64 k = d & 15u, c = rwc + k;
    const u32 want = (d >> 4) & 3u, field = d >> 8;
    const u64 i = c < rwc ? a.n_rw : tev_find_op(a, c);  // (a counter past 2^64 is no op's)
    if (i >= a.n_rw) return TEV_SITE_NO_OP;
    const u32 h = a.head[i];
    const u64 id = a.id[i], addr = a.addr[i], val = a.val[i], off = a.off[i];
    const u32 tag = (h >> TRW_H_TAG_SHIFT) & 0xfu;
    bool ok = !(h & TRW_H_WRITE);
    if (want == TEV_WANT_STACK) ok = ok && tag == TG_Stack && id == call_id && !(h & TRW_H_ADDR_POOL) && addr >= sp && addr - sp == k;
    else if (want == TEV_WANT_CONTEXT) ok = ok && tag == TG_CallContext && id == call_id && !(h & TRW_H_ADDR_POOL) && addr == field;
    else ok = ok && tag == TG_Account && ((h >> TRW_H_FIELD_SHIFT) & 0xffu) == field;
    if (!ok) return TEV_SITE_NOT_THE_OP;
    if (h & TRW_H_VALUE_POOL) {  // (the open checked that the heads consume exactly n_pool words: the index is inside the pool)
        const u64* p = a.pool + 4 * (off + ((h >> 20) & 1u) + ((h >> 21) & 1u));
        v.w[0] = p[0]; v.w[1] = p[1]; v.w[2] = p[2]; v.w[3] = p[3];
    } else {
        v.w[0] = val;
    }
    return 0;
}
// the lowest index in the code set of the code with hash h, or TEV_NO_CODE
ZK_HD u32 tev_code_of(const TevArgs& a, const TevWord& h) {
    u32 lo = 0, hi = a.n_codes;  // first entry whose hash is >= h
    while (lo < hi) {
        const u32 mid = lo + ((hi - lo) >> 1);
        const u64* m = a.dir_hash + 4 * (u64)mid;
        const u64 m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3];
        const bool less = m3 != h.w[3] ? m3 < h.w[3] : m2 != h.w[2] ? m2 < h.w[2] : m1 != h.w[1] ? m1 < h.w[1] : m0 < h.w[0];  // m < h
        if (less) lo = mid + 1; else hi = mid;
    }
    if (lo >= a.n_codes) return TEV_NO_CODE;
    const u64* m = a.dir_hash + 4 * (u64)lo;
    return (m[0] == h.w[0] && m[1] == h.w[1] && m[2] == h.w[2] && m[3] == h.w[3]) ? a.dir_idx[lo] : TEV_NO_CODE;
}
ZK_HD u32 tev_status(u32 site) { return ((u32)TEV_KIND_VALUE_ERROR << 24) | site; }

// Step s: its status; e.kind says what it emits (TEV_NONE with a non-zero status) and e holds that event.
ZK_HD u32 tev_step(const TevArgs& a, u64 s, TevEvent& e) {
    e.kind = TEV_NONE;
    const u64* r = a.steps + s * TRW_STEP_WORDS;
    const u64 w0 = r[0];
    const u32 state = (u32)(w0 & 0xffu);
    const bool root = (w0 >> 8) & 1u;
    // the ops the state reads, in ascending k
    uint16_t rd[TEV_READS] = {0, 0, 0, 0, 0, 0};
    switch (state) {
    case ES_BeginTx: case ES_RETURN: case ES_CREATE: case ES_CREATE2: case ES_CALL_OP: case ES_DATACOPY:
        return ((u32)TEV_KIND_UNSUPPORTED << 24) | 1u;  // their events are the caller's to supply
    case ES_SHA3: case ES_EXP:
        rd[0] = TEV_RD(0, TEV_WANT_STACK, 0); rd[1] = TEV_RD(1, TEV_WANT_STACK, 0);
        break;
    case ES_CALLDATACOPY:
        rd[0] = TEV_RD(0, TEV_WANT_STACK, 0); rd[1] = TEV_RD(1, TEV_WANT_STACK, 0); rd[2] = TEV_RD(2, TEV_WANT_STACK, 0);
        rd[3] = root ? TEV_RD(3, TEV_WANT_CONTEXT, CC_TxId) : TEV_RD(3, TEV_WANT_CONTEXT, CC_CallerId);
        rd[4] = TEV_RD(4, TEV_WANT_CONTEXT, CC_CallDataLength);
        if (!root) rd[5] = TEV_RD(5, TEV_WANT_CONTEXT, CC_CallDataOffset);
        break;
    case ES_CODECOPY:
        rd[0] = TEV_RD(0, TEV_WANT_STACK, 0); rd[1] = TEV_RD(1, TEV_WANT_STACK, 0); rd[2] = TEV_RD(2, TEV_WANT_STACK, 0);
        break;
    case ES_EXTCODECOPY:
        rd[0] = TEV_RD(1, TEV_WANT_STACK, 0); rd[1] = TEV_RD(2, TEV_WANT_STACK, 0); rd[2] = TEV_RD(3, TEV_WANT_STACK, 0);
        rd[3] = TEV_RD(8, TEV_WANT_ACCOUNT, ACC_CodeHash);
        break;
    case ES_RETURNDATACOPY:
        rd[0] = TEV_RD(0, TEV_WANT_STACK, 0); rd[1] = TEV_RD(2, TEV_WANT_STACK, 0);
        rd[2] = TEV_RD(3, TEV_WANT_CONTEXT, CC_LastCalleeId); rd[3] = TEV_RD(5, TEV_WANT_CONTEXT, CC_LastCalleeReturnDataOffset);
        break;
    case ES_LOG:
        rd[0] = TEV_RD(0, TEV_WANT_STACK, 0); rd[1] = TEV_RD(1, TEV_WANT_STACK, 0);
        rd[2] = TEV_RD(2, TEV_WANT_CONTEXT, CC_TxId); rd[3] = TEV_RD(5, TEV_WANT_CONTEXT, CC_IsPersistent);
        break;
    default:
        return 0;
    }
    const u64 rwc = r[1], call_id = r[2], pc = r[3], sp = r[4], log_id = r[8];
    TevWord hash;
    hash.w[0] = r[9]; hash.w[1] = r[10]; hash.w[2] = r[11]; hash.w[3] = r[12];
    TevWord v[TEV_READS];
    u32 site = 0;
#pragma unroll
    for (int q = 0; q < TEV_READS; q++) {
        u32 sq = 0;
        if (rd[q]) sq = tev_read(a, rwc, rd[q], call_id, sp, v[q]);
        else v[q].w[0] = v[q].w[1] = v[q].w[2] = v[q].w[3] = 0;
        if (!site) site = sq;  // (ascending k: the first failure wins)
    }
    if (site) return tev_status(site);
    // the event: `bad` collects site 3 over the operands and their sums (each addend below 2^62: no sum wraps)
    e.flag = 0; e.src_ref = 0; e.src_tag = 0; e.dst_tag = 0; e.log_id = 0; e.dst_id = call_id;
    e.src_addr = 0; e.src_end = 0; e.dst_addr = 0; e.length = 0; e.rwc = 0;
    e.src_id.w[0] = call_id; e.src_id.w[1] = e.src_id.w[2] = e.src_id.w[3] = 0;
    e.exponent = v[1];
    bool bad = rwc >= TEV_LIMIT;
    u32 code_site = 0;
    u64 k_rwc = 0;
    switch (state) {
    case ES_SHA3:
        if (tev_is_zero(v[1])) return 0;
        bad = bad || !tev_fits(v[0]) || !tev_fits(v[1]);
        e.src_tag = TEV_TAG_MEMORY; e.dst_tag = TEV_TAG_RLC_ACC;
        e.src_addr = v[0].w[0]; e.src_end = v[0].w[0] + v[1].w[0]; e.length = v[1].w[0];
        k_rwc = 3;
        break;
    case ES_CALLDATACOPY: {
        if (tev_is_zero(v[2])) return 0;
        bad = bad || !tev_fits(v[0]) || !tev_fits(v[1]) || !tev_fits(v[2]) || !tev_fits(v[3]) || !tev_fits(v[4]) || !tev_fits(v[5]);
        const u64 cdo = v[5].w[0];  // (0 in a root call: nothing is read there)
        if (root) {  // the tx's calldata: src_ref is the tx's index
            bad = bad || v[3].w[0] == 0 || v[3].w[0] - 1 > 0xffffffffull;
            e.src_ref = (u32)(v[3].w[0] - 1);
        }
        e.src_id = v[3];
        e.src_tag = root ? TEV_TAG_TX_CALLDATA : TEV_TAG_MEMORY; e.dst_tag = TEV_TAG_MEMORY;
        e.src_addr = cdo + v[1].w[0]; e.src_end = cdo + v[4].w[0]; e.dst_addr = v[0].w[0]; e.length = v[2].w[0];
        k_rwc = root ? 5 : 6;
        break;
    }
    case ES_CODECOPY: case ES_EXTCODECOPY: {
        if (tev_is_zero(v[2])) return 0;
        bad = bad || !tev_fits(v[0]) || !tev_fits(v[1]) || !tev_fits(v[2]);
        const bool ext = state == ES_EXTCODECOPY;
        e.src_id = ext ? v[3] : hash;
        e.flag = 1;  // the source id is a Word
        e.src_tag = TEV_TAG_BYTECODE; e.dst_tag = TEV_TAG_MEMORY;
        e.src_addr = v[1].w[0]; e.src_end = 0; e.dst_addr = v[0].w[0]; e.length = v[2].w[0];
        k_rwc = ext ? 9 : 3;
        if (!bad && !(ext && tev_is_zero(e.src_id))) {  // (a zero hash: an account without code, no byte is read)
            const u32 j = tev_code_of(a, e.src_id);
            if (j == TEV_NO_CODE) code_site = TEV_SITE_CODE;
            else { e.src_ref = j; e.src_end = a.code_off[j + 1] - a.code_off[j]; }
        }
        break;
    }
    case ES_RETURNDATACOPY:
        bad = bad || !tev_fits(v[0]) || !tev_fits(v[1]) || !tev_fits(v[2]) || !tev_fits(v[3]);
        e.src_id = v[2];
        e.src_tag = TEV_TAG_MEMORY; e.dst_tag = TEV_TAG_MEMORY;
        e.src_addr = v[3].w[0]; e.src_end = v[3].w[0] + v[1].w[0]; e.dst_addr = v[0].w[0]; e.length = v[1].w[0];
        k_rwc = 6;
        break;
    case ES_LOG: {
        if (tev_is_zero(v[1]) || v[3].w[0] != 1 || (v[3].w[1] | v[3].w[2] | v[3].w[3]) != 0) return 0;
        bad = bad || !tev_fits(v[0]) || !tev_fits(v[1]) || !tev_fits(v[2]) || log_id >= TEV_LIMIT - 1;
        e.dst_id = v[2].w[0];
        e.src_tag = TEV_TAG_MEMORY; e.dst_tag = TEV_TAG_TX_LOG;
        e.src_addr = v[0].w[0]; e.src_end = v[0].w[0] + v[1].w[0]; e.length = v[1].w[0]; e.log_id = log_id + 1;
        // the topic count is the opcode's: byte pc of the step's code (with site 4 the counter is taken without topics)
        u64 topics = 0;
        const u32 j = bad ? TEV_NO_CODE : tev_code_of(a, hash);
        if (!bad) {
            code_site = TEV_SITE_CODE;
            if (j != TEV_NO_CODE && pc < a.code_off[j + 1] - a.code_off[j]) {
                const u32 op = a.code[a.code_off[j] + pc];
                if (op >= OP_LOG0 && op <= OP_LOG4) { code_site = 0; topics = op - OP_LOG0; }
            }
        }
        k_rwc = 7 + 2 * topics;
        break;
    }
    default:  // ES_EXP
        if ((v[1].w[1] | v[1].w[2] | v[1].w[3]) == 0 && v[1].w[0] <= 1) return 0;
        e.src_id = v[0];
        k_rwc = 3;
        break;
    }
    bad = bad || e.src_addr >= TEV_LIMIT || e.src_end >= TEV_LIMIT || rwc + k_rwc >= TEV_LIMIT;
    if (bad) return tev_status(TEV_SITE_DOMAIN);
    if (code_site) return tev_status(code_site);
    e.rwc = rwc + k_rwc;
    e.kind = state == ES_EXP ? TEV_EXP : TEV_COPY;
    return 0;
}

// the event's cells: zk_copy_sources' events / flags / src_ref at `pos`, with the step that produced it
ZK_HD void tev_store_copy(const TevArgs& a, u64 pos, u64 s, const TevEvent& e) {
    u64* c = a.copy_events + pos * TEV_COPY_NCELLS * 4;
    const u64 cell[TEV_COPY_NCELLS][2] = {{e.src_id.w[0], e.src_id.w[1]}, {e.src_id.w[2], e.src_id.w[3]}, {e.src_tag, 0}, {e.dst_id, 0}, {0, 0},
                                          {e.dst_tag, 0}, {e.src_addr, 0}, {e.src_end, 0}, {e.dst_addr, 0}, {e.length, 0}, {e.log_id, 0}, {e.rwc, 0}};
#pragma unroll
    for (int q = 0; q < TEV_COPY_NCELLS; q++) { c[4 * q] = cell[q][0]; c[4 * q + 1] = cell[q][1]; c[4 * q + 2] = 0; c[4 * q + 3] = 0; }
    a.copy_flags[pos] = e.flag;
    a.copy_src_ref[pos] = e.src_ref;
    a.copy_step[pos] = (u32)s;
}
// zk_exp_events' row: identifier, base lo, hi, exponent lo, hi
ZK_HD void tev_store_exp(const TevArgs& a, u64 pos, u64 s, const TevEvent& e) {
    u64* c = a.exp_events + pos * TEV_EXP_NCELLS * 4;
    const u64 cell[TEV_EXP_NCELLS][2] = {{e.rwc, 0}, {e.src_id.w[0], e.src_id.w[1]}, {e.src_id.w[2], e.src_id.w[3]}, {e.exponent.w[0], e.exponent.w[1]},
                                         {e.exponent.w[2], e.exponent.w[3]}};
#pragma unroll
    for (int q = 0; q < TEV_EXP_NCELLS; q++) { c[4 * q] = cell[q][0]; c[4 * q + 1] = cell[q][1]; c[4 * q + 2] = 0; c[4 * q + 3] = 0; }
    a.exp_step[pos] = (u32)s;
}

// ---- the wider entry (zk_events_from_trace_ext*): BeginTx, RETURN / REVERT and DATACOPY derived too -----------------------------------
// Their gadgets (begin_tx.py:147-177, return_revert.py:54-93, dataCopy.py:38-61) look up 0, 1 or 2 events per step, read ops up to
// k = 22 under a call id that is not always the step's, read an Account WRITE, and write a code (a Word destination with a dst_ref).
//   tevx_read      one op of such a step: the counter offset, the stack position and the call id are arguments of their own
//   tevx_step      a step's status and its 0, 1 or 2 copy events (or its EXP event); every state tev_step derives goes through tev_step
//   tevx_store_copy  tev_store_copy with a 256-bit destination id and the dst_ref
enum { TEV_SITE_EXT = 5, TEV_FLAG_SRC_WORD = 1, TEV_FLAG_DST_WORD = 2, TEV_STEP_CREATE_BIT = 9, TEVX_BEGIN_TX_OPS = 23, TEVX_BEGIN_TX_COPY = 10 };
struct TevxArgs {
    TevArgs t;              // (t.blk: [2 * blocks of 256 steps] copy EVENTS / EXP events per block, then the events in front of the block)
    u32* copy_dst_ref;      // out [n_copy]
    u64 cap_copy;           // the capacity of the copy outputs: n_steps + the BeginTx and DATACOPY steps counted at open (EXP: n_steps)
};
struct TevxEvent {
    TevEvent e;
    TevWord dst;            // the destination id (e.dst_id is not read)
    u32 dst_ref;
};

// Op k of a step with counter rwc: a read (or, with `write`, a write) of `want`; a Stack / CallContext op has id == id, a Stack op the
// address sp + pos, a CallContext / Account op the field `pos`.  0 and the value, or site 1 / 2.
ZK_HD u32 tevx_read(const TevArgs& a, u64 rwc, u32 k, u32 want, bool write, u64 id, u64 sp, u32 pos, TevWord& v) {
    v.w[0] = v.w[1] = v.w[2] = v.w[3] = 0;
    const u64 c = rwc + k;
    const u64 i = c < rwc ? a.n_rw : tev_find_op(a, c);
    if (i >= a.n_rw) return TEV_SITE_NO_OP;
    const u32 h = a.head[i];
    const u64 oid = a.id[i], addr = a.addr[i], val = a.val[i], off = a.off[i];
    const u32 tag = (h >> TRW_H_TAG_SHIFT) & 0xfu;
    bool ok = ((h & TRW_H_WRITE) != 0) == write;
    if (want == TEV_WANT_STACK) ok = ok && tag == TG_Stack && oid == id && !(h & TRW_H_ADDR_POOL) && addr >= sp && addr - sp == pos;
    else if (want == TEV_WANT_CONTEXT) ok = ok && tag == TG_CallContext && oid == id && !(h & TRW_H_ADDR_POOL) && addr == pos;
    else ok = ok && tag == TG_Account && ((h >> TRW_H_FIELD_SHIFT) & 0xffu) == pos;
    if (!ok) return TEV_SITE_NOT_THE_OP;
    if (h & TRW_H_VALUE_POOL) {
        const u64* p = a.pool + 4 * (off + ((h >> 20) & 1u) + ((h >> 21) & 1u));
        v.w[0] = p[0]; v.w[1] = p[1]; v.w[2] = p[2]; v.w[3] = p[3];
    } else {
        v.w[0] = val;
    }
    return 0;
}
ZK_HD void tevx_clear(TevxEvent& x, u64 call_id) {
    TevEvent& e = x.e;
    e.kind = TEV_NONE; e.flag = 0; e.src_ref = 0; e.src_tag = TEV_TAG_MEMORY; e.dst_tag = TEV_TAG_MEMORY; e.log_id = 0; e.dst_id = 0;
    e.src_addr = 0; e.src_end = 0; e.dst_addr = 0; e.length = 0; e.rwc = 0;
    e.src_id.w[0] = call_id; e.src_id.w[1] = e.src_id.w[2] = e.src_id.w[3] = 0;
    e.exponent.w[0] = e.exponent.w[1] = e.exponent.w[2] = e.exponent.w[3] = 0;
    x.dst.w[0] = x.dst.w[1] = x.dst.w[2] = x.dst.w[3] = 0;
    x.dst_ref = 0;
}
// Step s: its status; x[0], x[1]: its events in the gadget's lookup order (x[1].e.kind != TEV_NONE only behind a copy event in x[0]).
// A failing step emits nothing.
ZK_HD u32 tevx_step(const TevArgs& a, u64 s, TevxEvent (&x)[2]) {
    const u64* r = a.steps + s * TRW_STEP_WORDS;
    const u64 w0 = r[0];
    const u32 state = (u32)(w0 & 0xffu);
    const u64 rwc = r[1], call_id = r[2], sp = r[4];
    tevx_clear(x[0], call_id);
    tevx_clear(x[1], call_id);
    if (state != ES_BeginTx && state != ES_RETURN && state != ES_DATACOPY) {  // (CREATE, CREATE2 and CALL_OP stay unsupported there)
        const u32 st = tev_step(a, s, x[0].e);
        x[0].dst.w[0] = x[0].e.dst_id;
        return st;
    }
    const bool root = (w0 >> 8) & 1u, create = (w0 >> TEV_STEP_CREATE_BIT) & 1u;
    const bool last = s + 1 >= a.n_steps;
    const u64* nx = a.steps + (last ? s : s + 1) * TRW_STEP_WORDS;  // (the last step: never used)
    TevWord v[TEV_READS];
#pragma unroll
    for (int q = 0; q < TEV_READS; q++) v[q].w[0] = v[q].w[1] = v[q].w[2] = v[q].w[3] = 0;
    u32 site = 0, sq;
    bool bad = rwc >= TEV_LIMIT;
    if (state == ES_RETURN) {
        if (root && !create) return 0;
        if (!create && last) return tev_status(TEV_SITE_EXT);
        sq = tevx_read(a, rwc, 1, TEV_WANT_STACK, false, call_id, sp, 0, v[0]); if (!site) site = sq;
        sq = tevx_read(a, rwc, 2, TEV_WANT_STACK, false, call_id, sp, 1, v[1]); if (!site) site = sq;
        if (create) {
            sq = tevx_read(a, rwc, 4, TEV_WANT_ACCOUNT, true, 0, 0, ACC_CodeHash, v[2]); if (!site) site = sq;
        } else {
            sq = tevx_read(a, rwc, 3, TEV_WANT_CONTEXT, false, call_id, 0, CC_ReturnDataOffset, v[2]); if (!site) site = sq;
            sq = tevx_read(a, rwc, 4, TEV_WANT_CONTEXT, false, call_id, 0, CC_ReturnDataLength, v[3]); if (!site) site = sq;
        }
        if (site) return tev_status(site);
        if (create && tev_is_zero(v[1])) return 0;
        bad = bad || !tev_fits(v[0]) || !tev_fits(v[1]) || (!create && (!tev_fits(v[2]) || !tev_fits(v[3])));
        TevEvent& e = x[0].e;
        e.src_addr = v[0].w[0]; e.src_end = v[0].w[0] + v[1].w[0];
        bad = bad || e.src_end >= TEV_LIMIT || rwc + 5 >= TEV_LIMIT;
        if (bad) return tev_status(TEV_SITE_DOMAIN);
        e.rwc = rwc + 5;
        if (create) {  // the deployed code: Memory -> the written code hash
            const u32 j = tev_code_of(a, v[2]);
            if (j == TEV_NO_CODE) return tev_status(TEV_SITE_CODE);
            e.flag = TEV_FLAG_DST_WORD; e.dst_tag = TEV_TAG_BYTECODE; e.length = v[1].w[0];
            x[0].dst = v[2]; x[0].dst_ref = j;
        } else {       // the return data: Memory -> the caller's Memory
            e.dst_addr = v[2].w[0]; e.length = v[1].w[0] < v[3].w[0] ? v[1].w[0] : v[3].w[0];
            x[0].dst.w[0] = nx[2];
        }
        e.kind = TEV_COPY;
        return 0;
    }
    if (state == ES_DATACOPY) {
        const u32 field[5] = {CC_CallerId, CC_CallDataOffset, CC_CallDataLength, CC_ReturnDataOffset, CC_ReturnDataLength};
#pragma unroll
        for (int q = 0; q < 5; q++) {
            sq = tevx_read(a, rwc, (u32)q + 1, TEV_WANT_CONTEXT, false, call_id, 0, field[q], v[q]); if (!site) site = sq;
        }
        if (site) return tev_status(site);
#pragma unroll
        for (int q = 0; q < 5; q++) bad = bad || !tev_fits(v[q]);
        const u64 c = v[0].w[0], cdo = v[1].w[0], cdl = v[2].w[0], rdo = v[3].w[0], rdl = v[4].w[0];
        const u64 len0 = rdo + rdl;                          // (the reference passes rdo + rdl as the first event's length)
        const u64 inc = len0 + (len0 < cdl ? len0 : cdl);    // its writes, and its reads below src_addr_end
        bad = bad || cdo + cdl >= TEV_LIMIT || len0 >= TEV_LIMIT || rwc + 6 + inc >= TEV_LIMIT;
        if (bad) return tev_status(TEV_SITE_DOMAIN);
#pragma unroll
        for (int q = 0; q < 2; q++) {
            TevEvent& e = x[q].e;
            e.src_id.w[0] = c; e.src_addr = cdo; e.src_end = cdo + cdl;
            e.kind = TEV_COPY;
        }
        x[0].dst.w[0] = c; x[0].e.dst_addr = rdo; x[0].e.length = len0; x[0].e.rwc = rwc + 6;
        x[1].dst.w[0] = call_id; x[1].e.length = rdl; x[1].e.rwc = rwc + 6 + inc;
        return 0;
    }
    // BeginTx: the create path with init code, told from the successor
    if (last) return tev_status(TEV_SITE_EXT);
    if (!((nx[0] >> TEV_STEP_CREATE_BIT) & 1u) || nx[1] < rwc || nx[1] - rwc != TEVX_BEGIN_TX_OPS) return 0;
    sq = tevx_read(a, rwc, 0, TEV_WANT_CONTEXT, false, rwc, 0, CC_TxId, v[0]); if (!site) site = sq;
    sq = tevx_read(a, rwc, 14, TEV_WANT_CONTEXT, false, rwc, 0, CC_CallDataLength, v[1]); if (!site) site = sq;
    sq = tevx_read(a, rwc, 22, TEV_WANT_CONTEXT, false, rwc, 0, CC_CodeHash, v[2]); if (!site) site = sq;
    if (site) return tev_status(site);
    if (tev_is_zero(v[1])) return tev_status(TEV_SITE_EXT);  // (that path needs calldata: begin_tx.py:130)
    bad = bad || !tev_fits(v[0]) || !tev_fits(v[1]) || v[0].w[0] == 0 || v[0].w[0] - 1 > 0xffffffffull || rwc + TEVX_BEGIN_TX_COPY >= TEV_LIMIT;
    if (bad) return tev_status(TEV_SITE_DOMAIN);
    const u32 j = tev_code_of(a, v[2]);
    if (j == TEV_NO_CODE) return tev_status(TEV_SITE_CODE);
#pragma unroll
    for (int q = 0; q < 2; q++) {
        TevEvent& e = x[q].e;
        e.src_id = v[0]; e.src_tag = TEV_TAG_TX_CALLDATA; e.src_ref = (u32)(v[0].w[0] - 1);
        e.src_end = v[1].w[0]; e.length = v[1].w[0]; e.rwc = rwc + TEVX_BEGIN_TX_COPY;
        e.kind = TEV_COPY;
    }
    x[0].e.dst_tag = TEV_TAG_RLC_ACC; x[0].dst.w[0] = rwc;
    x[1].e.dst_tag = TEV_TAG_BYTECODE; x[1].e.flag = TEV_FLAG_DST_WORD; x[1].dst = v[2]; x[1].dst_ref = j;
    return 0;
}
ZK_HD void tevx_store_copy(const TevxArgs& ax, u64 pos, u64 s, const TevxEvent& x) {
    const TevArgs& a = ax.t;
    const TevEvent& e = x.e;
    u64* c = a.copy_events + pos * TEV_COPY_NCELLS * 4;
    const u64 cell[TEV_COPY_NCELLS][2] = {{e.src_id.w[0], e.src_id.w[1]}, {e.src_id.w[2], e.src_id.w[3]}, {e.src_tag, 0}, {x.dst.w[0], x.dst.w[1]},
                                          {x.dst.w[2], x.dst.w[3]}, {e.dst_tag, 0}, {e.src_addr, 0}, {e.src_end, 0}, {e.dst_addr, 0}, {e.length, 0},
                                          {e.log_id, 0}, {e.rwc, 0}};
#pragma unroll
    for (int q = 0; q < TEV_COPY_NCELLS; q++) { c[4 * q] = cell[q][0]; c[4 * q + 1] = cell[q][1]; c[4 * q + 2] = 0; c[4 * q + 3] = 0; }
    a.copy_flags[pos] = e.flag;
    a.copy_src_ref[pos] = e.src_ref;
    ax.copy_dst_ref[pos] = x.dst_ref;
    a.copy_step[pos] = (u32)s;
}
// a step of one of the two states that may emit two events: what the copy capacity counts
ZK_HD u32 tevx_is_pair_state(u64 w0) { return (u32)(w0 & 0xffu) == ES_BeginTx || (u32)(w0 & 0xffu) == ES_DATACOPY; }

// ---- host form (CPU backend, hostsim): the steps in order, the events packed as they come -------------------------------------------
#if defined(ZK_HOSTSIM)
static inline void tevx_pass_host(const TevxArgs& ax, u32* status) {
    const TevArgs& a = ax.t;
    u64 n_copy = 0, n_exp = 0;
    for (u64 s = 0; s < a.n_steps; s++) {
        TevxEvent x[2];
        u32 st = tevx_step(a, s, x);
        const u32 k0 = x[0].e.kind, n = k0 == TEV_COPY ? (x[1].e.kind == TEV_COPY ? 2u : 1u) : 0u;
        if (n_copy + n > ax.cap_copy) st = tev_status(TEV_SITE_EXT);  // (records rewritten under the session; nothing is emitted)
        else if (k0 == TEV_EXP) tev_store_exp(a, n_exp++, s, x[0].e);
        else for (u32 q = 0; q < n; q++) tevx_store_copy(ax, n_copy++, s, x[q]);
        status[s] = st;
    }
    a.counts[0] = n_copy;
    a.counts[1] = n_exp;
}
static inline void tev_pass_host(const TevArgs& a, u32* status) {
    u64 n_copy = 0, n_exp = 0;
    for (u64 s = 0; s < a.n_steps; s++) {
        TevEvent e;
        status[s] = tev_step(a, s, e);
        if (e.kind == TEV_COPY) tev_store_copy(a, n_copy++, s, e);
        else if (e.kind == TEV_EXP) tev_store_exp(a, n_exp++, s, e);
    }
    a.counts[0] = n_copy;
    a.counts[1] = n_exp;
}
#endif
