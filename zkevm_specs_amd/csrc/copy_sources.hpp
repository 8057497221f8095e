// The Copy assignment's `data` array gathered from the block's raw inputs (zk_copy_assign_from_sources*).
//
// zk_copy_assign takes every source byte of every copy event as `value | is_code << 8`, collected on the host.  Those bytes already sit
// in the arrays the other from-raw entries take: a Bytecode source is a slice of the code set (zk_bytecode_from_code), a TxCalldata
// source a slice of the calldata (zk_evm_tables_from_block / zk_tx_assign), a Memory source the values of the Memory read ops of the
// trace records (zk_evm_witness_from_trace) — the ops CopyCircuit.copy appends to the RW table (typing.py:1122-1131).  Here the array is
// gathered where those inputs are, and the Copy assignment (copy_assign.hpp: cpa_chunk -> cpa_prefix -> cpa_write_row) runs over it
// unchanged: every output is what zk_copy_assign returns for the gathered data.
//
//   cps_byte      source byte i of an event: value | is_code << 8 and the site (4..6) when the byte cannot be gathered (then 0)
//   cps_status    an event's status word from its per-event site (CpsEv::site, the host plan: copy_sources_plan.hpp) and the packed
//                 minimum (i << 8 | site) over its failing bytes
//   is_code       one bit per byte of code, 64-byte chunks per code (a chunk never spans two codes): cps_code_mask_host is the
//                 definition (init_is_code, typing.py:317-324); k_copy_sources.hip computes the same bits from per-chunk counter maps
// The functions here define the results (CPU backend, tests/hostsim); k_copy_sources.hip maps lanes onto them.
#pragma once
#include "copy_assign.hpp"
#include "trace_witness.hpp"  // the head bits of a trace op
#include "bytecode_code.hpp"  // bcc_push_size

enum { CPS_CHUNK = 64,        // bytes per is_code mask word
       CPS_SEG_CHUNKS = 16,   // chunks one wavefront walks in the counter scan (a segment: 1 KiB of code)
       CPS_MAP_STRIDE = 36,   // 33 counters (0..32), padded
       CPS_KIND_VALUE_ERROR = 9,  // ZK_KIND_VALUE_ERROR (include/zkevm_hip.h)
       // sites: per event 1..3, per byte 4..6
       CPS_SITE_REF = 1, CPS_SITE_SRC_END = 2, CPS_SITE_DST_END = 3, CPS_SITE_NO_OP = 4, CPS_SITE_NOT_READ = 5, CPS_SITE_NOT_BYTE = 6,
       CPS_EV_HAS_CODE = 1, CPS_EV_CODE_IS_DST = 2 };
#define CPS_NO_FAIL (~0ull)

// Per-event plumbing of the gather, computed on the host at open from the event cells, the refs and the offsets (integers only)
struct CpsEv {
    u64 src0;    // Bytecode / TxCalldata source: offset of the source's byte 0 in `code` / `calldata`
    u32 chunk0;  // first mask word of the code is_code is read from (CPS_EV_HAS_CODE)
    u32 site;    // 0, or the per-event site 1..3: no byte of the event is gathered
    u32 mode;    // CPS_EV_* bits
    u32 pad;
};
struct CpsArgs {
    const u64* events;      // [n_events][12][4] (cells 0, 1: src_id lo, hi)
    const CpaEvent* ev;     // [n_events] the Copy assignment's plan
    const CpsEv* sev;       // [n_events]
    const u64* data0;       // [n_events + 1] first gathered byte of every event (binary-searched by the byte lanes)
    u64 n_events, n_data;
    const uint8_t* code;    // the caller's code bytes (read by every pass)
    const u64* code_mask;   // [n_chunks] is_code bits of the code set, written by every pass before the gather
    const uint8_t* calldata;
    const u32* head;        // [n_rw] the session's copy of the checked heads
    const u64* ctr;         // [n_rw] ... of the checked counters (null: rw_base + i)
    const u64 *id, *addr, *val;  // [n_rw] the caller's
    u64 n_rw, rw_base;
    uint16_t* data;         // out [n_data]
    unsigned long long* ev_fail;  // [n_events] min over the event's failing bytes of (i << 8 | site), CPS_NO_FAIL: none
};
// the is_code scan's own arguments (device form)
struct CpsCodeArgs {
    const uint8_t* code;
    const u64* offsets;     // [n_codes + 1] the session's copy
    const u32* chunk0;      // [n_codes + 1] first chunk of every code
    const u32* seg0;        // [n_codes + 1] first segment of every code
    u32 n_codes, n_segs;
    u64 n_chunks;
    uint8_t* chunk_in;      // [n_chunks][CPS_MAP_STRIDE]: counter entering the chunk for every counter entering its segment
    uint8_t* seg_map;       // [n_segs][CPS_MAP_STRIDE]: counter after the segment for every counter entering it
    uint8_t* seg_state;     // [n_segs] counter entering the segment
    u64* mask;              // out [n_chunks]
};

// index of the trace op with rw_counter `c`, or n_rw
ZK_HD u64 cps_find_op(const CpsArgs& a, u64 c) {
    if (!a.ctr) return (c >= a.rw_base && c - a.rw_base < a.n_rw) ? c - a.rw_base : a.n_rw;
    u64 lo = 0, hi = a.n_rw;  // first op whose counter is >= c (strictly ascending counters)
    while (lo < hi) {
        const u64 mid = lo + ((hi - lo) >> 1);
        if (a.ctr[mid] < c) lo = mid + 1; else hi = mid;
    }
    return (lo < a.n_rw && a.ctr[lo] == c) ? lo : a.n_rw;
}
// Source byte i < n_real of event ei: value | is_code << 8, site = 0; or 0 with the byte's site (4..6).  An event with a per-event site
// gathers zeros (site stays 0 here: cps_status reports the event's own).
ZK_HD u32 cps_byte(const CpsArgs& a, u64 ei, const CpaEvent& e, const CpsEv& x, u64 i, u32& site) {
    site = 0;
    if (x.site) return 0u;
    u32 value;
    if (e.src_tag == CPA_MEMORY) {
        const u64 stride = (e.dst_tag == CPA_MEMORY || e.dst_tag == CPA_TX_LOG) ? 2 : 1;  // a write op follows each read
        const u64 k = cps_find_op(a, e.rwc + i * stride);
        if (k >= a.n_rw) { site = CPS_SITE_NO_OP; return 0u; }
        // (independent loads: the checks follow them)
        const u32 h = a.head[k];
        const u64 id = a.id[k], addr = a.addr[k], v = a.val[k];
        const u64* sid = a.events + ei * CPA_EV_NCELLS * 4;  // src_id lo, hi
        const bool id_ok = sid[0] == id && (sid[1] | sid[2] | sid[3] | sid[4] | sid[5] | sid[6] | sid[7]) == 0;
        if ((h & TRW_H_WRITE) || ((h >> TRW_H_TAG_SHIFT) & 0xfu) != (u32)CPA_TARGET_MEMORY || (h & TRW_H_ADDR_POOL) || !id_ok || addr != e.src_addr + i) {
            site = CPS_SITE_NOT_READ;
            return 0u;
        }
        if ((h & TRW_H_VALUE_POOL) || v >= 256) { site = CPS_SITE_NOT_BYTE; return 0u; }
        value = (u32)v;
    } else {
        const uint8_t* src = e.src_tag == CPA_BYTECODE ? a.code : a.calldata;  // (the plans reject TxLog and RlcAcc sources)
        value = src[x.src0 + e.src_addr + i];
    }
    u32 is_code = 0;
    if (x.mode & CPS_EV_HAS_CODE) {
        const u64 pos = ((x.mode & CPS_EV_CODE_IS_DST) ? e.dst_addr : e.src_addr) + i;
        is_code = (u32)(a.code_mask[(u64)x.chunk0 + pos / CPS_CHUNK] >> (pos % CPS_CHUNK)) & 1u;
    }
    return value | (is_code << 8);
}
ZK_HD u32 cps_status(const CpsEv& x, unsigned long long fail) {
    const u32 site = x.site ? x.site : (fail != CPS_NO_FAIL ? (u32)(fail & 0xffu) : 0u);
    return site ? (((u32)CPS_KIND_VALUE_ERROR << 24) | site) : 0u;
}

// ---- host forms (CPU backend, hostsim): one event's bytes, and the is_code bits by the reference's recurrence ------------------------
#if defined(ZK_HOSTSIM)
static inline void cps_gather_event(const CpsArgs& a, u64 ei) {
    const CpaEvent& e = a.ev[ei];
    const u64 n_real = a.data0[ei + 1] - a.data0[ei];
    unsigned long long fail = CPS_NO_FAIL;
    for (u64 i = 0; i < n_real; i++) {
        u32 site;
        a.data[a.data0[ei] + i] = (uint16_t)cps_byte(a, ei, e, a.sev[ei], i, site);
        if (site && fail == CPS_NO_FAIL) fail = ((unsigned long long)i << 8) | site;
    }
    a.ev_fail[ei] = fail;
}
// mask[chunk0[j] + b / 64] bit b % 64 = is_code of byte b of code j (init_is_code: the push-data counter restarts per code)
static inline void cps_code_mask_host(const uint8_t* code, const u64* offsets, const u32* chunk0, u64 n_codes, u64* mask) {
    for (u64 j = 0; j < n_codes; j++) {
        const u64 len = offsets[j + 1] - offsets[j];
        u32 left = 0;
        for (u64 b = 0; b < len; b++) {
            u64& w = mask[(u64)chunk0[j] + b / CPS_CHUNK];
            if (b % CPS_CHUNK == 0) w = 0;
            if (left == 0) {
                w |= 1ull << (b % CPS_CHUNK);
                left = bcc_push_size(code[offsets[j] + b]);
            } else {
                left--;
            }
        }
    }
}
#endif
