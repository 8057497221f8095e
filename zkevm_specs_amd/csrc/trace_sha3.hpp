// SHA3 inputs and keccak rows derived from compact trace records (zk_sha3_from_trace*).
//
// The SHA3 gadget (execution/sha3.py) pops offset and size, pushes the digest, reads `size` Memory bytes through its copy lookup at the
// counters rw_counter + 3 + i and looks (size, RLC of those bytes) -> the pushed word up in the keccak table.  A producer of traces so
// far walked its memory image per SHA3 step, concatenated the bytes and uploaded them for zk_keccak_table; the same bytes already sit in
// HBM as the `val` of the Memory read ops behind the step.  Here the messages are gathered where the records are, the keccak table's own
// code (keccak_table.hpp, unchanged) runs over them, and the word the trace pushed is compared with the digest of the bytes it read.
//
//   ts3_operand   op k of a step: the checks of sites 1 and 2 and the op's value as a 256-bit integer
//   ts3_step      a step's open-time status (sites 1..3) and, when it is a message, its record
//   ts3_byte      byte i of a message: its value, or 0 with the byte's site (4..6)
//   ts3_check     a message's status of a pass: the lowest failing byte's site, else site 7 when the pushed word is not the row's digest
// What indexes a load or a store (which steps are messages, their sizes and first counters, the data offsets) is derived at open and kept
// by the session.  The functions here define the results (CPU backend, tests/hostsim); k_trace_sha3.hip maps lanes onto them.
#pragma once
#include "trace_events.hpp"  // TevArgs' record half, tev_find_op, TevWord
#include "keccak_table.hpp"

enum { TS3_KIND_VALUE_ERROR = 9,  // ZK_KIND_VALUE_ERROR (include/zkevm_hip.h)
       TS3_SITE_NO_OP = 1, TS3_SITE_NOT_THE_OP = 2, TS3_SITE_DOMAIN = 3, TS3_SITE_NO_BYTE_OP = 4, TS3_SITE_NOT_READ = 5, TS3_SITE_NOT_BYTE = 6,
       TS3_SITE_DIGEST = 7,
       // the open's verdict block (u64 words) behind the trace witness's: messages, bytes (each message counted up to 2^31), the step
       // that takes the byte total to 2^31
       TS3_V_MSGS = 0, TS3_V_BYTES = 1, TS3_V_CROSS = 2, TS3_V_WORDS = 4 };
#define TS3_NOT_MSG (~0ull)
#define TS3_NO_FAIL (~0ull)
#define TS3_BYTES_LIMIT (1ull << 31)

struct Ts3Msg {  // a message, as the open found it
    u64 call_id, offset, size, rwc;  // rwc: the step's rw_counter (byte i is op 3 + i, the pushed word op 2)
    u32 step, pad;
};
struct Ts3Args {
    TevArgs t;              // the records: head / ctr / off the session's copies, id / addr / val / pool / steps the caller's (code set unused)
    u32* st_open;           // [n_steps] the open-time status of every step
    u64* sz;                // [n_steps] the size of the step's message, TS3_NOT_MSG: the step is none
    u64* blk;               // [2 * blocks of 256 steps] messages / bytes per block, then the messages / bytes in front of the block
    u64* verdict;           // [TS3_V_WORDS]
    Ts3Msg* msg;            // [n_msgs]
    u64* data_off;          // [n_msgs + 1] the session's own offsets: the gather and the keccak table index with these
    u64 n_msgs, n_bytes;
    unsigned long long* fail;  // [n_msgs] per pass: min over the message's failing bytes of (i << 8 | site), TS3_NO_FAIL: none
    uint8_t* data;          // out [n_bytes]
    u64* rows;              // out [n_msgs][5][4]
    u32* step;              // out [n_msgs]
    u64* data_offsets;      // out [n_msgs + 1]
};

ZK_HD u32 ts3_status(u32 site) { return site ? (((u32)TS3_KIND_VALUE_ERROR << 24) | site) : 0u; }
// Op k of a step with counter rwc: a Stack read (write: a Stack write) of call_id at stack address sp + j.  0 and the op's value, or site
// 1 / 2.  The loads of the op stand together, the checks follow them; the three operands of a step do not depend on each other.
ZK_HD u32 ts3_operand(const TevArgs& t, u64 rwc, u32 k, bool write, u64 call_id, u64 sp, u32 j, TevWord& v) {
    v.w[0] = v.w[1] = v.w[2] = v.w[3] = 0;
    const u64 c = rwc + k;
    const u64 i = c < rwc ? t.n_rw : tev_find_op(t, c);  // (a counter past 2^64 is no op's)
    if (i >= t.n_rw) return TS3_SITE_NO_OP;
    const u32 h = t.head[i];
    const u64 id = t.id[i], addr = t.addr[i], val = t.val[i], off = t.off[i];
    const bool ok = ((h & TRW_H_WRITE) != 0) == write && ((h >> TRW_H_TAG_SHIFT) & 0xfu) == (u32)TG_Stack && id == call_id && !(h & TRW_H_ADDR_POOL) &&
                    addr >= sp && addr - sp == j;
    if (!ok) return TS3_SITE_NOT_THE_OP;
    if (h & TRW_H_VALUE_POOL) {  // (the open checks that the heads consume exactly n_pool words; until it has, the index is tested here)
        const u64 pi = off + ((h >> 20) & 1u) + ((h >> 21) & 1u);
        if (pi < t.n_pool) {
            const u64* p = t.pool + 4 * pi;
            v.w[0] = p[0]; v.w[1] = p[1]; v.w[2] = p[2]; v.w[3] = p[3];
        }
    } else {
        v.w[0] = val;
    }
    return 0;
}
// Step s at open: its status (0, or site 1..3).  m.size is the message's size, or TS3_NOT_MSG when the step is no message (another
// state, or a failing step); pushed: the word of op 2.
ZK_HD u32 ts3_step(const Ts3Args& a, u64 s, Ts3Msg& m, TevWord& pushed) {
    m.call_id = m.offset = m.rwc = 0; m.size = TS3_NOT_MSG; m.step = (u32)s; m.pad = 0;
    pushed.w[0] = pushed.w[1] = pushed.w[2] = pushed.w[3] = 0;
    const u64* r = a.t.steps + s * TRW_STEP_WORDS;
    if ((u32)(r[0] & 0xffu) != (u32)ES_SHA3) return 0;
    const u64 rwc = r[1], call_id = r[2], sp = r[4];
    TevWord off, size;
    const u32 s0 = ts3_operand(a.t, rwc, 0, false, call_id, sp, 0, off);
    const u32 s1 = ts3_operand(a.t, rwc, 1, false, call_id, sp, 1, size);
    const u32 s2 = ts3_operand(a.t, rwc, 2, true, call_id, sp, 1, pushed);
    const u32 site = s0 ? s0 : s1 ? s1 : s2;  // (ascending k: the first failure wins)
    if (site) return ts3_status(site);
    bool bad = !tev_fits(size);
    if (!bad && size.w[0] != 0)  // (a size of 0 reads no byte: the offset is not looked at)
        bad = !tev_fits(off) || off.w[0] + size.w[0] >= TEV_LIMIT || rwc >= TEV_LIMIT || rwc + 3 >= TEV_LIMIT;
    if (bad) return ts3_status(TS3_SITE_DOMAIN);
    m.call_id = call_id; m.rwc = rwc; m.size = size.w[0]; m.offset = size.w[0] ? off.w[0] : 0;
    return 0;
}
// what a message adds to the byte total: its size, counted up to 2^31 (no sum over fewer than 2^31 steps wraps)
ZK_HD u64 ts3_counted(u64 size) { return size == TS3_NOT_MSG ? 0 : size < TS3_BYTES_LIMIT ? size : TS3_BYTES_LIMIT; }
// Byte i < m.size of a message: the val of op 3 + i, a Memory read of call_id at offset + i below 256; else 0 and the site
ZK_HD u32 ts3_byte(const Ts3Args& a, const Ts3Msg& m, u64 i, u32& site) {
    site = 0;
    const u64 k = tev_find_op(a.t, m.rwc + 3 + i);  // (the open's site 3: rwc + 3 and the size are below 2^62)
    if (k >= a.t.n_rw) { site = TS3_SITE_NO_BYTE_OP; return 0u; }
    // (independent loads: the checks follow them)
    const u32 h = a.t.head[k];
    const u64 id = a.t.id[k], addr = a.t.addr[k], v = a.t.val[k];
    if ((h & TRW_H_WRITE) || ((h >> TRW_H_TAG_SHIFT) & 0xfu) != (u32)TG_Memory || (h & TRW_H_ADDR_POOL) || id != m.call_id || addr != m.offset + i) {
        site = TS3_SITE_NOT_READ;
        return 0u;
    }
    if ((h & TRW_H_VALUE_POOL) || v >= 256) { site = TS3_SITE_NOT_BYTE; return 0u; }
    return (u32)v;
}
// The word op 2 of a message pushed, as a pass reads it (the op was found and checked at open; its value is the caller's)
ZK_HD TevWord ts3_pushed(const Ts3Args& a, const Ts3Msg& m) {
    TevWord v;
    v.w[0] = v.w[1] = v.w[2] = v.w[3] = 0;
    const u64 i = tev_find_op(a.t, m.rwc + 2);
    if (i >= a.t.n_rw) return v;
    const u32 h = a.t.head[i];
    const u64 val = a.t.val[i], off = a.t.off[i];
    if (h & TRW_H_VALUE_POOL) {
        const u64 pi = off + ((h >> 20) & 1u) + ((h >> 21) & 1u);
        if (pi < a.t.n_pool) {
            const u64* p = a.t.pool + 4 * pi;
            v.w[0] = p[0]; v.w[1] = p[1]; v.w[2] = p[2]; v.w[3] = p[3];
        }
    } else {
        v.w[0] = val;
    }
    return v;
}
// Message mi after the gather and the keccak table of a pass: its status
ZK_HD u32 ts3_check(const Ts3Args& a, u64 mi, unsigned long long fail) {
    if (fail != TS3_NO_FAIL) return ts3_status((u32)(fail & 0xffu));
    const TevWord v = ts3_pushed(a, a.msg[mi]);
    const u64* row = a.rows + mi * (KT_NCELLS * 4);  // cells 3, 4: the digest's low and high 128 bits
    const bool same = row[12] == v.w[0] && row[13] == v.w[1] && row[16] == v.w[2] && row[17] == v.w[3];
    return same ? 0u : ts3_status(TS3_SITE_DIGEST);
}

// ---- the open's verdict (host side of both backends): 0, or the error code with its text in msg -------------------------------------
#define ZK_TS3_ERR_ROWS (-110)   // ZK_ERR_TS3_ROWS, ZK_ERR_TS3_BYTES (include/zkevm_hip.h)
#define ZK_TS3_ERR_BYTES (-111)
static inline int ts3_counts_check(u64 n_rw, u64 n_steps, char* msg, size_t msg_len) {
    if (n_rw < (1ull << 31) && n_steps < (1ull << 31)) return 0;
    snprintf(msg, msg_len, "zk_sha3_from_trace: %llu RW ops, %llu steps (2^31 or more)", (unsigned long long)n_rw, (unsigned long long)n_steps);
    return ZK_TS3_ERR_ROWS;
}
static inline int ts3_bytes_error(u64 cross_step, char* msg, size_t msg_len) {
    snprintf(msg, msg_len, "zk_sha3_from_trace: the message of step %llu takes the hashed bytes to 2^31 or more", (unsigned long long)cross_step);
    return ZK_TS3_ERR_BYTES;
}

// ---- host forms (CPU backend, hostsim): the steps in order ----------------------------------------------------------------------------
#if defined(ZK_HOSTSIM)
// the open's first half: st_open / sz of every step, the verdict's counts and the crossing step
static inline void ts3_count_host(const Ts3Args& a) {
    u64 n_msgs = 0, n_bytes = 0, cross = TS3_NOT_MSG;
    for (u64 s = 0; s < a.t.n_steps; s++) {
        Ts3Msg m;
        TevWord w;
        a.st_open[s] = ts3_step(a, s, m, w);
        a.sz[s] = m.size;
        if (m.size == TS3_NOT_MSG) continue;
        n_msgs++;
        const u64 before = n_bytes;
        n_bytes += ts3_counted(m.size);
        if (before < TS3_BYTES_LIMIT && n_bytes >= TS3_BYTES_LIMIT) cross = s;
    }
    a.verdict[TS3_V_MSGS] = n_msgs; a.verdict[TS3_V_BYTES] = n_bytes; a.verdict[TS3_V_CROSS] = cross;
}
// its second half: the records and the offsets (sizes from sz, the session's own)
static inline void ts3_write_host(const Ts3Args& a) {
    u64 pos = 0, at = 0;
    for (u64 s = 0; s < a.t.n_steps; s++) {
        if (a.sz[s] == TS3_NOT_MSG) continue;
        Ts3Msg m;
        TevWord w;
        (void)ts3_step(a, s, m, w);
        m.size = a.sz[s];
        a.msg[pos] = m;
        a.data_off[pos++] = at;
        at += m.size;
    }
    a.data_off[pos] = at;
}
// a pass: gather, keccak table, check; status per step
static inline void ts3_pass_host(const Ts3Args& a, const KeccakGenArgs& g, u32* status) {
    for (u64 s = 0; s < a.t.n_steps; s++) status[s] = a.st_open[s];
    for (u64 mi = 0; mi < a.n_msgs; mi++) {
        const Ts3Msg& m = a.msg[mi];
        unsigned long long fail = TS3_NO_FAIL;
        for (u64 i = 0; i < m.size; i++) {
            u32 site;
            a.data[a.data_off[mi] + i] = (uint8_t)ts3_byte(a, m, i, site);
            if (site && fail == TS3_NO_FAIL) fail = ((unsigned long long)i << 8) | site;
        }
        a.fail[mi] = fail;
    }
    for (u64 mi = 0; mi < a.n_msgs; mi++) {
        (void)keccak_table_row(g, mi);
        status[a.msg[mi].step] = ts3_check(a, mi, a.fail[mi]);
        a.step[mi] = a.msg[mi].step;
        a.data_offsets[mi] = a.data_off[mi];
    }
    a.data_offsets[a.n_msgs] = a.data_off[a.n_msgs];
}
#endif
