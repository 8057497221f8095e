// Host-side index plumbing of zk_copy_assign_from_sources* (csrc/copy_sources.hpp), shared by the HIP library and the CPU backend: the
// gathered array's offsets from the event cells, the Copy assignment's plan over them, where every event's bytes and is_code bits are
// (from the refs and the offsets), its per-event site, and the chunk / segment tables of the is_code scan.  Integers only.  Included
// after the translation unit has defined ARG_TRY / g_err.
#pragma once
#include <stdio.h>
#include <string>
#include <vector>
#include "copy_assign_plan.hpp"
#include "copy_sources.hpp"

#define ZK_CPS_ERR_OFFSETS (-90)  // ZK_ERR_CPS_OFFSETS, ZK_ERR_CPS_ROWS (include/zkevm_hip.h)
#define ZK_CPS_ERR_ROWS (-91)

struct CpsPlan {
    CpaPlan cpa;
    std::vector<u64> data0;         // [n + 1] running sum of n_real
    std::vector<CpsEv> sev;         // [n]
    std::vector<u32> chunk0, seg0;  // [n_codes + 1]
    u64 n_chunks = 0, n_segs = 0;
    bool any_code = false;          // an event has a Bytecode side: the is_code bits are read
};
// `name:` in front of the text behind the first colon of the current error (the texts are the Copy assignment's / the trace witness's)
static void cps_retitle(const char* name) {
    const std::string cur = g_err;
    const size_t c = cur.find(':');
    g_err = std::string(name) + (c == std::string::npos ? ": " + cur : cur.substr(c));
}
static int cps_offsets_check(const u64* off, u64 n, const char* what, const u64* total) {
    char msg[200];
    if (off[0] != 0) {
        snprintf(msg, sizeof msg, "zk_copy_assign_from_sources: %s[0] is %llu, not 0", what, (unsigned long long)off[0]);
        g_err = msg;
        return ZK_CPS_ERR_OFFSETS;
    }
    for (u64 j = 0; j < n; j++)
        if (off[j + 1] < off[j]) {
            snprintf(msg, sizeof msg, "zk_copy_assign_from_sources: %s decrease at entry %llu", what, (unsigned long long)(j + 1));
            g_err = msg;
            return ZK_CPS_ERR_OFFSETS;
        }
    if (total && off[n] != *total) {
        snprintf(msg, sizeof msg, "zk_copy_assign_from_sources: %s[n_codes] is %llu, n_code_bytes is %llu", what, (unsigned long long)off[n], (unsigned long long)*total);
        g_err = msg;
        return ZK_CPS_ERR_OFFSETS;
    }
    return 0;
}
// code_off / cd_off: host arrays of n_codes + 1 / n_txs + 1 entries (null with no codes / txs); dst_ref nullable
static int cps_plan(const u64* ev_cells, const u32* flags, const u32* src_ref, const u32* dst_ref, u64 n, const u64* code_off, u64 n_codes,
                    u64 n_code_bytes, const u64* cd_off, u64 n_txs, CpsPlan& pl) {
    int rc = 0;
    if (n_codes && (rc = cps_offsets_check(code_off, n_codes, "code_offsets", &n_code_bytes))) return rc;
    if (n_txs && (rc = cps_offsets_check(cd_off, n_txs, "calldata_offsets", nullptr))) return rc;
    ARG_TRY(n_codes || !n_code_bytes, "zk_copy_assign_from_sources: code bytes without a code");
    // The gathered array's offsets: n_real per event (cpa_n_real).  The cells themselves are cpa_plan's to check; errors come in event
    // order, so the walk stops at the first event whose address / length cells cpa_plan will reject, or at the event that takes the
    // array to 2^31 bytes (its row count, twice the lengths, would be cpa_plan's "too many rows" at that event or a later one).
    pl.data0.assign(n + 1, 0);
    u64 n_ok = n;  // events in front of the one with 2^31 bytes
    for (u64 e = 0; e < n; e++) {
        const u64* c = ev_cells + e * CPA_EV_NCELLS * 4;
        const u64 src_addr = c[6 * 4], src_end = c[7 * 4], length = c[9 * 4];
        bool wide = false;
        for (int k : {6, 7, 9}) wide = wide || (c[k * 4 + 1] | c[k * 4 + 2] | c[k * 4 + 3]) != 0 || c[k * 4] >= (1ull << 62);
        if (wide || length >= (1ull << 31)) break;  // (cpa_plan rejects this event, or one before it)
        const u64 room = src_end > src_addr ? src_end - src_addr : 0;
        pl.data0[e + 1] = pl.data0[e] + (room < length ? room : length);
        if (pl.data0[e + 1] >= (1ull << 31)) { n_ok = e; break; }
    }
    if ((rc = cpa_plan(ev_cells, flags, pl.data0.data(), n_ok, pl.cpa))) { cps_retitle("zk_copy_assign_from_sources"); return rc; }
    if (n_ok < n || n_code_bytes >= (1ull << 31) || n_codes >= (1ull << 31) || n_txs >= (1ull << 31)) {
        char msg[200];
        snprintf(msg, sizeof msg, "zk_copy_assign_from_sources: %llu source bytes up to event %llu, %llu code bytes, %llu codes, %llu txs (2^31 or more)",
                 (unsigned long long)pl.data0[n_ok < n ? n_ok + 1 : n], (unsigned long long)(n_ok < n ? n_ok : n - 1), (unsigned long long)n_code_bytes,
                 (unsigned long long)n_codes, (unsigned long long)n_txs);
        g_err = msg;
        return ZK_CPS_ERR_ROWS;
    }
    // the is_code scan's tables: 64-byte chunks per code, segments of CPS_SEG_CHUNKS chunks per code
    pl.chunk0.assign(n_codes + 1, 0);
    pl.seg0.assign(n_codes + 1, 0);
    for (u64 j = 0; j < n_codes; j++) {
        const u64 chunks = (code_off[j + 1] - code_off[j] + CPS_CHUNK - 1) / CPS_CHUNK;
        pl.chunk0[j + 1] = pl.chunk0[j] + (u32)chunks;
        pl.seg0[j + 1] = pl.seg0[j] + (u32)((chunks + CPS_SEG_CHUNKS - 1) / CPS_SEG_CHUNKS);
    }
    pl.n_chunks = pl.chunk0[n_codes];
    pl.n_segs = pl.seg0[n_codes];
    pl.sev.assign(n, CpsEv{0, 0, 0, 0, 0});
    for (u64 e = 0; e < n; e++) {
        const CpaEvent& x = pl.cpa.ev[e];
        CpsEv& s = pl.sev[e];
        const u64 n_real = pl.data0[e + 1] - pl.data0[e];
        ARG_TRY(x.src_tag != CPA_RLC_ACC, "zk_copy_assign_from_sources: RlcAcc is no source of raw bytes");
        const bool src_code = x.src_tag == CPA_BYTECODE, src_cd = x.src_tag == CPA_TX_CALLDATA, dst_code = x.dst_tag == CPA_BYTECODE;
        ARG_TRY(!dst_code || dst_ref, "zk_copy_assign_from_sources: an event writes a code and dst_ref is null");
        // site 1: a ref that is read is out of range
        if ((src_code && src_ref[e] >= n_codes) || (src_cd && src_ref[e] >= n_txs) || (dst_code && dst_ref[e] >= n_codes)) {
            s.site = CPS_SITE_REF;
            continue;
        }
        if (src_code || src_cd) {
            const u64* off = src_code ? code_off : cd_off;
            s.src0 = off[src_ref[e]];
            if (n_real && x.src_end > off[src_ref[e] + 1] - s.src0) s.site = CPS_SITE_SRC_END;  // site 2
        }
        if (dst_code && !s.site && x.dst_addr + n_real > code_off[dst_ref[e] + 1] - code_off[dst_ref[e]]) s.site = CPS_SITE_DST_END;  // site 3
        if (src_code || dst_code) {
            pl.any_code = true;
            s.mode = CPS_EV_HAS_CODE | (src_code ? 0 : CPS_EV_CODE_IS_DST);  // (the source's code when both sides are Bytecode)
            s.chunk0 = pl.chunk0[src_code ? src_ref[e] : dst_ref[e]];
        }
    }
    return 0;
}
