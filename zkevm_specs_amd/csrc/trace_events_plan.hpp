// Host side of zk_events_from_trace* (csrc/trace_events.hpp), shared by the HIP library and the CPU backend: the counts and the code
// offsets checked, the directory of the code hashes sorted.  Integers only.  Included after the translation unit has defined ARG_TRY /
// g_err (and after copy_sources_plan.hpp, whose cps_retitle puts this entry's name in front of the trace witness's error texts).
#pragma once
#include <stdio.h>
#include <algorithm>
#include <vector>
#include "copy_sources_plan.hpp"
#include "trace_events.hpp"

#define ZK_TEV_ERR_OFFSETS (-100)  // ZK_ERR_TEV_OFFSETS, ZK_ERR_TEV_ROWS (include/zkevm_hip.h)
#define ZK_TEV_ERR_ROWS (-101)

struct TevPlan {
    std::vector<u64> dir_hash;  // [n_codes][4] ascending
    std::vector<u32> dir_idx;   // [n_codes]
};
// the counts that need no array, before anything is read or allocated
static int tev_counts_check(u64 n_steps, u64 n_code_bytes, u64 n_codes) {
    if (n_steps >= (1ull << 31) || n_code_bytes >= (1ull << 31) || n_codes >= (1ull << 31)) {
        char msg[200];
        snprintf(msg, sizeof msg, "zk_events_from_trace: %llu steps, %llu code bytes, %llu codes (2^31 or more)", (unsigned long long)n_steps,
                 (unsigned long long)n_code_bytes, (unsigned long long)n_codes);
        g_err = msg;
        return ZK_TEV_ERR_ROWS;
    }
    ARG_TRY(n_codes || !n_code_bytes, "zk_events_from_trace: code bytes without a code");
    return 0;
}
// off: a host array of n_codes + 1 entries (not read with no codes)
static int tev_offsets_check(const u64* off, u64 n_codes, u64 n_code_bytes) {
    if (!n_codes) return 0;
    char msg[200];
    msg[0] = 0;
    if (off[0] != 0) snprintf(msg, sizeof msg, "zk_events_from_trace: code_offsets[0] is %llu, not 0", (unsigned long long)off[0]);
    for (u64 j = 0; j < n_codes && !msg[0]; j++)
        if (off[j + 1] < off[j]) snprintf(msg, sizeof msg, "zk_events_from_trace: code_offsets decrease at entry %llu", (unsigned long long)(j + 1));
    if (!msg[0] && off[n_codes] != n_code_bytes)
        snprintf(msg, sizeof msg, "zk_events_from_trace: code_offsets[n_codes] is %llu, n_code_bytes is %llu", (unsigned long long)off[n_codes],
                 (unsigned long long)n_code_bytes);
    if (!msg[0]) return 0;
    g_err = msg;
    return ZK_TEV_ERR_OFFSETS;
}
// hashes: a host array uint64[n_codes][4].  Sorted by (hash as a 256-bit integer, index): of equal hashes the lowest index comes first, and
// tev_code_of's lower bound finds it.
static void tev_dir_build(const u64* hashes, u64 n_codes, TevPlan& pl) {
    pl.dir_idx.resize(n_codes);
    for (u64 j = 0; j < n_codes; j++) pl.dir_idx[j] = (u32)j;
    std::sort(pl.dir_idx.begin(), pl.dir_idx.end(), [&](u32 x, u32 y) {
        const u64 *p = hashes + 4 * (u64)x, *q = hashes + 4 * (u64)y;
        for (int k = 3; k >= 0; k--)
            if (p[k] != q[k]) return p[k] < q[k];
        return x < y;
    });
    pl.dir_hash.resize(n_codes * 4);
    for (u64 j = 0; j < n_codes; j++)
        for (int k = 0; k < 4; k++) pl.dir_hash[4 * j + k] = hashes[4 * (u64)pl.dir_idx[j] + k];
}
