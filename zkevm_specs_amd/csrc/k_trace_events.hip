// Copy and EXP events from compact trace records (trace_events.hpp): a lane per step, the packed ordered lists by a count pass, a scan of
// the per-block counts and a write pass (a wavefront ballot plus the block's prefix inside each block; no atomic counter: the lists keep
// the step order)
#include "kernels.hpp"

enum { TEV_BLOCK = 256, TEV_WAVES = TEV_BLOCK / 64 };

// The events a block's waves hold: ballots of the two kinds, the counts per wave through LDS.  Returns the lane's rank among the block's
// lanes of its own kind (valid where kind != TEV_NONE); total[0..1]: the block's counts.
__device__ __forceinline__ u32 tev_block_rank(u32 kind, u32 (&wc)[TEV_WAVES][2], u32 (&total)[2]) {
    const u32 lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const unsigned long long m_copy = __ballot(kind == (u32)TEV_COPY), m_exp = __ballot(kind == (u32)TEV_EXP);
    if (lane == 0u) { wc[w][0] = (u32)__popcll(m_copy); wc[w][1] = (u32)__popcll(m_exp); }
    __syncthreads();
    const u32 ch = kind == (u32)TEV_EXP ? 1u : 0u;
    u32 before = 0;
    total[0] = total[1] = 0;
#pragma unroll
    for (u32 k = 0; k < (u32)TEV_WAVES; k++) {
        if (k < w) before += wc[k][ch];
        total[0] += wc[k][0];
        total[1] += wc[k][1];
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    return before + (u32)__popcll((ch ? m_exp : m_copy) & below);
}
// Pass 1: a step's status, what it emits, the tally; the block's two counts
__global__ __launch_bounds__(TEV_BLOCK) void tev_step_kernel(TevArgs a, u32* status, ZkTally* tally) {
    __shared__ u32 wc[TEV_WAVES][2];
    const u64 s = (u64)blockIdx.x * TEV_BLOCK + threadIdx.x;
    u32 st = 0, kind = TEV_NONE;
    if (s < a.n_steps) {
        TevEvent e;
        st = tev_step(a, s, e);
        kind = e.kind;
        status[s] = st;
        a.kind[s] = (uint8_t)kind;
    }
    tally_commit(tally, s, st);
    u32 total[2];
    (void)tev_block_rank(kind, wc, total);
    if (threadIdx.x == 0u) { a.blk[2 * (u64)blockIdx.x] = total[0]; a.blk[2 * (u64)blockIdx.x + 1] = total[1]; }
}
// Pass 2: the per-block counts to the events in front of each block, both kinds at once; one workgroup walks the blocks 1024 at a time (as
// trw_offset_scan_kernel walks its rows); the totals are the pass's counts
__global__ __launch_bounds__(1024) void tev_scan_kernel(TevArgs a, u32 n_blocks) {
    __shared__ u32 wsum[16][2];
    const u32 t = threadIdx.x, lane = t & 63u, w = t >> 6;
    u32 carry0 = 0, carry1 = 0;
    for (u32 base = 0; base < n_blocks; base += 1024u) {
        const u32 b = base + t;
        const u32 v0 = b < n_blocks ? a.blk[2 * (u64)b] : 0u, v1 = b < n_blocks ? a.blk[2 * (u64)b + 1] : 0u;
        u32 x0 = v0, x1 = v1;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const u32 y0 = (u32)__shfl_up((int)x0, d), y1 = (u32)__shfl_up((int)x1, d);
            if (lane >= (u32)d) { x0 += y0; x1 += y1; }
        }
        if (lane == 63u) { wsum[w][0] = x0; wsum[w][1] = x1; }
        __syncthreads();
        u32 before0 = 0, before1 = 0, total0 = 0, total1 = 0;
#pragma unroll
        for (u32 k = 0; k < 16; k++) {
            const u32 s0 = wsum[k][0], s1 = wsum[k][1];
            if (k < w) { before0 += s0; before1 += s1; }
            total0 += s0;
            total1 += s1;
        }
        if (b < n_blocks) { a.blk[2 * (u64)b] = carry0 + before0 + x0 - v0; a.blk[2 * (u64)b + 1] = carry1 + before1 + x1 - v1; }
        carry0 += total0;
        carry1 += total1;
        __syncthreads();
    }
    if (t == 0u) { a.counts[0] = carry0; a.counts[1] = carry1; }
}
// Pass 3: an emitting lane computes its event again (the few dependent gathers of its step) and stores it at the events in front of its
// block + its rank in the block.  Every position is below the pass's count, which is at most n_steps: the capacity of every output.
__global__ __launch_bounds__(TEV_BLOCK) void tev_write_kernel(TevArgs a) {
    __shared__ u32 wc[TEV_WAVES][2];
    const u64 s = (u64)blockIdx.x * TEV_BLOCK + threadIdx.x;
    const u32 kind = s < a.n_steps ? a.kind[s] : (u32)TEV_NONE;
    u32 total[2];
    const u32 rank = tev_block_rank(kind, wc, total);
    if (kind == (u32)TEV_NONE) return;
    TevEvent e;
    (void)tev_step(a, s, e);
    if (e.kind != kind) return;  // (a caller rewrote its records under the pass)
    const u64 pos = (u64)a.blk[2 * (u64)blockIdx.x + (kind == (u32)TEV_EXP ? 1u : 0u)] + rank;
    if (kind == (u32)TEV_COPY) tev_store_copy(a, pos, s, e);
    else tev_store_exp(a, pos, s, e);
}

// ---- the wider entry (zk_events_from_trace_ext*): a lane emits 0, 1 or 2 copy events, or an EXP event --------------------------------
enum { TEVX_NONE = 0, TEVX_COPY1 = 1, TEVX_EXP = 2, TEVX_COPY2 = 3 };  // what a step emits, as a.kind keeps it between the passes

// As tev_block_rank with lanes of 0..2 copy events: the ballots "emits at least one" and "emits two" give a wave's events (their two
// popcounts) and a lane's rank (the popcounts below the lane); total[0] counts EVENTS.  rank[0]: the lane's first copy event among the
// block's, rank[1]: its EXP event.
__device__ __forceinline__ void tevx_block_rank(u32 kind, u32 (&wc)[TEV_WAVES][2], u32 (&total)[2], u32 (&rank)[2]) {
    const u32 lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const unsigned long long m_one = __ballot(kind == (u32)TEVX_COPY1 || kind == (u32)TEVX_COPY2), m_two = __ballot(kind == (u32)TEVX_COPY2),
                             m_exp = __ballot(kind == (u32)TEVX_EXP);
    if (lane == 0u) { wc[w][0] = (u32)(__popcll(m_one) + __popcll(m_two)); wc[w][1] = (u32)__popcll(m_exp); }
    __syncthreads();
    rank[0] = rank[1] = 0;
    total[0] = total[1] = 0;
#pragma unroll
    for (u32 k = 0; k < (u32)TEV_WAVES; k++) {
        if (k < w) { rank[0] += wc[k][0]; rank[1] += wc[k][1]; }
        total[0] += wc[k][0];
        total[1] += wc[k][1];
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    rank[0] += (u32)(__popcll(m_one & below) + __popcll(m_two & below));
    rank[1] += (u32)__popcll(m_exp & below);
}
__device__ __forceinline__ u32 tevx_kind_of(const TevxEvent (&x)[2]) {
    return x[0].e.kind == (u32)TEV_EXP ? (u32)TEVX_EXP : x[0].e.kind != (u32)TEV_COPY ? (u32)TEVX_NONE : x[1].e.kind == (u32)TEV_COPY ? (u32)TEVX_COPY2 : (u32)TEVX_COPY1;
}
// The open's count: the BeginTx and DATACOPY steps (the copy capacity is n_steps + that), a ballot per wave and one add per wave
__global__ __launch_bounds__(TEV_BLOCK) void tevx_count_kernel(const u64* steps, u64 n_steps, unsigned long long* n_pair) {
    const u64 s = (u64)blockIdx.x * TEV_BLOCK + threadIdx.x;
    const bool pair = s < n_steps && tevx_is_pair_state(steps[s * TRW_STEP_WORDS]);
    const unsigned long long m = __ballot(pair);
    if ((threadIdx.x & 63u) == 0u && m) atomicAdd(n_pair, (unsigned long long)__popcll(m));
}
// Pass 1: as tev_step_kernel over tevx_step
__global__ __launch_bounds__(TEV_BLOCK) void tevx_step_kernel(TevxArgs ax, u32* status, ZkTally* tally) {
    __shared__ u32 wc[TEV_WAVES][2];
    const TevArgs& a = ax.t;
    const u64 s = (u64)blockIdx.x * TEV_BLOCK + threadIdx.x;
    u32 st = 0, kind = TEVX_NONE;
    if (s < a.n_steps) {
        TevxEvent x[2];
        st = tevx_step(a, s, x);
        kind = tevx_kind_of(x);
        status[s] = st;
        a.kind[s] = (uint8_t)kind;
    }
    tally_commit(tally, s, st);
    u32 total[2], rank[2];
    tevx_block_rank(kind, wc, total, rank);
    if (threadIdx.x == 0u) { a.blk[2 * (u64)blockIdx.x] = total[0]; a.blk[2 * (u64)blockIdx.x + 1] = total[1]; }
}
// Pass 3: as tev_write_kernel; a lane's events stand together.  With the records as the open saw them every position is below the
// capacity; a lane whose events would pass it (records rewritten under the session) stores nothing and its status becomes site 5.
__global__ __launch_bounds__(TEV_BLOCK) void tevx_write_kernel(TevxArgs ax, u32* status) {
    __shared__ u32 wc[TEV_WAVES][2];
    const TevArgs& a = ax.t;
    const u64 s = (u64)blockIdx.x * TEV_BLOCK + threadIdx.x;
    const u32 kind = s < a.n_steps ? a.kind[s] : (u32)TEVX_NONE;
    u32 total[2], rank[2];
    tevx_block_rank(kind, wc, total, rank);
    if (kind == (u32)TEVX_NONE) return;
    TevxEvent x[2];
    (void)tevx_step(a, s, x);
    if (tevx_kind_of(x) != kind) return;  // (a caller rewrote its records under the pass)
    if (kind == (u32)TEVX_EXP) {
        const u64 pos = (u64)a.blk[2 * (u64)blockIdx.x + 1] + rank[1];
        if (pos < a.n_steps) tev_store_exp(a, pos, s, x[0].e);
        return;
    }
    const u64 pos = (u64)a.blk[2 * (u64)blockIdx.x] + rank[0];
    const u32 n = kind == (u32)TEVX_COPY2 ? 2u : 1u;
    if (pos + n > ax.cap_copy) { status[s] = tev_status(TEV_SITE_EXT); return; }
    tevx_store_copy(ax, pos, s, x[0]);
    if (n == 2u) tevx_store_copy(ax, pos + 1, s, x[1]);
}

void zk_launch_trace_events_count(hipStream_t st, const u64* steps, u64 n_steps, u64* n_pair) {
    const u32 nb = (u32)((n_steps + TEV_BLOCK - 1) / TEV_BLOCK);
    if (nb) hipLaunchKernelGGL(tevx_count_kernel, dim3(nb), dim3(TEV_BLOCK), 0, st, steps, n_steps, (unsigned long long*)n_pair);
}
void zk_launch_trace_events_ext(hipStream_t st, const TevxArgs& ax, u32* status, ZkTally* tally) {
    const u32 nb = (u32)((ax.t.n_steps + TEV_BLOCK - 1) / TEV_BLOCK);
    if (nb) hipLaunchKernelGGL(tevx_step_kernel, dim3(nb), dim3(TEV_BLOCK), 0, st, ax, status, tally);
    hipLaunchKernelGGL(tev_scan_kernel, dim3(1), dim3(1024), 0, st, ax.t, nb);  // (the same scan: the block counts are events of either entry)
    if (nb) hipLaunchKernelGGL(tevx_write_kernel, dim3(nb), dim3(TEV_BLOCK), 0, st, ax, status);
}
void zk_launch_trace_events(hipStream_t st, const TevArgs& a, u32* status, ZkTally* tally) {
    const u32 nb = (u32)((a.n_steps + TEV_BLOCK - 1) / TEV_BLOCK);
    if (nb) hipLaunchKernelGGL(tev_step_kernel, dim3(nb), dim3(TEV_BLOCK), 0, st, a, status, tally);
    hipLaunchKernelGGL(tev_scan_kernel, dim3(1), dim3(1024), 0, st, a, nb);  // (no step: the counts are 0)
    if (nb) hipLaunchKernelGGL(tev_write_kernel, dim3(nb), dim3(TEV_BLOCK), 0, st, a);
}
