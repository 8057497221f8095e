// SHA3 inputs and keccak rows from compact trace records (trace_sha3.hpp).  Open: a lane per step (status, size), a scan of the per-block
// message / byte counts, the packed records and data offsets (a wavefront ballot and scan plus the block's prefix; no atomic counter: the
// messages keep the step order).  Every pass: a lane per message byte (the gather), the keccak table's own kernels over the gathered
// bytes (k_assign.hip), a lane per message and per step (the digest comparison, the statuses, the tally).
#include "kernels.hpp"

enum { TS3_BLOCK = 256, TS3_WAVES = TS3_BLOCK / 64 };

__device__ __forceinline__ u64 ts3_shfl_up64(u64 v, int d) {
    const u32 lo = (u32)__shfl_up((int)(u32)v, d), hi = (u32)__shfl_up((int)(u32)(v >> 32), d);
    return (u64)lo | ((u64)hi << 32);
}
// A block's messages and their bytes: the lane's rank among the block's messages and the bytes in front of its own inside the block
// (valid for a message lane); total[0..1]: the block's counts.  The wave's part by ballot and a 64-bit scan, the waves' through LDS.
__device__ __forceinline__ void ts3_block_prefix(bool is_msg, u64 bytes, u64 (&ws)[TS3_WAVES][2], u64& rank, u64& before, u64 (&total)[2]) {
    const u32 lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const unsigned long long m = __ballot(is_msg);
    u64 x = bytes;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u64 y = ts3_shfl_up64(x, d);
        if (lane >= (u32)d) x += y;
    }
    if (lane == 63u) { ws[w][0] = (u64)__popcll(m); ws[w][1] = x; }
    __syncthreads();
    rank = (u64)__popcll(m & ((1ull << lane) - 1ull));
    before = x - bytes;
    total[0] = total[1] = 0;
#pragma unroll
    for (u32 k = 0; k < (u32)TS3_WAVES; k++) {
        if (k < w) { rank += ws[k][0]; before += ws[k][1]; }
        total[0] += ws[k][0];
        total[1] += ws[k][1];
    }
}
// Open 1: a step's open-time status and size; the block's two counts
__global__ __launch_bounds__(TS3_BLOCK) void ts3_step_kernel(Ts3Args a) {
    __shared__ u64 ws[TS3_WAVES][2];
    const u64 s = (u64)blockIdx.x * TS3_BLOCK + threadIdx.x;
    u64 size = TS3_NOT_MSG;
    if (s < a.t.n_steps) {
        Ts3Msg m;
        TevWord w;
        a.st_open[s] = ts3_step(a, s, m, w);
        a.sz[s] = size = m.size;
    }
    u64 rank, before, total[2];
    ts3_block_prefix(size != TS3_NOT_MSG, ts3_counted(size), ws, rank, before, total);
    if (threadIdx.x == 0u) { a.blk[2 * (u64)blockIdx.x] = total[0]; a.blk[2 * (u64)blockIdx.x + 1] = total[1]; }
}
// Open 2: the per-block counts to the messages / bytes in front of each block; one workgroup walks the blocks 1024 at a time (as
// tev_scan_kernel); the totals go to the verdict block
__global__ __launch_bounds__(1024) void ts3_scan_kernel(Ts3Args a, u32 n_blocks) {
    __shared__ u64 wsum[16][2];
    const u32 t = threadIdx.x, lane = t & 63u, w = t >> 6;
    u64 carry0 = 0, carry1 = 0;
    for (u32 base = 0; base < n_blocks; base += 1024u) {
        const u32 b = base + t;
        const u64 v0 = b < n_blocks ? a.blk[2 * (u64)b] : 0ull, v1 = b < n_blocks ? a.blk[2 * (u64)b + 1] : 0ull;
        u64 x0 = v0, x1 = v1;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const u64 y0 = ts3_shfl_up64(x0, d), y1 = ts3_shfl_up64(x1, d);
            if (lane >= (u32)d) { x0 += y0; x1 += y1; }
        }
        if (lane == 63u) { wsum[w][0] = x0; wsum[w][1] = x1; }
        __syncthreads();
        u64 before0 = 0, before1 = 0, total0 = 0, total1 = 0;
#pragma unroll
        for (u32 k = 0; k < 16; k++) {
            const u64 s0 = wsum[k][0], s1 = wsum[k][1];
            if (k < w) { before0 += s0; before1 += s1; }
            total0 += s0;
            total1 += s1;
        }
        if (b < n_blocks) { a.blk[2 * (u64)b] = carry0 + before0 + x0 - v0; a.blk[2 * (u64)b + 1] = carry1 + before1 + x1 - v1; }
        carry0 += total0;
        carry1 += total1;
        __syncthreads();
    }
    if (t == 0u) { a.verdict[TS3_V_MSGS] = carry0; a.verdict[TS3_V_BYTES] = carry1; a.verdict[TS3_V_CROSS] = TS3_NOT_MSG; }
}
// Open 3: a message lane stores its record and data_off[rank]; the last one data_off[n_msgs] too.  The sizes are the session's own (sz),
// so every rank is below n_msgs and every offset what the scan counted.  cross_only: nothing is stored but the step that takes the byte
// total to 2^31 (the rejected open's error names it).
__global__ __launch_bounds__(TS3_BLOCK) void ts3_write_kernel(Ts3Args a, u32 cross_only) {
    __shared__ u64 ws[TS3_WAVES][2];
    const u64 s = (u64)blockIdx.x * TS3_BLOCK + threadIdx.x;
    const u64 size = s < a.t.n_steps ? a.sz[s] : TS3_NOT_MSG;
    u64 rank, before, total[2];
    ts3_block_prefix(size != TS3_NOT_MSG, ts3_counted(size), ws, rank, before, total);
    if (size == TS3_NOT_MSG) return;
    const u64 pos = a.blk[2 * (u64)blockIdx.x] + rank, at = a.blk[2 * (u64)blockIdx.x + 1] + before;
    if (cross_only) {
        if (at < TS3_BYTES_LIMIT && at + ts3_counted(size) >= TS3_BYTES_LIMIT) a.verdict[TS3_V_CROSS] = s;
        return;
    }
    if (pos >= a.n_msgs) return;  // (never: n_msgs is the scan's count of the same sizes)
    Ts3Msg m;
    TevWord w;
    (void)ts3_step(a, s, m, w);
    m.size = size;
    a.msg[pos] = m;
    a.data_off[pos] = at;
    if (pos + 1 == a.n_msgs) a.data_off[pos + 1] = at + size;
}
// Pass 1: a lane per message byte.  Its message by binary search over the session's offsets, its op in closed form, four independent
// loads, the checks, one byte stored (a wavefront stores 64 contiguous bytes); a failing byte leaves i << 8 | site in its message's word.
__global__ __launch_bounds__(TS3_BLOCK) void ts3_gather_kernel(Ts3Args a) {
    const u64 b = (u64)blockIdx.x * TS3_BLOCK + threadIdx.x;
    if (b >= a.n_bytes) return;
    u64 lo = 0, hi = a.n_msgs - 1;  // the first message whose end lies behind b (data_off[n_msgs] = n_bytes > b: there is one)
    while (lo < hi) {
        const u64 mid = lo + ((hi - lo) >> 1);
        if (a.data_off[mid + 1] <= b) lo = mid + 1; else hi = mid;
    }
    const u64 i = b - a.data_off[lo];
    const Ts3Msg m = a.msg[lo];
    u32 site = 0;
    const u32 v = i < m.size ? ts3_byte(a, m, i, site) : 0u;
    a.data[b] = (uint8_t)v;
    if (site) atomicMin(&a.fail[lo], ((unsigned long long)i << 8) | site);
}
// Pass 3: lanes [0, step lanes): a step that is no message gets its open-time status; the lanes behind them: a message's status (the
// gather's word, else the digest comparison) at its step, and its step / offset outputs.  Every lane enters the tally with its step.
__global__ __launch_bounds__(TS3_BLOCK) void ts3_check_kernel(Ts3Args a, u32 step_blocks, u32* status, ZkTally* tally) {
    u64 row = 0;
    u32 code = 0;
    if (blockIdx.x < step_blocks) {
        const u64 s = (u64)blockIdx.x * TS3_BLOCK + threadIdx.x;
        if (s < a.t.n_steps && a.sz[s] == TS3_NOT_MSG) {
            row = s;
            code = a.st_open[s];
            status[s] = code;
        }
    } else {
        const u64 mi = (u64)(blockIdx.x - step_blocks) * TS3_BLOCK + threadIdx.x;
        if (mi < a.n_msgs) {
            row = a.msg[mi].step;
            code = ts3_check(a, mi, a.fail[mi]);
            status[row] = code;
            a.step[mi] = (u32)row;
            a.data_offsets[mi] = a.data_off[mi];
            if (mi + 1 == a.n_msgs) a.data_offsets[mi + 1] = a.data_off[mi + 1];
        }
    }
    tally_commit(tally, row, code);
}

void zk_launch_trace_sha3_count(hipStream_t st, const Ts3Args& a) {
    const u32 nb = (u32)((a.t.n_steps + TS3_BLOCK - 1) / TS3_BLOCK);
    if (nb) hipLaunchKernelGGL(ts3_step_kernel, dim3(nb), dim3(TS3_BLOCK), 0, st, a);
    hipLaunchKernelGGL(ts3_scan_kernel, dim3(1), dim3(1024), 0, st, a, nb);  // (no step: the counts are 0)
}
void zk_launch_trace_sha3_write(hipStream_t st, const Ts3Args& a, bool cross_only) {
    const u32 nb = (u32)((a.t.n_steps + TS3_BLOCK - 1) / TS3_BLOCK);
    if (nb) hipLaunchKernelGGL(ts3_write_kernel, dim3(nb), dim3(TS3_BLOCK), 0, st, a, cross_only ? 1u : 0u);
}
void zk_launch_trace_sha3(hipStream_t st, const Ts3Args& a, const KeccakGenArgs& g, u32* status, ZkTally* tally) {
    const u32 sb = (u32)((a.t.n_steps + TS3_BLOCK - 1) / TS3_BLOCK), mb = (u32)((a.n_msgs + TS3_BLOCK - 1) / TS3_BLOCK);
    if (a.n_msgs) (void)hipMemsetAsync(a.fail, 0xff, (size_t)a.n_msgs * sizeof(unsigned long long), st);
    if (a.n_bytes) hipLaunchKernelGGL(ts3_gather_kernel, dim3((u32)((a.n_bytes + TS3_BLOCK - 1) / TS3_BLOCK)), dim3(TS3_BLOCK), 0, st, a);
    if (a.n_msgs) zk_launch_keccak_table(st, g, nullptr, tally);
    if (sb + mb) hipLaunchKernelGGL(ts3_check_kernel, dim3(sb + mb), dim3(TS3_BLOCK), 0, st, a, sb, status, tally);
}
