// Sig circuit witness assignment kernels (sig_assign.hpp), all on the session's stream; the key recovery is the Tx assignment's
// (zk_launch_secp_recover, k_tx_assign.hip):
//   sig_unit_kernel      one lane per signature: unit, keccak candidate row, sig-table candidate row, aux row
//   sig_keccak_first / sig_keccak_rank   the keccak table as a sorted set (keccak_set.hpp, shared with the Tx assignment)
//   sig_table_dup / sig_table_place      the sig table: rows with an equal row before them, then every other row at the count of such rows before it
#include "kernels.hpp"
#include "keccak_set.hpp"

__global__ __launch_bounds__(64) void sig_unit_kernel(SigAssignArgs a) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.n) sig_write_unit(a, i);
    if (i == 0) sig_write_zero_candidate(a);
}

__global__ __launch_bounds__(256) void sig_keccak_first_kernel(SigAssignArgs a, u64 m) { txk_first_pass(a.kcand, a.kfirst, a.n_keccak, m); }
__global__ __launch_bounds__(256) void sig_keccak_rank_kernel(SigAssignArgs a, u64 m) { txk_rank_pass(a.kcand, a.kfirst, a.keccak, m); }

// The sig table keeps input order, so a row needs no rank: only whether an equal row comes before it, and how many first occurrences
// do.  Block (x, y) compares the 256 rows of row block x with the tiles y, y + gridDim.y, ... <= x of 256 64-bit prefixes in LDS — the
// low word of sig_r: uniform for real signatures, so the full rows (36 words) are read only where two rows share their r.  A tile is one
// short, fully pipelined loop (eight prefixes per step, no early exit), and the n^2 / 2 comparisons spread over (n / 256)^2 / 2 blocks
// instead of one serial walk per lane: the one-walk form of the keccak passes cost this table 1.9 ms of a 7.0 ms pass at 2^14 signatures.
#define SGT_TILE 256
#define SGT_MAX_Y 1024u
__device__ __forceinline__ u64 sgt_prefix(const u64* row) { return row[12]; }
// sdup[i] = 1 where a row before i equals row i (zeroed before the launch)
__global__ __launch_bounds__(SGT_TILE) void sig_table_dup_kernel(SigAssignArgs a) {
    __shared__ u64 tile[SGT_TILE];
    const u64 n = a.n;
    const u64 bi = blockIdx.x;
    const u64 i = bi * SGT_TILE + threadIdx.x;
    const u64* mine = a.scand + (i < n ? i : 0) * SIG_TABLE_WORDS;
    const u64 pre = sgt_prefix(mine);
    bool dup = false;
    for (u64 bj = blockIdx.y; bj <= bi; bj += gridDim.y) {
        const u64 t0 = bj * SGT_TILE;
        __syncthreads();
        tile[threadIdx.x] = t0 + threadIdx.x < n ? sgt_prefix(a.scand + (t0 + threadIdx.x) * SIG_TABLE_WORDS) : 0ull;
        __syncthreads();
        const u32 lim = bj == bi ? threadIdx.x : (u32)SGT_TILE;  // rows t0 + j < i (every row of an earlier block exists)
        if (i < n && !dup) {
            for (u32 j0 = 0; j0 < SGT_TILE; j0 += 8) {
                u32 hit = 0;
#pragma unroll
                for (u32 k = 0; k < 8; k++) hit |= (u32)(tile[j0 + k] == pre && j0 + k < lim) << k;
                for (u32 k = 0; hit && k < 8; k++)
                    if (((hit >> k) & 1u) && sig_row_eq(mine, a.scand + (t0 + j0 + k) * SIG_TABLE_WORDS)) dup = true;
            }
        }
    }
    if (dup) a.sdup[i] = 1u;
}
// row i, if a first occurrence, goes to (first occurrences in the blocks before) + (those before it in its block)
__global__ __launch_bounds__(SGT_TILE) void sig_table_place_kernel(SigAssignArgs a) {
    __shared__ u32 scan[SGT_TILE];
    __shared__ u32 base_sh;
    const u64 n = a.n;
    const u32 t = threadIdx.x;
    const u64 start = (u64)blockIdx.x * SGT_TILE;  // <= n - 1
    const u64 i = start + t;
    u32 part = 0;
    for (u64 j = t; j < start; j += SGT_TILE) part += a.sdup[j] ? 0u : 1u;
    scan[t] = part;
    __syncthreads();
    for (u32 d = SGT_TILE / 2; d > 0; d >>= 1) {
        if (t < d) scan[t] += scan[t + d];
        __syncthreads();
    }
    if (t == 0) base_sh = scan[0];
    __syncthreads();
    const u32 base = base_sh;
    const u32 first = (i < n && !a.sdup[i]) ? 1u : 0u;
    __syncthreads();
    scan[t] = first;
    __syncthreads();
    for (u32 d = 1; d < SGT_TILE; d <<= 1) {  // inclusive scan
        const u32 add = t >= d ? scan[t - d] : 0u;
        __syncthreads();
        scan[t] += add;
        __syncthreads();
    }
    if (first) {
        const u64 pos = (u64)base + scan[t] - 1u;
        const u64* mine = a.scand + i * SIG_TABLE_WORDS;
#pragma unroll
        for (int q = 0; q < SIG_TABLE_WORDS; q++) a.sig_table[pos * SIG_TABLE_WORDS + q] = mine[q];
    }
    if (blockIdx.x == gridDim.x - 1 && t == SGT_TILE - 1) *a.n_sig_rows = base + scan[t];
}

void zk_launch_sig_assign(hipStream_t st, const SigAssignArgs& a, u32* status, ZkTally* tally) {
    zk_launch_secp_recover(st, sig_recover_args(a), status, tally);
    hipLaunchKernelGGL(sig_unit_kernel, dim3((u32)((a.n + 63) / 64 ? (a.n + 63) / 64 : 1)), dim3(64), 0, st, a);
    const u64 m = a.n + 1;
    (void)hipMemsetAsync(a.n_keccak, 0, sizeof(u32), st);
    hipLaunchKernelGGL(sig_keccak_first_kernel, dim3((u32)((m + 255) / 256)), dim3(256), 0, st, a, m);
    hipLaunchKernelGGL(sig_keccak_rank_kernel, dim3((u32)((m + 255) / 256)), dim3(256), 0, st, a, m);
    (void)hipMemsetAsync(a.n_sig_rows, 0, sizeof(u32), st);
    if (a.n) {
        const u32 blocks = (u32)((a.n + SGT_TILE - 1) / SGT_TILE);
        (void)hipMemsetAsync(a.sdup, 0, (size_t)a.n * sizeof(u32), st);
        hipLaunchKernelGGL(sig_table_dup_kernel, dim3(blocks, blocks < SGT_MAX_Y ? blocks : SGT_MAX_Y), dim3(SGT_TILE), 0, st, a);
        hipLaunchKernelGGL(sig_table_place_kernel, dim3(blocks), dim3(SGT_TILE), 0, st, a);
    }
}
