// ECC precompile calls (ecc_calls.hpp), all on the session's stream:
//   ecl_point_kernel       one lane per add / mul call: validity, the sum or the 256-bit chain, points entry, row, table candidate, aux
//   ecc_pair_stage1        (k_ecc.hip) one lane per (op, pair): the verifying session's flags and Miller value
//   ecl_pairing_kernel     one lane per pairing call over the records: validity, RLC, product, final exponentiation, outputs
//   ecl_table_dup / ecl_table_place   the ecc table: rows with an equal row before them, then every other row at the count of such
//                          rows before it (the sig table's rule and mechanism, k_sig_assign.hip, over 13-cell rows)
#include "kernels.hpp"

__global__ __launch_bounds__(64) void ecl_point_kernel(EccCallArgs a, u32* status) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.n_add + a.n_mul) {
        ecc_call_point(a, i);
        status[i] = 0u;
    }
}
__global__ __launch_bounds__(64) void ecl_pairing_kernel(EccCallArgs a, u32* status) {
    const u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < a.n_pairing) {
        ecc_call_pairing(a, k);
        status[a.n_add + a.n_mul + k] = 0u;
    }
}

// Block (x, y) compares the 256 rows of row block x with the tiles y, y + gridDim.y, ... <= x of 256 64-bit prefixes in LDS; the
// full rows (52 words) are read only where two prefixes agree.  The prefix mixes px, qx (the scalar of a mul) and input_rlc: one of
// them differs between almost any two distinct calls of a kind, and op_type separates the kinds in the full comparison.
#define ECT_TILE 256
#define ECT_MAX_Y 1024u
__device__ __forceinline__ u64 ect_prefix(const u64* row) { return row[4] ^ row[20] ^ row[36] ^ (row[12] << 1); }
__global__ __launch_bounds__(ECT_TILE) void ecl_table_dup_kernel(EccCallArgs a, u64 n) {
    __shared__ u64 tile[ECT_TILE];
    const u64 bi = blockIdx.x;
    const u64 i = bi * ECT_TILE + threadIdx.x;
    const u64* mine = a.tcand + (i < n ? i : 0) * ECL_ROW_WORDS;
    const u64 pre = ect_prefix(mine);
    bool dup = false;
    for (u64 bj = blockIdx.y; bj <= bi; bj += gridDim.y) {
        const u64 t0 = bj * ECT_TILE;
        __syncthreads();
        tile[threadIdx.x] = t0 + threadIdx.x < n ? ect_prefix(a.tcand + (t0 + threadIdx.x) * ECL_ROW_WORDS) : 0ull;
        __syncthreads();
        const u32 lim = bj == bi ? threadIdx.x : (u32)ECT_TILE;  // rows t0 + j < i (every row of an earlier block exists)
        if (i < n && !dup) {
            for (u32 j0 = 0; j0 < ECT_TILE; j0 += 8) {
                u32 hit = 0;
#pragma unroll
                for (u32 k = 0; k < 8; k++) hit |= (u32)(tile[j0 + k] == pre && j0 + k < lim) << k;
                for (u32 k = 0; hit && k < 8; k++)
                    if (((hit >> k) & 1u) && ecl_row_eq(mine, a.tcand + (t0 + j0 + k) * ECL_ROW_WORDS)) dup = true;
            }
        }
    }
    if (dup) a.tdup[i] = 1u;
}
// row i, if a first occurrence, goes to (first occurrences in the blocks before) + (those before it in its block)
__global__ __launch_bounds__(ECT_TILE) void ecl_table_place_kernel(EccCallArgs a, u64 n) {
    __shared__ u32 scan[ECT_TILE];
    __shared__ u32 base_sh;
    const u32 t = threadIdx.x;
    const u64 start = (u64)blockIdx.x * ECT_TILE;  // <= n - 1
    const u64 i = start + t;
    u32 part = 0;
    for (u64 j = t; j < start; j += ECT_TILE) part += a.tdup[j] ? 0u : 1u;
    scan[t] = part;
    __syncthreads();
    for (u32 d = ECT_TILE / 2; d > 0; d >>= 1) {
        if (t < d) scan[t] += scan[t + d];
        __syncthreads();
    }
    if (t == 0) base_sh = scan[0];
    __syncthreads();
    const u32 base = base_sh;
    const u32 first = (i < n && !a.tdup[i]) ? 1u : 0u;
    __syncthreads();
    scan[t] = first;
    __syncthreads();
    for (u32 d = 1; d < ECT_TILE; d <<= 1) {  // inclusive scan
        const u32 add = t >= d ? scan[t - d] : 0u;
        __syncthreads();
        scan[t] += add;
        __syncthreads();
    }
    if (first) {
        const u64 pos = (u64)base + scan[t] - 1u;  // <= i: a first occurrence never moves behind its own index
        const u64* mine = a.tcand + i * ECL_ROW_WORDS;
        for (int q = 0; q < ECL_ROW_WORDS; q++) a.ecc_table[pos * ECL_ROW_WORDS + q] = mine[q];
    }
    if (blockIdx.x == gridDim.x - 1 && t == ECT_TILE - 1) *a.n_table = base + scan[t];
}

void zk_launch_ecc_calls(hipStream_t st, const EccCallArgs& a, u32 n_pairs, u32* status) {
    const u64 np = a.n_add + a.n_mul, n = np + a.n_pairing;
    if (np) hipLaunchKernelGGL(ecl_point_kernel, dim3((u32)((np + 63) / 64)), dim3(64), 0, st, a, status);
    if (n_pairs) {
        EccPairArgs s{};
        s.a.pair_pts = a.pair_pts;  // (stage 1 reads nothing else of the ops)
        s.a.pair_off = a.pair_off;
        s.a.n_pairing = a.n_pairing;
        s.pair_flags = a.pair_flags;
        s.pair_f = a.pair_f;
        zk_launch_ecc_pair_stage1(st, s, 0u, n_pairs);
    }
    if (a.n_pairing) hipLaunchKernelGGL(ecl_pairing_kernel, dim3((u32)((a.n_pairing + 63) / 64)), dim3(64), 0, st, a, status);
    const u32 blocks = (u32)((n + ECT_TILE - 1) / ECT_TILE);
    (void)hipMemsetAsync(a.tdup, 0, (size_t)n * sizeof(u32), st);
    hipLaunchKernelGGL(ecl_table_dup_kernel, dim3(blocks, blocks < ECT_MAX_Y ? blocks : ECT_MAX_Y), dim3(ECT_TILE), 0, st, a, n);
    hipLaunchKernelGGL(ecl_table_place_kernel, dim3(blocks), dim3(ECT_TILE), 0, st, a, n);
}
