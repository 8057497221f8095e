// The keccak table of a witness assignment as a sorted set, on the device: shared by the Tx assignment (k_tx_assign.hip) and the Sig
// assignment (k_sig_assign.hip), each of which wraps the two passes in kernels of its own argument block.
//
// The keccak candidates (m rows of 20 words) as a sorted set.  Both passes compare every lane's row with all the others through
// tiles of 256 order-preserving 64-bit prefixes in LDS — (is_enabled, the top word of input_rlc): the rlc is below 2^254, so
// (is_enabled << 62) | rlc[3] orders as the tuple's first two cells do — and read the two full rows only where the prefixes tie (equal
// rows: a repeated sender, the all-zero row).  m <= 2^14 + 1 rows are 2^28 prefix comparisons per pass.
#pragma once
#include "keccak_table.hpp"

#define TXK_TILE 256
#define TXK_WORDS (KT_NCELLS * 4)
__device__ __forceinline__ u64 txk_prefix(const u64* row) { return (row[0] << 62) | row[7]; }
__device__ __forceinline__ int txk_cmp_full(const u64* x, const u64* y) {
    for (int c = 0; c < KT_NCELLS; c++)
        for (int q = 3; q >= 0; q--) {
            const u64 p = x[4 * c + q], r = y[4 * c + q];
            if (p != r) return p < r ? -1 : 1;
        }
    return 0;
}
// kfirst[i] = no row before i equals row i; n_keccak = their count.  One lane per row, blocks of TXK_TILE lanes.
__device__ __forceinline__ void txk_first_pass(const u64* kcand, u32* kfirst, u32* n_keccak, u64 m) {
    __shared__ u64 tile[TXK_TILE];
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64* mine = kcand + (i < m ? i : 0) * TXK_WORDS;
    const u64 pre = txk_prefix(mine);
    bool dup = false;
    const u64 end = (u64)blockIdx.x * blockDim.x + blockDim.x;  // rows before the block's last lane
    for (u64 t0 = 0; t0 < end && t0 < m; t0 += TXK_TILE) {
        __syncthreads();
        if (t0 + threadIdx.x < m) tile[threadIdx.x] = txk_prefix(kcand + (t0 + threadIdx.x) * TXK_WORDS);
        __syncthreads();
        if (i < m && !dup && t0 < i) {
            const u64 lim = i - t0 < TXK_TILE ? i - t0 : TXK_TILE;  // rows t0 + j < i
            for (u64 j = 0; j < lim; j++)
                if (tile[j] == pre && txk_cmp_full(mine, kcand + (t0 + j) * TXK_WORDS) == 0) { dup = true; break; }
        }
    }
    if (i < m) {
        kfirst[i] = dup ? 0u : 1u;
        if (!dup) atomicAdd(n_keccak, 1u);
    }
}
// each first occurrence goes to its rank among the first occurrences
__device__ __forceinline__ void txk_rank_pass(const u64* kcand, const u32* kfirst, u64* keccak, u64 m) {
    __shared__ u64 tile[TXK_TILE];
    __shared__ u32 tfirst[TXK_TILE];
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64* mine = kcand + (i < m ? i : 0) * TXK_WORDS;
    const u64 pre = txk_prefix(mine);
    const bool first = i < m && kfirst[i] != 0u;
    u64 rank = 0;
    for (u64 t0 = 0; t0 < m; t0 += TXK_TILE) {
        __syncthreads();
        if (t0 + threadIdx.x < m) {
            tile[threadIdx.x] = txk_prefix(kcand + (t0 + threadIdx.x) * TXK_WORDS);
            tfirst[threadIdx.x] = kfirst[t0 + threadIdx.x];
        }
        __syncthreads();
        if (first) {
            const u64 lim = m - t0 < TXK_TILE ? m - t0 : TXK_TILE;
            for (u64 j = 0; j < lim; j++) {
                const u64 pj = tile[j];
                if (!tfirst[j] || pj > pre) continue;
                if (pj < pre || txk_cmp_full(kcand + (t0 + j) * TXK_WORDS, mine) < 0) rank++;
            }
        }
    }
    if (first) {
#pragma unroll
        for (int q = 0; q < TXK_WORDS; q++) keccak[rank * TXK_WORDS + q] = mine[q];
    }
}
