// Tx circuit witness assignment kernels (tx_assign.hpp), all on the session's stream:
//   tx_hash_kernel      one lane per tx: RLP + keccak of the signing payload, calldata gas cost
//   tx_recover_kernel   public-key recovery in the ECDSA kernel's lane forms (L = 1, 2, 4 lanes per signature)
//   tx_slot_kernel      one lane per tx slot: fixed rows, SignVerify unit, keccak candidate row
//   tx_calldata_kernel  one lane per CallData row
//   tx_keccak_first / tx_keccak_rank   the keccak table as a sorted set: first occurrences, then each one's rank among them
#include "kernels.hpp"

__global__ __launch_bounds__(64) void tx_hash_kernel(TxAssignArgs a) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.n) tx_sign_hash(a, i);
}

// As ecdsa_verify_kernel (k_ecdsa.hip): the roles of a signature's lanes run the halves of the joint multiplication and meet through
// cross-lane exchanges; role 0 converts Q to affine and writes the status.
template <int L>
__global__ __launch_bounds__(L == 4 ? 256 : 64) void tx_recover_kernel(TxAssignArgs a, u32* status, ZkTally* tally) {
    const u64 gid = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 i = a.first + gid / L;
    const int role = (int)(gid % L);
    const bool valid = i < a.n;
    u32* tab = a.qtab + gid * (15u * 24u);
    EcdsaPrep pr;
    Fr u1, u2;
    u32 st = TX_BAD_SIGNATURE;
    SpPoint part = sp_infinity();
    if (valid) {
        st = tx_recover_prepare(a, i, pr, u1, u2);
        if (st == ECDSA_PENDING) part = L == 4 ? ecdsa_partial4(pr, role, tab, 1, a.gcomb)
                                               : ecdsa_partial(pr, L == 1 ? 0 : role, L == 1 ? 1 : role, tab, 1, a.gcomb);
        else if (st == TX_RECOVER_EXACT && role == 0) part = tx_recover_exact(pr, u1, u2);
    }
    if (L >= 2) {
        SpPoint other;
#pragma unroll
        for (int w = 0; w < 8; w++) {
            other.X.v[w] = (u32)__shfl_xor((int)part.X.v[w], 1);
            other.Y.v[w] = (u32)__shfl_xor((int)part.Y.v[w], 1);
            other.Z.v[w] = (u32)__shfl_xor((int)part.Z.v[w], 1);
        }
        if (valid && (role & 1) == 0 && st == ECDSA_PENDING) sp_add_ip(part, other);
    }
    if (L == 4) {
        SpPoint other;
#pragma unroll
        for (int w = 0; w < 8; w++) {
            other.X.v[w] = (u32)__shfl_xor((int)part.X.v[w], 2);
            other.Y.v[w] = (u32)__shfl_xor((int)part.Y.v[w], 2);
            other.Z.v[w] = (u32)__shfl_xor((int)part.Z.v[w], 2);
        }
        if (valid && role == 0 && st == ECDSA_PENDING) sp_add_ip(part, other);
    }
    u32 code = 0;
    if (valid && role == 0) {
        if (st == ECDSA_PENDING || st == TX_RECOVER_EXACT) {
            code = tx_recover_finish(a, i, part);
        } else {
            code = st;
            tx_recover_fail(a, i);
        }
        a.status[i] = code;
        if (status && status != a.status) status[i] = code;
    }
    tally_commit(tally, i, code);
}

__global__ __launch_bounds__(64) void tx_slot_kernel(TxAssignArgs a) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.max_txs) tx_write_slot(a, i);
    if (i == 0) tx_write_zero_candidate(a);
}
__global__ __launch_bounds__(256) void tx_calldata_kernel(TxAssignArgs a) {
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < a.max_calldata) tx_write_calldata_row(a, j);
}

// The keccak candidates (n + 1 rows of 20 words) as a sorted set.  Both passes compare every lane's row with all the others through
// tiles of 256 order-preserving 64-bit prefixes in LDS — (is_enabled, the top word of input_rlc): the rlc is below 2^254, so
// (is_enabled << 62) | rlc[3] orders as the tuple's first two cells do — and read the two full rows only where the prefixes tie (equal
// rows: a repeated sender, the all-zero row).  n + 1 <= 2^14 + 1 rows are 2^28 prefix comparisons per pass.
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
// kfirst[i] = no row before i equals row i; n_keccak = their count
__global__ __launch_bounds__(256) void tx_keccak_first_kernel(TxAssignArgs a, u64 m) {
    __shared__ u64 tile[TXK_TILE];
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64* mine = a.kcand + (i < m ? i : 0) * TXK_WORDS;
    const u64 pre = txk_prefix(mine);
    bool dup = false;
    const u64 end = (u64)blockIdx.x * blockDim.x + blockDim.x;  // rows before the block's last lane
    for (u64 t0 = 0; t0 < end && t0 < m; t0 += TXK_TILE) {
        __syncthreads();
        if (t0 + threadIdx.x < m) tile[threadIdx.x] = txk_prefix(a.kcand + (t0 + threadIdx.x) * TXK_WORDS);
        __syncthreads();
        if (i < m && !dup && t0 < i) {
            const u64 lim = i - t0 < TXK_TILE ? i - t0 : TXK_TILE;  // rows t0 + j < i
            for (u64 j = 0; j < lim; j++)
                if (tile[j] == pre && txk_cmp_full(mine, a.kcand + (t0 + j) * TXK_WORDS) == 0) { dup = true; break; }
        }
    }
    if (i < m) {
        a.kfirst[i] = dup ? 0u : 1u;
        if (!dup) atomicAdd(a.n_keccak, 1u);
    }
}
// each first occurrence goes to its rank among the first occurrences
__global__ __launch_bounds__(256) void tx_keccak_rank_kernel(TxAssignArgs a, u64 m) {
    __shared__ u64 tile[TXK_TILE];
    __shared__ u32 tfirst[TXK_TILE];
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64* mine = a.kcand + (i < m ? i : 0) * TXK_WORDS;
    const u64 pre = txk_prefix(mine);
    const bool first = i < m && a.kfirst[i] != 0u;
    u64 rank = 0;
    for (u64 t0 = 0; t0 < m; t0 += TXK_TILE) {
        __syncthreads();
        if (t0 + threadIdx.x < m) {
            tile[threadIdx.x] = txk_prefix(a.kcand + (t0 + threadIdx.x) * TXK_WORDS);
            tfirst[threadIdx.x] = a.kfirst[t0 + threadIdx.x];
        }
        __syncthreads();
        if (first) {
            const u64 lim = m - t0 < TXK_TILE ? m - t0 : TXK_TILE;
            for (u64 j = 0; j < lim; j++) {
                const u64 pj = tile[j];
                if (!tfirst[j] || pj > pre) continue;
                if (pj < pre || txk_cmp_full(a.kcand + (t0 + j) * TXK_WORDS, mine) < 0) rank++;
            }
        }
    }
    if (first) {
#pragma unroll
        for (int q = 0; q < TXK_WORDS; q++) a.keccak[rank * TXK_WORDS + q] = mine[q];
    }
}

void zk_launch_tx_assign(hipStream_t st, const TxAssignArgs& a0, u32* status, ZkTally* tally) {
    TxAssignArgs a = a0;
    if (a.n) hipLaunchKernelGGL(tx_hash_kernel, dim3((u32)((a.n + 63) / 64)), dim3(64), 0, st, a);
    const u64 per_chunk = a.qtab_lanes / a.lanes_per_sig;
    for (a.first = 0; a.first < a.n; a.first += per_chunk) {
        const u64 m = a.n - a.first < per_chunk ? a.n - a.first : per_chunk;
        const u32 grid = (u32)((m * a.lanes_per_sig + 63) / 64);
        if (a.lanes_per_sig == 4) hipLaunchKernelGGL(HIP_KERNEL_NAME(tx_recover_kernel<4>), dim3((grid + 3) / 4), dim3(256), 0, st, a, status, tally);
        else if (a.lanes_per_sig == 2) hipLaunchKernelGGL(HIP_KERNEL_NAME(tx_recover_kernel<2>), dim3(grid), dim3(64), 0, st, a, status, tally);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(tx_recover_kernel<1>), dim3(grid), dim3(64), 0, st, a, status, tally);
    }
    a.first = 0;
    const u64 slots = a.max_txs ? a.max_txs : 1;
    hipLaunchKernelGGL(tx_slot_kernel, dim3((u32)((slots + 63) / 64)), dim3(64), 0, st, a);
    if (a.max_calldata) hipLaunchKernelGGL(tx_calldata_kernel, dim3((u32)((a.max_calldata + 255) / 256)), dim3(256), 0, st, a);
    const u64 m = a.n + 1;
    (void)hipMemsetAsync(a.n_keccak, 0, sizeof(u32), st);
    hipLaunchKernelGGL(tx_keccak_first_kernel, dim3((u32)((m + 255) / 256)), dim3(256), 0, st, a, m);
    hipLaunchKernelGGL(tx_keccak_rank_kernel, dim3((u32)((m + 255) / 256)), dim3(256), 0, st, a, m);
}
