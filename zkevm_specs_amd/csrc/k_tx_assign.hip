// Tx circuit witness assignment kernels (tx_assign.hpp), all on the session's stream:
//   tx_hash_kernel       one lane per tx: RLP + keccak of the signing payload, calldata gas cost
//   secp_recover_kernel  public-key recovery in the lane forms (secp_lanes.hpp: L = 1, 2, 4 lanes per signature); the Sig assignment's too
//   tx_slot_kernel       one lane per tx slot: fixed rows, SignVerify unit, keccak candidate row
//   tx_calldata_kernel   one lane per CallData row
//   tx_keccak_first / tx_keccak_rank   the keccak table as a sorted set: first occurrences, then each one's rank among them
#include "kernels.hpp"
#include "keccak_set.hpp"

__global__ __launch_bounds__(64) void tx_hash_kernel(TxAssignArgs a) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.n) tx_sign_hash(a, i);
}

// As ecdsa_verify_kernel (k_ecdsa.hip): the roles of a signature's lanes run the halves of the joint multiplication and meet through
// cross-lane exchanges; role 0 converts Q to affine and writes the key and the status.
template <int L>
__global__ __launch_bounds__(L == 4 ? 256 : 64) void secp_recover_kernel(SecpRecoverArgs a, u32* status, ZkTally* tally) {
    const u64 gid = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 i = a.lanes.first + gid / L;
    const int role = (int)(gid % L);
    const bool valid = i < a.n;
    u32* tab = a.lanes.qtab + gid * (15u * 24u);
    EcdsaPrep pr;
    Fr u1, u2;
    u32 st = TX_BAD_SIGNATURE;
    SpPoint part = sp_infinity();
    if (valid) {
        st = tx_recover_prepare(a, i, pr, u1, u2);
        if (st == ECDSA_PENDING) part = L == 4 ? ecdsa_partial4(pr, role, tab, 1, a.lanes.gcomb)
                                               : ecdsa_partial(pr, L == 1 ? 0 : role, L == 1 ? 1 : role, tab, 1, a.lanes.gcomb);
        else if (st == TX_RECOVER_EXACT && role == 0) part = tx_recover_exact(pr, u1, u2);
    }
    secp_lanes_meet<L>(part, valid && st == ECDSA_PENDING, role);
    u32 code = 0;
    if (valid && role == 0) {
        if (st == ECDSA_PENDING || st == TX_RECOVER_EXACT) {
            code = tx_recover_finish_to(a.pk + i * 8, part);
        } else {
            code = st;
            tx_recover_fail_to(a.pk + i * 8);
        }
        a.status[i] = code;
        if (status && status != a.status) status[i] = code;
    }
    tally_commit(tally, i, code);
}
void zk_launch_secp_recover(hipStream_t st, const SecpRecoverArgs& a0, u32* status, ZkTally* tally) {
    SecpRecoverArgs a = a0;
    const u32 L = a.lanes.lanes_per_sig;
    const auto kernel = L == 4 ? secp_recover_kernel<4> : L == 2 ? secp_recover_kernel<2> : secp_recover_kernel<1>;
    for (SecpChunk c = secp_chunk(a.n, a.lanes, 0); c.count; c = secp_chunk(a.n, a.lanes, c.first + c.count)) {
        a.lanes.first = c.first;
        hipLaunchKernelGGL(kernel, dim3(c.grid), dim3(c.block), 0, st, a, status, tally);
    }
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

// The keccak candidates (n + 1 rows) as a sorted set: the two tiled passes of keccak_set.hpp (shared with the Sig assignment)
__global__ __launch_bounds__(256) void tx_keccak_first_kernel(TxAssignArgs a, u64 m) { txk_first_pass(a.kcand, a.kfirst, a.n_keccak, m); }
__global__ __launch_bounds__(256) void tx_keccak_rank_kernel(TxAssignArgs a, u64 m) { txk_rank_pass(a.kcand, a.kfirst, a.keccak, m); }

void zk_launch_tx_assign(hipStream_t st, const TxAssignArgs& a, u32* status, ZkTally* tally) {
    if (a.n) hipLaunchKernelGGL(tx_hash_kernel, dim3((u32)((a.n + 63) / 64)), dim3(64), 0, st, a);
    zk_launch_secp_recover(st, tx_recover_args(a), status, tally);
    const u64 slots = a.max_txs ? a.max_txs : 1;
    hipLaunchKernelGGL(tx_slot_kernel, dim3((u32)((slots + 63) / 64)), dim3(64), 0, st, a);
    if (a.max_calldata) hipLaunchKernelGGL(tx_calldata_kernel, dim3((u32)((a.max_calldata + 255) / 256)), dim3(256), 0, st, a);
    const u64 m = a.n + 1;
    (void)hipMemsetAsync(a.n_keccak, 0, sizeof(u32), st);
    hipLaunchKernelGGL(tx_keccak_first_kernel, dim3((u32)((m + 255) / 256)), dim3(256), 0, st, a, m);
    hipLaunchKernelGGL(tx_keccak_rank_kernel, dim3((u32)((m + 255) / 256)), dim3(256), 0, st, a, m);
}
