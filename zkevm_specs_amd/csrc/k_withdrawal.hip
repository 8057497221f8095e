// Withdrawal circuit kernels (withdrawal_circuit.hpp): one lane per row for the verification (a +-1-row stencil: row i reads row
// i + 1's id and row i - 1's root), one lane per withdrawal for the assignment.
#include "kernels.hpp"

// held rows [lo, hi) of a session: status[j] for held row j; the block lookup rides on the lane of global row MAX - 1
__global__ __launch_bounds__(256) void withdrawal_rows_kernel(WithdrawalArgs a, u64 lo, u64 hi, u32* status, ZkTally* tally) {
    tally_clear_twin(tally);
    const u64 j = lo + (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u32 code = 0;
    if (j < hi) {
        code = wd_verify_row(a, j);
        if (status) status[j] = code;
    }
    tally_commit(tally, j, code);
}
// rows [0, n_out): the RLP goes through LDS (136 B per lane: the message block, zero-padded) so that no byte array sits in scratch
__global__ __launch_bounds__(64) void withdrawal_assign_kernel(WithdrawalArgs a) {
    __shared__ uint8_t msg[64][136];
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.n_out) wd_assign_row(a, i, msg[threadIdx.x]);
}

void zk_launch_withdrawal_rows(hipStream_t st, const WithdrawalArgs& a, u64 lo, u64 hi, u32* status, ZkTally* tally) {
    hipLaunchKernelGGL(withdrawal_rows_kernel, dim3((u32)((hi - lo + 255) / 256)), dim3(256), 0, st, a, lo, hi, status, tally);
}
void zk_launch_withdrawal_assign(hipStream_t st, const WithdrawalArgs& a) {
    if (a.n_out) hipLaunchKernelGGL(withdrawal_assign_kernel, dim3((u32)((a.n_out + 63) / 64)), dim3(64), 0, st, a);
}
