// ECC circuit kernels (ecc_circuit.hpp): one lane per add / mul row, one lane per pairing op.
#include "kernels.hpp"

// add / mul rows: a 254-step Jacobian chain per mul lane (8 VGPRs per Fq); `assign` selects circuit2rows or verify
__global__ __launch_bounds__(64) void ecc_point_rows_kernel(EccArgs a, u32 assign, u32* status, ZkTally* tally) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 n = a.n_add + a.n_mul;
    u32 code = 0;
    if (i < n) {
        if (assign) ecc_assign_point_row(a, i, a.rows_out + i * (ECC_NCELLS * 4));
        else code = ecc_verify_point_row(a, i);
        if (status) status[i] = code;
    }
    if (!assign) tally_commit(tally, i, code);
}
// pairing ops: the whole op in one lane (subgroup checks, RLC, one Miller loop per pair into one Fq12 product, one final
// exponentiation); rows n_add + n_mul + k
__global__ __launch_bounds__(64) void ecc_pairing_rows_kernel(EccArgs a, u32 assign, u32* status, ZkTally* tally) {
    const u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 i = a.n_add + a.n_mul + k;
    u32 code = 0;
    if (k < a.n_pairing) {
        if (assign) ecc_assign_pairing_row(a, k, a.rows_out + i * (ECC_NCELLS * 4));
        else code = ecc_verify_pairing_row(a, i);
        if (status) status[i] = code;
    }
    if (!assign) tally_commit(tally, i, code);
}
// zk_fr_op 19..25: one Fq12 operation (or one pairing, one G2 chain) per lane, 12 elements each
__global__ __launch_bounds__(64) void ecc_fq12_op_kernel(int op, const u64* x, const u64* y, u64* out, u64 n12) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n12) ecc_fq12_op_hook(op, x + 48 * i, y + 48 * i, out + 48 * i);
}

void zk_launch_ecc(hipStream_t st, const EccArgs& a, bool assign, u32* status, ZkTally* tally) {
    const u64 np = a.n_add + a.n_mul;
    if (np) hipLaunchKernelGGL(ecc_point_rows_kernel, dim3((u32)((np + 63) / 64)), dim3(64), 0, st, a, (u32)assign, status, tally);
    if (a.n_pairing)
        hipLaunchKernelGGL(ecc_pairing_rows_kernel, dim3((u32)((a.n_pairing + 63) / 64)), dim3(64), 0, st, a, (u32)assign, status, tally);
}
void zk_launch_fq12_op(hipStream_t st, int op, const u64* x, const u64* y, u64* out, u64 n12) {
    hipLaunchKernelGGL(ecc_fq12_op_kernel, dim3((u32)((n12 + 63) / 64)), dim3(64), 0, st, op, x, y, out, n12);
}
