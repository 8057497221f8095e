// ECC circuit kernels (ecc_circuit.hpp): one lane per add / mul row, one lane per pairing op (one-shots); a session's pass splits the
// pairing ops into one lane per (op, pair) and one lane per op.
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
// ---- a session's pass (zk_ecc_open): rows [lo, hi) of the circuit, the pairing rows in two stages ---------------------------------
// add / mul rows [lo, hi_pt): the per-row functions of ecc_point_rows_kernel behind a lane index offset by lo.  Always launched (one
// block at least): its first lane readies the twin tally for the pass after this one.
__global__ __launch_bounds__(64) void ecc_range_point_rows_kernel(EccArgs a, u64 lo, u64 hi_pt, u32* status, ZkTally* tally) {
    tally_clear_twin(tally);
    const u64 i = lo + (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u32 code = 0;
    if (i < hi_pt) {
        code = ecc_verify_point_row(a, i);
        status[i] = code;
    }
    tally_commit(tally, i, code);
}
// stage 1: one lane per pair [t_lo, t_hi) of the points array (the pairs of the pairing ops in range: pair_off[k_lo] .. pair_off[k_hi])
__global__ __launch_bounds__(64) void ecc_pair_stage1_kernel(EccPairArgs s, u32 t_lo, u32 t_hi) {
    const u64 t = (u64)t_lo + (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < t_hi) ecc_pair_stage1(s, (u32)t);
}
// stage 2: one lane per pairing row [lo_pr, hi) (global row numbers), over the records stage 1 left
__global__ __launch_bounds__(64) void ecc_pair_stage2_kernel(EccPairArgs s, u64 lo_pr, u64 hi, u32* status, ZkTally* tally) {
    const u64 i = lo_pr + (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u32 code = 0;
    if (i < hi) {
        code = ecc_pair_stage2(s, i);
        status[i] = code;
    }
    tally_commit(tally, i, code);
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
void zk_launch_ecc_range(hipStream_t st, const EccPairArgs& s, u64 lo, u64 hi, u32 t_lo, u32 t_hi, u32* status, ZkTally* tally) {
    const u64 np = s.a.n_add + s.a.n_mul;
    const u64 hi_pt = hi < np ? hi : np, lo_pr = lo > np ? lo : np;
    const u64 n_pt = hi_pt > lo ? hi_pt - lo : 0;
    hipLaunchKernelGGL(ecc_range_point_rows_kernel, dim3((u32)(n_pt ? (n_pt + 63) / 64 : 1)), dim3(64), 0, st, s.a, lo, hi_pt, status, tally);
    if (t_hi > t_lo) hipLaunchKernelGGL(ecc_pair_stage1_kernel, dim3((t_hi - t_lo + 63) / 64), dim3(64), 0, st, s, t_lo, t_hi);
    if (hi > lo_pr) hipLaunchKernelGGL(ecc_pair_stage2_kernel, dim3((u32)((hi - lo_pr + 63) / 64)), dim3(64), 0, st, s, lo_pr, hi, status, tally);
}
void zk_launch_ecc_pair_stage1(hipStream_t st, const EccPairArgs& s, u32 t_lo, u32 t_hi) {
    if (t_hi > t_lo) hipLaunchKernelGGL(ecc_pair_stage1_kernel, dim3((t_hi - t_lo + 63) / 64), dim3(64), 0, st, s, t_lo, t_hi);
}
void zk_launch_fq12_op(hipStream_t st, int op, const u64* x, const u64* y, u64* out, u64 n12) {
    hipLaunchKernelGGL(ecc_fq12_op_kernel, dim3((u32)((n12 + 63) / 64)), dim3(64), 0, st, op, x, y, out, n12);
}
