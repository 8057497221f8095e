// Exp circuit witness assignment kernels (exp_assign.hpp), all on the session's stream:
//   open:  exa_size_kernel    one lane per event: domain checks, step count
//          exa_scan_kernel    one block: exclusive scan of the counts -> first row per event, total
//          exa_ident_kernel   one lane per event: identifiers of row-producing events strictly increase
//   pass:  exa_chain_kernel   one lane per event: the power chain, d of every step into the scratch array
//          exa_rows_kernel    one lane per output row: 21 column-major cells + 11 table cells
#include "kernels.hpp"

__global__ __launch_bounds__(256) void exa_size_kernel(ExaArgs a) {
    const u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.n_events) return;
    const u32 reason = exa_event_size(a, e);
    if (reason) atomicMin((unsigned long long*)a.meta, (unsigned long long)exa_reject_word(e, reason));
}

// Every thread sums a contiguous slice of the counts, the slice totals are scanned in LDS, then every thread writes its slice's
// offsets.  One block: the counts are 4 bytes per event and the open waits for the total anyway.
#define EXA_SCAN_BLOCK 1024
__global__ __launch_bounds__(EXA_SCAN_BLOCK) void exa_scan_kernel(ExaArgs a) {
    __shared__ u64 s_sum[EXA_SCAN_BLOCK];
    const u64 per = (a.n_events + EXA_SCAN_BLOCK - 1) / EXA_SCAN_BLOCK;
    const u64 lo = (u64)threadIdx.x * per < a.n_events ? (u64)threadIdx.x * per : a.n_events;
    const u64 hi = lo + per < a.n_events ? lo + per : a.n_events;
    u64 sum = 0;
    for (u64 e = lo; e < hi; e++) sum += a.count[e];
    s_sum[threadIdx.x] = sum;
    __syncthreads();
    for (u32 s = 1; s < EXA_SCAN_BLOCK; s <<= 1) {
        const u64 x = threadIdx.x >= s ? s_sum[threadIdx.x - s] : 0ull;
        __syncthreads();
        s_sum[threadIdx.x] += x;
        __syncthreads();
    }
    u64 run = s_sum[threadIdx.x] - sum;
    for (u64 e = lo; e < hi; e++) {
        a.row0[e] = run;
        run += a.count[e];
    }
    if (threadIdx.x == EXA_SCAN_BLOCK - 1) {
        a.row0[a.n_events] = s_sum[threadIdx.x];
        a.meta[1] = s_sum[threadIdx.x];
    }
}
__global__ __launch_bounds__(256) void exa_ident_kernel(ExaArgs a) {
    const u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.n_events) return;
    const u32 reason = exa_ident_check(a, e);
    if (reason) atomicMin((unsigned long long*)a.meta, (unsigned long long)exa_reject_word(e, reason));
}

// One wavefront per block: a lane's chain is up to 510 dependent 256-bit products, and at a few thousand events the wavefronts
// are what spreads the work over the CUs.
__global__ __launch_bounds__(64) void exa_chain_kernel(ExaArgs a) {
    const u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < a.n_events) exa_chain(a, e);
}
__global__ __launch_bounds__(256) void exa_rows_kernel(ExaArgs a, u32* status, ZkTally* tally) {
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < a.n_rows) {
        exa_write_row(a, j);
        if (status) status[j] = 0;  // the assignment has no failure modes of its own (domain checks happen at open)
    }
    tally_commit(tally, j, 0);
}

// open: counts, first rows and the reject word (a.meta[0] preset to EXA_NO_REJECT, a.meta[1] to 0 by the caller)
void zk_launch_exp_assign_sizes(hipStream_t st, const ExaArgs& a) {
    if (!a.n_events) return;
    hipLaunchKernelGGL(exa_size_kernel, dim3((u32)((a.n_events + 255) / 256)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(exa_scan_kernel, dim3(1), dim3(EXA_SCAN_BLOCK), 0, st, a);
    hipLaunchKernelGGL(exa_ident_kernel, dim3((u32)((a.n_events + 255) / 256)), dim3(256), 0, st, a);
}
void zk_launch_exp_assign(hipStream_t st, const ExaArgs& a, u32* status, ZkTally* tally) {
    if (a.n_step) hipLaunchKernelGGL(exa_chain_kernel, dim3((u32)((a.n_events + 63) / 64)), dim3(64), 0, st, a);
    if (a.n_rows) hipLaunchKernelGGL(exa_rows_kernel, dim3((u32)((a.n_rows + 255) / 256)), dim3(256), 0, st, a, status, tally);
}
