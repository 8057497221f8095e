// PI circuit witness assignment kernels (pi_assign.hpp), all on the session's stream:
//   open:  pia_check_kernel      one lane per input field / offset pair: the reject word
//          pia_rpow_kernel       keccak_rand^k in Montgomery form, k <= PIA_TILE
//          pia_inv_small_kernel  k^-1 for the small integers the calldata rows divide by (tx ids, their differences, bytes): one
//                                Fermat chain per entry, max(MAX_TXS, 255) + 1 lanes — the byte table and the lane per tx of one
//                                kernel, at open only (the host backend derives the same table from one inversion of a factorial)
//   pass:  pia_gas_tile_kernel   calldata gas cost: prefix sums inside tiles of 4,096 bytes (16 per lane + an LDS scan)
//          pia_gas_scan_kernel   one block: exclusive scan of the tile totals
//          pia_tx_inv_kernel     one lane per fixed tx-table row: value.lo^-1 (Fermat), one wavefront per block
//          pia_bytes_kernel      one lane per row: its byte into the generation-order buffer
//          (the keccak-table kernels over that buffer: digest, input RLC, length — on the device's side stream)
//          pia_rlc_tile_kernel   suffix RLC of 8 rows per lane + an LDS scan over the 256 lanes of a tile
//          pia_rlc_carry_kernel  one block: the suffix scan over the tile totals
//          pia_rows_kernel       one lane per row: 24 column-major cells, table rows, constraints
//          pia_patch_kernel      one lane: what depends on the digest
#include "kernels.hpp"

__global__ __launch_bounds__(256) void pia_check_kernel(PiaArgs a) {
    const u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < PIA_N_CHECKS(a) && !pia_check(a, k)) atomicMin((unsigned long long*)a.meta, (unsigned long long)k);
}
__global__ __launch_bounds__(256) void pia_rpow_kernel(PiaArgs a) {
    const u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (k <= (u64)PIA_TILE) pia_store_fr(a.rpow + 4 * k, pia_pow_mont(fr_to_mont(a.rand), k));
}
__global__ __launch_bounds__(64) void pia_inv_small_kernel(PiaArgs a) {
    const u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < a.n_inv) pia_small_inverse(a, k);
}
__global__ __launch_bounds__(64) void pia_tx_inv_kernel(PiaArgs a) {
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < PIA_TX_LEN * a.max_txs) pia_tx_inverse(a, r);
}

__global__ __launch_bounds__(256) void pia_gas_tile_kernel(PiaArgs a) {
    __shared__ u32 s_sum[256];
    const u64 base = ((u64)blockIdx.x * 256 + threadIdx.x) * PIA_GAS_LANE;
    u32 sum = 0;
    for (u32 k = 0; k < (u32)PIA_GAS_LANE; k++)
        if (base + k < a.total_cd) sum += a.calldata[base + k] ? 16u : 4u;
    s_sum[threadIdx.x] = sum;
    __syncthreads();
    for (u32 s = 1; s < 256; s <<= 1) {
        const u32 x = threadIdx.x >= s ? s_sum[threadIdx.x - s] : 0u;
        __syncthreads();
        s_sum[threadIdx.x] += x;
        __syncthreads();
    }
    u32 run = s_sum[threadIdx.x] - sum;
    for (u32 k = 0; k < (u32)PIA_GAS_LANE; k++)
        if (base + k < a.total_cd) {
            run += a.calldata[base + k] ? 16u : 4u;
            a.gas_local[base + k] = run;
        }
    if (threadIdx.x == 255) a.gas_tile[blockIdx.x] = s_sum[255];
}
#define PIA_SCAN_BLOCK 1024
__global__ __launch_bounds__(PIA_SCAN_BLOCK) void pia_gas_scan_kernel(PiaArgs a) {
    __shared__ u64 s_sum[PIA_SCAN_BLOCK];
    const u64 nt = a.n_gas_tiles, per = (nt + PIA_SCAN_BLOCK - 1) / PIA_SCAN_BLOCK;
    const u64 lo = (u64)threadIdx.x * per < nt ? (u64)threadIdx.x * per : nt;
    const u64 hi = lo + per < nt ? lo + per : nt;
    u64 sum = 0;
    for (u64 k = lo; k < hi; k++) sum += a.gas_tile[k];
    s_sum[threadIdx.x] = sum;
    __syncthreads();
    for (u32 s = 1; s < PIA_SCAN_BLOCK; s <<= 1) {
        const u64 x = threadIdx.x >= s ? s_sum[threadIdx.x - s] : 0ull;
        __syncthreads();
        s_sum[threadIdx.x] += x;
        __syncthreads();
    }
    u64 run = s_sum[threadIdx.x] - sum;
    for (u64 k = lo; k < hi; k++) {
        const u64 t = a.gas_tile[k];
        a.gas_tile[k] = run;
        run += t;
    }
}

__global__ __launch_bounds__(256) void pia_bytes_kernel(PiaArgs a) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.n) pia_row_byte(a, i);
}

// A lane folds its slice of 8 rows, then the 256 slices of the tile are scanned from the back: after the step with distance d
// lane t holds the sum over slices t .. t + 2d - 1, each weighted with rand^(8 (slice - t)).
__global__ __launch_bounds__(256) void pia_rlc_tile_kernel(PiaArgs a) {
    __shared__ Fr s_acc[256];
    const u64 s = (u64)blockIdx.x * 256 + threadIdx.x;
    Fr acc = pia_horner(a, s * PIA_SLICE, (s + 1) * PIA_SLICE);
    s_acc[threadIdx.x] = acc;
    __syncthreads();
    for (u32 d = 1; d < 256; d <<= 1) {
        const bool has = threadIdx.x + d < 256u;
        const Fr other = has ? s_acc[threadIdx.x + d] : fr_zero();
        __syncthreads();
        if (has) acc = fr_add(acc, fr_mulc(other, fr_load(a.rpow + 4 * (u64)(PIA_SLICE * d))));
        s_acc[threadIdx.x] = acc;
        __syncthreads();
    }
    pia_store_fr(a.slice_acc + 4 * s, acc);
    if (threadIdx.x == 0) pia_store_fr(a.tile_acc + 4 * (u64)blockIdx.x, acc);
}
// carry[k] = tile_acc[k] + rand^PIA_TILE * carry[k + 1]: a lane folds its run of tiles, the runs are scanned from the back with
// rand^(PIA_TILE * per), and every lane walks its run once more with the value that comes in from behind it
__global__ __launch_bounds__(PIA_SCAN_BLOCK) void pia_rlc_carry_kernel(PiaArgs a) {
    __shared__ Fr s_acc[PIA_SCAN_BLOCK];
    const u64 nt = a.n_tiles, per = (nt + PIA_SCAN_BLOCK - 1) / PIA_SCAN_BLOCK;
    const u64 lo = (u64)threadIdx.x * per < nt ? (u64)threadIdx.x * per : nt;
    const u64 hi = lo + per < nt ? lo + per : nt;
    const Fr tile_m = fr_load(a.rpow + 4 * (u64)PIA_TILE);
    Fr acc = fr_zero();
    for (u64 k = hi; k-- > lo;) acc = fr_add(fr_mulc(acc, tile_m), fr_load(a.tile_acc + 4 * k));
    s_acc[threadIdx.x] = acc;
    __syncthreads();
    Fr step_m = pia_pow_mont(tile_m, per);
    for (u32 d = 1; d < PIA_SCAN_BLOCK; d <<= 1) {
        const bool has = threadIdx.x + d < (u32)PIA_SCAN_BLOCK;
        const Fr other = has ? s_acc[threadIdx.x + d] : fr_zero();
        __syncthreads();
        if (has) acc = fr_add(acc, fr_mulc(other, step_m));
        s_acc[threadIdx.x] = acc;
        step_m = fr_mont(step_m, step_m);
        __syncthreads();
    }
    Fr c = threadIdx.x + 1 < (u32)PIA_SCAN_BLOCK ? s_acc[threadIdx.x + 1] : fr_zero();
    for (u64 k = hi; k-- > lo;) {
        c = fr_add(fr_mulc(c, tile_m), fr_load(a.tile_acc + 4 * k));
        pia_store_fr(a.carry + 4 * k, c);
    }
    if (threadIdx.x == 0) pia_store_fr(a.carry + 4 * nt, fr_zero());
}

__global__ __launch_bounds__(256) void pia_rows_kernel(PiaArgs a, u32* status, ZkTally* tally) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.n) {
        pia_write_row(a, i);
        if (status) status[i] = 0;  // the assignment has no failure modes of its own (domain checks happen at open)
    }
    tally_commit(tally, i, 0);
}
__global__ void pia_patch_kernel(PiaArgs a) {
    if (blockIdx.x == 0 && threadIdx.x == 0) pia_patch(a);
}

// sizes / open: the reject word (a.meta[0] preset to PIA_NO_REJECT by the caller)
void zk_launch_pi_assign_check(hipStream_t st, const PiaArgs& a) {
    hipLaunchKernelGGL(pia_check_kernel, dim3((u32)((PIA_N_CHECKS(a) + 255) / 256)), dim3(256), 0, st, a);
}
// open: the power table and the small inverses
void zk_launch_pi_assign_tables(hipStream_t st, const PiaArgs& a) {
    hipLaunchKernelGGL(pia_rpow_kernel, dim3((PIA_TILE + 256) / 256), dim3(256), 0, st, a);
    hipLaunchKernelGGL(pia_inv_small_kernel, dim3((u32)((a.n_inv + 63) / 64)), dim3(64), 0, st, a);
}
// One pass.  The digest only feeds pia_patch_kernel: with a side stream the keccak kernels fork off behind the byte pass and the scans
// and the row writer run beside them; the patch kernel waits for the join.
void zk_launch_pi_assign(hipStream_t st, hipStream_t side, hipEvent_t ev_fork, hipEvent_t ev_join, const PiaArgs& a, const KeccakGenArgs& g,
                         u32* status, ZkTally* tally) {
    if (a.total_cd) {
        hipLaunchKernelGGL(pia_gas_tile_kernel, dim3((u32)a.n_gas_tiles), dim3(256), 0, st, a);
        hipLaunchKernelGGL(pia_gas_scan_kernel, dim3(1), dim3(PIA_SCAN_BLOCK), 0, st, a);
    }
    hipLaunchKernelGGL(pia_tx_inv_kernel, dim3((u32)((PIA_TX_LEN * a.max_txs + 63) / 64)), dim3(64), 0, st, a);
    hipLaunchKernelGGL(pia_bytes_kernel, dim3((u32)((a.n + 255) / 256)), dim3(256), 0, st, a);
    if (side) {
        (void)hipEventRecord(ev_fork, st);
        (void)hipStreamWaitEvent(side, ev_fork, 0);
        zk_launch_keccak_table(side, g, nullptr, tally);
        (void)hipEventRecord(ev_join, side);
    } else {
        zk_launch_keccak_table(st, g, nullptr, tally);
    }
    hipLaunchKernelGGL(pia_rlc_tile_kernel, dim3((u32)a.n_tiles), dim3(256), 0, st, a);
    hipLaunchKernelGGL(pia_rlc_carry_kernel, dim3(1), dim3(PIA_SCAN_BLOCK), 0, st, a);
    hipLaunchKernelGGL(pia_rows_kernel, dim3((u32)((a.n + 255) / 256)), dim3(256), 0, st, a, status, tally);
    if (side) (void)hipStreamWaitEvent(st, ev_join, 0);
    hipLaunchKernelGGL(pia_patch_kernel, dim3(1), dim3(64), 0, st, a);
}
