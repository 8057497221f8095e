// EVM circuit witness from compact trace records (trace_witness.hpp): the open's check / offset kernels and the row writer
#include "kernels.hpp"

__global__ void trw_verdict_reset_kernel(u64* v) {
    if (threadIdx.x < TRW_V_WORDS) v[threadIdx.x] = threadIdx.x == TRW_V_POOL ? 0ull : TRW_NONE;
}
// The open's checks, a lane per record: blocks [0, nb_rw) the RW ops — reserved head bits, strictly ascending counters (a lane loads
// its neighbour's) — and the session's own copies of the heads and counters; the rest the steps' word 0.  The first offender of each
// kind lands in the verdict block by atomicMin.
__global__ __launch_bounds__(256) void trw_check_kernel(TrwArgs a, u32 nb_rw) {
    if (blockIdx.x < nb_rw) {
        const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
        if (i >= a.n_rw) return;
        const u32 h = a.head_in[i];
        a.head[i] = h;
        if (trw_head_bad(h)) atomicMin((unsigned long long*)&a.verdict[TRW_V_HEAD], (unsigned long long)i);
        if (a.ctr_in) {
            const u64 c = a.ctr_in[i];
            a.ctr[i] = c;
            if (i && c <= a.ctr_in[i - 1]) atomicMin((unsigned long long*)&a.verdict[TRW_V_ORDER], (unsigned long long)i);
        }
    } else {
        const u64 i = (u64)(blockIdx.x - nb_rw) * 256 + threadIdx.x;
        if (i < a.n_steps && trw_step_bad(a.steps_in[i * TRW_STEP_WORDS])) atomicMin((unsigned long long*)&a.verdict[TRW_V_STEP], (unsigned long long)i);
    }
}
// Pool words per row (a popcount of the session's head) and their exclusive prefix: one workgroup walks the rows 1024 at a time, as
// btb_gas_scan_kernel does; the total is the verdict's pool word.
__global__ __launch_bounds__(1024) void trw_offset_scan_kernel(TrwArgs a) {
    __shared__ u32 wsum[16];
    const u32 t = threadIdx.x, lane = t & 63u, w = t >> 6;
    u64 carry = 0;
    for (u64 base = 0; base < a.n_rw; base += 1024) {
        const u64 b = base + t;
        const u32 v = b < a.n_rw ? trw_head_words(a.head[b]) : 0u;
        u32 x = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const u32 y = (u32)__shfl_up((int)x, d);
            if (lane >= (u32)d) x += y;
        }
        if (lane == 63u) wsum[w] = x;
        __syncthreads();
        u32 before = 0, total = 0;
#pragma unroll
        for (u32 k = 0; k < 16; k++) {
            const u32 s = wsum[k];
            if (k < w) before += s;
            total += s;
        }
        if (b < a.n_rw) a.off[b] = carry + before + x - v;
        carry += total;
        __syncthreads();
    }
    if (t == 0) a.verdict[TRW_V_POOL] = carry;
}
void zk_launch_trace_witness_check(hipStream_t st, const TrwArgs& a, bool with_offsets) {
    hipLaunchKernelGGL(trw_verdict_reset_kernel, dim3(1), dim3(64), 0, st, a.verdict);
    const u32 nb_rw = (u32)((a.n_rw + 255) / 256), nb_steps = (u32)((a.n_steps + 255) / 256);
    if (nb_rw + nb_steps) hipLaunchKernelGGL(trw_check_kernel, dim3(nb_rw + nb_steps), dim3(256), 0, st, a, nb_rw);
    if (a.n_rw && with_offsets) hipLaunchKernelGGL(trw_offset_scan_kernel, dim3(1), dim3(1024), 0, st, a);
}

// One launch, three ranges of workgroups:
//   [0, nb_rw)       the RW table, a lane per 16-byte piece of the row-major output (28 per row): lane L stores at byte 16 L, so a
//                    wavefront's store is a contiguous KiB, TRW_WAVE_TILES of them per wavefront, 4 KiB apart (btb_rows_kernel's shape).
//                    A wavefront spans 3 or 4 rows; the lanes of a row load its head and offset from one address.
//   [.., + nb_steps) the step table in the same shape (26 pieces per row)
//   the rest         the flags and the per-row status, a lane per row (uint32 streams)
enum { TRW_WAVE_TILES = 4 };
__global__ __launch_bounds__(256) void trw_rows_kernel(TrwArgs a, u32 nb_rw, u32 nb_steps, u32* status) {
    const u32 blk = blockIdx.x;
    if (blk < nb_rw) {
        const u64 n_pieces = a.n_rw * TRW_RW_PIECES;
        const u64 L0 = (u64)blk * (256 * TRW_WAVE_TILES), row0 = L0 / TRW_RW_PIECES;  // (block-uniform: the one 64-bit division)
        const u32 q0 = (u32)(L0 - row0 * TRW_RW_PIECES);
#pragma unroll
        for (u32 j = 0; j < TRW_WAVE_TILES; j++) {  // (independent KiB pieces: their loads overlap)
            const u32 l = j * 256 + threadIdx.x;
            const u64 L = L0 + l;
            if (L >= n_pieces) break;  // (L grows with j)
            const u32 dr = (q0 + l) / TRW_RW_PIECES;  // (32-bit, by a constant)
            const u64 row = row0 + dr;
            const u32 q = q0 + l - dr * TRW_RW_PIECES;
            u64 w0, w1;
            trw_rw_piece(a, row, a.head[row], a.off[row], q, w0, w1);
            *(uint4*)(a.rw + 2 * L) = make_uint4((u32)w0, (u32)(w0 >> 32), (u32)w1, (u32)(w1 >> 32));
        }
    } else if (blk < nb_rw + nb_steps) {
        const u64 n_pieces = a.n_steps * TRW_STEP_PIECES;
        const u64 L0 = (u64)(blk - nb_rw) * (256 * TRW_WAVE_TILES), row0 = L0 / TRW_STEP_PIECES;
        const u32 q0 = (u32)(L0 - row0 * TRW_STEP_PIECES);
#pragma unroll
        for (u32 j = 0; j < TRW_WAVE_TILES; j++) {
            const u32 l = j * 256 + threadIdx.x;
            const u64 L = L0 + l;
            if (L >= n_pieces) break;
            const u32 dr = (q0 + l) / TRW_STEP_PIECES;
            const u32 q = q0 + l - dr * TRW_STEP_PIECES;
            u64 w0, w1;
            trw_step_piece(a, row0 + dr, q, w0, w1);
            *(uint4*)(a.steps + 2 * L) = make_uint4((u32)w0, (u32)(w0 >> 32), (u32)w1, (u32)(w1 >> 32));
        }
    } else {
        const u64 r = (u64)(blk - nb_rw - nb_steps) * 256 + threadIdx.x;
        if (r >= a.n_rw) return;
        a.rw_flags[r] = trw_rw_flag(a.head[r]);
        if (status) status[r] = 0;  // the assignment has no failing case
    }
}
void zk_launch_trace_witness(hipStream_t st, const TrwArgs& a, u32* status) {
    const u32 per = 256 * TRW_WAVE_TILES;
    const u32 nb_rw = (u32)((a.n_rw * TRW_RW_PIECES + per - 1) / per), nb_steps = (u32)((a.n_steps * TRW_STEP_PIECES + per - 1) / per);
    const u32 nb_flags = (u32)((a.n_rw + 255) / 256);
    if (nb_rw + nb_steps + nb_flags)
        hipLaunchKernelGGL(trw_rows_kernel, dim3(nb_rw + nb_steps + nb_flags), dim3(256), 0, st, a, nb_rw, nb_steps, status);
}
