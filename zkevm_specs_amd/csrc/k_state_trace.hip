// State circuit from compact trace records (state_trace.hpp): the re-keying's front end over records in input order, the op list and the
// sorted packed op stream behind the radix passes of k_rekey.hip, and the fused State pass over that stream.
//   open:    strc_offset_*_kernel  the per-row pool offsets by a chunked scan (behind the trace session's trw_check_kernel)
//            strc_scan_kernel      class masks and counts, rwk_scan_kernel's layout                       -> host plan (rwk_build_plan)
//   launch:  strc_collect_kernel   members of the plan's rank jobs (then rwk_rank_kernel)
//            strc_pack_kernel / strc_pack64_kernel   compact keys + per-row status + tally (then the radix passes)
//            strc_emit_kernel      ops[12][n_ops] + flags in sorted order (ops form)
//            strc_stream_kernel    the sorted packed op stream (verdict form), then the MPT passes of k_assign.hip over it
//            state_rows_trace_kernel   the State circuit on rows computed from the stream in registers
// The front-end kernels are rwk_scan / collect / pack / pack64 / emit with the row source exchanged: one lane per record, every array
// read once, coalesced (4-8 bytes per lane and array against 448 bytes per lane of the wire rows).
#include "kernels.hpp"
#include "state_trace.hpp"

#define STRC_BLOCK 256
#define STRC_MASK_WORDS (RWK_NCLASSES * RWK_NFIELDS * 8)
#define STRC_SCAN_BLOCK 1024

__device__ __forceinline__ u32 strc_wave_or(u32 v) {  // (rwk_wave_or)
    v |= (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, false);   // quad_perm [1, 0, 3, 2]
    v |= (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, false);   // quad_perm [2, 3, 0, 1]
    v |= (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, false);  // row_half_mirror
    v |= (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xf, 0xf, false);  // row_mirror
    return (u32)__builtin_amdgcn_readlane((int)v, 0) | (u32)__builtin_amdgcn_readlane((int)v, 16) |
           (u32)__builtin_amdgcn_readlane((int)v, 32) | (u32)__builtin_amdgcn_readlane((int)v, 48);
}

// ---- open: the per-row pool offsets ------------------------------------------------------------------------------------------------------
// trw_offset_scan_kernel's result (off[i] = pool words of the rows before i, the total in the verdict block) in three launches instead of
// one workgroup walking the table: that walk is 0.625 ms for 696 k rows, two thirds of a whole one-shot here, where the trace session pays
// it once per open.  Chunks of 1024 rows: their sums, one workgroup's exclusive scan over the sums, then every chunk's local scan.
#define STRC_OFF_CHUNK 1024
__device__ __forceinline__ u32 strc_chunk_scan(u32 v, u32* wsum, u32& total) {  // inclusive scan over the block's 1024 lanes (wsum: 16 words of LDS)
    const u32 t = threadIdx.x, lane = t & 63u, w = t >> 6;
    u32 x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u32 y = (u32)__shfl_up((int)x, d);
        if (lane >= (u32)d) x += y;
    }
    if (lane == 63u) wsum[w] = x;
    __syncthreads();
    u32 before = 0;
    total = 0;
#pragma unroll
    for (u32 k = 0; k < 16; k++) {
        const u32 s = wsum[k];
        if (k < w) before += s;
        total += s;
    }
    __syncthreads();
    return before + x;
}
__global__ __launch_bounds__(STRC_OFF_CHUNK) void strc_offset_sums_kernel(const u32* head, u64 n, u64* sums) {
    __shared__ u32 wsum[16];
    const u64 i = (u64)blockIdx.x * STRC_OFF_CHUNK + threadIdx.x;
    u32 total;
    strc_chunk_scan(i < n ? trw_head_words(head[i]) : 0u, wsum, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
// sums[c] -> the words before chunk c; the grand total is the verdict's pool word (one workgroup, 1024 chunks per round)
__global__ __launch_bounds__(STRC_OFF_CHUNK) void strc_offset_base_kernel(u64* sums, u32 n_chunks, u64* verdict) {
    __shared__ u32 wsum[16];
    u64 carry = 0;
    for (u32 base = 0; base < n_chunks; base += STRC_OFF_CHUNK) {
        const u32 c = base + threadIdx.x;
        const u32 v = c < n_chunks ? (u32)sums[c] : 0u;  // (a chunk holds at most 5 * 1024 words)
        u32 total;
        const u32 incl = strc_chunk_scan(v, wsum, total);
        if (c < n_chunks) sums[c] = carry + incl - v;
        carry += total;
    }
    if (threadIdx.x == 0) verdict[TRW_V_POOL] = carry;
}
__global__ __launch_bounds__(STRC_OFF_CHUNK) void strc_offset_rows_kernel(const u32* head, u64 n, const u64* sums, u64* off) {
    __shared__ u32 wsum[16];
    const u64 i = (u64)blockIdx.x * STRC_OFF_CHUNK + threadIdx.x;
    const u32 v = i < n ? trw_head_words(head[i]) : 0u;
    u32 total;
    const u32 incl = strc_chunk_scan(v, wsum, total);
    if (i < n) off[i] = sums[blockIdx.x] + incl - v;
}
// the trace session's checks (its kernels, without its single-workgroup scan), then the offsets; sums: [ceil(n_rw / 1024)] words of scratch
void zk_launch_state_trace_check(hipStream_t st, const TrwArgs& a, u64* sums) {
    zk_launch_trace_witness_check(st, a, false);
    const u32 n_chunks = (u32)((a.n_rw + STRC_OFF_CHUNK - 1) / STRC_OFF_CHUNK);
    hipLaunchKernelGGL(strc_offset_sums_kernel, dim3(n_chunks), dim3(STRC_OFF_CHUNK), 0, st, a.head, a.n_rw, sums);
    hipLaunchKernelGGL(strc_offset_base_kernel, dim3(1), dim3(STRC_OFF_CHUNK), 0, st, sums, n_chunks, a.verdict);
    hipLaunchKernelGGL(strc_offset_rows_kernel, dim3(n_chunks), dim3(STRC_OFF_CHUNK), 0, st, a.head, a.n_rw, sums, a.off);
}

// ---- open: class masks (masks: u32[2][16][5][8] OR / OR of complements, then u32[16] row counts) --------------------------------------
// Field words are those of the 256-bit cell: zero for the words a uint64 cannot reach, the pool word's for wide cells; the "seen zero"
// shortcut of rwk_scan_kernel takes almost all of them.
__global__ __launch_bounds__(STRC_SCAN_BLOCK) void strc_scan_kernel(RekeyArgs a, StrcArgs src) {
    __shared__ u32 s_or[STRC_MASK_WORDS], s_nand[STRC_MASK_WORDS], s_cnt[RWK_NCLASSES], s_zero[RWK_NCLASSES][2];
    for (u32 t = threadIdx.x; t < STRC_MASK_WORDS; t += STRC_SCAN_BLOCK) { s_or[t] = 0; s_nand[t] = 0; }
    if (threadIdx.x < RWK_NCLASSES) { s_cnt[threadIdx.x] = 0; s_zero[threadIdx.x][0] = 0; s_zero[threadIdx.x][1] = 0; }
    __syncthreads();
    const u32 lane = threadIdx.x & 63u;
    for (u64 base = (u64)blockIdx.x * STRC_SCAN_BLOCK; base < a.n; base += (u64)gridDim.x * STRC_SCAN_BLOCK) {
        const u64 i = base + threadIdx.x;
        const bool valid = i < a.n;
        RwkKey k;
        if (valid) k = strc_key(strc_load_row(src, i));
        else { k.cls = RWK_CLASS_DROPPED; k.status = 0; for (int f = 0; f < RWK_NFIELDS; f++) k.f[f] = fr_zero(); }
        unsigned long long rem = __ballot(valid);
        while (rem) {  // one round per class present in the wave
            const int first = __ffsll((long long)rem) - 1;
            const u32 c = (u32)__builtin_amdgcn_readlane((int)k.cls, first);
            const unsigned long long inc = __ballot(valid && k.cls == c);
            rem &= ~inc;
            const bool in = valid && k.cls == c;
            if (lane == 0) atomicAdd(&s_cnt[c], (u32)__popcll(inc));
            if (c == RWK_CLASS_DROPPED) continue;
            u32 zero_lo = 0, zero_hi = 0;  // (f * 8 + w): words 0..31 / 32..39
#pragma unroll
            for (int f = 0; f < RWK_NFIELDS; f++) {
#pragma unroll
                for (int w = 0; w < 8; w++) {
                    const u32 v = k.f[f].v[w];
                    if (__ballot(in && v != 0u) == 0ull) {
                        if (f * 8 + w < 32) zero_lo |= 1u << ((f * 8 + w) & 31);
                        else zero_hi |= 1u << ((f * 8 + w) & 31);
                        continue;
                    }
                    const u32 v0 = (u32)__builtin_amdgcn_readlane((int)v, first);
                    u32 orv = v0, nandv = ~v0;
                    if (__ballot(in && v != v0)) {
                        orv = strc_wave_or(in ? v : 0u);
                        nandv = strc_wave_or(in ? ~v : 0u);
                    }
                    if (lane == 0) {
                        const u32 slot = (c * RWK_NFIELDS + f) * 8 + w;
                        atomicOr(&s_or[slot], orv);
                        atomicOr(&s_nand[slot], nandv);
                    }
                }
            }
            if (lane == 0) {
                if (zero_lo) atomicOr(&s_zero[c][0], zero_lo);
                if (zero_hi) atomicOr(&s_zero[c][1], zero_hi);
            }
        }
    }
    __syncthreads();
    for (u32 t = threadIdx.x; t < STRC_MASK_WORDS; t += STRC_SCAN_BLOCK) {
        const u32 c = t / (RWK_NFIELDS * 8), fw = t % (RWK_NFIELDS * 8);
        const u32 o = s_or[t], nn = s_nand[t] | (((s_zero[c][fw >> 5] >> (fw & 31)) & 1u) ? 0xffffffffu : 0u);
        if (o && (__atomic_load_n(&a.masks[t], __ATOMIC_RELAXED) & o) != o) atomicOr(&a.masks[t], o);
        if (nn && (__atomic_load_n(&a.masks[STRC_MASK_WORDS + t], __ATOMIC_RELAXED) & nn) != nn) atomicOr(&a.masks[STRC_MASK_WORDS + t], nn);
    }
    if (threadIdx.x < RWK_NCLASSES && s_cnt[threadIdx.x]) atomicAdd(&a.masks[2 * STRC_MASK_WORDS + threadIdx.x], s_cnt[threadIdx.x]);
}

// ---- launch: rank-job members, compact keys ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(STRC_BLOCK) void strc_collect_kernel(RekeyArgs a, StrcArgs src) {
    const u64 i = (u64)blockIdx.x * STRC_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const RwkKey k = strc_key(strc_load_row(src, i));
    for (u32 j = 0; j < a.n_jobs; j++) {
        const RwkRankJob job = a.jobs[j];
        if (job.cls != k.cls) continue;
        const u32 pos = atomicAdd(&a.job_cursor[j], 1u);
        a.job_rows[job.base + pos] = (u32)i;
        Fr v = fr_zero();
#pragma unroll
        for (int f = 0; f < RWK_NFIELDS; f++)
            if (job.field == (u32)f) v = k.f[f];
        rwk_store(a.job_vals + (u64)(job.base + pos) * 4, v);
    }
}
__global__ __launch_bounds__(STRC_BLOCK) void strc_pack_kernel(RekeyArgs a, StrcArgs src, u32* status, ZkTally* tally) {
    __shared__ RwkPlan s_plan;
    {
        const u32* from = (const u32*)a.plan;
        u32* dst = (u32*)&s_plan;
        for (u32 t = threadIdx.x; t < sizeof(RwkPlan) / 4; t += STRC_BLOCK) dst[t] = from[t];
    }
    __syncthreads();
    const u64 i = (u64)blockIdx.x * STRC_BLOCK + threadIdx.x;
    u32 code = 0;
    if (i < a.n) {
        const RwkKey k = strc_key(strc_load_row(src, i));
        u32 ranks[RWK_NFIELDS];
#pragma unroll
        for (int f = 0; f < RWK_NFIELDS; f++) ranks[f] = a.ranks[f] ? a.ranks[f][i] : 0u;
        rwk_pack(s_plan, s_plan.cls[k.cls], k, ranks, a.keys + i, a.n);
        code = k.status;
        if (status) status[i] = code;
    }
    tally_commit(tally, i, code);
}
// keys of at most 64 bits: one u64 per row and the digit histograms of all passes on the way (rwk_pack64_kernel)
__global__ __launch_bounds__(1024) void strc_pack64_kernel(RekeyArgs a, StrcArgs src, u32* status, ZkTally* tally) {
    __shared__ RwkPlan s_plan;
    __shared__ u32 s_gh[8 * 256];
    {
        const u32* from = (const u32*)a.plan;
        u32* dst = (u32*)&s_plan;
        for (u32 t = threadIdx.x; t < sizeof(RwkPlan) / 4; t += 1024) dst[t] = from[t];
        for (u32 t = threadIdx.x; t < 8 * 256; t += 1024) s_gh[t] = 0;
    }
    __syncthreads();
    for (u64 base = (u64)blockIdx.x * 1024; base < a.n; base += (u64)gridDim.x * 1024) {
        const u64 i = base + threadIdx.x;
        u32 code = 0;
        if (i < a.n) {
            const RwkKey k = strc_key(strc_load_row(src, i));
            u32 ranks[RWK_NFIELDS];
#pragma unroll
            for (int f = 0; f < RWK_NFIELDS; f++) ranks[f] = a.ranks[f] ? a.ranks[f][i] : 0u;
            u32 w[2] = {0u, 0u};
            rwk_pack(s_plan, s_plan.cls[k.cls], k, ranks, w, 1);
            const u64 key = a.key_words == 2u ? (((u64)w[0] << 32) | (u64)w[1]) : (u64)w[0];
            a.key64_a[i] = key;
            for (u32 p = 0; p < a.n_passes; p++) atomicAdd(&s_gh[p * 256 + (u32)((key >> (8u * p)) & 0xffull)], 1u);
            code = k.status;
            if (status) status[i] = code;
        }
        tally_commit(tally, i, code);
    }
    __syncthreads();
    for (u32 t = threadIdx.x; t < a.n_passes * 256; t += 1024)
        if (s_gh[t]) atomicAdd(&a.sweep[RWK_SWEEP_GHIST + t], s_gh[t]);
}

// ---- behind the sort: the op list (ops form), the sorted packed op stream (verdict form) ---------------------------------------------------
__global__ __launch_bounds__(STRC_BLOCK) void strc_emit_kernel(RekeyArgs a, StrcArgs src, const u32* order) {
    const u64 j = (u64)blockIdx.x * STRC_BLOCK + threadIdx.x;
    if (j >= a.n_ops) return;
    if (j == 0) { rwk_emit_start(a.ops, a.op_flags, a.n_ops); return; }
    const StrcRow R = strc_load_row(src, order[j - 1]);
    const RwkKey k = strc_key(R);
    rwk_emit(a.ops, a.op_flags, a.n_ops, j, k, strc_op(R, k));
}
__global__ __launch_bounds__(STRC_BLOCK) void strc_stream_kernel(StrcArgs src, const u32* order, u64 n_ops) {
    const u64 j = (u64)blockIdx.x * STRC_BLOCK + threadIdx.x;
    if (j >= n_ops) return;
    strc_stream_store(src.stream, j, j == 0 ? strc_stream_start() : strc_load(src, order[j - 1]));
}

void zk_launch_state_trace_scan(hipStream_t st, const RekeyArgs& a, const StrcArgs& src) {
    u32 grid = (u32)((a.n + STRC_SCAN_BLOCK - 1) / STRC_SCAN_BLOCK);
    if (grid > 256u) grid = 256u;
    hipLaunchKernelGGL(strc_scan_kernel, dim3(grid), dim3(STRC_SCAN_BLOCK), 0, st, a, src);
}
// the re-keying and the sort over records; then the op list (a.ops set) or the packed stream (src.stream set)
void zk_launch_state_trace_rekey(hipStream_t st, const RekeyArgs& a, const StrcArgs& src, u32* status, ZkTally* tally) {
    const u32 grid = (u32)((a.n + STRC_BLOCK - 1) / STRC_BLOCK);
    if (a.n_jobs) {
        hipMemsetAsync(a.job_cursor, 0, sizeof(u32) * a.n_jobs, st);
        hipLaunchKernelGGL(strc_collect_kernel, dim3(grid), dim3(STRC_BLOCK), 0, st, a, src);
        zk_launch_rekey_rank_jobs(st, a);
    }
    if (a.fast) {
        zk_rekey_sweep_begin(st, a);
        const u32 g64 = (u32)((a.n + 1023) / 1024);
        hipLaunchKernelGGL(strc_pack64_kernel, dim3(g64 > 256u ? 256u : g64), dim3(1024), 0, st, a, src, status, tally);
    } else {
        hipLaunchKernelGGL(strc_pack_kernel, dim3(grid), dim3(STRC_BLOCK), 0, st, a, src, status, tally);
    }
    const u32* order = zk_launch_rekey_passes(st, a);
    const u32 grid_ops = (u32)((a.n_ops + STRC_BLOCK - 1) / STRC_BLOCK);
    if (a.ops) hipLaunchKernelGGL(strc_emit_kernel, dim3(grid_ops), dim3(STRC_BLOCK), 0, st, a, src, order);
    if (src.stream) hipLaunchKernelGGL(strc_stream_kernel, dim3(grid_ops), dim3(STRC_BLOCK), 0, st, src, order, a.n_ops);
}

// ---- the State circuit on rows computed from the stream (state_rows_fused_kernel's shape: one lane per row, the previous row from the
// neighbouring lane; two tallies) ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void state_rows_trace_kernel(StateTraceArgs a, u32* status, ZkTally* tally, ZkTally* asg_tally) {
    const u32 lane = threadIdx.x & 63u;
    const u64 wave = (u64)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const u64 first = a.eval_lo + wave * ST_ROWS_PER_WAVE;
    const u64 n = a.rows.n;
    const u64 i_raw = lane == 0 ? (first == 0 ? n - 1 : first - 1) : first + lane - 1;
    const bool evaluate = lane != 0 && i_raw < a.eval_hi;
    const u64 i = i_raw >= n ? n - 1 : i_raw;
    StRow C;
    u32 code = 0, asg_code = 0;
    state_row_from_stream(a, i, C, code, asg_code);
    code = state_check_loaded<1>(a, i, C, C, code);
    if (!evaluate) code = asg_code = 0;
    else if (status) status[i] = code;
    tally_commit(tally, i, code);
    tally_commit(asg_tally, i, asg_code);
}
void zk_launch_state_rows_trace(hipStream_t st, const StateArgs& sa, const AssignArgs& g, const StrcArgs& src, u32* status, ZkTally* tally, ZkTally* asg_tally) {
    const int block = 256;
    const u64 rows_per_block = (u64)(block / 64) * ST_ROWS_PER_WAVE;
    const u32 grid = (u32)((sa.eval_hi - sa.eval_lo + rows_per_block - 1) / rows_per_block);
    StateTraceArgs a;
    (StateArgs&)a = sa;
    a.asg = g;
    a.src = src;
    hipLaunchKernelGGL(state_rows_trace_kernel, dim3(grid), dim3(block), 0, st, a, status, tally, asg_tally);
}
