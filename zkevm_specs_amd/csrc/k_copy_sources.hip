// The Copy assignment's source data gathered from code, calldata and trace records (copy_sources.hpp): the is_code scan of the code set,
// the gather (a lane per source byte) and the per-event status
#include "kernels.hpp"

// ---- is_code of every byte of the code set ---------------------------------------------------------------------------------------------
// The push-data counter is a recurrence over a code's bytes.  As in bytecode_code.hpp it is cut into 64-byte chunks whose effect is a map
// "counter after the chunk for every counter (0..32) before it"; here a chunk is one wavefront (a lane per byte) and the map needs no
// table: entered with counter 0 at position p the walk p -> p + 1 + push_size(byte p) leaves the chunk at some position >= count, and
// the overshoot is the counter handed on.  Six rounds of pointer doubling (cross-lane reads, no LDS) give every lane its exit.  Entered
// with counter s the chunk is skipped for s bytes and entered with 0 at position s.

// the code that owns unit g of a per-code prefix array first[0..n]: the j with first[j] <= g < first[j + 1] (codes without units are skipped)
__device__ __forceinline__ u32 cps_code_of(const u32* first, u32 n, u32 g) {
    u32 lo = 0, hi = n;  // first[lo] <= g < first[hi]
    while (hi - lo > 1u) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (first[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}
// the chunk's exits: lane p < count gets the overshoot of the walk that enters position p with counter 0; every other lane 0
__device__ __forceinline__ u32 cps_chunk_exits(u32 byte, u32 lane, u32 count) {
    u32 j = lane + 1u + bcc_push_size(byte);
#pragma unroll
    for (int r = 0; r < 6; r++) {  // (every lane reads; only a walk still inside the chunk moves on)
        const u32 t = (u32)__shfl((int)j, (int)(j & 63u));
        if (j < count) j = t;
    }
    return lane < count ? j - count : 0u;
}
// A wavefront per segment of CPS_SEG_CHUNKS chunks of one code: lanes 0..32 carry "the counter entering the current chunk when the segment
// is entered with counter `lane`" through the segment's chunks, leaving it per chunk (chunk_in) and for the whole segment (seg_map).
__global__ __launch_bounds__(256) void cps_seg_kernel(CpsCodeArgs c) {
    const u32 g = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (g >= c.n_segs) return;  // (wavefront-uniform)
    const u32 j = cps_code_of(c.seg0, c.n_codes, g);
    const u64 o0 = c.offsets[j], len = c.offsets[j + 1] - o0;
    const u32 first = (g - c.seg0[j]) * CPS_SEG_CHUNKS;
    const u32 code_chunks = (u32)((len + CPS_CHUNK - 1) / CPS_CHUNK);
    const u32 nch = code_chunks - first < (u32)CPS_SEG_CHUNKS ? code_chunks - first : (u32)CPS_SEG_CHUNKS;
    const uint8_t* bytes = c.code + o0 + (u64)first * CPS_CHUNK;
    const u64 left0 = len - (u64)first * CPS_CHUNK;  // bytes from the segment's start to the end of the code
    u32 cur = lane;
    u32 next = lane < left0 ? bytes[lane] : 0u;
    for (u32 q = 0; q < nch; q++) {
        const u64 left = left0 - (u64)q * CPS_CHUNK;
        const u32 count = left < (u64)CPS_CHUNK ? (u32)left : (u32)CPS_CHUNK;
        const u32 byte = next;
        if (q + 1u < nch) next = (u64)lane + CPS_CHUNK < left ? bytes[(u64)(q + 1u) * CPS_CHUNK + lane] : 0u;  // (the next chunk's byte, under this chunk's rounds)
        if (lane < 33u) c.chunk_in[((u64)c.chunk0[j] + first + q) * CPS_MAP_STRIDE + lane] = (uint8_t)cur;
        const u32 z = cps_chunk_exits(byte, lane, count);
        const u32 t = (u32)__shfl((int)z, (int)(cur & 63u));  // (lane `count` holds 0: a counter that ends with the chunk)
        cur = cur <= count ? t : cur - count;
    }
    if (lane < 33u) c.seg_map[(u64)g * CPS_MAP_STRIDE + lane] = (uint8_t)cur;
}
// A lane per code: the counter entering each of its segments (one dependent byte load per KiB of code)
__global__ __launch_bounds__(64) void cps_code_prefix_kernel(CpsCodeArgs c) {
    const u32 j = blockIdx.x * 64u + threadIdx.x;
    if (j >= c.n_codes) return;
    u32 state = 0;
    for (u32 s = c.seg0[j]; s < c.seg0[j + 1]; s++) {
        c.seg_state[s] = (uint8_t)state;
        state = c.seg_map[(u64)s * CPS_MAP_STRIDE + state];
    }
}
// A wavefront per chunk: the opcode positions are the walk from the chunk's entry counter; the walk itself is wavefront-uniform over
// values the lanes already hold (no load inside it), at most one step per opcode of the chunk.
__global__ __launch_bounds__(256) void cps_mask_kernel(CpsCodeArgs c) {
    const u64 gc = (u64)blockIdx.x * 4u + (threadIdx.x >> 6);
    const u32 lane = threadIdx.x & 63u;
    if (gc >= c.n_chunks) return;  // (wavefront-uniform)
    const u32 j = cps_code_of(c.chunk0, c.n_codes, (u32)gc);
    const u64 o0 = c.offsets[j], len = c.offsets[j + 1] - o0;
    const u32 cc = (u32)gc - c.chunk0[j];
    const u64 left = len - (u64)cc * CPS_CHUNK;
    const u32 count = left < (u64)CPS_CHUNK ? (u32)left : (u32)CPS_CHUNK;
    const u32 byte = lane < count ? c.code[o0 + (u64)cc * CPS_CHUNK + lane] : 0u;
    const u32 entry = c.chunk_in[gc * CPS_MAP_STRIDE + c.seg_state[c.seg0[j] + cc / CPS_SEG_CHUNKS]];
    const u32 step = lane + 1u + bcc_push_size(byte);
    u32 pos = (u32)__builtin_amdgcn_readfirstlane((int)entry);
    u64 m = 0;
    while (pos < count) {
        m |= 1ull << pos;
        pos = (u32)__builtin_amdgcn_readlane((int)step, (int)pos);
    }
    if (lane == 0u) c.mask[gc] = m;
}

// ---- the gather ------------------------------------------------------------------------------------------------------------------------
// A lane per source byte: its event by binary search over the events' first bytes (as the row lanes search row0), cps_byte, one 2-byte
// store (a wavefront's: 128 contiguous bytes).  A failing byte leaves (i << 8 | site) in its event's word by atomicMin.
__global__ __launch_bounds__(256) void cps_gather_kernel(CpsArgs a) {
    const u64 d = (u64)blockIdx.x * 256u + threadIdx.x;
    if (d >= a.n_data) return;
    u64 lo = 0, hi = a.n_events;  // data0[lo] <= d < data0[hi]
    while (hi - lo > 1) {
        const u64 mid = (lo + hi) >> 1;
        if (a.data0[mid] <= d) lo = mid; else hi = mid;
    }
    const u64 i = d - a.data0[lo];
    u32 site;
    const u32 v = cps_byte(a, lo, a.ev[lo], a.sev[lo], i, site);
    a.data[d] = (uint16_t)v;
    if (site) atomicMin(&a.ev_fail[lo], ((unsigned long long)i << 8) | site);
}
// A lane per event: the status word and the tally
__global__ __launch_bounds__(256) void cps_status_kernel(CpsArgs a, u32* status, ZkTally* tally) {
    const u64 e = (u64)blockIdx.x * 256u + threadIdx.x;
    u32 st = 0;
    if (e < a.n_events) {
        st = cps_status(a.sev[e], a.ev_fail[e]);
        status[e] = st;
    }
    tally_commit(tally, e, st);
}

void zk_launch_copy_sources(hipStream_t st, const CpsArgs& a, const CpsCodeArgs& c, u32* status, ZkTally* tally) {
    if (c.n_segs) {  // (0: no event has a Bytecode side, the mask is never read)
        hipLaunchKernelGGL(cps_seg_kernel, dim3((c.n_segs + 3u) / 4u), dim3(256), 0, st, c);
        hipLaunchKernelGGL(cps_code_prefix_kernel, dim3((c.n_codes + 63u) / 64u), dim3(64), 0, st, c);
        hipLaunchKernelGGL(cps_mask_kernel, dim3((u32)((c.n_chunks + 3) / 4)), dim3(256), 0, st, c);
    }
    (void)hipMemsetAsync(a.ev_fail, 0xff, (size_t)a.n_events * 8, st);
    if (a.n_data) hipLaunchKernelGGL(cps_gather_kernel, dim3((u32)((a.n_data + 255) / 256)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(cps_status_kernel, dim3((u32)((a.n_events + 255) / 256)), dim3(256), 0, st, a, status, tally);
}
