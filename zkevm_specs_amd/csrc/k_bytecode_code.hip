// Bytecode table + Bytecode-circuit witness + keccak rows from raw contract code (bytecode_code.hpp): the wavefront forms
#include "kernels.hpp"

__device__ __forceinline__ Fr bcc_shfl_up(const Fr& x, int d) {
    Fr r;
#pragma unroll
    for (int k = 0; k < 8; k++) r.v[k] = (u32)__shfl_up((int)x.v[k], d);
    return r;
}
// A wavefront per 64-byte chunk, a lane per byte: ONE coalesced 64-byte load per chunk.  (1) Horner prefix of the chunk's bytes as an
// inclusive scan of the affine maps x -> x r + byte (at distance d the left neighbour's partial times r^d, the table's Montgomery
// powers): lane t ends with sum_{i <= t} byte_i r^(t - i), the chunk's last byte with the chunk's Horner value.  (2) the
// counter-after-the-chunk map by pointer jumping over "the next position entered with 0", as bca_chunk_wave_kernel does over rows.
__global__ __launch_bounds__(64) void bcc_chunk_wave_kernel(BccArgs a) {
    const u64 c = blockIdx.x;
    if (c >= a.p.n_chunks) return;
    const BcaChunk ch = a.p.chunks[c];
    const u32 t = threadIdx.x;
    const bool valid = t < ch.count;
    const u64 g = (u64)ch.start + t;
    const u32 byte = valid ? (u32)a.code[g] : 0u;
    Fr B = fr_from_u64(byte);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const Fr Bp = bcc_shfl_up(B, d);
        const Fr rd = fr_load(a.p.rpow + 4 * (u64)d);
        if (valid && t >= (u32)d) B = fr_add(fr_mont(Bp, rd), B);
    }
    if (valid) bca_store(a.part + 4 * g, B);
    if (t == ch.count - 1u) {
        bca_store(a.p.chunk_acc + 4 * c, B);
        a.p.chunk_m[c] = ch.count;
    }
    const u32 sz = valid ? bcc_push_size(byte) : 0u;
    // zero_out[p] = counter after the chunk when position p is entered with 0: follow nxt until a terminal value
    //   nxt = p + 1 (no push) or p + sz + 1 (push data inside the chunk); terminal: the data runs past the chunk (value = what is left), or p == count (0)
    u32 nxt = t + (sz ? sz + 1u : 1u), val = 0;
    bool term = !valid;  // lanes at and past `count`: terminal 0
    if (valid && sz && t + sz + 1u > ch.count) { term = true; val = sz - (ch.count - 1u - t); }
#pragma unroll
    for (int round = 0; round < 7; round++) {  // (six doublings cover a chain of 64 links; one more for the final adoption)
        const u32 src = nxt < 64u ? nxt : 63u;
        const u32 n_term = (u32)__shfl((int)(term ? 1u : 0u), (int)src), n_val = (u32)__shfl((int)val, (int)src), n_nxt = (u32)__shfl((int)nxt, (int)src);
        if (!term) {
            if (nxt >= ch.count) { term = true; val = 0; }  // position `count`: the chunk ends with the counter at 0
            else if (n_term) { term = true; val = n_val; }
            else nxt = n_nxt;
        }
    }
    // map[left], left = 0..32: the first `left` bytes are push data, then position `left` is entered with 0 (lane t holds zero_out[t])
    uint8_t* map = a.p.chunk_map + c * BCA_MAP_STRIDE;
    if (t <= 32u) map[t] = (uint8_t)(t < ch.count ? val : (t == ch.count ? 0u : t - ch.count));
}
// A lane per OUTPUT row: table row i and circuit row i (bcc_write_row), over max(table rows, 2^k) lanes
__global__ __launch_bounds__(256) void bcc_rows_kernel(BccArgs a, u64 n_lanes, u32* status, ZkTally* tally) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_lanes) {
        bcc_write_row(a, i);
        if (status && i < a.n_rows) status[i] = 0;  // the assignment has no failure modes of its own
    }
    tally_commit(tally, i, 0);
}
// One pass.  The keccak rows only feed the row writer (the code hash): with a side stream the keccak kernels — the long-message one
// is a chain of len / 136 permutations per code — fork off first and the byte scans run beside them; the row writer waits for the join.
// Without one they follow the scans on st.
void zk_launch_bytecode_from_code(hipStream_t st, hipStream_t side, hipEvent_t ev_fork, hipEvent_t ev_join, const BccArgs& a,
                                  const KeccakGenArgs& g, u32* status, ZkTally* tally) {
    if (a.n_codes && side) {
        (void)hipEventRecord(ev_fork, st);
        (void)hipStreamWaitEvent(side, ev_fork, 0);
        zk_launch_keccak_table(side, g, nullptr, tally);
        (void)hipEventRecord(ev_join, side);
    }
    if (a.p.n_chunks) {
        hipLaunchKernelGGL(bcc_chunk_wave_kernel, dim3((u32)a.p.n_chunks), dim3(64), 0, st, a);
        zk_launch_bca_prefix(st, a.p);
    }
    if (a.n_codes && !side) zk_launch_keccak_table(st, g, nullptr, tally);
    if (a.n_codes && side) (void)hipStreamWaitEvent(st, ev_join, 0);
    const u64 n_lanes = a.n_rows > a.n_out ? a.n_rows : a.n_out;
    if (n_lanes) hipLaunchKernelGGL(bcc_rows_kernel, dim3((u32)((n_lanes + 255) / 256)), dim3(256), 0, st, a, n_lanes, status, tally);
}
