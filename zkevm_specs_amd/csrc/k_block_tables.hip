// EVM circuit tx, block and withdrawal tables from raw block data (block_tables.hpp): the lane mappings
#include "kernels.hpp"

// Non-zero calldata bytes per block of BTB_GAS_BLOCK bytes: a lane per aligned 16-byte piece (a wavefront loads a contiguous KiB),
// sixteen lanes per block.  The pieces that stick out of the buffer at its two ends are read byte by byte (btb_gas_chunk).
__global__ __launch_bounds__(256) void btb_gas_block_kernel(BtbArgs a) {
    const u64 c = (u64)blockIdx.x * 256 + threadIdx.x;
    u32 n = btb_gas_chunk(a, c, a.mis, a.mis + a.n_bytes);  // (0, without a load, for the pieces behind the buffer)
#pragma unroll
    for (int d = BTB_GAS_PIECES / 2; d > 0; d >>= 1) n += (u32)__shfl_xor((int)n, d);
    const u64 b = c / BTB_GAS_PIECES;
    if ((threadIdx.x & (BTB_GAS_PIECES - 1)) == 0 && b < a.n_gas_blocks) a.gas_part[b] = n;
}
// Exclusive prefix of the blocks' counts: one workgroup walks them 1024 at a time (4096 counts per MiB of calldata)
__global__ __launch_bounds__(1024) void btb_gas_scan_kernel(BtbArgs a) {
    __shared__ u32 wsum[16];
    const u32 t = threadIdx.x, lane = t & 63u, w = t >> 6;
    u32 carry = 0;
    for (u64 base = 0; base < a.n_gas_blocks; base += 1024) {
        const u64 b = base + t;
        const u32 v = b < a.n_gas_blocks ? a.gas_part[b] : 0u;
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
        if (b < a.n_gas_blocks) a.gas_pre[b] = carry + before + x - v;
        carry += total;
        __syncthreads();
    }
    if (t == 0) a.gas_pre[a.n_gas_blocks] = carry;
}
// One launch, three ranges of workgroups:
//   [0, nb_pieces)   the tx table, a lane per 16-byte piece of the row-major output (ten per row): lane L stores at byte 16 L, a
//                    wavefront's store is a contiguous KiB, BTB_WAVE_TILES of them per wavefront, 4 KiB apart.  A wavefront spans at most 8 rows and a tx has at least 12, so the rows'
//                    tx is the one of the wavefront's first row — a.wave_tx, made from the offsets at open — or the next: the index and
//                    three offsets are wave-uniform loads, and no lane searches (with a binary search per wavefront, ten dependent loads in
//                    front of every store, a pass over 2^20 calldata bytes took 0.122 ms; with the index 0.069)
//   [.., + nb_flags) the flags and the per-row status, a lane per row (uint32 streams); the row's tx from the same index
//   the rest         the block table and the withdrawal table, a lane per row
enum { BTB_WAVE_TILES = 4 };  // KiB of the tx table per wavefront (one KiB per wavefront: the same pass 0.069 ms, four: 0.065)
__global__ __launch_bounds__(256) void btb_rows_kernel(BtbArgs a, u32 nb_pieces, u32 nb_flags, u32* status) {
    const u32 blk = blockIdx.x;
    if (blk < nb_pieces) {
        const u64 n_pieces = a.n_tx_rows * BTB_TX_PIECES;
        const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
#pragma unroll
        for (u32 j = 0; j < BTB_WAVE_TILES; j++) {  // (independent KiB pieces: their loads overlap)
            const u64 w = ((u64)blk * BTB_WAVE_TILES + j) * 4 + wave;
            const u64 L0 = 64 * w;
            if (L0 >= n_pieces) break;
            u64 i = a.wave_tx[w];
            const bool more = i + 1 < a.n_txs;
            u64 o0 = a.offs[i], o1 = a.offs[i + 1];
            const u64 o2 = more ? a.offs[i + 2] : o1;
            const u64 L = L0 + (threadIdx.x & 63u);
            if (L >= n_pieces) break;  // (the table's last, partial KiB: nothing follows it)
            const u64 row = L / BTB_TX_PIECES;
            const u32 q = (u32)(L - row * BTB_TX_PIECES);
            if (more && (u64)BTB_TX_FIXED * (i + 1) + o1 <= row) { i++; o0 = o1; o1 = o2; }
            u64 w0, w1;
            btb_tx_piece(a, i, o0, o1, row, q, w0, w1);
            *(uint4*)(a.tx + 2 * L) = make_uint4((u32)w0, (u32)(w0 >> 32), (u32)w1, (u32)(w1 >> 32));
        }
    } else if (blk < nb_pieces + nb_flags) {
        const u64 r = (u64)(blk - nb_pieces) * 256 + threadIdx.x;
        if (r >= a.n_tx_rows) return;
        u64 i = a.wave_tx[(r * BTB_TX_PIECES) >> 6];  // the tx of a row at or before r, less than 12 rows before it
        if (i + 1 < a.n_txs && btb_tx_row0(a, i + 1) <= r) i++;
        a.tx_flags[r] = btb_tx_flag(i, a.offs[i], r);
        if (status) status[r] = 0;  // the assignment has no failing case
    } else {
        const u64 r = (u64)(blk - nb_pieces - nb_flags) * 256 + threadIdx.x;
        if (r < a.n_block_rows) btb_block_row(a, r);
        else if (r - a.n_block_rows < a.n_wd) btb_wd_row(a, r - a.n_block_rows);
    }
}
void zk_launch_block_tables(hipStream_t st, const BtbArgs& a, u32* status) {
    if (a.n_gas_blocks) {
        hipLaunchKernelGGL(btb_gas_block_kernel, dim3((u32)((a.n_gas_blocks * BTB_GAS_PIECES + 255) / 256)), dim3(256), 0, st, a);
        hipLaunchKernelGGL(btb_gas_scan_kernel, dim3(1), dim3(1024), 0, st, a);
    }
    const u32 nb_pieces = (u32)((a.n_tx_rows * BTB_TX_PIECES + 256 * BTB_WAVE_TILES - 1) / (256 * BTB_WAVE_TILES)), nb_flags = (u32)((a.n_tx_rows + 255) / 256);
    const u32 nb_small = (u32)((a.n_block_rows + a.n_wd + 255) / 256);
    if (nb_pieces + nb_flags + nb_small)
        hipLaunchKernelGGL(btb_rows_kernel, dim3(nb_pieces + nb_flags + nb_small), dim3(256), 0, st, a, nb_pieces, nb_flags, status);
}
