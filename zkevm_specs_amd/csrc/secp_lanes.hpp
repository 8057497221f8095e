// The secp256k1 lane forms: a signature's joint multiplication u1 G + u2 Q runs on 1, 2 or 4 lanes (lanes_per_sig).  One lane runs
// both halves of the GLV split; a lane pair runs one half each; a lane quad adds two lanes for the halves of u1 G (secp256k1.hpp
// ecdsa_partial / ecdsa_partial4).  ECDSA verification (k_ecdsa.hip) and the key recovery of the Tx and Sig witness assignments
// (k_tx_assign.hip) run in these forms; what they share is here: the argument block, the meeting of the lanes' partial sums, the
// choice of form for a batch, and the launches of a batch larger than its key tables.  This file is the argument block and the host
// side, plain C++ that stands alone; the meeting of the partial sums is device code next to the point addition (secp256k1.hpp
// secp_lanes_meet).
#pragma once
#include <stdint.h>
#include <stdlib.h>

#define ZK_ECDSA_CHUNK_LANES (1ull << 17)  // lanes per launch (x 1,440 B of key tables = 189 MB); a multiple of 64

struct SecpLanes {
    // per-lane tables of the key's multiples 1..15 (24 words each): lane l's at qtab + l * 360, contiguous — the window digit is data
    // dependent, so the lanes of a wavefront read different entries, and with a lane-interleaved layout every 4-byte word came out of a
    // different 64-byte sector (FETCH_SIZE 5.2 GB per 2^17-signature launch, profiles/r02_row_kernels_profile.json)
    uint32_t* qtab;
    uint64_t qtab_lanes;     // lanes the tables were allocated for: a launch covers at most this many
    uint32_t lanes_per_sig;  // 1, 2 or 4
    const uint32_t* gcomb;   // optional: the 8-bit fixed-base table of G built on the device (ecdsa_comb_entry), nullptr: 4-bit constant table
    uint64_t first;          // first signature of this launch (secp_chunk)
};

// ---- host side: no device calls ----------------------------------------------------------------------------------------------------
// The form of a batch of n signatures.  Lane pairs while the batch cannot fill the chip anyway (the pass is then bound by one lane's
// dependent chain: halve it); one lane per signature beyond that (less total work); lane quads up to 2^14 signatures — one wavefront per
// SIMD at most —, where the two extra lanes take u1 G off the pair's chain (secp256k1.hpp ecdsa_partial4: 1.09-1.11 -> 0.99-1.02 ms;
// 2^15 signatures as quads are two wavefronts per SIMD: 1.67 ms against 1.13).  `forced` (the value of ZK_ECDSA_LANES, or null):
// "4" and "2" choose that form, anything else one lane (tuning / tests).  The four-lane form takes u1 G from the comb table: without
// one it falls back to pairs.  The key tables cover the batch rounded up to whole wavefronts, at least one, at most
// ZK_ECDSA_CHUNK_LANES lanes: a larger batch runs as consecutive launches over one set of tables (secp_chunk).
struct SecpLaneForm {
    uint32_t lanes_per_sig;
    uint64_t qtab_lanes;
};
static inline SecpLaneForm secp_lane_form(uint64_t n, bool have_comb, const char* forced) {
    SecpLaneForm f;
    f.lanes_per_sig = n <= (1ull << 14) ? 4u : n <= (1ull << 16) ? 2u : 1u;
    if (forced) { const int v = atoi(forced); f.lanes_per_sig = v == 4 ? 4u : v == 2 ? 2u : 1u; }
    if (f.lanes_per_sig == 4u && !have_comb) f.lanes_per_sig = 2u;
    f.qtab_lanes = ((n * f.lanes_per_sig + 63) / 64) * 64;
    if (f.qtab_lanes == 0) f.qtab_lanes = 64;
    if (f.qtab_lanes > ZK_ECDSA_CHUNK_LANES) f.qtab_lanes = ZK_ECDSA_CHUNK_LANES;
    return f;
}

// The launch that starts at signature `first` of n: `count` signatures (0: past the end) as `grid` blocks of `block` lanes.  A batch
// runs as for (c = secp_chunk(n, l, 0); c.count; c = secp_chunk(n, l, c.first + c.count)), in order on one stream, so a chunk's tables
// are free when the next one starts.  64-lane blocks: 2^14 signatures are only 256 (512 as lane pairs) wavefronts; the four-lane form in
// 256-lane blocks: its wavefronts are few, and four of them on one CU share its instruction cache — one wavefront per CU took 1.21 ms
// at 2^11 signatures where four per CU take 1.01.
struct SecpChunk {
    uint64_t first, count;
    uint32_t grid, block;
};
static inline SecpChunk secp_chunk(uint64_t n, const SecpLanes& l, uint64_t first) {
    SecpChunk c = {first, 0, 0, l.lanes_per_sig == 4 ? 256u : 64u};
    if (first >= n) return c;
    const uint64_t per_chunk = l.qtab_lanes / l.lanes_per_sig;  // signatures per launch
    c.count = n - first < per_chunk ? n - first : per_chunk;
    const uint32_t waves = (uint32_t)((c.count * l.lanes_per_sig + 63) / 64);
    c.grid = l.lanes_per_sig == 4 ? (waves + 3) / 4 : waves;
    return c;
}
