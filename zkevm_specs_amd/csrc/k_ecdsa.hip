// secp256k1 ECDSA verification kernel (secp256k1.hpp)
#include "kernels.hpp"

// One lane per signature (L = 1) or a lane pair per signature (L = 2: each lane runs one half of the GLV split with its own
// 128-doubling chain, the partial sums meet through one DPP-free cross-lane exchange at the end), or four (L = 4, round 6: lanes 2 / 3
// carry the halves of u1 G and add them in the ladder's addition slots, secp256k1.hpp ecdsa_partial4; 256-lane blocks).  Integer-ALU bound.
template <int L>
__global__ __launch_bounds__(L == 4 ? 256 : 64) void ecdsa_verify_kernel(EcdsaArgs a, u32* status, ZkTally* tally) {
    const u64 gid = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 i = a.lanes.first + gid / L;
    const int role = (int)(gid % L);
    const bool valid = i < a.n;
    u32* tab = a.lanes.qtab + gid * (15u * 24u);  // the lane's own table, contiguous (secp_lanes.hpp)
    EcdsaPrep pr;
    u32 st = ECDSA_NOT_VERIFIED;
    SpPoint part = sp_infinity();
    if (valid) {
        st = ecdsa_prepare(a, i, pr, role == 0);
        if (st == ECDSA_PENDING) part = L == 4 ? ecdsa_partial4(pr, role, tab, 1, a.lanes.gcomb)
                                               : ecdsa_partial(pr, L == 1 ? 0 : role, L == 1 ? 1 : role, tab, 1, a.lanes.gcomb);
    }
    secp_lanes_meet<L>(part, valid && st == ECDSA_PENDING, role);
    u32 code = 0;
    if (valid && role == 0) {
        code = st == ECDSA_PENDING ? ecdsa_verdict(pr, part) : st;
        if (status) status[i] = code;
        if (i < a.n0) { if (a.out) a.out[i * a.out_stride] = code; }
        else if (a.out1) a.out1[(i - a.n0) * a.out_stride1] = code;
    }
    tally_commit(tally, i, code);
}

__global__ __launch_bounds__(64) void ecdsa_comb_build_kernel(u32* table) {
    const u32 e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < ECDSA_COMB_ENTRIES) ecdsa_comb_entry(e, table);
}
void zk_launch_ecdsa_comb_build(hipStream_t st, u32* table) {
    hipLaunchKernelGGL(ecdsa_comb_build_kernel, dim3((ECDSA_COMB_ENTRIES + 63) / 64), dim3(64), 0, st, table);
}
void zk_launch_ecdsa(hipStream_t st, const EcdsaArgs& a0, u32* status, ZkTally* tally) {
    // The per-lane key tables cost 1,440 bytes per lane: a batch larger than its tables runs as consecutive launches (secp_chunk)
    EcdsaArgs a = a0;
    const u32 L = a.lanes.lanes_per_sig;
    const auto kernel = L == 4 ? ecdsa_verify_kernel<4> : L == 2 ? ecdsa_verify_kernel<2> : ecdsa_verify_kernel<1>;
    for (SecpChunk c = secp_chunk(a.n, a.lanes, 0); c.count; c = secp_chunk(a.n, a.lanes, c.first + c.count)) {
        a.lanes.first = c.first;
        hipLaunchKernelGGL(kernel, dim3(c.grid), dim3(c.block), 0, st, a, status, tally);
    }
}
