// Device helpers shared by every kernel translation unit + the host launchers the C-ABI layer (zkevm_hip.hip) calls.
// The library is built from several translation units compiled in parallel (build.sh): each k_*.hip defines its kernels
// and a plain C++ launcher; no relocatable device code is needed.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include "state_circuit.hpp"
#include "evm_circuit.hpp"
#include "row_circuits.hpp"
#include "copy_circuit.hpp"
#include "sign_circuit.hpp"
#include "keccak_table.hpp"
#include "state_assign.hpp"
#include "secp256k1.hpp"
#include "bytecode_assign.hpp"
#include "bytecode_code.hpp"
#include "block_tables.hpp"
#include "trace_witness.hpp"
#include "state_trace.hpp"
#include "copy_assign.hpp"
#include "copy_sources.hpp"
#include "trace_events.hpp"
#include "trace_sha3.hpp"
#include "pi_circuit.hpp"
#include "state_rekey.hpp"
#include "ecc_circuit.hpp"
#include "ecc_calls.hpp"
#include "withdrawal_circuit.hpp"
#include "tx_assign.hpp"
#include "sig_assign.hpp"
#include "exp_assign.hpp"
#include "pi_assign.hpp"

// The single-kernel row sessions keep two tallies and alternate between them: a pass accumulates into one and its first
// lane clears the other for the pass after it, so that no reset kernel sits in front of every evaluation kernel (a kernel
// boundary costs ~10 us of the 77 us State pass at 2^16 rows).  `tally` and its twin are 16 B apart in one 32 B-aligned block.
__device__ __forceinline__ void tally_clear_twin(ZkTally* tally) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ZkTally* twin = (ZkTally*)((uintptr_t)tally ^ (uintptr_t)sizeof(ZkTally));
        twin->fail_count = 0ull;
        twin->first_fail = ~0ull;
    }
}
static_assert(sizeof(ZkTally) == 16, "tally_clear_twin assumes 16-byte tallies");

// One wave-level ballot, then at most one counter atomic per wave and one atomicMin per
// failing lane (failures are rare on real witnesses; the hot path issues no atomics at all).
__device__ __forceinline__ void tally_commit(ZkTally* tally, u64 row, u32 code) {
    const unsigned long long ballot = __ballot(code != 0u);
    if (ballot != 0ull) {
        if (code != 0u) atomicMin(&tally->first_fail, (row << 32) | (unsigned long long)code);
        const int lane = threadIdx.x & 63;
        if (lane == __ffsll((long long)ballot) - 1) atomicAdd(&tally->fail_count, (unsigned long long)__popcll(ballot));
    }
}

#define ST_ROWS_PER_WAVE 63

// ---- launchers (defined in the k_*.hip units) ------------------------------------------------------------------------
// e0 / e1 (optional): the pass's start / stop events ride on the dispatch itself (no event packets between back-to-back passes) when
// zk_state_rows_events_ride(a) says the launch is one kernel of a form that takes them; otherwise the caller records them around the call
void zk_launch_state_rows(hipStream_t st, const StateArgs& a, u32* status, ZkTally* tally, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
bool zk_state_rows_events_ride(const StateArgs& a);
// hot: e0 rides on the dispatch as its start event; cold: e1 as its stop event (either may be null)
void zk_launch_evm_hot(hipStream_t st, u32 grid, const EvmArgs& a, const u32* group_start, u32* status, ZkTally* tally, hipEvent_t e0, hipEvent_t e1 = nullptr);
void zk_launch_evm_warm(hipStream_t st, u32 grid, u32 warm_lanes, const EvmArgs& a, const u32* group_start, u32* status, ZkTally* tally, hipEvent_t e1);
void zk_launch_evm_cold(hipStream_t st, u32 grid, const EvmArgs& a, const u32* group_start, u32* status, ZkTally* tally, hipEvent_t e1);
// the pairs the hot (fast) kernel deferred, evaluated by the general build (k_evm_slow.hip); launched only when there are any
void zk_launch_evm_deferred(hipStream_t st, const EvmArgs& a, u32* status, ZkTally* tally);
void zk_launch_bytecode_rows(hipStream_t st, const BytecodeArgs& a, u64 lo, u64 hi, u32* status, ZkTally* tally);
void zk_launch_copy_rows(hipStream_t st, const CopyArgs& a, u64 lo, u64 hi, u32* status, ZkTally* tally);
void zk_launch_sign_units(hipStream_t st, const SignArgs& a, u64 lo, u64 hi, u32* status, ZkTally* tally);
void zk_launch_exp_rows(hipStream_t st, const ExpArgs& a, u64 lo, u64 hi, u32* status, ZkTally* tally);
void zk_launch_fr_to_mont(hipStream_t st, const Fr& x, u64* out);
void zk_launch_sign_rpow(hipStream_t st, const Fr& r, u64* out);
void zk_launch_keccak_rpow(hipStream_t st, const Fr& r, u64* out);
void zk_launch_keccak_table(hipStream_t st, const KeccakGenArgs& g, u32* status, ZkTally* tally);
void zk_launch_state_assign(hipStream_t st, const AssignArgs& a, u32* status, ZkTally* tally);
// state_fused.hpp: the State circuit on rows computed from the ops (after zk_launch_state_assign with a.root_rank set)
void zk_launch_state_rows_fused(hipStream_t st, const StateArgs& sa, const AssignArgs& g, u32* status, ZkTally* tally, ZkTally* asg_tally);
void zk_launch_rekey_scan(hipStream_t st, const RekeyArgs& a);  // open-time class masks of the RW -> State re-keying
void zk_launch_state_rekey(hipStream_t st, const RekeyArgs& a, u32* status, ZkTally* tally);
// its pieces, for a front end over another row source: the rank kernels of a.jobs, the fast sort's per-launch reset, the radix passes over
// packed keys (-> the sorted order of the kept rows, then the left-out ones)
void zk_launch_rekey_rank_jobs(hipStream_t st, const RekeyArgs& a);
void zk_rekey_sweep_begin(hipStream_t st, const RekeyArgs& a);
const u32* zk_launch_rekey_passes(hipStream_t st, const RekeyArgs& a);
// State circuit from compact trace records (state_trace.hpp, k_state_trace.hip): the open's checks with the pool offsets by a chunked scan
// (sums: ceil(n_rw / 1024) words of scratch) and its class scan; the re-keying and the sort, then
// the op list (a.ops) or the sorted packed op stream (src.stream); the MPT passes over that stream (k_assign.hip: the roots alone); the
// State circuit on rows computed from it
void zk_launch_state_trace_check(hipStream_t st, const TrwArgs& a, u64* sums);
void zk_launch_state_trace_scan(hipStream_t st, const RekeyArgs& a, const StrcArgs& src);
void zk_launch_state_trace_rekey(hipStream_t st, const RekeyArgs& a, const StrcArgs& src, u32* status, ZkTally* tally);
void zk_launch_state_assign_trace(hipStream_t st, const AssignArgs& a, const StrcArgs& src);
void zk_launch_state_assign_rows_trace(hipStream_t st, const AssignArgs& a, const StrcArgs& src, u32* status, ZkTally* tally);
void zk_launch_state_rows_trace(hipStream_t st, const StateArgs& sa, const AssignArgs& g, const StrcArgs& src, u32* status, ZkTally* tally, ZkTally* asg_tally);
void zk_launch_bca_rpow(hipStream_t st, const Fr& r, u64* out);
void zk_launch_bytecode_assign(hipStream_t st, const BcaArgs& a, u32* status, ZkTally* tally);
void zk_launch_bca_prefix(hipStream_t st, const BcaArgs& a);  // its prefix pass alone (value_rlc and counter entering every chunk)
// Bytecode table + circuit rows + keccak rows from raw code (k_bytecode_code.hip); side / ev_fork / ev_join as zk_launch_pi_assign
void zk_launch_bytecode_from_code(hipStream_t st, hipStream_t side, hipEvent_t ev_fork, hipEvent_t ev_join, const BccArgs& a,
                                  const KeccakGenArgs& g, u32* status, ZkTally* tally);
// EVM circuit tx / block / withdrawal tables from raw block data (k_block_tables.hip): the calldata's non-zero counts, then every row
void zk_launch_block_tables(hipStream_t st, const BtbArgs& a, u32* status);
// EVM circuit witness from compact trace records (k_trace_witness.hip): the open's checks + pool offsets into a.verdict / a.head / a.ctr /
// a.off, and a pass's row writer
// (with_offsets = false: the checks alone — a.off and the verdict's pool word are then the caller's to fill, zk_launch_state_trace_check)
void zk_launch_trace_witness_check(hipStream_t st, const TrwArgs& a, bool with_offsets = true);
void zk_launch_trace_witness(hipStream_t st, const TrwArgs& a, u32* status);
void zk_launch_pi_rows(hipStream_t st, const PiArgs& a, u64 lo, u64 hi, u32* status, ZkTally* tally);
void zk_launch_pi_copy(hipStream_t st, const PiCopyArgs& a, u32* status, ZkTally* tally);
void zk_launch_cpa_rpow(hipStream_t st, const Fr& r, u64* out);
void zk_launch_copy_assign(hipStream_t st, const CpaArgs& a, u32* status, ZkTally* tally);
// The Copy assignment's source data from code, calldata and trace records (k_copy_sources.hip): the is_code scan of the code set (c.n_segs
// > 0), the gather into a.data, the status per event and its tally; zk_launch_copy_assign over a.data follows in stream order
void zk_launch_copy_sources(hipStream_t st, const CpsArgs& a, const CpsCodeArgs& c, u32* status, ZkTally* tally);
// Copy and EXP events from compact trace records (k_trace_events.hip): a status per step and its tally, what each step emits, a scan of the
// per-block counts into a.blk / a.counts, the packed ordered stores
void zk_launch_trace_events(hipStream_t st, const TevArgs& a, u32* status, ZkTally* tally);
void zk_launch_trace_events_count(hipStream_t st, const u64* steps, u64 n_steps, u64* n_pair);
void zk_launch_trace_events_ext(hipStream_t st, const TevxArgs& ax, u32* status, ZkTally* tally);
// SHA3 inputs and keccak rows from compact trace records (k_trace_sha3.hip).  _count: every step's open-time status and size, the scan of
// the per-block counts, the totals in a.verdict;  _write: the message records and the session's data offsets (cross_only: nothing but
// the step that takes the byte total to 2^31);  the pass: the gather into a.data, zk_launch_keccak_table over it (g), the digest
// comparison, a status per step and its tally
void zk_launch_trace_sha3_count(hipStream_t st, const Ts3Args& a);
void zk_launch_trace_sha3_write(hipStream_t st, const Ts3Args& a, bool cross_only);
void zk_launch_trace_sha3(hipStream_t st, const Ts3Args& a, const KeccakGenArgs& g, u32* status, ZkTally* tally);
void zk_launch_ecdsa(hipStream_t st, const EcdsaArgs& a, u32* status, ZkTally* tally);
void zk_launch_ecdsa_comb_build(hipStream_t st, u32* table);  // the device's 8-bit fixed-base table of G (522 KB), built once
// ECC circuit (k_ecc.hip): assign = circuit2rows into a.rows_out, else verify a.rows (status / tally)
void zk_launch_ecc(hipStream_t st, const EccArgs& a, bool assign, u32* status, ZkTally* tally);
// rows [lo, hi) of an ECC session: add / mul rows, then the pairs [t_lo, t_hi) of the pairing ops in range (stage 1) and those ops'
// rows (stage 2), three launches in stream order (twin tally; status is never null)
void zk_launch_ecc_range(hipStream_t st, const EccPairArgs& s, u64 lo, u64 hi, u32 t_lo, u32 t_hi, u32* status, ZkTally* tally);
// stage 1 alone, over the pairs [t_lo, t_hi) (the launch zk_launch_ecc_range makes; ECC precompile calls run it ahead of their own stage 2)
void zk_launch_ecc_pair_stage1(hipStream_t st, const EccPairArgs& s, u32 t_lo, u32 t_hi);
// ECC precompile calls (k_ecc_calls.hip): add / mul calls, pairing stage 1 over n_pairs pairs, pairing calls, the ecc table; status all 0
void zk_launch_ecc_calls(hipStream_t st, const EccCallArgs& a, u32 n_pairs, u32* status);
void zk_launch_fq12_op(hipStream_t st, int op, const u64* x, const u64* y, u64* out, u64 n12);  // zk_fr_op 19..25
// Withdrawal circuit (k_withdrawal.hip): verify held rows [lo, hi) (status / twin tally); assign rows [0, a.n_out) (+ keccak rows)
void zk_launch_withdrawal_rows(hipStream_t st, const WithdrawalArgs& a, u64 lo, u64 hi, u32* status, ZkTally* tally);
void zk_launch_withdrawal_assign(hipStream_t st, const WithdrawalArgs& a);
// secp256k1 key recovery in the lane forms (k_tx_assign.hip): pk and status (+ status / tally) per signature of the batch
void zk_launch_secp_recover(hipStream_t st, const SecpRecoverArgs& a, u32* status, ZkTally* tally);
// Tx circuit witness assignment (k_tx_assign.hip): sign hashes, key recovery (status / tally per tx), rows, units, keccak set
void zk_launch_tx_assign(hipStream_t st, const TxAssignArgs& a, u32* status, ZkTally* tally);
// Sig circuit witness assignment (k_sig_assign.hip): key recovery (status / tally per signature), units, keccak set, sig table, aux rows
void zk_launch_sig_assign(hipStream_t st, const SigAssignArgs& a, u32* status, ZkTally* tally);
// Exp circuit witness assignment (k_exp_assign.hip): the open's counts / first rows / reject word, then chain + rows per pass
void zk_launch_exp_assign_sizes(hipStream_t st, const ExaArgs& a);
void zk_launch_exp_assign(hipStream_t st, const ExaArgs& a, u32* status, ZkTally* tally);
// PI circuit witness assignment (k_pi_assign.hip): the reject word of sizes / open; the open's power table and small inverses; one pass
// (g: the keccak kernels' arguments over the generation-order byte buffer; side: a second stream of the device for them, forked and
// joined with the two events, or null: everything on st)
void zk_launch_pi_assign_check(hipStream_t st, const PiaArgs& a);
void zk_launch_pi_assign_tables(hipStream_t st, const PiaArgs& a);
void zk_launch_pi_assign(hipStream_t st, hipStream_t side, hipEvent_t ev_fork, hipEvent_t ev_join, const PiaArgs& a, const KeccakGenArgs& g,
                         u32* status, ZkTally* tally);
