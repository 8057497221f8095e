/* zkevm_hip.h — C ABI of the MI355X constraint-evaluation engine (libzkevm_hip.so).
 *
 * The reference (privacy-scaling-explorations/zkevm-specs, pure Python) has no FFI: its seam
 * is the set of module-level callables its tests import by name.  Each entry
 * point below replaces the per-row Python loop of one of them; INTEGRATION.md shows the
 * ctypes stub a maintainer would add on the reference side.
 *
 * Wire format: one field cell = 4 x uint64 little-endian canonical (== `FQ.n`,
 * src/zkevm_specs/util/arithmetic.py:41-63).  Witness rows are column-major
 * uint64[n_cells][n_rows][4]; lookup tables are row-major uint64[n_rows][n_cells][4];
 * per-row type bits (is_word of WordOrValue cells, util/arithmetic.py:171-195) are uint32[n_rows].
 *
 * Ownership: the caller owns every buffer for the duration of the call (or of the session
 * for zk_*_open); nothing is retained after zk_*_close / after a one-shot call returns.
 * Immutability: the tables a session was opened over are IMMUTABLE for the session's lifetime, also with
 * ZK_OPT_DEVICE_PTRS (where the session reads the caller's buffers in place).  zk_*_open derives state from them that
 * later passes rely on — lookup indices, packed key / step / bytecode records, the dense-RW verdict, EndBlock's whole-table
 * aggregates, and (EVM) which of the warm / cold lane ranges are empty, after which those kernels are no longer launched.
 * A witness that changed is a new witness: close the session and open another one (an EVM open at 2^18 steps is ~0.1 ms
 * of device time).  Editing a table between passes is undefined: stale records would be evaluated, silently.
 * Errors: every function returns 0 on success and a negative code on infrastructure errors
 * (bad arguments, HIP failures — text via zk_last_error()); constraint failures are NOT
 * errors, they are reported in zk_result.  Nothing throws across this boundary.
 * Threading / re-entrancy: a session (zk_session*) is the context.  It captures the device and the stream that are
 * current for the calling thread when it is opened, owns its buffers, events and tally, and every later call on it
 * (zk_launch / zk_collect / zk_read_status / zk_close) works on that device and stream whatever other sessions or
 * threads do in between.  Different sessions may be driven from different threads concurrently; one session is driven
 * by one thread at a time.  zk_init / zk_set_stream select the *calling thread's* current device / stream,
 * zk_last_error returns the calling thread's last error text.  The only process-wide state is one lazily created
 * stream per device.
 */
#ifndef ZKEVM_HIP_H
#define ZKEVM_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Status code of one row/step: 0 = satisfied, else (kind << 24) | site.  `kind` is the Python
 * exception class the reference raises at the first failing check of that row. */
enum zk_kind {
    ZK_KIND_OK = 0,
    ZK_KIND_ASSERTION_ERROR = 1,      /* constrain_* / assert (caught by verify_steps, main.py:36) */
    ZK_KIND_CONSTRAINT_UNSAT = 2,     /* ConstraintUnsatFailure raised (instruction.py:483,534) */
    ZK_KIND_LOOKUP_UNSAT = 3,         /* LookupUnsatFailure (table.py:688,880) */
    ZK_KIND_LOOKUP_AMBIGUOUS = 4,     /* LookupAmbiguousFailure (table.py:882) */
    ZK_KIND_WRONG_QUERY_KEY = 5,
    ZK_KIND_NOT_IMPLEMENTED = 6,      /* NotImplementedError (main.py:63) */
    ZK_KIND_TYPE_ERROR = 7,
    ZK_KIND_OVERFLOW_ERROR = 8,
    ZK_KIND_VALUE_ERROR = 9,
    ZK_KIND_ZERO_DIVISION = 10,
    ZK_KIND_INDEX_ERROR = 12,
    ZK_KIND_ATTRIBUTE_ERROR = 13,
    ZK_KIND_NAME_ERROR = 11,          /* UnboundLocalError (execution/block_ctx.py:24) */
    ZK_KIND_UNSUPPORTED = 15          /* gadget not implemented by this engine */
};

typedef struct zk_result {
    uint64_t fail_count;       /* rows whose status != 0 */
    uint64_t first_fail_row;   /* smallest failing row index, UINT64_MAX if none */
    uint32_t first_fail_code;  /* status code of that row */
    uint32_t launches;         /* kernel launches covered by this result */
    uint64_t rows_evaluated;   /* rows per launch */
    double kernel_ms;          /* mean device time of the evaluation kernel per launch (HIP events) */
} zk_result;

#define ZK_OPT_DEVICE_PTRS 1u  /* every data pointer is a device (HBM) pointer */
/* State rows without the limb / byte columns (zk_state_open, zk_state_assign_open, zk_state_assign_from_rw_open): the witness is
 * uint64[15][n][4] — rw_counter, is_write, tag, id, address, field_tag, storage_key lo / hi, then value lo / hi, initial_value lo / hi,
 * root lo / hi, lexicographic_ordering_selector (columns 0..7 and 50..56 of the 57-cell row) — and the ten 16-bit address limbs and 32
 * storage-key bytes (columns 8..49; Row.key2_limbs / key45_bytes, state_circuit.py:63-96) are DERIVED from the address and storage-key
 * cells where the circuit's checks use them, as assign_state_circuit's op2row derives them (:834-842).  For witnesses assigned on the
 * device: the assignment does not write, and the circuit does not read back, 1,344 of a row's 1,824 bytes.  What it gives up: the limb /
 * byte cells are no independent inputs, so their range and recomposition checks (state_circuit.py:505-517) reduce to "address < 2^160,
 * key halves < 2^128" (sites 5 and 7).  Every other check, the ordering, the lookups and the per-tag rules are evaluated as always.
 * Not for witnesses from outside (a tampered limb cell cannot be expressed): those use the 57-cell form. */
#define ZK_OPT_STATE_COMPACT 32u
#define ZK_OPT_BLOCK_STATE_ROWS 64u /* zk_block_verify: materialise the State witness (57-cell rows) instead of the fused form */

/* Select the GPU (HIP ordinal) for the calling thread; creates that device's engine stream on first use.  Idempotent.
 * Selecting another device drops a stream set with zk_set_stream (it belongs to the previous device). */
int zk_init(int device);
void zk_shutdown(void);
/* Sessions opened by this thread from now on run on the caller's HIP stream (e.g. torch's current stream);
 * NULL = the engine's own (non-blocking) stream of the device.  NOTE: HIP's legacy default stream is handle 0 = NULL
 * here, i.e. "engine's own": to order the engine with work of another library, hand over a real (non-default) stream. */
int zk_set_stream(void* hip_stream);
const char* zk_last_error(void);
/* BN254-Fr vector ops on the device: op 0 add, 1 sub, 2 mul, 3 montmul, 4 neg, 5 inv (of a; inv(0) = 0 as py_ecc's
 * prime_field_inv), 6 div (a * inv(b)); 16 / 17: the secp256k1 BASE-field product a * b / square a^2 mod 2^256 - 2^32 - 977
 * (operands are residues below that prime; unit-test hooks of the ECDSA kernel's multiplier).
 * 18: the BN254 BASE-field product a * b mod p (p = 2188...8583, residues in and out; unit-test hook of csrc/bn254_fq.hpp);
 * 19: the Fq12 product a * b, n a multiple of 12, every 12 consecutive elements one Fq12 in tower order (c0.c0.c0, c0.c0.c1,
 * c0.c1.c0, ..., c1.c2.c1: Fq12 = Fq6 + Fq6 w, Fq6 = Fq2 + Fq2 v + Fq2 v^2, Fq2 = Fq + Fq u; residues in and out).
 * 20..25: per 12 elements of a, as 19 (b is not read but must not be null): 20 a^2, 21 a^-1 (0 -> 0), 22 a^p (Frobenius),
 * 23 the final exponentiation of the pairing, f^((p^12 - 1) / r * m) with the fixed m = 2x(6x^2 + 3x + 1) of its hard part;
 * 24 the pairing of one pair, final_exp(miller_loop(P, Q)): a holds the six words of a zk_ecc_ops pairing point (EIP-197 order
 * p.x, p.y, x.c1, x.c0, y.c1, y.c0, reduced mod p), then zeros; a pair with a point at infinity gives 1.  Neither point is checked;
 * 25 the G2 scalar chain of the ECC circuit (py_ecc's multiply over Fq2, exact also off the twist): a = Q (x.c1, x.c0, y.c1, y.c0,
 * reduced mod p, all zero = None), then the scalar as a 256-bit integer, then zeros; out = affine x.c0, x.c1, y.c0, y.c1, then
 * 1 if the result is None (its coordinates 0) else 0, then zeros.
 * 26 / 27: the secp256k1 BASE-field chains of zk_tx_assign's key recovery, a^((P + 1) / 4) (the square root when there is one) and
 * a^(P - 2) (the inverse, 0 -> 0); residues in, b is not read but must not be null.
 * (reference: FQ.__add__/__sub__/__mul__/__neg__/__truediv__ via py_ecc and FQ.inv, util/arithmetic.py:41-60) */
int zk_fr_op(int op, const uint64_t* a, const uint64_t* b, uint64_t* out, uint64_t n, uint32_t opts);

/* ---- State circuit: replaces the `for row: check_state_row(row, prev, next, tables)` loop
 *      (src/zkevm_specs/state_circuit.py:492; loop tests/test_state_circuit.py:26-30).
 *      rows: uint64[57][n][4] + flags uint32[n] (bit0 value.is_word, bit1 initial.is_word);
 *      mpt: uint64[n_mpt][12][4] (MPTTableRow, evm_circuit/table.py:461-468). */
typedef struct zk_session zk_session;
int zk_state_open(const uint64_t* rows, const uint32_t* flags, uint64_t n,
                  const uint64_t* mpt, uint64_t n_mpt, uint32_t opts, zk_session** out);
/* Multi-GPU row sharding: evaluate only rows [row_lo, row_hi) of the uploaded block; the rows
 * outside the range are a read-only halo (prev/next of the boundary rows).  Default: all rows,
 * neighbours wrapping modulo n as in the reference's driver. */
int zk_state_set_range(zk_session* s, uint64_t row_lo, uint64_t row_hi);
/* The same for every row-circuit session (State, Bytecode, Copy, Exp, Tx / Sig units, PI): a rank of a row-sharded
 * run opens its session over rows [lo, hi + halo) of the global witness (halo = the rows after the range that the
 * range's last rows read: State 1 before + 1 after, Bytecode / Exp / PI 1 after, Copy 2 after, Tx / Sig none;
 * SURVEY.md §8e) and evaluates [0, hi - lo) (State: [1, 1 + hi - lo)).  Withdrawal: 1 before + 1 after without wrap-around — a
 * rank opens over rows [max(lo - 1, 0), min(hi + 1, len(rows))) with row_base = max(lo - 1, 0) and evaluates the held rows of
 * [lo, hi) (a held row whose neighbour is missing reports ZK_UNSUPPORTED).  zk_result.rows_evaluated reports the range.
 * EVM sessions shard by the step rows they are opened over (pairs [lo, hi) need steps [lo, hi]). */
int zk_set_range(zk_session* s, uint64_t row_lo, uint64_t row_hi);
/* One-shot convenience: open + launch + collect (+ copy per-row status to host) + close. */
int zk_state_verify(const uint64_t* rows, const uint32_t* flags, uint64_t n,
                    const uint64_t* mpt, uint64_t n_mpt, uint32_t opts,
                    uint32_t* status_out /* nullable, n entries, host unless DEVICE_PTRS */,
                    zk_result* result);

/* ---- EVM circuit: replaces the `for (curr, next) in zip(steps, steps[1:]): verify_step(...)` loop of
 *      verify_steps (src/zkevm_specs/evm_circuit/main.py:14-44): one status per step PAIR
 *      (n_steps - 1 of them).  steps: ROW-major uint64[n_steps][13][4] (StepState, step.py:16-75 —
 *      lanes visit steps in state-sorted order, so each step's cells stay contiguous; the dummy
 *      EndBlock step of main.py:21-22 is appended by the caller when end_with_last_step);
 *      rw uint64[n][14][4] + flags (bit0 value.is_word, bit1 value_prev.is_word) — RWTableRow,
 *      table.py:447-457; bytecode uint64[n][6][4] (:438-443); tx uint64[n][5][4] + flags (:421-426);
 *      block uint64[n][4][4] + flags (:413-417).  Fixed-table lookups (table.py:14-103) are
 *      evaluated in closed form on the device.  Tables are sets: callers de-duplicate rows. */
typedef struct zk_evm_tables {
    const uint64_t* steps;      uint64_t n_steps;
    const uint64_t* rw;         const uint32_t* rw_flags;    uint64_t n_rw;
    const uint64_t* bytecode;   uint64_t n_bytecode;
    const uint64_t* tx;         const uint32_t* tx_flags;    uint64_t n_tx;
    const uint64_t* block;      const uint32_t* block_flags; uint64_t n_block;
    uint32_t begin_with_first_step;
    uint32_t end_with_last_step;
    /* tables only the copy / SHA3 / EXP gadgets look up (Tables.copy_table / keccak_table / exp_table,
     * table.py:614-619); n == 0 when absent.  copy uint64[n][14][4] (CopyTableRow :494-507: is_first,
     * src_id lo/hi, src_tag, dst_id lo/hi, dst_tag, src_addr, src_addr_end, dst_addr, length, rlc_acc,
     * rw_counter, rwc_inc); keccak uint64[n][5][4] (KeccakTableRow :511-515); exp uint64[n][11][4]
     * (ExpTableRow :538-548: is_step, identifier, is_last, base_limb0..3, exponent lo/hi,
     * exponentiation lo/hi). */
    const uint64_t* copy;       uint64_t n_copy;
    const uint64_t* keccak;     uint64_t n_keccak;
    const uint64_t* exp;        uint64_t n_exp;
    /* StepState.aux_data (step.py:44), optional (NULL = absent for every step): aux uint64[n_steps][aux_cells][4] and
     * aux_kind uint32[n_steps]: 0 none, 1 Word (lo, hi), 2 int < 2^256 (lo, hi), 3 pair of ints < p (CALL into a
     * precompile: input / return length), 4 not representable (a gadget that reads it reports ZK_UNSUPPORTED),
     * 5 ecRecover [PrecompileAuxData, randomness]: msg_hash, sig_v, sig_r, sig_s as lo/hi, recovered_addr, input_rlc,
     * output_rlc, keccak_randomness (12 cells, ecrecover.py:15-44), 6 ecAdd [px, py, qx, qy, outx, outy] (10 cells),
     * 7 ecMul [px, py, s, outx, outy] (8 cells), 8 ecPairing [input_rlc, input_pairs, is_valid_input, output] (4). */
    const uint64_t* aux;        const uint32_t* aux_kind;
    /* Tables.withdrawal_table (WithdrawalTableRow, table.py:430-434: id, validator_id, address, amount), optional:
     * uint64[n][4][4], sorted by id (the order end_block.py:152 walks them in).  Only EndBlock's last step reads it. */
    const uint64_t* withdrawals; uint64_t n_withdrawals;
    /* Tables.sig_table / ecc_table (table.py:552-575), optional: sig uint64[n][9][4] (msg_hash lo/hi, sig_v, sig_r lo/hi,
     * sig_s lo/hi, recovered_addr, is_valid); ecc uint64[n][13][4] (op_type, px lo/hi, py lo/hi, qx lo/hi, qy lo/hi,
     * input_rlc, out_x, out_y, is_valid).  Only the ecRecover / ecAdd / ecMul / ecPairing precompile states read them. */
    const uint64_t* sig;        uint64_t n_sig;
    const uint64_t* ecc;        uint64_t n_ecc;
    uint32_t aux_cells;         /* cells per step in `aux`: 0 = 2 (kinds 0-3), 12 when kinds 5-8 are present */
    uint32_t reserved;
} zk_evm_tables;
#define ZK_OPT_NO_STATE_SORT 2u /* evaluate step pairs in trace order (no state-sorted lane mapping) */
#define ZK_OPT_GENERIC_INDEX 4u /* skip the dense RW index / bytecode directory; open-addressing indices only */
#define ZK_OPT_SINGLE_PASS 8u   /* EVM sessions: the session will evaluate ONE pass (what zk_evm_verify does): skip the packed step
                                 * records, a one-off streaming pass over the step table that only pays for itself from the second
                                 * evaluation pass on; results are identical either way */
#define ZK_OPT_SIDE_STREAM 16u  /* EVM sessions: every pass runs its warm / cold gadget launches on a second stream of the device
                                 * beside the hot one (fork and join by events, results final in the session's stream order as
                                 * always).  Costs two cross-queue barriers (~8 us) and saves the sum of the two launches: a gain
                                 * when the device is shared with other sessions' passes (the Super circuit), a loss alone */
int zk_evm_open(const zk_evm_tables* t, uint32_t opts, zk_session** out);
/* One-shot: open + one pass + collect + close.  Two things differ from a session opened with zk_evm_open, results never:
 *  - The packed RW key records of the last ZK_P2_RW_TAIL per-mille of the rows (environment, read once; default 50, 0 = none:
 *    the launch geometry of a session) are built by the open's second launch beside the step sort, not by its first.  The head
 *    ends on a 64-row boundary:
 *    n_head = (n_rw - n_rw * tail / 1000) rounded up to a multiple of 64, rows [n_head, n_rw) are the tail, row 0 is always head.
 *    The dense RW index needs consecutive rw_counters over the whole table; whether the tail has them is only known after that
 *    launch, which is also the one that would have built the open-addressing index.  A table that is consecutive up to n_head and
 *    not behind it is therefore verified TWICE: the first result is discarded and the call repeated as with ZK_OPT_GENERIC_INDEX
 *    (a caller's status buffer is rewritten; zk_timing_sums counts the call once, zk_last_host_phases adds the discarded run to the
 *    open).  A witness whose rw_counters are not consecutive is off the fast path and may pay double here; it pays once when the
 *    gap lies in the head or when the caller passes ZK_OPT_GENERIC_INDEX itself.
 *  - Without a status buffer (status_out == NULL, and always in the batch form) no per-pair status is stored anywhere:
 *    zk_result's fail_count / first_fail_row / first_fail_code carry the verdict. */
int zk_evm_verify(const zk_evm_tables* t, uint32_t opts,
                  uint32_t* status_out /* nullable, n_steps-1 entries */, zk_result* result);
/* Batch form: n independent witnesses (e.g. the blocks of a queue), each verified exactly as zk_evm_verify does — its own open
 * (indices, key records, sort), one evaluation pass, its own tally in results[i] — software-pipelined two deep on two streams of
 * the device: the HBM-bound open of witness i + 1 runs under the latency-bound evaluation of witness i.  The caller's current
 * stream is synchronised first (uploads it enqueued are complete).  Per-pair statuses are not returned. */
int zk_evm_verify_batch(const zk_evm_tables* const* tables, uint64_t n, uint32_t opts, zk_result* results);

/* ---- Bytecode circuit: replaces the `for row: check_bytecode_row(row, next, push_table, keccak_table, r)`
 *      loop (src/zkevm_specs/bytecode_circuit.py:37-100; loop tests/test_bytecode_circuit.py:26-47, next row
 *      wraps modulo n).  rows: column-major uint64[12][n][4] (Row, bytecode_circuit.py:15-26: q_first,
 *      q_last, hash lo, hi, tag, index, value, is_code, push_data_left, value_rlc, length,
 *      push_data_size); keccak: uint64[m][5][4] (KeccakTableRow, table.py:511-515); randomness: one
 *      cell (keccak_randomness).  The push table (:174-179) is evaluated in closed form. */
int zk_bytecode_open(const uint64_t* rows, uint64_t n, const uint64_t* keccak, uint64_t n_keccak,
                     const uint64_t* randomness, uint32_t opts, zk_session** out);
int zk_bytecode_verify(const uint64_t* rows, uint64_t n, const uint64_t* keccak, uint64_t n_keccak,
                       const uint64_t* randomness, uint32_t opts, uint32_t* status_out, zk_result* result);

/* ---- Exp circuit: replaces the loop of verify_exp_circuit (src/zkevm_specs/exp_circuit.py:88-97,
 *      verify_step :14-85; next row wraps).  rows: column-major uint64[21][n][4] (ExpCircuitRow,
 *      table.py:519-535: q_usable, is_step, identifier, is_last, base, exponent, exponentiation,
 *      a, b, c, d, q as lo/hi pairs, r). */
int zk_exp_open(const uint64_t* rows, uint64_t n, uint32_t opts, zk_session** out);
int zk_exp_verify(const uint64_t* rows, uint64_t n, uint32_t opts, uint32_t* status_out, zk_result* result);

/* ---- Copy circuit: replaces the loop of verify_copy_table (src/zkevm_specs/copy_circuit.py:92-130:
 *      verify_row :23-59 + verify_step :62-89 on the window (i, i+1, i+2) mod n, then the RW / bytecode /
 *      tx lookups of row i).  rows: column-major uint64[20][n][4] (CopyCircuitRow, table.py:472-491: q_step,
 *      is_first, is_last, id lo, hi, tag, addr, src_addr_end, bytes_left, value, rlc_acc, is_code, is_pad,
 *      rw_counter, rwc_inc_left, is_memory, is_bytecode, is_tx_calldata, is_tx_log, is_rlc_acc) + row_flags
 *      (bit0 id.is_word); randomness: one cell; tables as for the EVM circuit. */
typedef struct zk_copy_tables {
    const uint64_t* rows;       const uint32_t* row_flags;   uint64_t n_rows;
    const uint64_t* randomness;
    const uint64_t* rw;         const uint32_t* rw_flags;    uint64_t n_rw;
    const uint64_t* bytecode;   uint64_t n_bytecode;
    const uint64_t* tx;         const uint32_t* tx_flags;    uint64_t n_tx;
} zk_copy_tables;
int zk_copy_open(const zk_copy_tables* t, uint32_t opts, zk_session** out);
int zk_copy_verify(const zk_copy_tables* t, uint32_t opts, uint32_t* status_out, zk_result* result);

/* ---- Tx and Sig circuits: replace the per-tx loop of tx_circuit.verify_circuit (src/zkevm_specs/tx_circuit.py:
 *      253-291: SignVerifyChip.verify :205-243 + the copy constraints to the tx-table rows) and the per-row
 *      loop of sig_circuit.verify_circuit (sig_circuit.py:113-122: Row.verify :64-104).  One unit = one tx
 *      slot / one signature row.  bytes: uint8[n][9][32] (pk_x, pk_y, ecdsa pk_x, pk_y, msg_hash_bytes, ecdsa
 *      msg_hash_bytes, pub_key_hash, ecdsa sig_r LE, ecdsa sig_s LE); cells: column-major uint64[8][n][4]
 *      (address, msg_hash lo, hi, sig_v, sig_r lo, hi, sig_s lo, hi); meta: uint32[n][4] (ecdsa_status: 0
 *      verified / 1 not verified / (kind<<24) exception of the third-party secp256k1 call, expected is_valid,
 *      malformed-attribute mask, the ECDSA chip's v for Sig units); keccak: uint64[m][5][4] (is_enabled, input_rlc, input_len, output lo, hi;
 *      tx_circuit.py:38-61); tx_rows: uint64[rows][5][4] + flags (Tx circuit only). */
typedef struct zk_sign_units {
    const uint8_t* bytes;       const uint64_t* cells;       const uint32_t* meta;      uint64_t n_units;
    const uint64_t* randomness;
    const uint64_t* keccak;     uint64_t n_keccak;
    const uint64_t* tx_rows;    const uint32_t* tx_flags;    uint64_t n_tx_rows;
    uint32_t is_sig;            /* 0 = Tx circuit semantics, 1 = Sig circuit semantics */
} zk_sign_units;
int zk_sign_open(const zk_sign_units* t, uint32_t opts, zk_session** out);
int zk_sign_verify(const zk_sign_units* t, uint32_t opts, uint32_t* status_out, zk_result* result);

/* ---- Keccak table generation: one table row per byte string.
 *      mode 0 = KeccakCircuit.add (evm_circuit/typing.py:854-865; assign_keccak_table,
 *               bytecode_circuit.py:182-186): row = (2, RLC(reversed(data), r), len, Word(int.from_bytes(digest, "big")));
 *      mode 1 = KeccakTable.add (util/tables.py:18-27, tx_circuit.py:48-58):
 *               row = (1, RLC(reversed(data), r, n_bytes = 64), len, Word(digest bytes)); inputs longer
 *               than 64 bytes are rejected with status ZK_KIND_VALUE_ERROR like the reference's RLC.
 *      data: the messages back to back; offsets: uint64[n_msgs + 1] byte offsets into data
 *      (message i = data[offsets[i] .. offsets[i+1])); rows: uint64[n_msgs][5][4] row-major, the
 *      layout every keccak-table argument above takes.  With ZK_OPT_DEVICE_PTRS data, offsets,
 *      randomness and rows are device pointers (rows_dev may be NULL: the session then owns the
 *      rows and zk_keccak_read_rows copies them out).  zk_launch / zk_collect / zk_read_status work
 *      as for the circuits (status = per-message code, kernel_ms = device time of the pass). */
int zk_keccak_open(const uint8_t* data, uint64_t n_bytes, const uint64_t* offsets, uint64_t n_msgs,
                   const uint64_t* randomness, uint32_t mode, uint64_t* rows_dev, uint32_t opts, zk_session** out);
int zk_keccak_read_rows(zk_session* s, uint64_t* rows_host);
int zk_keccak_table(const uint8_t* data, uint64_t n_bytes, const uint64_t* offsets, uint64_t n_msgs,
                    const uint64_t* randomness, uint32_t mode, uint64_t* rows_out, uint32_t opts,
                    uint32_t* status_out, zk_result* result);

/* ---- State-circuit witness assignment: replaces assign_state_circuit
 *      (src/zkevm_specs/state_circuit.py:855-884: op2row :827-852 per op + the root back-fill :866-878) and
 *      mpt_table_from_ops (:887-888, _mock_mpt_updates :904-934).
 *      ops: COLUMN-major uint64[12][n][4], one slot per field of `Operation` (:616-630): rw_counter, rw, tag, id,
 *      address, field_tag, storage_key as the op's 256-bit Python ints (NOT reduced mod p: `FQ(...)` happens on the
 *      device, and `_mpt_key` compares the raw tag), then value lo/hi, initial_value lo/hi and
 *      lexicographic_ordering_selector as field cells.  op_flags uint32[n]: bit0 value.is_word, bit1
 *      initial_value.is_word, bit2 isinstance(field_tag, AccountFieldTag) (selects the account proof types, :915).
 *      Outputs: rows uint64[57][n][4] + row_flags uint32[n] — exactly what zk_state_open takes — and the mock MPT
 *      rows uint64[n_mpt][12][4] in first-occurrence order (capacity: n rows).  Per-op status: AssertionError (site 1
 *      value / 2 initial_value: Word(x.int_value()) >= 2^256 inside _mock_mpt_updates, first op of a key only),
 *      OverflowError (site 3: address wider than 160 bits in op2row); the reference raises the first site-1/2
 *      failure if there is one, else the first site-3 failure.
 *      With ZK_OPT_DEVICE_PTRS every pointer is a device pointer and rows_dev / row_flags_dev / mpt_dev (each
 *      nullable: the session then owns the buffer) receive the outputs in place. */
int zk_state_assign_open(const uint64_t* ops, const uint32_t* op_flags, uint64_t n, uint64_t* rows_dev,
                         uint32_t* row_flags_dev, uint64_t* mpt_dev, uint32_t opts, zk_session** out);
/* Copy the outputs of the last pass to HOST buffers (each nullable); n_mpt_out = number of MPT rows. */
int zk_state_assign_read(zk_session* s, uint64_t* rows_host, uint32_t* row_flags_host, uint64_t* mpt_host,
                         uint64_t mpt_capacity_rows, uint64_t* n_mpt_out);
int zk_state_assign(const uint64_t* ops, const uint32_t* op_flags, uint64_t n, uint64_t* rows_out,
                    uint32_t* row_flags_out, uint64_t* mpt_out /* capacity n rows */, uint64_t* n_mpt_out,
                    uint32_t opts, uint32_t* status_out, zk_result* result);

/* ---- RW table -> State-circuit operations (the "RW-table lexicographic sort" half): from the EVM circuit's
 *      RW table to the op list zk_state_assign_open takes, on the device.  The reference never links the two in code (SURVEY.md
 *      Appendix A.14); its State witnesses are lists of `Operation`s (src/zkevm_specs/state_circuit.py:616-825) in the order
 *      the circuit checks — (tag, id, address, field_tag, storage_key, rw_counter) strictly increasing (:552-570) — handed to
 *      assign_state_circuit (:855-884), and a block's RW rows come out of `RWDictionary` (evm_circuit/typing.py:464-845) under
 *      the EVM side's `Target` numbering (evm_circuit/table.py:184-204).  This entry re-keys every RW row (Target -> Tag; the
 *      CallContext field tag from the address cell; Account rows without an id; the TxLog address cell unpacked into log_id /
 *      field_tag / index; initial_value = aux0 for Account / AccountStorage rows), sorts the ops by that key — stable: equal
 *      keys keep their table order, like Python's sorted() — and puts a StartOp in front.
 *      rw: uint64[n][14][4] + rw_flags uint32[n] (nullable), the EVM circuit's RW table as in zk_evm_tables.
 *      Outputs: ops COLUMN-major uint64[12][n_ops][4] + op_flags uint32[n_ops], exactly what zk_state_assign_open takes;
 *      n_ops = 1 + the rows kept, known when zk_state_ops_from_rw_open returns (*n_ops_out; at most n + 1).  Left out:
 *      CallContext rows whose field tag exceeds the State circuit's MAX_FIELD_TAG (24, state_circuit.py:34,334) — not an error —
 *      and rejected rows: status (ZK_KIND_VALUE_ERROR << 24) | 1 = the target cell is not a Target, (ZK_KIND_OVERFLOW_ERROR
 *      << 24) | 2 = storage_key hi cell >= 2^128 (lo | hi << 128 does not fit the 256-bit slot).  Status is per RW ROW (n
 *      entries); the tally counts the rejected rows.
 *      With ZK_OPT_DEVICE_PTRS rw / rw_flags are device pointers and ops_dev / op_flags_dev (each nullable: the session then owns
 *      the buffer; capacity (n + 1) ops when given) receive the outputs in place, packed for n_ops.
 *      zk_state_ops_from_rw_open runs the class scan (one streaming pass over the table) and waits for it: the sort key is
 *      compacted to the bits that vary inside each tag class, which decides the number of radix passes.  zk_launch enqueues the
 *      rest (key packing, the radix passes, the op list) asynchronously; zk_collect / zk_read_status as for the circuits. */
int zk_state_ops_from_rw_open(const uint64_t* rw, const uint32_t* rw_flags, uint64_t n, uint64_t* ops_dev, uint32_t* op_flags_dev,
                              uint32_t opts, uint64_t* n_ops_out, zk_session** out);
/* Copy the outputs of the last pass to HOST buffers (each nullable; ops_host holds n_ops ops). */
int zk_state_ops_from_rw_read(zk_session* s, uint64_t* ops_host, uint32_t* op_flags_host, uint64_t* n_ops_out);
int zk_state_ops_from_rw(const uint64_t* rw, const uint32_t* rw_flags, uint64_t n, uint64_t* ops_out /* capacity n + 1 ops */,
                         uint32_t* op_flags_out, uint64_t* n_ops_out, uint32_t opts, uint32_t* status_out, zk_result* result);

/* The two steps in one session — RW table in, State-circuit witness out: the re-keying and the sort as above, then
 * assign_state_circuit / mpt_table_from_ops (zk_state_assign_open) over ops that are read straight from the RW rows through the
 * sorted order; the op list is never written to memory.  Outputs as zk_state_assign_open's, for n_ops rows (*n_ops_out, known
 * when this returns; buffers given with ZK_OPT_DEVICE_PTRS have capacity n_rw + 1 rows and are packed for n_ops:
 * rows uint64[57][n_ops][4], row_flags uint32[n_ops], mpt uint64[n_mpt][12][4]).  zk_launch / zk_collect / zk_read_status
 * (one code per OP) / zk_state_assign_read as for zk_state_assign_open; RW rows the re-keying rejects (codes above) count in
 * the same tally, first_fail_row then being the RW row. */
int zk_state_assign_from_rw_open(const uint64_t* rw, const uint32_t* rw_flags, uint64_t n_rw, uint64_t* rows_dev,
                                 uint32_t* row_flags_dev, uint64_t* mpt_dev, uint32_t opts, uint64_t* n_ops_out, zk_session** out);

/* RW table in, State-circuit VERDICT out — `check_state_circuit(assign_state_circuit(ops, r), ...)` over the ops of an EVM-circuit RW
 * table without the witness in between (state_circuit.py:827-889 then :492-613; tests/test_state_circuit.py's `verify(ops, tables,
 * randomness)` is this composition): the re-keying, the sort and the mock MPT updates as zk_state_assign_from_rw_open, but op2row's
 * rows are evaluated in the registers they are computed in and never stored (1,824 B per row that the two-step form writes and reads
 * back).  zk_launch (status_dev: uint32[n_ops], the State circuit's code per row) / zk_collect (the State circuit's zk_result) /
 * zk_read_status as for zk_state_open; results identical to zk_state_assign_from_rw_open + zk_state_open on its outputs.  An RW row
 * the re-keying rejects or an op assign_state_circuit raises on (codes of zk_state_assign_*) means there is no witness: zk_collect
 * then returns -1 with the count, the first row and its code in zk_last_error() (libzkevm_cpu.so: the open does).
 * Resident passes: the RW table of a session does not change, so once a zk_collect has seen a pass with a witness the session keeps the
 * sorted order, the first-access links, the MPT rows and the root ranks, and every later zk_launch enqueues the evaluation kernel
 * alone (libzkevm_hip.so; 694,509 rows: 0.29 ms for the first pass, 0.13-0.15 ms for the later ones). */
int zk_state_verify_from_rw_open(const uint64_t* rw, const uint32_t* rw_flags, uint64_t n_rw, uint32_t opts, uint64_t* n_ops_out,
                                 zk_session** out);
int zk_state_verify_from_rw(const uint64_t* rw, const uint32_t* rw_flags, uint64_t n, uint32_t opts, uint32_t* status_out /* n_ops <= n + 1 codes */,
                            uint64_t* n_ops_out, zk_result* result);

/* ---- secp256k1 ECDSA verification: computes the `ecdsa_status` column of the Tx / Sig units
 *      on the device instead of taking it from the host.  Replaces `ECDSAVerifyChip.verify`
 *      (src/zkevm_specs/tx_circuit.py:147-158, util/ec.py:109-117), i.e. eth-keys 0.4.0's
 *      `KeyAPI.Signature(vrs=...)` validation + `KeyAPI().ecdsa_verify(msg_hash, signature, public_key)`.
 *      bytes: layout 0 = packed uint8[n][5][32]: pk_x LE, pk_y LE, msg_hash BE, sig_r LE, sig_s LE;
 *             layout 1 / 2 = the byte rows uint8[n][9][32] of the Tx / Sig units of zk_sign_units (rows 2, 3, 5, 7, 8
 *             are those five; the Tx chip keeps msg_hash little-endian, tx_circuit.py:131, the Sig chip big-endian,
 *             util/ec.py:93).
 *      v: optional recovery ids, v[i * v_stride] (the Sig circuit's chip builds Signature(vrs=[v, r, s]) — for Sig
 *      units pass meta + 3 with stride 4; NULL = the Tx circuit's fixed 0).  Status per signature: 0 verified, 1 not verified, (ZK_KIND_UNSUPPORTED << 24) | 1 = eth_keys
 *      BadSignature (v outside {0, 1}, r or s outside (0, N)), (ZK_KIND_UNSUPPORTED << 24) | 2 = a public key with y == P exactly
 *      (the one value outside the engine's domain: eth-keys' `if not p[1]` sees it as non-zero; any other coordinate >= P is
 *      reduced mod P, as eth-keys' formulas do implicitly).  Public keys that are not on the curve are evaluated with eth-keys'
 *      Jacobian case analysis (a Y == 0 point is the point at infinity, inv(0) == 0), so their verdicts are reproducible too.
 *      (zk_tx_assign's key recovery reports BadSignature with the same kind: site 1 as here, plus site 3 = no curve point with
 *      x = r and site 4 = the recovered key is the point at infinity; site 2 stays this entry's.)
 *      These verdicts for keys off the curve / coordinates >= P are those of eth-keys' NATIVE backend (pure Python,
 *      eth_keys/backends/native/ecdsa.py — what the reference's pinned environment uses); an environment with `coincurve`
 *      installed makes KeyAPI use libsecp256k1, which rejects such keys up front.  Well-formed keys verify identically either way.
 *      out_dev (DEVICE pointer, optional): out_dev[i * out_stride] = status, e.g. meta + 0 with stride 4 to fill the
 *      units' meta column in place.  zk_launch / zk_collect / zk_read_status as for the circuits (the tally counts
 *      the signatures that did not verify).
 *      Device memory: the kernel keeps a 1,440-byte table of the key's multiples per lane (one lane per signature above 2^16
 *      signatures, a lane pair below, four lanes up to 2^14): at most 2^17 lanes' worth (189 MB) is allocated per session; larger batches run as
 *      consecutive launches over the same tables. */
int zk_ecdsa_open(const uint8_t* bytes, uint32_t layout, const uint32_t* v, uint32_t v_stride, uint64_t n,
                  uint32_t* out_dev, uint32_t out_stride, uint32_t opts, zk_session** out);
/* One or two signature arrays verified by ONE launch (statuses: batch 0's signatures first): the Tx circuit's and the Sig
 * circuit's chips of a block are independent arrays with different layouts, and one dispatch of their union places its
 * wavefronts better than two concurrent launches do (2 x 2^14 signatures: 1.4 ms against 1.9 ms). */
typedef struct zk_ecdsa_batch {
    const uint8_t* bytes; uint32_t layout; const uint32_t* v; uint32_t v_stride; uint64_t n; uint32_t* out_dev; uint32_t out_stride;
} zk_ecdsa_batch;
int zk_ecdsa_open_batches(const zk_ecdsa_batch* batches, uint32_t n_batches /* 1 or 2 */, uint32_t opts, zk_session** out);
int zk_ecdsa_verify(const uint8_t* bytes, uint32_t layout, const uint32_t* v, uint32_t v_stride, uint64_t n,
                    uint32_t opts, uint32_t* status_out, zk_result* result);

/* ---- Bytecode-circuit witness assignment: replaces assign_bytecode_circuit(k, bytecodes,
 *      keccak_randomness) (src/zkevm_specs/bytecode_circuit.py:104-167: push-data tracking, running value_rlc, length,
 *      q_first / q_last, truncation at 2^k rows, EMPTY_HASH padding).
 *      in_rows: the BytecodeTableRows of the UnrolledBytecodes (:31-33) back to back, ROW-major uint64[n_rows][6][4]
 *      (hash lo/hi, tag, index, is_code, value — the EVM circuit's bytecode-table layout, in input order);
 *      offsets uint64[n_codes + 1]: first row of every bytecode (offsets[0] = 0, offsets[n_codes] = n_rows);
 *      lengths uint64[n_codes]: len(bytecode.bytes).  Output: COLUMN-major uint64[12][2^k][4], what zk_bytecode_open
 *      takes.  With ZK_OPT_DEVICE_PTRS rows_dev (nullable: the session then owns the rows) receives them in place.
 *      The assignment itself cannot fail: the tally is always clean. */
int zk_bytecode_assign_open(const uint64_t* in_rows, uint64_t n_rows, const uint64_t* offsets, const uint64_t* lengths,
                            uint64_t n_codes, uint32_t k, const uint64_t* randomness, uint64_t* rows_dev, uint32_t opts,
                            zk_session** out);
int zk_bytecode_assign_read(zk_session* s, uint64_t* rows_host /* uint64[12][2^k][4] */);
int zk_bytecode_assign(const uint64_t* in_rows, uint64_t n_rows, const uint64_t* offsets, const uint64_t* lengths,
                       uint64_t n_codes, uint32_t k, const uint64_t* randomness, uint64_t* rows_out, uint32_t opts,
                       zk_result* result);

/* ---- Public-inputs (PI) circuit: replaces the `for i: check_row(rows[i], rows[(i + 1) % n], ...)` loop of
 *      pi_circuit.verify_circuit (src/zkevm_specs/pi_circuit.py:447-459; check_row :150-322).  rows: COLUMN-major
 *      uint64[24][n][4] (pi_circuit.Row :104-134 flattened: q_bytes_last, q_tx_table, q_tx_calldata, q_tx_calldata_start,
 *      q_rpi_keccak_lookup, q_rpi_value_start, tx_id_inv, tx_value_lo_inv, tx_id_diff_inv, calldata_gas_cost, is_final,
 *      q_withdrawal_table, rpi_bytes, rpi_bytes_keccakrlc, rpi_value_lc, rpi_digest_word lo, hi, q_rpi_byte_enable,
 *      tx_table.tx_id, .tag, .index, .value.lo, withdrawal_table.id, .amount); keccak: uint64[m][5][4] (is_enabled, input_rlc,
 *      input_len, output lo, hi; KeccakTable :74-101); gas: uint64[k][3][4] (TxCallDataGasCostAccRow :64-68: tx_id, is_final,
 *      gas_cost_acc); circuit_len (Witness.circuit_len); keccak_rand / byte_pow_base: one cell each (the module constants
 *      :834-836).  The fixed u16 table (:351) is a range check.  The copy constraints of verify_circuit (:355-445) compare
 *      table cells with byte strings of the witness on the host (zkevm_specs_amd/pi_circuit.py). */
int zk_pi_open(const uint64_t* rows, uint64_t n, const uint64_t* keccak, uint64_t n_keccak, const uint64_t* gas, uint64_t n_gas,
               uint64_t circuit_len, const uint64_t* keccak_rand, const uint64_t* byte_pow_base, uint32_t opts, zk_session** out);
int zk_pi_verify(const uint64_t* rows, uint64_t n, const uint64_t* keccak, uint64_t n_keccak, const uint64_t* gas, uint64_t n_gas,
                 uint64_t circuit_len, const uint64_t* keccak_rand, const uint64_t* byte_pow_base, uint32_t opts,
                 uint32_t* status_out, zk_result* result);
/* PI circuit copy constraints (pi_circuit.py:355-445): constraint i asserts cells[i] == bytes_to_fq(entry_i[::-1]), entry_i =
 * bytes[i][0 .. lens[i]) (an element of `witness.copy_constrains` as popped, big-endian, left-aligned in its 32-byte slot;
 * lens[i] > 31 fails bytes_to_fq's own assert, util/arithmetic.py:227-229); lens[i] == 0xFFFFFFFF: bytes[i] is a canonical cell
 * (little-endian) compared as is (the word equality of pi_circuit.py:358).  The host side lists the constraints in the
 * reference's statement order; the tally's first failing index is the reference's first failing assert.  Status per
 * constraint: 0, or (ZK_KIND_ASSERTION_ERROR << 24) | site (1 = length assert, 2 = equality). */
int zk_pi_copy_open(const uint64_t* cells, const uint8_t* bytes, const uint32_t* lens, uint64_t n, uint32_t opts, zk_session** out);
int zk_pi_copy_verify(const uint64_t* cells, const uint8_t* bytes, const uint32_t* lens, uint64_t n, uint32_t opts,
                      uint32_t* status_out, zk_result* result);

/* ---- Copy-circuit witness assignment: replaces `CopyCircuit.copy(r, rw_dict, src_id, src_tag, dst_id,
 *      dst_tag, src_addr, src_addr_end, dst_addr, copy_length, src_data, log_id)` (src/zkevm_specs/evm_circuit/typing.py:
 *      1010-1091, _append_row :1093-1151), the RW rows it appends to the RWDictionary (memory_read / memory_write /
 *      tx_log_write, :482-492, :532-556) and the copy-table row `Tables._convert_copy_circuit_to_table` derives
 *      (evm_circuit/table.py:627-651).  One event = one call of copy():
 *      events ROW-major uint64[n][12][4]: src_id lo, hi, src_tag, dst_id lo, hi, dst_tag (CopyDataTypeTag, table.py:308-315),
 *             src_addr, src_addr_end, dst_addr, copy_length, log_id, rw_counter (rw_dict.rw_counter when copy() is called);
 *      flags uint32[n]: bit0 src_id is a Word, bit1 dst_id is a Word (WordOrValue type bits of the rows' id);
 *      data uint16[]: per event the source bytes read below src_addr_end (i < copy_length with src_addr + i < src_addr_end),
 *             value | is_code << 8, events back to back; data_offsets uint64[n + 1].
 *      Domain: source values are bytes, addresses / lengths / counters are below 2^62, TxLog is never a source (the
 *      reference asserts that) — anything else is rejected with an error code, never guessed.
 *      Outputs: rows COLUMN-major uint64[20][n_rows][4] + row_flags uint32[n_rows] (n_rows = 2 * sum of the lengths: what
 *      zk_copy_open takes), table uint64[n_table][14][4] (what zk_evm_tables.copy takes; one row per event that copies
 *      something, in event order), rw uint64[n_rw][14][4] + rw_flags uint32[n_rw] (the RW rows, in rw_counter order per
 *      event).  zk_copy_assign_sizes computes the three counts (host arithmetic over the events).  With
 *      ZK_OPT_DEVICE_PTRS every pointer is a device pointer and the outputs land in the caller's buffers (each nullable:
 *      the session then owns it), ready for zk_copy_open / zk_evm_open without leaving the device. */
typedef struct zk_copy_events {
    const uint64_t* events;     const uint32_t* flags;       uint64_t n_events;
    const uint16_t* data;       const uint64_t* data_offsets;
    const uint64_t* randomness;
} zk_copy_events;
int zk_copy_assign_sizes(const zk_copy_events* ev, uint32_t opts, uint64_t* n_rows, uint64_t* n_table, uint64_t* n_rw);
int zk_copy_assign_open(const zk_copy_events* ev, uint64_t* rows_dev, uint32_t* row_flags_dev, uint64_t* table_dev,
                        uint64_t* rw_dev, uint32_t* rw_flags_dev, uint32_t opts, zk_session** out);
int zk_copy_assign_read(zk_session* s, uint64_t* rows_host, uint32_t* row_flags_host, uint64_t* table_host,
                        uint64_t* rw_host, uint32_t* rw_flags_host);
int zk_copy_assign(const zk_copy_events* ev, uint64_t* rows_out, uint32_t* row_flags_out, uint64_t* table_out,
                   uint64_t* rw_out, uint32_t* rw_flags_out, uint32_t opts, zk_result* result);

/* ---- A block as a ONE-SHOT (BASELINE config 5; round 6): everything the Super circuit derives on the device and one evaluation pass of
 *      its six circuits, from the block's raw device-resident inputs, in one call.  The reference has no super-circuit driver (SURVEY.md
 *      Appendix A.14); the inputs are what its own constructors take: the EVM circuit's tables and steps (`Tables`, evm_circuit/table.py:
 *      583-625), the byte strings the block hashes (`KeccakCircuit.add`, evm_circuit/typing.py:854-865: the contracts first, then the
 *      SHA3 inputs), the copy events (`CopyCircuit.copy`, :1010-1091), the Exp circuit's rows, the Tx units.  Derived inside: the keccak
 *      table (zk_keccak_*: rows [0, n_codes) are the Bytecode circuit's table, the rest the EVM circuit's), the Bytecode circuit's rows
 *      (zk_bytecode_assign_*: the unrolled bytecodes ARE evm.bytecode, cut by code_offsets / code_lengths), the Copy circuit's rows and
 *      the EVM circuit's copy table (zk_copy_assign_*; the Copy circuit looks up evm.rw / evm.bytecode / evm.tx), the State circuit's
 *      Exp circuit's rows and the EVM circuit's exp table when exp_events.n_events > 0 (zk_exp_assign_*: launched on the EVM chain ahead
 *      of the open, the Exp circuit's pass on the last chain ordered behind it by an event; exp_rows / evm.exp must then be absent:
 *      passing both forms is an error; with n_events == 0 they are taken as given, as before), the State circuit's
 *      verdict from evm.rw (zk_state_verify_from_rw_open: the State rows are evaluated where they are computed; with
 *      ZK_OPT_BLOCK_STATE_ROWS or ZK_OPT_STATE_COMPACT the witness is written and read back as zk_state_assign_from_rw_open +
 *      zk_state_open do — the same results, for comparison).  evm.copy / evm.keccak are ignored.  Four host threads drive four chains on
 *      four streams of the calling thread's device: State | keccak of the contracts -> Bytecode circuit | copy assignment -> Copy
 *      circuit, keccak of the SHA3 inputs -> EVM open + pass | Bytecode assignment, Exp, Tx (the EVM circuit's keccak table holds the
 *      SHA3 rows only, so its chain never waits for the long pass over the contracts).
 *      Every pointer is a device pointer (opts must carry ZK_OPT_DEVICE_PTRS; ZK_OPT_STATE_COMPACT is honoured).  results[c]: the
 *      tally of circuit c (enum below; rows_evaluated == 0 for a circuit without rows); a failing witness ASSIGNMENT (keccak input,
 *      State op, ...) is an error return with the text in zk_last_error.  chain_ms (nullable, ten doubles; a measurement aid): host
 *      milliseconds from the call to the end of each chain [0..3], to its start [4..7], to the end of the last one [8] and to the
 *      return [9]. */
/* EXP events, the input of zk_exp_assign_* (documented with those entries below): ROW-major uint64[n][5][4] — identifier, base lo,
 * base hi, exponent lo, exponent hi */
typedef struct zk_exp_events {
    const uint64_t* events;     uint64_t n_events;
    uint64_t max_exp_steps;     /* ExpCircuit(max_exp_steps): pad with dummy rows up to 7 * max_exp_steps rows; 0 = no padding */
} zk_exp_events;
typedef struct zk_block {
    zk_evm_tables evm;
    const uint8_t* hashed_data; uint64_t hashed_bytes; const uint64_t* hashed_offsets;  /* n_hashed + 1 offsets */
    uint64_t n_codes, n_hashed;
    const uint64_t* randomness;                                                          /* one cell: the block's keccak randomness */
    const uint64_t* code_offsets; const uint64_t* code_lengths; uint64_t n_bytecodes; uint32_t k; uint32_t reserved;
    zk_copy_events copy_events;                                                          /* n_events == 0: no Copy circuit rows */
    const uint64_t* exp_rows; uint64_t n_exp_rows;                                       /* column-major uint64[21][n][4] */
    zk_sign_units tx;                                                                    /* n_units == 0: no Tx circuit */
    zk_exp_events exp_events;                                                            /* n_events > 0: the Exp rows and evm.exp are derived */
} zk_block;
enum { ZK_BLOCK_EVM = 0, ZK_BLOCK_STATE = 1, ZK_BLOCK_BYTECODE = 2, ZK_BLOCK_TX = 3, ZK_BLOCK_COPY = 4, ZK_BLOCK_EXP = 5, ZK_BLOCK_NCIRCUITS = 6 };
int zk_block_verify(const zk_block* b, uint32_t opts, zk_result* results /* [ZK_BLOCK_NCIRCUITS] */, double* chain_ms /* [10], nullable */);

/* ---- Session protocol shared by every circuit.
 * launch: enqueue one evaluation pass (asynchronous) on the session's stream.  status_dev: optional DEVICE buffer of
 *         n uint32 receiving the per-row status codes.  A caller-provided status_dev is final in stream order: once the
 *         work enqueued by zk_launch has completed (the caller's own event / stream synchronisation on the session's stream,
 *         no zk_collect needed) every row's code is there — for EVM sessions this includes the pairs the fast kernel hands
 *         to the general build (malformed word cells, generic-index fallbacks): that kernel is enqueued behind the pass
 *         whenever status_dev is given.  Without status_dev the codes go to the session's own buffer and are final once
 *         zk_collect or zk_read_status has returned (they run the general build only if the pass left such pairs).
 *         One-shot EVM sessions (ZK_OPT_SINGLE_PASS, no status_dev, no ZK_OPT_SIDE_STREAM) launch lazily: zk_launch enqueues the
 *         build that holds BASELINE config 3's states, and the builds for the rarer state groups are enqueued by the first
 *         zk_collect / zk_read_status / zk_launch that follows — only if the open's sort, which tells the host through the session's
 *         page-locked block, found steps of theirs (ZK_LAZY_TAIL=0: always, from zk_launch).  Results are the same either way.
 * collect: wait for all enqueued passes, return the tally of the LAST pass and the mean kernel
 *         time over the passes since the previous collect. */
int zk_launch(zk_session* s, uint32_t* status_dev);
int zk_collect(zk_session* s, zk_result* result);
/* Copy the per-row status of the last pass into a HOST buffer (n entries).  Fails when that pass wrote its statuses
 * to a caller-provided status_dev (they are the caller's then); all zero before the first pass. */
int zk_read_status(zk_session* s, uint32_t* status_host);
/* Device-side time spans, measured by HIP events that ride on the kernel dispatches themselves (measurement aid of bench.py;
 * EVM sessions, -1 where not measured).  zk_session_timing, after a zk_collect: open_ms = first to last kernel of zk_evm_open
 * (index, packed-record and first-pass sort builds), span_ms = first open kernel to the end of the session's FIRST pass.
 * zk_last_timing: the same for the calling thread's last one-shot zk_evm_verify, plus its pass span (== zk_result.kernel_ms). */
int zk_session_timing(zk_session* s, double* open_ms, double* span_ms);
int zk_last_timing(double* open_ms, double* pass_ms, double* span_ms);
/* The same three spans SUMMED over the calling thread's one-shot zk_evm_verify calls since the last reset (sums_ms[3]: open, pass,
 * span; *count = calls summed; reset != 0 clears them after reading): a caller that wants the mean span of K timed calls reads once
 * behind the loop instead of once per call (bench.py's timed region: one foreign call per step instead of two). */
int zk_timing_sums(double* sums_ms, uint64_t* count, int reset);
/* Host microseconds the calling thread's last one-shot zk_evm_verify spent inside its open / launch / collect / close calls
 * (tuning aid: where the wall time beyond the device span goes). */
int zk_last_host_phases(double* us4);

/* ---- Multi-GPU tally (§2 (vii) "RCCL all-reduce of {fail_count: SUM, first_fail_row: MIN}").  Rows shard across
 *      the GPUs of a node with no data-path collective; the only exchange is the pass / fail tally.  These entries put it behind
 *      the C ABI for hosts without torch.distributed: ONE RCCL collective per call — an all-gather of three 64-bit words per rank
 *      (fail count, first failing GLOBAL row, its status code) on the communicator's own stream, read back once; SUM and the
 *      lexicographic MIN are then taken on the host, identically on every rank (the same exchange the Python mirror makes through
 *      torch.distributed, zkevm_specs_amd/distributed.py reduce_tally).  librccl.so.1 is loaded on first use (dlopen): processes
 *      that never call these entries do not depend on it.
 *        zk_dist_unique_id  rank 0: a fresh communicator id (ncclGetUniqueId); the host carries it to the other ranks
 *        zk_dist_init       every rank, after zk_init(device): joins the communicator (collective: blocks until all ranks call)
 *        zk_dist_tally      collective.  local: this rank's zk_collect result; row_offset: global index of its row 0.
 *                           global->fail_count = SUM, first_fail_row / first_fail_code = those of the smallest failing global
 *                           row (UINT64_MAX / 0 if none), rows_evaluated = SUM, launches = local's, kernel_ms = MAX over ranks
 *        zk_dist_close      leaves the communicator
 *      The CPU backend implements them for world == 1 (the identity with the offset applied). */
#define ZK_DIST_ID_BYTES 128
typedef struct zk_comm zk_comm;
int zk_dist_unique_id(uint8_t* id /* ZK_DIST_ID_BYTES */);
int zk_dist_init(const uint8_t* id /* ZK_DIST_ID_BYTES */, int rank, int world, zk_comm** out);
int zk_dist_tally(zk_comm* c, const zk_result* local, uint64_t row_offset, zk_result* global);
int zk_dist_close(zk_comm* c);
/* Re-bind a session to another stream of its device (NULL = the engine's own); waits for its enqueued passes first. */
int zk_session_set_stream(zk_session* s, void* hip_stream);
int zk_close(zk_session* s);

/* ---- ECC circuit: replaces circuit2rows + the row loop of ecc_circuit.verify_circuit (src/zkevm_specs/ecc_circuit.py:386-433;
 *      EccCircuitRow.assign* :35-232, verify :234-333, util/ec.py ECCVerifyChip / ECCPairingVerifyChip :120-201).
 *      Rows in circuit2rows order: the n_add adds, the n_mul muls, then the n_pairing pairings.
 *      points: uint64[n_add + n_mul][6][4], 256-bit words (4 x u64 little-endian, NOT reduced):
 *              add: p.x, p.y, q.x, q.y, out.x, out.y;   mul: p.x, p.y, s, 0, out.x, out.y.
 *      pair_pts: uint64[pair_off[n_pairing]][6][4], one entry per (g1_pts[i], g2_pts[i]) in EIP-197 order:
 *              p.x, p.y, x.c1, x.c0, y.c1, y.c0 (imaginary part first); pairing op k owns entries [pair_off[k], pair_off[k + 1]).
 *      pair_off: uint32[n_pairing + 1], pair_off[0] = 0, non-decreasing.   pair_out: uint64[n_pairing][4], the op's `out` word.
 *      randomness: one cell (keccak_randomness).  max_add / max_mul / max_pairing: the circuit's max_*_ops (clamped to 0 / 1 by the
 *      caller: the reference's counters are locals of verify(), so only a max below 1 can fail).
 *      rows (zk_ecc_assign's output, zk_ecc_verify's input): uint64[n][13][4], the EccTableRow cells as flatten_ecc_table lays them
 *      out — op_type, px lo / hi, py lo / hi, qx lo / hi, qy lo / hi, input_rlc, out_x, out_y, is_valid.  zk_ecc_verify checks
 *      the rows against the chips built from the ops, as verify_circuit does (status: (kind << 24) | site, csrc/ecc_circuit.hpp). */
typedef struct zk_ecc_ops {
    const uint64_t* points;     uint64_t n_add;              uint64_t n_mul;
    const uint64_t* pair_pts;   const uint32_t* pair_off;    const uint64_t* pair_out;   uint64_t n_pairing;
    const uint64_t* randomness;
    uint32_t max_add, max_mul, max_pairing;
} zk_ecc_ops;
int zk_ecc_assign(const zk_ecc_ops* ops, uint32_t opts, uint64_t* rows_out);
int zk_ecc_verify(const zk_ecc_ops* ops, const uint64_t* rows, uint32_t opts, uint32_t* status_out, zk_result* result);
/* ECC sessions: the ops stay resident and the rows are evaluated pass after pass (zk_launch / zk_collect / zk_read_status /
 * zk_session_set_stream / zk_close as for every row circuit; twin tally; status_dev or the session's own buffer, uint32[n]).
 * zk_ecc_open: host pointers are staged once at open; with ZK_OPT_DEVICE_PTRS the arrays of `ops` (the struct itself is host memory),
 *      `rows` and `randomness` are device pointers used in place.  pair_off (4 B per op) is read back at open to validate it
 *      (pair_off[0] = 0, non-decreasing) and to size the per-pair work, the randomness cell to check that it is canonical; points and
 *      rows are never read back.  Status codes are those of zk_ecc_verify, bit for bit, including which check of a row fails first.
 *      zk_set_range(s, lo, hi) evaluates rows [lo, hi) of the n_add + n_mul + n_pairing rows (circuit2rows order; ops and rows are
 *      replicated on every rank, only the range differs).  The range may cut through the adds, the muls or the pairings and — for this
 *      circuit only — may be empty (lo == hi).  rows_evaluated == hi - lo, first_fail_row is a global row, statuses outside the range
 *      are zero after zk_set_range.
 *      A pass is three launches in stream order: the add / mul rows of the range (one lane per row), then the pairing rows in two
 *      stages — one lane per (op, pair) computes the pair's subgroup / on-curve / infinity flags and its Miller value into a record the
 *      session owns, then one lane per op runs the row's checks in their order over the records, multiplies the Miller values and does
 *      the final exponentiation.  status_dev is final in stream order.
 * zk_ecc_assign_open / zk_ecc_assign_read: circuit2rows over resident ops.  The 13-cell rows go to rows_dev (a device buffer
 *      uint64[n][13][4]; needs ZK_OPT_DEVICE_PTRS) or, when it is null, to the session's own buffer, which zk_ecc_assign_read copies
 *      to the host.  The output is what zk_ecc_open takes as `rows`. */
int zk_ecc_open(const zk_ecc_ops* ops, const uint64_t* rows, uint32_t opts, zk_session** out);
int zk_ecc_assign_open(const zk_ecc_ops* ops, uint64_t* rows_dev, uint32_t opts, zk_session** out);
int zk_ecc_assign_read(zk_session* s, uint64_t* rows_host);

/* ---- Withdrawal circuit: replaces the row loop of withdrawal_circuit.verify_circuit (src/zkevm_specs/withdrawal_circuit.py:128-201)
 *      and the reference test's withdrawals2witness (tests/test_withdrawal_circuit.py).
 *      rows: uint64[n_rows][8][4] — id, validator_id, address, amount, hash lo, hash hi, root lo, root hi (canonical cells).
 *      mpt: uint64[n_mpt][12][4], the State circuit's MPT-table layout (zk_state_open).   keccak: uint64[n_keccak][5][4] —
 *      is_enabled, input_rlc, input_len, output lo, hi (the (0, 0, 0, 0, 0) row is in it only when the caller put it there).
 *      block: uint64[n_block][4][4] — field_tag, block_number_or_zero, value lo, hi.   randomness: one cell (keccak_randomness).
 *      max_withdrawals: MAX_WITHDRAWALS (rows at or beyond it are not read; fewer rows than it raise IndexError, as the reference).
 *      total_rows: len(rows) of the whole witness; row_base: the global index of rows[0] (0 unless the session holds a shard).
 *      The session evaluates global rows [row_base, row_base + n) with n = max(1, min(max_withdrawals, total_rows)) - row_base,
 *      capped at n_rows (status[j] is global row row_base + j); the WithdrawalRoot block lookup rides on the row max_withdrawals - 1.
 *      Status: (kind << 24) | site, csrc/withdrawal_circuit.hpp (1 id chain, 2 keccak, 3 MPT, 4 block lookup).
 *      zk_withdrawal_assign: withdrawals uint64[n][5][4] — id, validator_id, address, amount (canonical cells), root (a 256-bit word)
 *      -> rows_out uint64[max(n, max_withdrawals)][8][4], the digest keccak(rlp([id, validator_id, address, amount])) computed on the
 *      device, rows from n on padding rows (0, 0, 0, 0, Word(0), the last root); keccak_out (optional) uint64[n][5][4], the rows
 *      KeccakTable.add makes: (1, RLC of the RLP, its length, digest lo, hi). */
typedef struct zk_withdrawal_witness {
    const uint64_t* rows;     uint64_t n_rows;    uint64_t row_base;   uint64_t total_rows;   uint64_t max_withdrawals;
    const uint64_t* mpt;      uint64_t n_mpt;
    const uint64_t* keccak;   uint64_t n_keccak;
    const uint64_t* block;    uint64_t n_block;
    const uint64_t* randomness;
} zk_withdrawal_witness;
int zk_withdrawal_open(const zk_withdrawal_witness* w, uint32_t opts, zk_session** out);
int zk_withdrawal_verify(const zk_withdrawal_witness* w, uint32_t opts, uint32_t* status_out, zk_result* result);
int zk_withdrawal_assign(const uint64_t* withdrawals, uint64_t n, uint64_t max_withdrawals, const uint64_t* randomness, uint32_t opts,
                         uint64_t* rows_out, uint64_t* keccak_out);

/* ---- Tx circuit witness assignment: replaces txs2witness (src/zkevm_specs/tx_circuit.py:432-481; tx2witness :332-406, padding_tx
 *      :315-329, the dummy chip of the padding slots :409-425).  From raw legacy transactions to the wire flatten_tx_witness makes.
 *      Inputs (zk_tx_inputs): fields uint64[n][8][4], per tx the 256-bit words nonce, gas_price, gas, to, value, sig_v, sig_r, sig_s;
 *      to_is_none uint32[n] (1: tx.to is None — IsCreate, rlp's empty string); calldata: the txs' data back to back with byte offsets
 *      uint64[n + 1] (offsets[0] = 0, non-decreasing, offsets[n] <= max_calldata_bytes); chain_id; MAX_TXS (>= n) and
 *      MAX_CALLDATA_BYTES; randomness: one cell (keccak_randomness).  `to` must be below 2^160 (the caller rejects wider values as
 *      encode_to's OverflowError does).
 *      Per tx: rlp([nonce, gas_price, gas, to_bytes, value, data, chain_id, 0, 0]) is hashed with keccak-256 on the device; the
 *      sender's key is recovered from (v, r, s, hash) as eth_keys does (oracle/refshim/eth_keys/__init__.py:99-140); keccak of the
 *      key gives the address.  Status per tx: 0, or (ZK_KIND_UNSUPPORTED << 24) | site for eth_keys' BadSignature — site 1 the
 *      parity v - 35 - 2 chain_id outside {0, 1} or r / s outside (0, N), site 3 no curve point with x = r, site 4 Q at infinity.
 *      The outputs of a tx whose status is not 0 are unspecified (the reference raises there).
 *      Outputs (zk_tx_wire):
 *        tx_rows uint64[max_txs * 12 + max_calldata_bytes][5][4] (tx_id, tag, index, value lo, hi) + tx_flags uint32[..] (is_word):
 *          the 12 fixed rows of every tx (GasPrice, Value, TxSignHash are Words), padding_tx(i + 1) for the slots from n on
 *          (GasPrice / Value Word(0), TxSignHash FQ(0)), the CallData rows in tx order, then (0, CallData, 0, 0) rows;
 *        bytes uint8[max_txs][9][32], cells column-major uint64[8][max_txs][4], meta uint32[max_txs][4]: the SignVerify units in
 *          zk_sign_units' Tx layout (padding slots: DUMMY_PUBLIC_KEY / DUMMY_SIGNATURE / DUMMY_MSG_HASH, address 0); meta[:, 0] is
 *          0xffffffff (pending) for the ECDSA pass (zk_ecdsa_open, layout 1, out_dev = meta, out_stride 4) to fill;
 *        keccak uint64[n + 1 capacity][5][4]: KeccakTable's rows as a set, sorted, without duplicates, the all-zero row included
 *          (flatten_keccak_tuples); their number comes out of zk_tx_assign_read / zk_tx_assign (n_keccak).
 *      zk_tx_assign_open: with ZK_OPT_DEVICE_PTRS every input is a device pointer and the non-null pointers of `out_dev` receive
 *      the outputs in place (null ones: the session owns the buffer); without it `out_dev` must be null.  zk_launch (status_dev:
 *      uint32[n]) / zk_collect (tally over the txs) / zk_read_status as for the circuits; zk_tx_assign_read copies the last pass's
 *      outputs to the non-null HOST pointers of `host` and the keccak row count to *n_keccak_out (nullable). */
typedef struct zk_tx_inputs {
    const uint64_t* fields;     const uint32_t* to_is_none;  uint64_t n_txs;
    const uint8_t* calldata;    const uint64_t* calldata_offsets;
    uint64_t chain_id;          uint64_t max_txs;            uint64_t max_calldata_bytes;
    const uint64_t* randomness;
} zk_tx_inputs;
typedef struct zk_tx_wire {
    uint64_t* tx_rows;  uint32_t* tx_flags;
    uint8_t* bytes;     uint64_t* cells;     uint32_t* meta;
    uint64_t* keccak;
} zk_tx_wire;
int zk_tx_assign_open(const zk_tx_inputs* in, const zk_tx_wire* out_dev, uint32_t opts, zk_session** out);
int zk_tx_assign_read(zk_session* s, const zk_tx_wire* host, uint64_t* n_keccak_out);
int zk_tx_assign(const zk_tx_inputs* in, const zk_tx_wire* out, uint32_t opts, uint32_t* status_out, uint64_t* n_keccak_out, zk_result* result);

/* ---- Exp circuit witness assignment: replaces ExpCircuit.add_event / fill_dummy_events (src/zkevm_specs/evm_circuit/typing.py:
 *      868-994) and the exp-table rows Tables._convert_exp_circuit_to_table derives (evm_circuit/table.py:654-671).
 *      One event = one add_event(base, exponent, identifier): events ROW-major uint64[n][5][4] — identifier, base lo, base hi,
 *      exponent lo, exponent hi (canonical cells; the halves of the two Words below 2^128).  An event with exponent 0 or 1
 *      contributes no rows; any other bit_length(exponent) - 1 + popcount(exponent) - 1 step rows, from the full exponent down to
 *      base * base (exponent 2), d = base^exponent mod 2^256 on every row.
 *      Outputs: rows COLUMN-major uint64[21][n_rows][4] (what zk_exp_open takes): the step rows of all events in event order, then
 *      the dummy rows of fill_dummy_events while n_rows < 7 * max_exp_steps (none when the step rows reach or exceed that);
 *      table uint64[n_table][11][4] (what zk_evm_tables.exp takes): one row per step row in the same order, plus ONE row
 *      (1, 0, 0, 1, 0, 0, 0, 1, 0, 1, 0) for the dummy rows when there is at least one (the reference's table is a set).
 *      zk_exp_assign_sizes: the three counts; they depend on the exponents' bits, so with ZK_OPT_DEVICE_PTRS they are computed on
 *      the device and read back (one small read).  n_events == 0 is allowed (dummy rows only).
 *      zk_exp_assign_open: with ZK_OPT_DEVICE_PTRS `events` is a device pointer and rows_dev / table_dev (each nullable: the
 *      session then owns the buffer), sized with zk_exp_assign_sizes, receive the outputs, ready for zk_exp_open / zk_evm_open
 *      without leaving the device.  zk_launch / zk_collect / zk_read_status as for the circuits (one status per row, always 0:
 *      the domain is checked at open).  An assignment without any row (n_rows == 0) cannot be opened.
 *      Domain, rejected at sizes / open with an error code and its text in zk_last_error, never guessed:
 *        ZK_ERR_EXP_CELL   a cell is not canonical (identifier >= p, a lo / hi half >= 2^128);
 *        ZK_ERR_EXP_ORDER  the identifiers of row-producing events are not strictly increasing (the reference's set would merge,
 *                          or make ambiguous, what a plain row list cannot; a trace produces them in rw_counter order);
 *        ZK_ERR_EXP_ROWS   2^31 rows or more. */
#define ZK_ERR_EXP_CELL (-40)
#define ZK_ERR_EXP_ORDER (-41)
#define ZK_ERR_EXP_ROWS (-42)
/* (zk_exp_events: defined in front of zk_block, which carries one) */
int zk_exp_assign_sizes(const zk_exp_events* ev, uint32_t opts, uint64_t* n_rows, uint64_t* n_step_rows, uint64_t* n_table);
int zk_exp_assign_open(const zk_exp_events* ev, uint64_t* rows_dev, uint64_t* table_dev, uint32_t opts, zk_session** out);
int zk_exp_assign_read(zk_session* s, uint64_t* rows_host, uint64_t* table_host);
int zk_exp_assign(const zk_exp_events* ev, uint64_t* rows_out, uint64_t* table_out, uint32_t opts, zk_result* result);
/* the three counts of an open session (what zk_exp_assign_sizes returns for its events), without a second size pass */
int zk_exp_assign_counts(zk_session* s, uint64_t* n_rows, uint64_t* n_step_rows, uint64_t* n_table);

/* ---- PI circuit witness assignment: replaces public_data2witness (src/zkevm_specs/pi_circuit.py:839-1073) — from the block header,
 *      its transactions and its withdrawals to everything zk_pi_open and zk_pi_copy_open take, and to the small tables of the Witness.
 *      Inputs (zk_pi_inputs), 256-bit words as 4 x u64 little-endian:
 *        chain_id; block uint64[9][4]: hash, coinbase, state_root, prev_randao, number, gas_limit, time, base_fee, withdrawals_root
 *        (the fields public_data2witness reads); state_root_prev uint64[4]; block_hashes uint64[256][4];
 *        tx_fields uint64[n_txs][7][4]: nonce, gas_price, gas, from_addr, to_addr (0 when None), value, tx_sign_hash; to_is_none uint32[n_txs];
 *        calldata: the txs' data back to back with byte offsets uint64[n_txs + 1] (offsets[0] = 0, non-decreasing), as zk_tx_inputs;
 *        withdrawals uint64[n_withdrawals][4][4]: id (a canonical cell: the table's FQ(id)), validator_id, address, amount;
 *        max_txs, max_calldata_bytes, max_withdrawals; keccak_rand, byte_pow_base: one cell each (the module constants, :834-836).
 *      Outputs (zk_pi_wire), circuit_len = 8454 + 336 max_txs + max_calldata_bytes + 56 max_withdrawals rows:
 *        rows          uint64[24][circuit_len][4] column-major: flatten_pi_rows, what zk_pi_open takes;
 *        gas           uint64[1 + calldata bytes][3][4]: the (0, 0, 0) row, then one row per calldata byte in tx / index order
 *                      (the reference's set, sorted: flatten_pi_gas_table);
 *        keccak        uint64[2][5][4]: the all-zero row, then (1, input RLC, circuit_len, digest lo, hi);
 *        cc_cells uint64[n][4], cc_bytes uint8[n][32], cc_lens uint32[n]: the copy constraints in verify_circuit's statement order
 *                      (:355-445), what zk_pi_copy_open takes; n = 538 + 4 (10 max_txs + 1) + 2 max_calldata_bytes + 5 max_withdrawals;
 *        block_table   uint64[268][2][4] (lo, hi) + block_flags uint32[268] (is_word): the 265 entries of the value column, then block hash,
 *                      state root, previous state root;
 *        tx_table      uint64[10 max_txs + 1 + max_calldata_bytes][5][4] (tx_id, tag, index, value lo, hi) + tx_flags uint32[..] (is_word);
 *        wd_table      uint64[max_withdrawals][5][4]: id, validator_id, address lo, hi, amount;
 *        public_inputs uint64[4][2][4]: pi_keccak, block_hash, state_root, state_root_prev as lo, hi;
 *        raw_bytes uint8[circuit_len] + raw_lens uint32[n_values]: Witness.copy_constrains, its byte strings back to back and their
 *                      lengths; n_values = 533 + 33 max_txs + max_calldata_bytes + 5 max_withdrawals.
 *      zk_pi_assign_open: with ZK_OPT_DEVICE_PTRS every input is a device pointer and the non-null pointers of `out_dev` receive the
 *      outputs in place (null ones, or a null out_dev: the session owns the buffer); without it out_dev must be null.  zk_launch /
 *      zk_collect / zk_read_status as for the circuits (one status per row, always 0: the domain is checked at open); zk_pi_assign_read
 *      copies the last pass's outputs to the non-null HOST pointers of `host`.
 *      Domain, rejected at sizes / open with an error code and its text in zk_last_error:
 *        ZK_ERR_PI_TXS          no tx, or more than max_txs (the reference's asserts);
 *        ZK_ERR_PI_WITHDRAWALS  no withdrawal, or more than max_withdrawals;
 *        ZK_ERR_PI_CALLDATA     more calldata bytes than max_calldata_bytes;
 *        ZK_ERR_PI_FIELD        a field wider than the bytes to_bytes gives it (coinbase / from_addr / to_addr 20; number, gas_limit, time,
 *                               nonce, gas, validator_id, amount 8), a withdrawal id that is no canonical cell, offsets that decrease;
 *        ZK_ERR_PI_ROWS         2^31 rows or more. */
#define ZK_ERR_PI_TXS (-50)
#define ZK_ERR_PI_WITHDRAWALS (-51)
#define ZK_ERR_PI_CALLDATA (-52)
#define ZK_ERR_PI_FIELD (-53)
#define ZK_ERR_PI_ROWS (-54)
typedef struct zk_pi_inputs {
    uint64_t chain_id;
    const uint64_t* block;      const uint64_t* state_root_prev;   const uint64_t* block_hashes;
    const uint64_t* tx_fields;  const uint32_t* to_is_none;        uint64_t n_txs;
    const uint8_t* calldata;    const uint64_t* calldata_offsets;
    const uint64_t* withdrawals; uint64_t n_withdrawals;
    uint64_t max_txs;           uint64_t max_calldata_bytes;       uint64_t max_withdrawals;
    const uint64_t* keccak_rand; const uint64_t* byte_pow_base;
} zk_pi_inputs;
typedef struct zk_pi_wire {
    uint64_t* rows;         uint64_t* gas;          uint64_t* keccak;
    uint64_t* cc_cells;     uint8_t* cc_bytes;      uint32_t* cc_lens;
    uint64_t* block_table;  uint32_t* block_flags;
    uint64_t* tx_table;     uint32_t* tx_flags;
    uint64_t* wd_table;     uint64_t* public_inputs;
    uint8_t* raw_bytes;     uint32_t* raw_lens;
} zk_pi_wire;
int zk_pi_assign_sizes(const zk_pi_inputs* in, uint32_t opts, uint64_t* circuit_len, uint64_t* n_gas, uint64_t* n_constraints);
int zk_pi_assign_open(const zk_pi_inputs* in, const zk_pi_wire* out_dev, uint32_t opts, zk_session** out);
int zk_pi_assign_read(zk_session* s, const zk_pi_wire* host);
int zk_pi_assign(const zk_pi_inputs* in, const zk_pi_wire* out, uint32_t opts, zk_result* result);

/* ---- Sig circuit witness assignment: from signed data (msg_hash, v, r, s) to the Sig circuit's witness — what the reference's
 *      tests build in signedData2witness (tests/test_sig_circuit.py:40-67) — and, from the same key recovery, the EVM circuit's sig
 *      table and the aux cells of the ecRecover precompile (tests/evm/precompiles/test_ecRecover.py:78-112).
 *      Inputs (zk_sig_inputs): fields uint64[n][4][4], per signature the 256-bit words msg_hash (the word of the hash's 32 bytes,
 *      little-endian: Word(msg_hash_bytes); z is the same bytes read big-endian), sig_v, sig_r, sig_s; addr (nullable) the CLAIMED
 *      address per signature; expect_valid (nullable); v_offset: 0 where v is the parity (SignedData), 27 where it is the
 *      precompile's input word; randomness: one cell (keccak_randomness).
 *      Status per signature: 0, or (ZK_KIND_UNSUPPORTED << 24) | site as zk_tx_assign's key recovery — site 1 the parity
 *      v - v_offset outside {0, 1} (a v above 2^64 included) or r / s outside (0, N), site 3 no curve point with x = r, site 4 Q at
 *      infinity.
 *      Outputs (zk_sig_wire), n rows each unless said otherwise:
 *        bytes uint8[n][9][32], cells column-major uint64[8][n][4], meta uint32[n][4]: the units in zk_sign_units' Sig layout.
 *          Byte rows: key x, y, x, y (little-endian), the hash's 32 bytes twice, keccak256(x BE || y BE), r, s (little-endian).
 *          Cells: the claimed address (addr null: the recovered one), msg_hash lo, hi, FQ(v.lo) - FQ(v_offset) (the parity), r lo, hi,
 *          s lo, hi.  Meta: (0xffffffff pending, expect_valid or 1, 0, v - v_offset — 0xffffffff where that does not fit 32 bits), ready
 *          for zk_ecdsa_open (layout 2, v = meta + 3 with stride 4, out_dev = meta, out_stride 4);
 *        keccak uint64[n + 1 capacity][5][4]: KeccakTable.add's row of every recovered key, as a set, sorted, without duplicates, the
 *          all-zero row included (flatten_keccak_tuples); their number in n_keccak;
 *        sig_table uint64[n capacity][9][4]: (msg_hash lo, hi, FQ(v.lo) - FQ(v_offset), r lo, hi, s lo, hi, recovered_addr, is_valid)
 *          per signature — the recovered address (never the claimed one) and 1, or 0 and 0 — the first occurrence of every distinct
 *          row, in input order; their number in n_sig_rows (zk_evm_tables.sig / n_sig);
 *        aux uint64[n][12][4], row i for signature i (zk_evm_tables.aux, kind 5): msg_hash, v as given, r, s as lo / hi, the recovered
 *          address, input_rlc (Horner over msg_hash || v || r || s, each 32 bytes as in `fields`, first byte highest power),
 *          output_rlc (the same over the address's 32 little-endian bytes), randomness.
 *      A signature whose status is not 0 has defined outputs: key rows and key hash zero, the rest of its unit as given, cell 0 the
 *      claimed address or 0, no keccak row, recovered address / is_valid / output_rlc 0.
 *      The session protocol is zk_tx_assign's: zk_sig_assign_open with ZK_OPT_DEVICE_PTRS takes device inputs and writes the non-null
 *      pointers of `out_dev` in place (null ones: the session owns the buffer); zk_launch (status_dev: uint32[n]) / zk_collect
 *      (tally over the signatures) / zk_read_status; zk_sig_assign_read copies the last pass's outputs to the non-null HOST pointers
 *      of `host` and the two row counts out (each nullable). */
typedef struct zk_sig_inputs {
    const uint64_t* fields;        /* uint64[n][4][4]: msg_hash, sig_v, sig_r, sig_s as 256-bit words */
    const uint64_t* addr;          /* nullable uint64[n][4]: the CLAIMED address -> cells[0]; NULL: the recovered one */
    const uint32_t* expect_valid;  /* nullable uint32[n] -> meta[:, 1]; NULL: 1 */
    uint64_t n;
    uint32_t v_offset;             /* 0: v is the parity (SignedData); 27: v is the precompile's input word */
    uint32_t reserved;
    const uint64_t* randomness;    /* one cell: keccak_randomness */
} zk_sig_inputs;
typedef struct zk_sig_wire {
    uint8_t* bytes; uint64_t* cells; uint32_t* meta;   /* the units, zk_sign_units' Sig layout */
    uint64_t* keccak;                                  /* capacity n + 1 rows */
    uint64_t* sig_table;                               /* uint64[n capacity][9][4] */
    uint64_t* aux;                                     /* uint64[n][12][4], aux kind 5, input order */
} zk_sig_wire;
int zk_sig_assign_open(const zk_sig_inputs* in, const zk_sig_wire* out_dev, uint32_t opts, zk_session** out);
int zk_sig_assign_read(zk_session* s, const zk_sig_wire* host, uint64_t* n_keccak_out, uint64_t* n_sig_rows_out);
int zk_sig_assign(const zk_sig_inputs* in, const zk_sig_wire* out, uint32_t opts, uint32_t* status_out,
                  uint64_t* n_keccak_out, uint64_t* n_sig_rows_out, zk_result* result);

/* ---- Bytecode table and Bytecode-circuit witness from raw contract code: replaces Bytecode(code).table_assignments()
 *      (src/zkevm_specs/evm_circuit/typing.py:317-324 init_is_code, :387-427) for a set of contracts, then assign_bytecode_circuit
 *      (src/zkevm_specs/bytecode_circuit.py:104-167) over those rows and assign_keccak_table (:182-186) over the same codes — from the
 *      contracts' BYTES (1 byte per byte of code in, where zk_bytecode_assign takes the 192-byte unrolled row).
 *      Inputs (zk_code_set): the codes back to back with their byte offsets; k (0: no circuit rows); randomness: one cell.
 *      Outputs (zk_code_wire), T = n_bytes + n_codes table rows:
 *        table uint64[T][6][4] row-major (hash lo, hi, tag, index, is_code, value): per code in input order a Header row
 *          (hash, 1, 0, 0, len) and a Byte row (hash, 2, i, is_code_i, byte_i) per byte — zk_evm_tables.bytecode, and zk_bytecode_assign's
 *          in_rows.  hash = keccak-256 of the code as Word lo / hi.  is_code as init_is_code: the push-data counter starts at 0 per
 *          code, PUSH1..PUSH32 set it to 1..32, every other byte (0x5f included) to 0.  Duplicate codes are not removed.
 *        rows uint64[12][2^k][4] column-major (k > 0): cell for cell zk_bytecode_assign's output for (table, row offsets, lengths, k,
 *          randomness), truncation at 2^k rows and EMPTY_HASH padding included; n_codes == 0: padding only.
 *        keccak uint64[n_codes][5][4]: zk_keccak_table's rows of the codes (mode 0, KeccakCircuit.add), input order.
 *      zk_bytecode_from_code_open: with ZK_OPT_DEVICE_PTRS every input is a device pointer and the non-null pointers of `out_dev`
 *      receive the outputs in place (null: the session owns that buffer); without the flag out_dev must be NULL.  The offsets are read
 *      at open and fixed for the session; the code bytes are read by every pass.  zk_launch / zk_collect / zk_close as for the other
 *      assignments: the assignment has no failing case (the tally is always clean; rows_evaluated = T, status uint32[T] all 0).
 *      zk_bytecode_from_code_read copies the last pass's outputs to the non-null HOST pointers of `host`.
 *      Errors (never a guess): offsets that decrease, offsets[0] != 0, offsets[n_codes] != n_bytes, n_bytes + n_codes >= 2^31,
 *      k > 28, `rows` asked for with k == 0. */
typedef struct zk_code_set {
    const uint8_t* code;  uint64_t n_bytes;   /* the contracts' bytes back to back */
    const uint64_t* offsets;                  /* uint64[n_codes + 1]: offsets[0] = 0, non-decreasing, offsets[n_codes] = n_bytes */
    uint64_t n_codes;
    uint32_t k;  uint32_t reserved;           /* Bytecode circuit of 2^k rows (1..28); 0 = no circuit rows */
    const uint64_t* randomness;               /* one cell: keccak_randomness */
} zk_code_set;
typedef struct zk_code_wire {                 /* each pointer nullable */
    uint64_t* table;   /* uint64[n_bytes + n_codes][6][4] row-major */
    uint64_t* rows;    /* uint64[12][2^k][4] column-major: what zk_bytecode_open takes (k > 0 only) */
    uint64_t* keccak;  /* uint64[n_codes][5][4] */
} zk_code_wire;
int zk_bytecode_from_code_open(const zk_code_set* in, const zk_code_wire* out_dev, uint32_t opts, zk_session** out);
int zk_bytecode_from_code_read(zk_session* s, const zk_code_wire* host);
int zk_bytecode_from_code(const zk_code_set* in, const zk_code_wire* out, uint32_t opts, zk_result* result);

/* ---- EVM circuit tx, block and withdrawal tables from raw block data: replaces Transaction.table_assignments(),
 *      Block.table_assignments() and Withdrawal.table_assignments() (src/zkevm_specs/evm_circuit/typing.py:209-281, 116-137, 306-314)
 *      over a block's objects, followed by flatten_tx_table / flatten_block_table / flatten_withdrawal_table and the upload of the
 *      result (one 160-byte row + a flag per byte of calldata; the calldata itself is 1 byte).
 *      Inputs (zk_block_data), 256-bit words as 4 x u64 little-endian:
 *        tx_fields uint64[n_txs][9][4]: id, nonce, gas, gas_price, caller_address, callee_address (0 when None), value, invalid_tx,
 *          tx_sign_hash (the reference's mock 1234, typing.py:265, is data here); to_is_none uint32[n_txs] (non-zero: IsCreate = 1);
 *        access_list uint32[n_txs][2]: access tuples a, storage keys over all of them k -> AccessListGasCost = 2400 a + 1900 k;
 *        calldata: the txs' data back to back, at any byte alignment, with byte offsets uint64[n_txs + 1] (offsets[0] = 0,
 *          non-decreasing; offsets[n_txs] bytes are read), as zk_tx_inputs;
 *        block uint64[8][4], nullable (NULL: no block table; n_history must be 0 then): coinbase, gas_limit, number, timestamp,
 *          prev_randao, base_fee, chainid, withdrawal_root; history_hashes uint64[n_history][4], oldest first (the reference's list,
 *          [-1] the latest); withdrawals uint64[n_withdrawals][4][4]: id, validator_id, address, amount.
 *      Outputs (zk_block_tables), cell for cell and flag for flag what the flatten_* functions return for the same objects — the rows
 *      in the set's order (ascending over the cells as integers), is_word in bit 0 of the flag:
 *        tx uint64[12 n_txs + offsets[n_txs]][5][4] (tx_id, tag, index, value lo, hi) + tx_flags uint32[..]: per tx in id order the rows of
 *          tags 1..12 (Nonce, Gas, GasPrice, CallerAddress, CalleeAddress, IsCreate, Value, CallDataLength, CallDataGasCost, TxInvalid,
 *          AccessListGasCost, TxSignHash), then a CallData row (tag 13) per byte in index order.  GasPrice, CallerAddress, CalleeAddress
 *          and Value are Words (flag 1, lo / hi split at 128 bits); every other value is FQ(v): the 256-bit input reduced mod the BN254
 *          scalar modulus p, hi = 0, flag 0.  CallDataGasCost = 4 per zero byte + 16 per non-zero byte;
 *        block uint64[8 + n_history][4][4] (tag, number, value lo, hi) + block_flags uint32[..]: tags 1..7, then the HistoryHash rows
 *          (tag 8) in ascending order of their number cell FQ(number - n_history + j) for history_hashes[j], then WithdrawalRoot (tag 9).
 *          Coinbase, PrevRandao, BaseFee and HistoryHash are Words, the rest values reduced mod p;
 *        withdrawals uint64[n_withdrawals][4][4]: the four cells reduced mod p, in id order (zk_evm_tables.withdrawals).
 *      zk_evm_tables_from_block_sizes: the three row counts.  zk_evm_tables_from_block_open: with ZK_OPT_DEVICE_PTRS every input is a
 *      device pointer and the non-null pointers of `out_dev` receive the outputs in place (null: the session owns that buffer);
 *      without the flag out_dev must be NULL.  What is checked at open — the tx and withdrawal ids, the offsets, the block number — is
 *      read back once when device-resident and fixed for the session (the session keeps its own copy); the other fields and the
 *      calldata bytes are read by every pass.  zk_launch / zk_collect / zk_close as for the other assignments: there is no failing
 *      case (the tally is always clean; rows_evaluated = the tx table's rows, status uint32[that] all 0).
 *      zk_evm_tables_from_block_read copies the last pass's outputs to the non-null HOST pointers of `host`.
 *      Domain, rejected at sizes / open with an error code and its text in zk_last_error, never guessed:
 *        ZK_ERR_BTB_ID       a tx or withdrawal id is no canonical cell (>= p), or the ids are not strictly ascending (with distinct
 *                            ascending ids the reference's sets have no duplicate rows and their order is closed-form);
 *        ZK_ERR_BTB_OFFSETS  offsets[0] != 0, or offsets that decrease;
 *        ZK_ERR_BTB_HISTORY  n_history > min(256, number) (the reference's assert, typing.py:104);
 *        ZK_ERR_BTB_ROWS     2^31 rows or more in one table. */
#define ZK_ERR_BTB_ID (-60)
#define ZK_ERR_BTB_OFFSETS (-61)
#define ZK_ERR_BTB_HISTORY (-62)
#define ZK_ERR_BTB_ROWS (-63)
typedef struct zk_block_data {
    const uint64_t* tx_fields;   const uint32_t* to_is_none;  const uint32_t* access_list;  uint64_t n_txs;
    const uint8_t* calldata;     const uint64_t* calldata_offsets;   /* uint64[n_txs + 1] */
    const uint64_t* block;                                            /* uint64[8][4], nullable */
    const uint64_t* history_hashes;  uint64_t n_history;             /* oldest first */
    const uint64_t* withdrawals;     uint64_t n_withdrawals;
} zk_block_data;
typedef struct zk_block_tables {               /* each pointer nullable */
    uint64_t* tx;           uint32_t* tx_flags;     /* uint64[12 n_txs + calldata bytes][5][4], uint32[..] */
    uint64_t* block;        uint32_t* block_flags;  /* uint64[8 + n_history][4][4], uint32[..] (no rows when zk_block_data.block is NULL) */
    uint64_t* withdrawals;                          /* uint64[n_withdrawals][4][4] */
} zk_block_tables;
int zk_evm_tables_from_block_sizes(const zk_block_data* in, uint32_t opts, uint64_t* n_tx_rows, uint64_t* n_block_rows, uint64_t* n_withdrawal_rows);
int zk_evm_tables_from_block_open(const zk_block_data* in, const zk_block_tables* out_dev, uint32_t opts, zk_session** out);
int zk_evm_tables_from_block_read(zk_session* s, const zk_block_tables* host);
int zk_evm_tables_from_block(const zk_block_data* in, const zk_block_tables* out, uint32_t opts, zk_result* result);

/* ---- EVM circuit witness from compact trace records: replaces flatten_rw_table / flatten_steps over RWTableRow / StepState objects
 *      (src/zkevm_specs/evm_circuit/table.py:447-457, step.py:6-75) and the upload of their result: 14 cells x 32 B + a flag per RW row,
 *      13 x 32 B per step.  A producer of traces holds these values in their natural widths; the records below carry them so.
 *      Inputs (zk_trace), integers little-endian, a "pool word" 256 bits as 4 x u64:
 *        RW ops: head uint32[n_rw], id / addr / val / prev uint64[n_rw]; rw_counter uint64[n_rw], nullable (NULL: the counter of op i is
 *          rw_base + i); pool uint64[n_pool][4].  head: bit 0 is_write, bits 1-4 tag, bits 8-15 field_tag, bit 16 value.is_word, bit 17
 *          value_prev.is_word, bit 20 the address is a pool word, bit 21 storage_key is present, bit 22 value is a pool word, bit 23
 *          value_prev is a pool word, bit 24 aux0 is present; every other bit must be zero.  An op consumes its pool words in the order
 *          address, key, value, prev, aux, and the ops consume the pool in their order: the offsets are computed, not passed.
 *        steps uint64[n_steps][13]: w0 = execution_state (bits 0-7) | is_root << 8 | is_create << 9 (other bits zero); w1..w8 rw_counter,
 *          call_id, program_counter, stack_pointer, gas_left, memory_word_size, reversible_write_counter, log_id; w9..w12 the code hash.
 *      Outputs (zk_trace_witness): rw uint64[n_rw][14][4], rw_flags uint32[n_rw], steps uint64[n_steps][13][4] - the arrays zk_evm_tables
 *      takes, cell for cell and flag for flag what flatten_rw_table / flatten_steps return for the same rows:
 *        rw_counter, is_write, tag, id, field_tag and every step integer are FQ(u64); address FQ(addr), a pool word reduced mod the BN254
 *        scalar modulus p; storage_key and aux0 Word(w) split at 128 bits, absent Word(0); value / value_prev: narrow (v, 0) with either
 *        flag, wide with the is_word bit (w mod 2^128, w >> 128), wide without it (w mod p, 0); the flag word is head bits 16-17; the
 *        step cells in flatten_steps' order, the code hash as a Word.
 *      zk_evm_witness_from_trace_sizes: the checks below, and the row counts.  zk_evm_witness_from_trace_open: with ZK_OPT_DEVICE_PTRS
 *      every input is a device pointer and the non-null pointers of `out_dev` receive the outputs in place (null: the session owns that
 *      buffer); without the flag out_dev must be NULL.  The checks run on the device at open and one verdict block of 32 bytes is read
 *      back, not the arrays.  The session keeps its own copy of the heads, of the counters and of the per-row pool offsets: a caller that
 *      rewrites a head between passes cannot move a store.  id, addr, val, prev, the pool and the steps are read by every pass (on the
 *      CPU backend from the caller's arrays, which are that backend's resident memory and must outlive the session).
 *      zk_launch / zk_collect / zk_close as for the other assignments: there is no failing case (the tally is always clean;
 *      rows_evaluated = n_rw, status uint32[n_rw] all 0).  zk_evm_witness_from_trace_read copies the last pass's outputs to the non-null
 *      HOST pointers of `host`.
 *      Domain, rejected at sizes / open with an error code and its text in zk_last_error, never guessed:
 *        ZK_ERR_TRC_HEAD   a reserved bit of a head or of a step's w0 is set;
 *        ZK_ERR_TRC_ORDER  the rw_counters are not strictly ascending, or rw_base + n_rw passes 2^64 (strictly ascending counters make
 *                          the set's order the input order and leave no duplicates);
 *        ZK_ERR_TRC_POOL   n_pool differs from the words the heads consume;
 *        ZK_ERR_TRC_ROWS   2^31 rows or more. */
#define ZK_ERR_TRC_HEAD (-70)
#define ZK_ERR_TRC_ORDER (-71)
#define ZK_ERR_TRC_POOL (-72)
#define ZK_ERR_TRC_ROWS (-73)
typedef struct zk_trace {
    const uint32_t* head;  const uint64_t* id;  const uint64_t* addr;  const uint64_t* val;  const uint64_t* prev;  /* [n_rw] each */
    const uint64_t* rw_counter;  uint64_t rw_base;   /* uint64[n_rw], nullable: rw_base + i */
    uint64_t n_rw;
    const uint64_t* pool;  uint64_t n_pool;          /* uint64[n_pool][4] */
    const uint64_t* steps; uint64_t n_steps;         /* uint64[n_steps][13] */
} zk_trace;
typedef struct zk_trace_witness {                    /* each pointer nullable */
    uint64_t* rw;  uint32_t* rw_flags;               /* uint64[n_rw][14][4], uint32[n_rw] */
    uint64_t* steps;                                 /* uint64[n_steps][13][4] */
} zk_trace_witness;
int zk_evm_witness_from_trace_sizes(const zk_trace* in, uint32_t opts, uint64_t* n_rw_rows, uint64_t* n_step_rows);
int zk_evm_witness_from_trace_open(const zk_trace* in, const zk_trace_witness* out_dev, uint32_t opts, zk_session** out);
int zk_evm_witness_from_trace_read(zk_session* s, const zk_trace_witness* host);
int zk_evm_witness_from_trace(const zk_trace* in, const zk_trace_witness* out, uint32_t opts, zk_result* result);

/* ---- State circuit from the same compact trace records: the State verdict (zk_state_verify_from_trace*) and the State op list
 *      (zk_state_ops_from_trace*) of the RW ops of a zk_trace, without the 448-byte wire rows in between.
 *      DEFINED BY COMPOSITION: for records zk_evm_witness_from_trace accepts, every output - n_ops, the statuses (per op in sorted order
 *      with op 0 the StartOp; per RW row for the ops form), the zk_result, the op list uint64[12][n_ops][4] and its flags - is bit for bit
 *      what the matching _from_rw entry returns over the rw / rw_flags zk_evm_witness_from_trace writes for the same records, and so is a
 *      return of -1 when there is no witness (see zk_state_verify_from_rw_open), with the same text under this entry's name.  The wire's
 *      reductions are part of that: a pool address is FQ(w) (the "wider than 160 bits" check sees the reduced value), a wide value without
 *      its is_word bit (w mod p, 0), with it (w mod 2^128, w >> 128), an absent storage_key or aux0 Word(0); a head whose tag nibble is
 *      not one of Target's values gives the re-keying's (ZK_KIND_VALUE_ERROR << 24) | 1.
 *      Of zk_trace the RW half is read: head, id, addr, val, rw_counter / rw_base, n_rw (> 0), pool, n_pool.  prev is never read and may
 *      be NULL (the State circuit has no value_prev; its pool words still count in the offsets); steps / n_steps are ignored.
 *      The records' domain is checked at open exactly as zk_evm_witness_from_trace_open checks it: ZK_ERR_TRC_HEAD / _ORDER / _POOL /
 *      _ROWS with the same text under this entry's name, on the device, one verdict block read back; the counts that need no array are
 *      checked before any array is read.
 *      ZK_OPT_DEVICE_PTRS, zk_launch, zk_collect, zk_read_status, zk_close, zk_session_set_stream: as for the _from_rw entries
 *      (ops_dev / op_flags_dev: capacity n_rw + 1 ops).  Resident passes of the verdict session keep what the first collected pass built:
 *      the ops in State order as one 48-byte record each, the first-access links, the MPT rows and the root ranks; later passes stream
 *      those records and evaluate.  The session keeps its own copy of the heads, counters and pool offsets.  id, addr, val and the pool
 *      stay the caller's: with ZK_OPT_DEVICE_PTRS they must stay valid and unchanged for the session's life (the first pass reads id /
 *      addr / val, every pass reads the pool words of wide cells); host arrays are copied at open. */
int zk_state_verify_from_trace_open(const zk_trace* in, uint32_t opts, uint64_t* n_ops_out, zk_session** out);
int zk_state_verify_from_trace(const zk_trace* in, uint32_t opts, uint32_t* status_out /* n_ops <= n_rw + 1 */, uint64_t* n_ops_out,
                               zk_result* result);
int zk_state_ops_from_trace_open(const zk_trace* in, uint64_t* ops_dev, uint32_t* op_flags_dev, uint32_t opts, uint64_t* n_ops_out,
                                 zk_session** out);
int zk_state_ops_from_trace_read(zk_session* s, uint64_t* ops_host, uint32_t* op_flags_host, uint64_t* n_ops_out);
int zk_state_ops_from_trace(const zk_trace* in, uint64_t* ops_out, uint32_t* op_flags_out, uint64_t* n_ops_out, uint32_t opts,
                            uint32_t* status_out /* n_rw */, zk_result* result);
/* The State WITNESS of the same records (zk_state_assign_from_trace*): the third member of the family, the twin of
 * zk_state_assign_from_rw_open.  By the same composition rule every output - n_ops, the rows uint64[57][n_ops][4] (uint64[15][n_ops][4]
 * with ZK_OPT_STATE_COMPACT), row_flags uint32[n_ops], the MPT rows uint64[n_mpt][12][4] in first-occurrence order and n_mpt, the status
 * per OP and the zk_result - is bit for bit what zk_state_assign_from_rw_open returns over the rw / rw_flags zk_evm_witness_from_trace
 * writes for the same records; rejected RW rows count in the same tally, first_fail_row then being the RW row.  Inputs read, domain
 * errors (under this entry's name) and resident data as for the two entries above.  With ZK_OPT_DEVICE_PTRS rows_dev / row_flags_dev /
 * mpt_dev (each nullable: the session then owns the buffer) have capacity n_rw + 1 rows, are packed for n_ops and receive the outputs in
 * place.  zk_launch / zk_collect / zk_read_status / zk_state_assign_read / zk_session_set_stream / zk_close as on a
 * zk_state_assign_from_rw_open session.  Every zk_launch runs the whole chain (re-keying, sort, op stream, MPT passes, row writer), as
 * the from-RW twin does: nothing is carried from one pass to the next, so a second pass gives the same outputs whatever the first saw.
 * The one-shot writes HOST buffers of capacity n_rw + 1 rows (mpt_out: n_rw + 1 rows), or with ZK_OPT_DEVICE_PTRS the device buffers. */
int zk_state_assign_from_trace_open(const zk_trace* in, uint64_t* rows_dev, uint32_t* row_flags_dev, uint64_t* mpt_dev,
                                    uint32_t opts, uint64_t* n_ops_out, zk_session** out);
int zk_state_assign_from_trace(const zk_trace* in, uint64_t* rows_out, uint32_t* row_flags_out, uint64_t* mpt_out,
                               uint64_t* n_mpt_out, uint64_t* n_ops_out, uint32_t opts, uint32_t* status_out, zk_result* result);

/* ---- ECC precompile calls: from the INPUT words of ecAdd / ecMul / ecPairing calls to what both circuits derive from them.  Where
 *      zk_ecc_ops takes every op's result from the caller (points[..][4..5], pair_out) and zk_ecc_assign copies it into rows, this
 *      entry computes the result on the device: the ECC circuit's ops and rows (circuit2rows, src/zkevm_specs/ecc_circuit.py:386-421),
 *      and the EVM circuit's ecc table and aux rows of kinds 6 / 7 / 8, which the reference's tests build with py_ecc
 *      (tests/evm/precompiles/test_ecAdd.py:80-101, test_ecMul.py, test_ecPairing.py:180-222).
 *      Inputs (zk_ecc_calls), 256-bit words as 4 x u64 little-endian, NOT reduced, each the integer of one 32-byte word of the
 *      precompile's input; order and layout of the pairing arrays are zk_ecc_ops', so those can be reused:
 *        add_in uint64[n_add][4][4]: p.x, p.y, q.x, q.y;   mul_in uint64[n_mul][3][4]: p.x, p.y, s;
 *        pair_pts uint64[pair_off[n_pairing]][6][4] in EIP-197 order (p.x, p.y, x.c1, x.c0, y.c1, y.c0), pair_off uint32[n_pairing + 1]
 *        (pair_off[0] = 0, non-decreasing; an op may have no pair); randomness: one cell (keccak_randomness).
 *        A pairing call whose byte length is no multiple of 192 cannot be expressed in pairs and stays the caller's to handle (its
 *        aux row is (rlc, pairs, 0, 0)).  The reference disagrees with itself there: its EVM test takes the RLC over ALL the bytes
 *        (test_ecPairing.py:180-200) while assign_pairing takes it over whole pairs (ecc_circuit.py:204-227).
 *      Semantics, n = n_add + n_mul + n_pairing calls in circuit2rows order (adds, muls, pairings):
 *        is_valid is what EccCircuitRow.assign_add / assign_mul / assign_pairing compute (ecc_circuit.py:49-232): every coordinate below
 *        the base modulus p, (0, 0) the point at infinity, the point on the curve (G2: on the twist), and for pairings both subgroup
 *        checks ([r]P, [r]Q at infinity).  A valid call's result is the precompile's (EIP-196 / EIP-197): p + q; [s]P with s the full
 *        256-bit integer, infinity as (0, 0); 1 or 0 for the pairing product, 1 for the empty input.  An invalid call's result is zero
 *        with is_valid 0, what ecadd.py:29-35 and ecpairing.py:34-61 require of a failed call.  input_rlc is assign_pairing's
 *        (ecc_circuit.py:204-227: the words p.x, p.y, x.c0, x.c1, y.c0, y.c1 of every pair as 32 little-endian bytes, reversed); 0 for
 *        add / mul.  (The reference's EVM test orders the G2 words as the input does, x.c1 first, test_ecPairing.py:181-190: the same
 *        bytes in another order.  Table and aux row come from one value here, so the lookup of ecpairing.py:51-61 holds either way.)
 *        Quirk, pinned: ECCVerifyChip takes ecMul's scalar as FP(s) (util/ec.py:120-166, ecc_circuit.py:125-129), i.e. s mod p, while the
 *        group's order is r and the row carries Word(s).  For s >= p the ECC circuit (zk_ecc_verify / zk_ecc_open) therefore REJECTS the
 *        row of the correct EVM result this entry returns: already at the scalar's own copy constraint (ECC_COPY_QX: the chip holds s mod
 *        p, the row s), and its product [s mod p]P would differ from [s]P as well.  The entry returns the EVM result.  Likewise a
 *        coordinate >= p fails its copy constraint there, and an invalid pairing call has no satisfying row (verify_pairing insists on
 *        the subgroup checks): such calls are well-defined EVM-side (is_valid 0, zero result) and rejected by the ECC circuit.
 *      Outputs (zk_ecc_call_wire), every member nullable:
 *        points uint64[n_add + n_mul][6][4], pair_out uint64[n_pairing][4]: with the caller's pair_pts / pair_off a complete zk_ecc_ops;
 *        rows uint64[n][13][4]: circuit2rows' rows, what zk_ecc_open takes (out_x / out_y: the residue mod p, as zk_ecc_assign writes it);
 *        ecc_table uint64[n capacity][13][4]: every call's row with out_x / out_y as FQ cells (the residue reduced mod the scalar
 *          modulus) — the first occurrence of every distinct row, in input order (the EVM tables are sets: sig_table's rule); the row
 *          count comes out of zk_ecc_from_calls_read / zk_ecc_from_calls (zk_evm_tables.ecc / n_ecc);
 *        aux uint64[n][12][4] + aux_kind uint32[n], row i for call i in zk_evm_tables.aux's layout: kind 6 px, py, qx, qy as lo / hi then
 *          outx, outy; kind 7 px, py, s as lo / hi then outx, outy; kind 8 input_rlc, input_pairs, is_valid_input, output; unused cells 0.
 *      Session protocol as zk_sig_assign_*: with ZK_OPT_DEVICE_PTRS the inputs are device pointers and the non-null members of out_dev
 *      are written in place (null, or a null out_dev: the session owns that buffer); without it out_dev must be NULL.  zk_launch
 *      (status_dev: uint32[n], always 0 — an invalid call has defined outputs, there is no failing case) / zk_collect / zk_read_status /
 *      zk_close.  The open reads back pair_off and the randomness cell only (pair_off is fixed for the session: it keeps its own copy);
 *      points are never read back, and the call words are read by every pass (on the CPU backend from the caller's arrays, which are
 *      that backend's resident memory and must outlive the session).  A pass is the add / mul
 *      launch (one lane per call), pairing stage 1 (one lane per pair: zk_ecc_open's record), pairing stage 2 (one lane per call) and
 *      the table's two launches; every output is final in stream order.  zk_ecc_from_calls_read copies the last pass's outputs to the
 *      non-null HOST pointers of `host` (nullable) and the table's row count out (nullable).
 *      Domain, rejected at open with an error code and its text in zk_last_error, never guessed:
 *        ZK_ERR_ECL_OFFSETS     pair_off[0] != 0, or offsets that decrease;
 *        ZK_ERR_ECL_ROWS        2^31 calls or pairs, or more;
 *        ZK_ERR_ECL_RANDOMNESS  the randomness cell is not canonical. */
#define ZK_ERR_ECL_OFFSETS (-80)
#define ZK_ERR_ECL_ROWS (-81)
#define ZK_ERR_ECL_RANDOMNESS (-82)
typedef struct zk_ecc_calls {
    const uint64_t* add_in;     uint64_t n_add;      /* uint64[n_add][4][4] */
    const uint64_t* mul_in;     uint64_t n_mul;      /* uint64[n_mul][3][4] */
    const uint64_t* pair_pts;   const uint32_t* pair_off;   uint64_t n_pairing;
    const uint64_t* randomness;                      /* one cell: keccak_randomness */
} zk_ecc_calls;
typedef struct zk_ecc_call_wire {                    /* each pointer nullable */
    uint64_t* points;    uint64_t* pair_out;         /* uint64[n_add + n_mul][6][4], uint64[n_pairing][4] */
    uint64_t* rows;                                  /* uint64[n][13][4] */
    uint64_t* ecc_table;                             /* uint64[n capacity][13][4] */
    uint64_t* aux;       uint32_t* aux_kind;         /* uint64[n][12][4], uint32[n] */
} zk_ecc_call_wire;
int zk_ecc_from_calls_open(const zk_ecc_calls* in, const zk_ecc_call_wire* out_dev, uint32_t opts, zk_session** out);
int zk_ecc_from_calls_read(zk_session* s, const zk_ecc_call_wire* host, uint64_t* n_table_rows_out);
int zk_ecc_from_calls(const zk_ecc_calls* in, const zk_ecc_call_wire* out, uint32_t opts, uint32_t* status_out,
                      uint64_t* n_table_rows_out, zk_result* result);

/* ---- Copy-circuit witness from raw code, calldata and trace records: zk_copy_assign without its `data` array.  zk_copy_assign takes
 *      every source byte of every copy event as value | is_code << 8, collected by a host loop per byte (and, for Bytecode copies, a host
 *      is_code scan of the contract).  Those bytes are already on the device in the same block: a Bytecode source is a slice of the code
 *      set zk_bytecode_from_code takes, a TxCalldata source a slice of the calldata zk_evm_tables_from_block / zk_tx_assign take, a
 *      Memory source the values of the Memory read ops of the zk_trace records — the ops CopyCircuit.copy appends to the RW table
 *      (typing.py:1122-1131).  This entry gathers `data` there and runs the Copy assignment over it.  What it removes is a host pass and a
 *      second copy of data the device holds; it is not a bandwidth saving (the upload it drops is 2 bytes per source byte).
 *      DEFINED BY COMPOSITION: for inputs it accepts, every output of zk_copy_assign - rows, row_flags, table, rw, rw_flags, the counts - is
 *      bit for bit what zk_copy_assign returns for the same events with the `data` / `data_offsets` defined below.  The new outputs are
 *      the gathered data uint16[n_data], data_offsets uint64[n_events + 1] and a status per EVENT.
 *      Inputs (zk_copy_sources):
 *        events, flags, n_events, randomness: exactly zk_copy_events', with the same domain checks; RlcAcc, like TxLog, is no source;
 *        src_ref uint32[n_events]: for a Bytecode source the index of the code in the code set, for a TxCalldata source the index of the
 *          tx in calldata_offsets; ignored otherwise.  dst_ref uint32[n_events]: for a Bytecode destination the index of the written
 *          code; NULL when no event has one.  The refs are read at open, for every event of their kind (whatever its length);
 *        code, n_code_bytes, code_offsets, n_codes: as zk_code_set; calldata, calldata_offsets, n_txs: as zk_block_data, at any byte
 *          alignment; trace: a zk_trace of which head, id, addr, val, rw_counter / rw_base and n_rw (which may be 0) are read - pool,
 *          prev and steps never are and may be NULL.
 *        The events' id cells (code hash, call id, tx id) are NOT matched against the sources: the refs say where the bytes are, and the
 *        Copy circuit's own bytecode / tx / RW lookups remain the check of the ids.
 *      Gathered data: per event n_real = min(length, max(src_addr_end - src_addr, 0)) bytes; data_offsets is the running sum (host
 *      arithmetic over the event cells).  Byte i < n_real of an event:
 *        Bytecode source: byte src_addr + i of code src_ref;  TxCalldata source: byte src_addr + i of the calldata of tx src_ref;
 *        Memory source: val of the trace op whose rw_counter is event.rw_counter + i * stride, stride 2 when the destination is Memory or
 *          TxLog (a write op follows each read), else 1 (padded reads are a suffix and consume no counter).  With rw_counter NULL the op's
 *          index is counter - rw_base, else it is found by binary search.  The op must be a Memory read: head bit 0 clear, tag nibble
 *          Target.Memory (9), no address pool bit, id == the event's src_id lo with src_id hi zero, addr == src_addr + i;
 *        is_code: 0 when neither side is Bytecode, else init_is_code (as zk_bytecode_from_code: PUSH1..PUSH32 open 1..32 data bytes, 0x5f
 *          none, the counter restarts per code) of the Bytecode side's code - the source's when both sides are - at position
 *          src_addr + i, or dst_addr + i when that code is the destination.  Every pass scans the code set for it (64-byte chunks, a
 *          wavefront each; no code is walked serially by one lane).
 *      Status per event (zk_launch: status_dev uint32[n_events]; the zk_result's tally runs over events, rows_evaluated = n_events):
 *      0, or (ZK_KIND_VALUE_ERROR << 24) | site, never a guess:
 *        1  a ref that is read is out of range;     2  src_addr_end lies beyond the source code / calldata (only when n_real > 0);
 *        3  dst_addr + n_real lies beyond the destination code;
 *        4  no trace op has the counter a read needs;     5  the op at that counter is not the Memory read described above;
 *        6  the op's value is no byte (256 or more, or the head marks it as a pool word).
 *      Sites 1-3 are per event, 4-6 per byte: an event's status is its lowest per-event site, else the site of its failing byte with the
 *      lowest i.  A failing byte is gathered as 0 (is_code 0) and the event's other bytes normally; every byte of an event with site
 *      1-3 is 0.  The rows are zk_copy_assign's over the data as gathered, failing inputs included.
 *      zk_copy_assign_from_sources_sizes: the checks below and the counts.  _open: with ZK_OPT_DEVICE_PTRS every input is a device pointer
 *      and rows_dev / row_flags_dev / table_dev / rw_dev / rw_flags_dev / data_dev uint16[n_data] receive the outputs in place (each
 *      nullable: the session then owns that buffer); without the flag they must be NULL.  The events' integer cells, the refs, the
 *      offsets and the trace's heads and counters are read at open and kept by the session (nothing a caller rewrites later can move a
 *      load or a store); code, calldata, id / addr / val and the events' id cells stay the caller's and are read by every pass.  Every
 *      zk_launch runs the whole chain (is_code scan, gather, Copy assignment): nothing is carried from one pass to the next.  zk_launch /
 *      zk_collect / zk_read_status / zk_session_set_stream / zk_close as on a zk_copy_assign_open session; _read copies what
 *      zk_copy_assign_read copies, plus data_host and data_offsets_host (always a HOST array).  The one-shot's status_out is a device
 *      pointer with ZK_OPT_DEVICE_PTRS, like its other outputs.
 *      Domain, rejected at sizes / open with an error code and its text in zk_last_error:
 *        ZK_ERR_CPS_OFFSETS  code or calldata offsets that do not start at 0 or that decrease, code_offsets[n_codes] != n_code_bytes;
 *        ZK_ERR_CPS_ROWS     2^31 or more source bytes (or code bytes, codes, txs);
 *        ZK_ERR_TRC_HEAD / _ORDER / _ROWS as zk_evm_witness_from_trace_open reports them, on the device with one verdict block read
 *        back (_POOL is not checked: the pool is not read); the event-field errors of zk_copy_assign, with their texts - all under this
 *        entry's name. */
#define ZK_ERR_CPS_OFFSETS (-90)
#define ZK_ERR_CPS_ROWS (-91)
typedef struct zk_copy_sources {
    const uint64_t* events;     const uint32_t* flags;       uint64_t n_events;
    const uint32_t* src_ref;    const uint32_t* dst_ref;     /* uint32[n_events]; dst_ref nullable */
    const uint64_t* randomness;
    const uint8_t* code;        uint64_t n_code_bytes;       const uint64_t* code_offsets;  uint64_t n_codes;
    const uint8_t* calldata;    const uint64_t* calldata_offsets;   uint64_t n_txs;   /* offsets uint64[n_txs + 1] */
    zk_trace trace;
} zk_copy_sources;
int zk_copy_assign_from_sources_sizes(const zk_copy_sources* in, uint32_t opts, uint64_t* n_rows, uint64_t* n_table, uint64_t* n_rw,
                                      uint64_t* n_data);
int zk_copy_assign_from_sources_open(const zk_copy_sources* in, uint64_t* rows_dev, uint32_t* row_flags_dev, uint64_t* table_dev,
                                     uint64_t* rw_dev, uint32_t* rw_flags_dev, uint16_t* data_dev, uint32_t opts, zk_session** out);
int zk_copy_assign_from_sources_read(zk_session* s, uint64_t* rows_host, uint32_t* row_flags_host, uint64_t* table_host,
                                     uint64_t* rw_host, uint32_t* rw_flags_host, uint16_t* data_host, uint64_t* data_offsets_host);
int zk_copy_assign_from_sources(const zk_copy_sources* in, uint64_t* rows_out, uint32_t* row_flags_out, uint64_t* table_out,
                                uint64_t* rw_out, uint32_t* rw_flags_out, uint16_t* data_out, uint64_t* data_offsets_out,
                                uint32_t opts, uint32_t* status_out, zk_result* result);

/* ---- Copy and EXP events from compact trace records: the event lists zk_copy_assign_from_sources / zk_copy_assign / zk_exp_assign take,
 *      which a producer of traces so far built in a host loop beside its trace.  Every field of those events is in the trace: they are the
 *      arguments of the copy_lookup / exp_lookup calls of the reference's gadgets (execution/sha3.py:20, calldatacopy.py:41, codecopy.py:
 *      26, extcodecopy.py:39, returndatacopy.py:36, log.py:65, exp.py:31), computed from the step and from the RW ops at fixed offsets
 *      behind step.rw_counter.  With this entry a caller uploads trace records, code and block data, and every table and witness of the
 *      block follows on the device.
 *      Inputs (zk_trace_sources): trace - a zk_trace of which head, id, addr, val, rw_counter / rw_base, n_rw, pool, n_pool, steps and
 *      n_steps are read (prev never is and may be NULL); the code set code, n_code_bytes, code_offsets, n_codes as in zk_copy_sources;
 *      code_hashes uint64[n_codes][4], the 256-bit hash of each code.  The hashes and the offsets are read at open and kept by the
 *      session (a sorted directory); of duplicate hashes the lowest index wins.
 *      Outputs (zk_trace_events), each pointer nullable, each with capacity n_steps: copy_events uint64[n_copy][12][4], copy_flags
 *      uint32[n_copy], copy_src_ref uint32[n_copy] - exactly the events / flags / src_ref zk_copy_sources takes (no derived event
 *      writes a code: dst_ref is never needed); copy_step uint32[n_copy], the step that produced each copy event; exp_events
 *      uint64[n_exp][5][4], zk_exp_events' rows; exp_step uint32[n_exp].  Both lists are packed, in step order.
 *      Derivation.  "Op k" is the op whose counter is step.rw_counter + k (rw_counter NULL: its index is counter - rw_base; else it is
 *      found by binary search).  A stack read j is a read with tag Stack, id == call_id and addr == stack_pointer + j; a CallContext
 *      read is a read with tag CallContext, id == call_id and addr == the field tag (neither address a pool word).  Values are taken as
 *      integers: val, or the pool word when the head says so.  rwc = step.rw_counter; event = (src id, tag -> dst id, tag; src_addr,
 *      src_addr_end, dst_addr, length; log_id; rw_counter):
 *        SHA3            ops 0 offset, 1 size: (call_id Memory -> call_id RlcAcc; offset, offset + size, 0, size; 0; rwc + 3) when size != 0;
 *        CALLDATACOPY    ops 0 mem, 1 data, 2 len, 3 TxId (root) / CallerId, 4 CallDataLength, 5 CallDataOffset (cdo; not read and 0 in a
 *                        root call): (v3 TxCalldata (root) / Memory -> call_id Memory; cdo + data, cdo + CallDataLength, mem, len; 0;
 *                        rwc + 5 (root) / rwc + 6) when len != 0;
 *        CODECOPY        ops 0 mem, 1 code offset, 2 size: (the step's code hash (a Word: flag bit 0) Bytecode -> call_id Memory; code
 *                        offset, the length of that code, mem, size; 0; rwc + 3) when size != 0;
 *        EXTCODECOPY     ops 1 mem, 2 code offset, 3 size, 8 the Account read of CodeHash (a read, tag Account, field_tag CodeHash): (that
 *                        hash (a Word) Bytecode -> call_id Memory; code offset, the code's length (0 for a zero hash), mem, size; 0;
 *                        rwc + 9) when size != 0;
 *        RETURNDATACOPY  ops 0 mem, 2 size, 3 LastCalleeId, 5 LastCalleeReturnDataOffset (rdo): (v3 Memory -> call_id Memory; rdo, rdo +
 *                        size, mem, size; 0; rwc + 6) always, also with size 0 (the reference looks it up unconditionally, and ignores
 *                        the popped data offset);
 *        LOG             ops 0 mstart, 1 msize, 2 TxId, 5 IsPersistent: (call_id Memory -> tx_id TxLog; mstart, mstart + msize, 0, msize;
 *                        step.log_id + 1; rwc + 7 + 2 t, t = code[pc] - 0xA0 in the step's code) when msize != 0 and IsPersistent == 1;
 *        EXP             ops 0 base, 1 exponent: (rwc + 3, base lo, hi, exponent lo, hi) when exponent > 1.
 *      src_ref: a Bytecode source's index in the code set (0 for the zero hash, whose event reads no byte); tx_id - 1 for a TxCalldata
 *      source; else 0.  The code set is consulted only for an event that is emitted.
 *      Status per step (zk_launch: status_dev uint32[n_steps]; the zk_result's tally runs over the steps, rows_evaluated = n_steps): 0,
 *      or (ZK_KIND_VALUE_ERROR << 24) | site, never a guess; a failing step emits nothing:
 *        1  no op has a counter the step reads;     2  the op there is not the one described above (1 and 2 are checked in ascending k,
 *           the first failure wins);
 *        3  an integer of an emitted event is 2^62 or more (the domain of zk_copy_assign): step.rw_counter, the event's rw_counter, a
 *           value that enters an address, a length, a log id or an integer id, or one of the sums; or the tx_id of a TxCalldata
 *           source is 0 or above 2^32 (src_ref could not hold tx_id - 1);
 *        4  the code hash is not in the set, pc lies outside the code, or the byte at pc is not 0xA0..0xA4 (with site 3 and site 4
 *           both, 3 is reported; the LOG event's counter is then tested without its topics).
 *      The states whose gadgets call copy_lookup with arguments this entry does not derive - BeginTx, RETURN, CREATE, CREATE2, CALL_OP and
 *      DATACOPY (begin_tx.py, return_revert.py, create.py, callop.py, dataCopy.py) - get (ZK_KIND_UNSUPPORTED << 24) | 1 and emit
 *      nothing: a caller then knows to supply those events itself (or calls zk_events_from_trace_ext below, which derives BeginTx,
 *      RETURN and DATACOPY too).  They count in fail_count.  Every other state has status 0.
 *      (The keccak lookups are not this entry's: zk_sha3_from_trace below derives the SHA3 steps' keccak rows; CREATE2's keccak lookup
 *      of its init code is derived by neither.)
 *      zk_events_from_trace_sizes: the checks below, and the capacity every output needs (n_steps).  _open: with ZK_OPT_DEVICE_PTRS
 *      every input is a device pointer and the non-null pointers of `out_dev` receive the outputs in place (null: the session owns that
 *      buffer); without the flag out_dev must be NULL.  The session keeps its own copy of the heads, the counters, the pool offsets,
 *      the code offsets and the hash directory; id, addr, val, the pool, the steps and the code bytes stay the caller's and are read
 *      by every pass.  zk_launch (with status_dev) / zk_collect / zk_read_status / zk_session_set_stream / zk_close as on the other
 *      assignment sessions; every launch runs the whole chain (the steps, a scan of the per-block counts, the packed stores): nothing
 *      is carried from one pass to the next.  _counts returns n_copy and n_exp of the last pass; _read copies the outputs to the
 *      non-null HOST pointers of `host` and returns the counts.  The one-shot's status_out is a device pointer with
 *      ZK_OPT_DEVICE_PTRS, like its other outputs.
 *      Domain, rejected at sizes / open with an error code and its text in zk_last_error:
 *        ZK_ERR_TRC_HEAD / _ORDER / _POOL / _ROWS exactly as zk_evm_witness_from_trace_open reports them (on the device, with one
 *        verdict block read back), under this entry's name;
 *        ZK_ERR_TEV_OFFSETS  code offsets that do not start at 0, that decrease, or whose last value differs from n_code_bytes;
 *        ZK_ERR_TEV_ROWS     2^31 or more steps, code bytes or codes. */
#define ZK_ERR_TEV_OFFSETS (-100)
#define ZK_ERR_TEV_ROWS (-101)
typedef struct zk_trace_sources {
    zk_trace trace;
    const uint8_t* code;        uint64_t n_code_bytes;       const uint64_t* code_offsets;  uint64_t n_codes;
    const uint64_t* code_hashes;                             /* uint64[n_codes][4] */
} zk_trace_sources;
typedef struct zk_trace_events {                             /* each pointer nullable; capacity n_steps each */
    uint64_t* copy_events;      uint32_t* copy_flags;        uint32_t* copy_src_ref;        uint32_t* copy_step;
    uint64_t* exp_events;       uint32_t* exp_step;
} zk_trace_events;
int zk_events_from_trace_sizes(const zk_trace_sources* in, uint32_t opts, uint64_t* capacity);
int zk_events_from_trace_open(const zk_trace_sources* in, const zk_trace_events* out_dev, uint32_t opts, zk_session** out);
int zk_events_from_trace_read(zk_session* s, const zk_trace_events* host, uint64_t* n_copy, uint64_t* n_exp);
int zk_events_from_trace_counts(zk_session* s, uint64_t* n_copy, uint64_t* n_exp);
int zk_events_from_trace(const zk_trace_sources* in, const zk_trace_events* out, uint32_t opts, uint32_t* status_out, uint64_t* n_copy,
                         uint64_t* n_exp, zk_result* result);

/* ---- The same, with the copy events of BeginTx, RETURN / REVERT and DATACOPY (begin_tx.py:147-177, return_revert.py:54-93, dataCopy.py:
 *      38-61): the states of which every block has one per tx and one per call, and whose events may WRITE a code (a deployment, a create
 *      tx's init code), which zk_trace_events cannot say.  zk_events_from_trace* above is unchanged; this family stands beside it.
 *      Inputs: zk_trace_sources, exactly as above.
 *      Outputs (zk_trace_events_ext), each pointer nullable: copy_events, copy_flags, copy_src_ref, copy_step, exp_events, exp_step as
 *      above, and copy_dst_ref uint32[n_copy]: for an event with a Bytecode destination the index in the code set of the code it writes
 *      (the dst_ref zk_copy_sources takes), else 0.  Both lists are packed, in step order; the events of one step are in the order its
 *      gadget calls copy_lookup.  Capacities (zk_events_from_trace_ext_sizes returns both): the exp_* outputs n_steps; the copy_* outputs
 *      n_steps + the number of steps whose state is BeginTx or DATACOPY (the two states that may emit two events), counted at sizes /
 *      open where the steps' word 0 is read anyway.
 *      Derivation.  Every state zk_events_from_trace derives has the same event, status and refs here (one per-step function serves
 *      both), with copy_dst_ref 0.  CREATE, CREATE2 and CALL_OP keep (ZK_KIND_UNSUPPORTED << 24) | 1: no reference-recorded case reaches
 *      their copy_lookup (CALL_OP's lengths are aux_data, which a step record does not carry).  Terms as above: rwc, "op k", values
 *      taken as integers; a stack read at position j is a read with tag Stack, id == call_id, addr == stack_pointer + j (here j is not
 *      k); `next` is step record i + 1; is_create is bit 9 and is_root bit 8 of a record's word 0.
 *        RETURN (RETURN and REVERT)  op 1 off (stack position 0), op 2 len (position 1); op 0 (IsSuccess) is not read: the reference's
 *                        `if curr.is_create and is_success` tests an FQ object, so the branch is is_create alone.
 *                        is_create:  op 4 the Account WRITE of CodeHash (a write, tag Account, field_tag CodeHash), value the word h:
 *                          (call_id Memory -> h (a Word: flag bit 1) Bytecode; off, off + len, 0, len; 0; rwc + 5) when len != 0,
 *                          dst_ref the index of h;
 *                        neither is_root nor is_create:  ops 3 ReturnDataOffset (ro), 4 ReturnDataLength (rl), CallContext reads:
 *                          (call_id Memory -> next.call_id Memory; off, off + len, ro, min(len, rl); 0; rwc + 5) always, also with
 *                          length 0 (the reference looks it up unconditionally);
 *                        is_root and not is_create:  nothing, status 0, no op is read.
 *        DATACOPY        ops 1 CallerId (c), 2 CallDataOffset (cdo), 3 CallDataLength (cdl), 4 ReturnDataOffset (rdo), 5 ReturnDataLength
 *                        (rdl), CallContext reads with id == call_id.  Two events, always:
 *                          (c Memory -> c Memory; cdo, cdo + cdl, rdo, rdo + rdl; 0; rwc + 6) - the reference passes rdo + rdl as the
 *                          length, and so does this entry;
 *                          (c Memory -> call_id Memory; cdo, cdo + cdl, 0, rdl; 0; rwc + 6 + inc), inc = the counters the first event
 *                          consumes: with L = rdo + rdl its L writes plus its reads below src_addr_end, inc = L + min(L, cdl)
 *                          (CopyCircuit.copy appends a Memory write per byte and a Memory read per byte with src_addr + i <
 *                          src_addr_end; copy_lookup returns that row's rwc_inc).
 *        BeginTx         the gadget's branch is in the tx table; here it is told from the successor: the create path with init code is
 *                        taken iff next.is_create and next.rw_counter == rwc + 23 (ten ops up to the transfer, thirteen CallContext
 *                        lookups; the other paths end at rwc + 10 or have is_create clear).  On that path the call id is rwc itself:
 *                        ops 0 TxId (tx), 14 CallDataLength (n), 22 CodeHash (the word h), CallContext reads with id == rwc:
 *                          (tx TxCalldata -> rwc RlcAcc; 0, n, 0, n; 0; rwc + 10), then
 *                          (tx TxCalldata -> h (a Word: flag bit 1) Bytecode; 0, n, 0, n; 0; rwc + 10);
 *                        both with src_ref tx - 1, the second with dst_ref the index of h.  Every other BeginTx: nothing, status 0.
 *      Status per step: as above (sites 1 and 2 in ascending k, then 3, then 4; site 4 also when h is not in the code set; site 3's tx
 *      check is CALLDATACOPY's; the values c, cdo, cdl, rdo, rdl, ro, rl, off, len, tx, n and the sums off + len, cdo + cdl, rdo + rdl
 *      and every event counter are in site 3's domain), and a step emits all of its events or none.  One more site:
 *        5  the step needs a successor and is the last step (a RETURN that is neither root nor create, every BeginTx; checked before
 *           any op is read); or BeginTx's create path has n == 0 (checked after sites 1 and 2); or the step's events would lie past the
 *           copy capacity the session computed.  The last cannot happen while the steps are as the open saw them and is checked anyway:
 *           no store passes a capacity, the counts read back never exceed it; on the device the write pass sets that status behind
 *           the tally.
 *      Sessions, ZK_OPT_DEVICE_PTRS, zk_launch / zk_collect / zk_read_status / zk_session_set_stream / zk_close, what the session keeps
 *      a copy of, _read and _counts: all as zk_events_from_trace_open.  Domain errors: ZK_ERR_TRC_* and ZK_ERR_TEV_* exactly as above,
 *      under this entry's name. */
typedef struct zk_trace_events_ext {                         /* each pointer nullable; copy_*: the copy capacity, exp_*: n_steps */
    uint64_t* copy_events;      uint32_t* copy_flags;        uint32_t* copy_src_ref;        uint32_t* copy_dst_ref;
    uint32_t* copy_step;        uint64_t* exp_events;        uint32_t* exp_step;
} zk_trace_events_ext;
int zk_events_from_trace_ext_sizes(const zk_trace_sources* in, uint32_t opts, uint64_t* copy_capacity, uint64_t* exp_capacity);
int zk_events_from_trace_ext_open(const zk_trace_sources* in, const zk_trace_events_ext* out_dev, uint32_t opts, zk_session** out);
int zk_events_from_trace_ext_read(zk_session* s, const zk_trace_events_ext* host, uint64_t* n_copy, uint64_t* n_exp);
int zk_events_from_trace_ext_counts(zk_session* s, uint64_t* n_copy, uint64_t* n_exp);
int zk_events_from_trace_ext(const zk_trace_sources* in, const zk_trace_events_ext* out, uint32_t opts, uint32_t* status_out, uint64_t* n_copy,
                             uint64_t* n_exp, zk_result* result);

/* ---- SHA3 inputs and keccak rows from compact trace records: the keccak rows the SHA3 steps look up (zk_evm_tables' keccak table), which a
 *      producer of traces so far got by walking its memory image per SHA3 step, concatenating the bytes, uploading them and calling
 *      zk_keccak_table.  The bytes are in the trace already: execution/sha3.py pops offset and size and pushes the digest; its copy
 *      lookup reads `size` Memory bytes at the counters rw_counter + 3 + i; its keccak lookup is (size, RLC of those bytes) -> the
 *      pushed word.  This entry gathers the messages where the records are, runs the keccak table's own code over them and checks what
 *      no other entry does: that the word the trace pushed is the digest of the bytes the trace read.
 *      Of zk_trace, head, id, addr, val, rw_counter / rw_base, n_rw, pool, n_pool, steps and n_steps are read; prev never is and may be
 *      NULL.  randomness: uint64[4], the keccak randomness (as zk_keccak_table's).
 *      Outputs (zk_trace_sha3), each pointer nullable: rows uint64[n_msgs][5][4], zk_keccak_table's mode-0 rows (KeccakCircuit.add), one
 *      per message in step order, duplicates kept; step uint32[n_msgs], the step that produced each row; data uint8[n_bytes], the hashed
 *      bytes back to back; data_offsets uint64[n_msgs + 1].  Each row is bit for bit what zk_keccak_table(data, data_offsets, mode 0)
 *      returns over the gathered data / data_offsets.
 *      Derivation.  "Op k" of a step is the op whose counter is step.rw_counter + k (rw_counter NULL: its index is counter - rw_base;
 *      else it is found by binary search).  Values are taken as integers: val, or the pool word when the head says so.  For a step
 *      whose execution state is SHA3: op 0 is a Stack read of call_id at stack_pointer (the offset), op 1 a Stack read at stack_pointer
 *      + 1 (the size), op 2 a Stack WRITE at stack_pointer + 1 (the pushed word); none of the three addresses is a pool word.  Byte i
 *      of the message is the val of op 3 + i, which must be a Memory read (not a write) of id == call_id at addr == offset + i (not a
 *      pool word) with a value below 256 (not a pool word).  A step with size 0 is a message too, the empty string: row (2, 0, 0,
 *      keccak256("")), which is what sha3.py looks up; its offset is not read for anything (it may be a pool word), as
 *      memory_offset_and_length ignores it.  Steps of any other state have status 0 and produce nothing; CREATE2's keccak lookup of
 *      its init code is not derived.
 *      Status per step (zk_launch: status_dev uint32[n_steps]; the zk_result's tally runs over the steps, rows_evaluated = n_steps): 0,
 *      or (ZK_KIND_VALUE_ERROR << 24) | site, never a guess.  Sites 1 and 2 are checked in ascending k and the first failure wins, then
 *      site 3, then the lowest failing byte index, then site 7:
 *        1  no op has the counter of op 0, 1 or 2;     2  the op there is not the one described;
 *        3  the size taken as an integer is 2^62 or more; or, with size != 0, the offset is, or offset + size is, or step.rw_counter + 3
 *           is (the domain of zk_copy_assign and zk_events_from_trace's site 3: the two entries accept the same SHA3 steps);
 *        4  no op has the counter of byte i;     5  the op there is not a Memory read of call_id at offset + i;
 *        6  its value is 256 or more;
 *        7  every byte was read, but the 256-bit word pushed by op 2 differs from the digest.
 *      A step failing 1-3 is no message: it gets no row and no bytes.  A step failing 4-6 keeps its place: the failing byte is gathered
 *      as 0 (as zk_copy_assign_from_sources gathers it) and the row is the one over the data as gathered.  A step failing 7 has a
 *      correct row; the status is the finding.
 *      Sessions.  What indexes a load or a store is derived on the device at _sizes / _open and kept by the session: which steps are
 *      messages, their call_id, offset, size and first counter, the data offsets, the heads, the counters and the pool offsets.  Sites
 *      1-3 are decided at open; sites 4-7 by every pass.  The randomness is read at open, as zk_keccak_open reads it (its powers are
 *      the session's); id / addr / val and the pool are re-read by every pass (a caller that rewrites val between passes changes
 *      bytes, rows and site 7, and cannot move a store).  zk_sha3_from_trace_sizes: the checks below and n_msgs / n_bytes; rows, step and
 *      data_offsets are sized by n_msgs (+ 1), data by n_bytes.  _open: with ZK_OPT_DEVICE_PTRS every input is a device pointer and the
 *      non-null pointers of `out_dev` receive the outputs in place, every pass (null: the session owns that buffer; a caller's data
 *      buffer is read in whole aligned 64-bit words, as zk_keccak_open reads its data); without the flag out_dev must be NULL.
 *      zk_launch (with status_dev) / zk_collect / zk_read_status / zk_session_set_stream / zk_close as on the other assignment
 *      sessions; every launch runs the whole pass (the gather, the keccak table, the comparison) and carries nothing over.  _read copies
 *      the outputs to the non-null HOST pointers of `host` and returns the counts.  The one-shot's status_out is a device pointer with
 *      ZK_OPT_DEVICE_PTRS, like its other outputs.
 *      Domain, rejected at sizes / open with an error code and its text in zk_last_error:
 *        ZK_ERR_TRC_HEAD / _ORDER / _POOL exactly as zk_evm_witness_from_trace_open reports them (on the device, one verdict block read
 *        back, which also holds n_msgs and n_bytes), under this entry's name;
 *        ZK_ERR_TS3_ROWS   2^31 or more steps or RW ops;
 *        ZK_ERR_TS3_BYTES  the messages hold 2^31 bytes or more; the text names the step that takes the total there. */
#define ZK_ERR_TS3_ROWS (-110)
#define ZK_ERR_TS3_BYTES (-111)
typedef struct zk_trace_sha3 {                               /* each pointer nullable */
    uint64_t* rows;             /* uint64[n_msgs][5][4] */
    uint32_t* step;             /* uint32[n_msgs] */
    uint8_t* data;              /* uint8[n_bytes] */
    uint64_t* data_offsets;     /* uint64[n_msgs + 1] */
} zk_trace_sha3;
int zk_sha3_from_trace_sizes(const zk_trace* in, uint32_t opts, uint64_t* n_msgs, uint64_t* n_bytes);
int zk_sha3_from_trace_open(const zk_trace* in, const uint64_t* randomness, const zk_trace_sha3* out_dev, uint32_t opts, zk_session** out);
int zk_sha3_from_trace_read(zk_session* s, const zk_trace_sha3* host, uint64_t* n_msgs, uint64_t* n_bytes);
int zk_sha3_from_trace(const zk_trace* in, const uint64_t* randomness, const zk_trace_sha3* out, uint32_t opts, uint32_t* status_out,
                       uint64_t* n_msgs, uint64_t* n_bytes, zk_result* result);

#ifdef __cplusplus
}
#endif
#endif
