"""ctypes binding of libzkevm_hip.so (C ABI: include/zkevm_hip.h).

There is deliberately NO fallback: if the HIP library is missing or no GPU is usable the
engine raises — the product path never routes through a CPU implementation on its own.

ZK_BACKEND=cpu (an explicit choice, read once when the library is first loaded) binds the same C ABI to libzkevm_cpu.so
instead: the kernels' own per-row device functions compiled for the host and run with OpenMP (csrc/cpu_backend.cpp) —
BASELINE configs[0]'s "pure CPU path" through the real boundary and the optimised-CPU line of bench.py.  It implements every
entry of include/zkevm_hip.h — the verify / open / launch / collect entries of every circuit, the keccak-table and ECDSA entries
and (round 4) the State / Bytecode / Copy witness assignments; ZK_OPT_DEVICE_PTRS has no meaning there (inputs are host arrays).
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
BACKEND = os.environ.get("ZK_BACKEND", "hip")
if BACKEND not in ("hip", "cpu"):
    raise ImportError(f"ZK_BACKEND={BACKEND!r}: expected 'hip' (default) or 'cpu'")
CPU_LIB_PATH = os.path.join(_HERE, "libzkevm_cpu.so")
LIB_PATH = CPU_LIB_PATH if BACKEND == "cpu" else (os.environ.get("ZK_HIP_LIB") or os.path.join(_HERE, "libzkevm_hip.so"))  # ZK_HIP_LIB: tuning builds (tools/)

EXPORTED_SYMBOLS = [
    "zk_init", "zk_shutdown", "zk_set_stream", "zk_session_set_stream", "zk_last_error", "zk_fr_op",
    "zk_state_open", "zk_state_set_range", "zk_set_range", "zk_state_verify", "zk_evm_open", "zk_evm_verify", "zk_evm_verify_batch", "zk_bytecode_open", "zk_bytecode_verify", "zk_exp_open", "zk_exp_verify", "zk_copy_open", "zk_copy_verify", "zk_sign_open", "zk_sign_verify",
    "zk_keccak_open", "zk_keccak_read_rows", "zk_keccak_table", "zk_state_assign_open", "zk_state_assign_read", "zk_state_assign", "zk_state_ops_from_rw_open", "zk_state_ops_from_rw_read", "zk_state_ops_from_rw", "zk_state_assign_from_rw_open", "zk_state_verify_from_rw_open", "zk_state_verify_from_rw", "zk_block_verify", "zk_ecdsa_open", "zk_ecdsa_open_batches", "zk_ecdsa_verify", "zk_bytecode_assign_open", "zk_bytecode_assign_read", "zk_bytecode_assign", "zk_pi_open", "zk_pi_verify", "zk_pi_copy_open", "zk_pi_copy_verify", "zk_copy_assign_sizes", "zk_copy_assign_open", "zk_copy_assign_read", "zk_copy_assign", "zk_launch", "zk_collect", "zk_read_status", "zk_close", "zk_session_timing", "zk_last_timing", "zk_timing_sums", "zk_last_host_phases", "zk_dist_unique_id", "zk_dist_init", "zk_dist_tally", "zk_dist_close",
    "zk_ecc_assign", "zk_ecc_verify", "zk_ecc_open", "zk_ecc_assign_open", "zk_ecc_assign_read", "zk_withdrawal_open", "zk_withdrawal_verify", "zk_withdrawal_assign",
    "zk_tx_assign_open", "zk_tx_assign_read", "zk_tx_assign",
    "zk_exp_assign_sizes", "zk_exp_assign_open", "zk_exp_assign_read", "zk_exp_assign", "zk_exp_assign_counts",
    "zk_pi_assign_sizes", "zk_pi_assign_open", "zk_pi_assign_read", "zk_pi_assign",
    "zk_sig_assign_open", "zk_sig_assign_read", "zk_sig_assign",
    "zk_bytecode_from_code_open", "zk_bytecode_from_code_read", "zk_bytecode_from_code",
    "zk_evm_tables_from_block_sizes", "zk_evm_tables_from_block_open", "zk_evm_tables_from_block_read", "zk_evm_tables_from_block",
    "zk_evm_witness_from_trace_sizes", "zk_evm_witness_from_trace_open", "zk_evm_witness_from_trace_read", "zk_evm_witness_from_trace",
    "zk_ecc_from_calls_open", "zk_ecc_from_calls_read", "zk_ecc_from_calls",
    "zk_state_verify_from_trace_open", "zk_state_verify_from_trace", "zk_state_ops_from_trace_open", "zk_state_ops_from_trace_read", "zk_state_ops_from_trace",
    "zk_state_assign_from_trace_open", "zk_state_assign_from_trace",
    "zk_copy_assign_from_sources_sizes", "zk_copy_assign_from_sources_open", "zk_copy_assign_from_sources_read", "zk_copy_assign_from_sources",
    "zk_events_from_trace_sizes", "zk_events_from_trace_open", "zk_events_from_trace_read", "zk_events_from_trace_counts", "zk_events_from_trace",
    "zk_sha3_from_trace_sizes", "zk_sha3_from_trace_open", "zk_sha3_from_trace_read", "zk_sha3_from_trace",
    "zk_events_from_trace_ext_sizes", "zk_events_from_trace_ext_open", "zk_events_from_trace_ext_read", "zk_events_from_trace_ext_counts",
    "zk_events_from_trace_ext",
]

OPT_DEVICE_PTRS = 1


class ZkResult(ctypes.Structure):
    _fields_ = [
        ("fail_count", ctypes.c_uint64),
        ("first_fail_row", ctypes.c_uint64),
        ("first_fail_code", ctypes.c_uint32),
        ("launches", ctypes.c_uint32),
        ("rows_evaluated", ctypes.c_uint64),
        ("kernel_ms", ctypes.c_double),
    ]


class ZkEvmTables(ctypes.Structure):
    _fields_ = [
        ("steps", ctypes.c_void_p), ("n_steps", ctypes.c_uint64),
        ("rw", ctypes.c_void_p), ("rw_flags", ctypes.c_void_p), ("n_rw", ctypes.c_uint64),
        ("bytecode", ctypes.c_void_p), ("n_bytecode", ctypes.c_uint64),
        ("tx", ctypes.c_void_p), ("tx_flags", ctypes.c_void_p), ("n_tx", ctypes.c_uint64),
        ("block", ctypes.c_void_p), ("block_flags", ctypes.c_void_p), ("n_block", ctypes.c_uint64),
        ("begin_with_first_step", ctypes.c_uint32), ("end_with_last_step", ctypes.c_uint32),
        ("copy", ctypes.c_void_p), ("n_copy", ctypes.c_uint64),
        ("keccak", ctypes.c_void_p), ("n_keccak", ctypes.c_uint64),
        ("exp", ctypes.c_void_p), ("n_exp", ctypes.c_uint64),
        ("aux", ctypes.c_void_p), ("aux_kind", ctypes.c_void_p),
        ("withdrawals", ctypes.c_void_p), ("n_withdrawals", ctypes.c_uint64),
        ("sig", ctypes.c_void_p), ("n_sig", ctypes.c_uint64),
        ("ecc", ctypes.c_void_p), ("n_ecc", ctypes.c_uint64),
        ("aux_cells", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
    ]


class ZkCopyTables(ctypes.Structure):
    _fields_ = [
        ("rows", ctypes.c_void_p), ("row_flags", ctypes.c_void_p), ("n_rows", ctypes.c_uint64),
        ("randomness", ctypes.c_void_p),
        ("rw", ctypes.c_void_p), ("rw_flags", ctypes.c_void_p), ("n_rw", ctypes.c_uint64),
        ("bytecode", ctypes.c_void_p), ("n_bytecode", ctypes.c_uint64),
        ("tx", ctypes.c_void_p), ("tx_flags", ctypes.c_void_p), ("n_tx", ctypes.c_uint64),
    ]


class ZkSignUnits(ctypes.Structure):
    _fields_ = [
        ("bytes", ctypes.c_void_p), ("cells", ctypes.c_void_p), ("meta", ctypes.c_void_p), ("n_units", ctypes.c_uint64),
        ("randomness", ctypes.c_void_p),
        ("keccak", ctypes.c_void_p), ("n_keccak", ctypes.c_uint64),
        ("tx_rows", ctypes.c_void_p), ("tx_flags", ctypes.c_void_p), ("n_tx_rows", ctypes.c_uint64),
        ("is_sig", ctypes.c_uint32),
    ]


class ZkEccOps(ctypes.Structure):
    _fields_ = [("points", ctypes.c_void_p), ("n_add", ctypes.c_uint64), ("n_mul", ctypes.c_uint64),
                ("pair_pts", ctypes.c_void_p), ("pair_off", ctypes.c_void_p), ("pair_out", ctypes.c_void_p), ("n_pairing", ctypes.c_uint64),
                ("randomness", ctypes.c_void_p),
                ("max_add", ctypes.c_uint32), ("max_mul", ctypes.c_uint32), ("max_pairing", ctypes.c_uint32)]


class ZkWithdrawalWitness(ctypes.Structure):
    _fields_ = [("rows", ctypes.c_void_p), ("n_rows", ctypes.c_uint64), ("row_base", ctypes.c_uint64), ("total_rows", ctypes.c_uint64),
                ("max_withdrawals", ctypes.c_uint64), ("mpt", ctypes.c_void_p), ("n_mpt", ctypes.c_uint64), ("keccak", ctypes.c_void_p),
                ("n_keccak", ctypes.c_uint64), ("block", ctypes.c_void_p), ("n_block", ctypes.c_uint64), ("randomness", ctypes.c_void_p)]


class ZkTxInputs(ctypes.Structure):
    _fields_ = [("fields", ctypes.c_void_p), ("to_is_none", ctypes.c_void_p), ("n_txs", ctypes.c_uint64), ("calldata", ctypes.c_void_p),
                ("calldata_offsets", ctypes.c_void_p), ("chain_id", ctypes.c_uint64), ("max_txs", ctypes.c_uint64),
                ("max_calldata_bytes", ctypes.c_uint64), ("randomness", ctypes.c_void_p)]


class ZkTxWire(ctypes.Structure):
    _fields_ = [("tx_rows", ctypes.c_void_p), ("tx_flags", ctypes.c_void_p), ("bytes", ctypes.c_void_p), ("cells", ctypes.c_void_p),
                ("meta", ctypes.c_void_p), ("keccak", ctypes.c_void_p)]


class ZkSigInputs(ctypes.Structure):
    _fields_ = [("fields", ctypes.c_void_p), ("addr", ctypes.c_void_p), ("expect_valid", ctypes.c_void_p), ("n", ctypes.c_uint64),
                ("v_offset", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("randomness", ctypes.c_void_p)]


class ZkSigWire(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("bytes", "cells", "meta", "keccak", "sig_table", "aux")]


class ZkCodeSet(ctypes.Structure):
    _fields_ = [("code", ctypes.c_void_p), ("n_bytes", ctypes.c_uint64), ("offsets", ctypes.c_void_p), ("n_codes", ctypes.c_uint64),
                ("k", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("randomness", ctypes.c_void_p)]


class ZkCodeWire(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("table", "rows", "keccak")]


class ZkBlockData(ctypes.Structure):
    _fields_ = [("tx_fields", ctypes.c_void_p), ("to_is_none", ctypes.c_void_p), ("access_list", ctypes.c_void_p), ("n_txs", ctypes.c_uint64),
                ("calldata", ctypes.c_void_p), ("calldata_offsets", ctypes.c_void_p), ("block", ctypes.c_void_p),
                ("history_hashes", ctypes.c_void_p), ("n_history", ctypes.c_uint64), ("withdrawals", ctypes.c_void_p), ("n_withdrawals", ctypes.c_uint64)]


class ZkBlockTables(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("tx", "tx_flags", "block", "block_flags", "withdrawals")]


class ZkTrace(ctypes.Structure):
    _fields_ = [("head", ctypes.c_void_p), ("id", ctypes.c_void_p), ("addr", ctypes.c_void_p), ("val", ctypes.c_void_p), ("prev", ctypes.c_void_p),
                ("rw_counter", ctypes.c_void_p), ("rw_base", ctypes.c_uint64), ("n_rw", ctypes.c_uint64), ("pool", ctypes.c_void_p),
                ("n_pool", ctypes.c_uint64), ("steps", ctypes.c_void_p), ("n_steps", ctypes.c_uint64)]


class ZkCopySources(ctypes.Structure):
    """zk_copy_sources (include/zkevm_hip.h): copy events with refs into a code set, calldata and trace records"""
    _fields_ = [("events", ctypes.c_void_p), ("flags", ctypes.c_void_p), ("n_events", ctypes.c_uint64),
                ("src_ref", ctypes.c_void_p), ("dst_ref", ctypes.c_void_p), ("randomness", ctypes.c_void_p),
                ("code", ctypes.c_void_p), ("n_code_bytes", ctypes.c_uint64), ("code_offsets", ctypes.c_void_p), ("n_codes", ctypes.c_uint64),
                ("calldata", ctypes.c_void_p), ("calldata_offsets", ctypes.c_void_p), ("n_txs", ctypes.c_uint64),
                ("trace", ZkTrace)]


class ZkTraceSources(ctypes.Structure):
    """zk_trace_sources (include/zkevm_hip.h): trace records, a code set and the codes' hashes"""
    _fields_ = [("trace", ZkTrace), ("code", ctypes.c_void_p), ("n_code_bytes", ctypes.c_uint64), ("code_offsets", ctypes.c_void_p),
                ("n_codes", ctypes.c_uint64), ("code_hashes", ctypes.c_void_p)]


class ZkTraceEvents(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("copy_events", "copy_flags", "copy_src_ref", "copy_step", "exp_events", "exp_step")]


class ZkTraceEventsExt(ctypes.Structure):
    """zk_trace_events_ext (include/zkevm_hip.h): zk_trace_events with the dst_ref of the events that write a code"""
    _fields_ = [(k, ctypes.c_void_p) for k in ("copy_events", "copy_flags", "copy_src_ref", "copy_dst_ref", "copy_step", "exp_events", "exp_step")]


class ZkTraceSha3(ctypes.Structure):
    """zk_trace_sha3 (include/zkevm_hip.h): the keccak rows of the SHA3 steps, their steps, the hashed bytes and their offsets"""
    _fields_ = [(k, ctypes.c_void_p) for k in ("rows", "step", "data", "data_offsets")]


class ZkTraceWitness(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("rw", "rw_flags", "steps")]


class ZkEccCalls(ctypes.Structure):
    _fields_ = [("add_in", ctypes.c_void_p), ("n_add", ctypes.c_uint64), ("mul_in", ctypes.c_void_p), ("n_mul", ctypes.c_uint64),
                ("pair_pts", ctypes.c_void_p), ("pair_off", ctypes.c_void_p), ("n_pairing", ctypes.c_uint64), ("randomness", ctypes.c_void_p)]


class ZkEccCallWire(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("points", "pair_out", "rows", "ecc_table", "aux", "aux_kind")]


class ZkEcdsaBatch(ctypes.Structure):
    _fields_ = [("bytes", ctypes.c_void_p), ("layout", ctypes.c_uint32), ("v", ctypes.c_void_p), ("v_stride", ctypes.c_uint32),
                ("n", ctypes.c_uint64), ("out_dev", ctypes.c_void_p), ("out_stride", ctypes.c_uint32)]


class ZkCopyEvents(ctypes.Structure):
    _fields_ = [
        ("events", ctypes.c_void_p), ("flags", ctypes.c_void_p), ("n_events", ctypes.c_uint64),
        ("data", ctypes.c_void_p), ("data_offsets", ctypes.c_void_p),
        ("randomness", ctypes.c_void_p),
    ]


class ZkExpEvents(ctypes.Structure):
    _fields_ = [("events", ctypes.c_void_p), ("n_events", ctypes.c_uint64), ("max_exp_steps", ctypes.c_uint64)]


class ZkPiInputs(ctypes.Structure):
    _fields_ = [("chain_id", ctypes.c_uint64), ("block", ctypes.c_void_p), ("state_root_prev", ctypes.c_void_p), ("block_hashes", ctypes.c_void_p),
                ("tx_fields", ctypes.c_void_p), ("to_is_none", ctypes.c_void_p), ("n_txs", ctypes.c_uint64), ("calldata", ctypes.c_void_p),
                ("calldata_offsets", ctypes.c_void_p), ("withdrawals", ctypes.c_void_p), ("n_withdrawals", ctypes.c_uint64),
                ("max_txs", ctypes.c_uint64), ("max_calldata_bytes", ctypes.c_uint64), ("max_withdrawals", ctypes.c_uint64),
                ("keccak_rand", ctypes.c_void_p), ("byte_pow_base", ctypes.c_void_p)]


class ZkPiWire(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("rows", "gas", "keccak", "cc_cells", "cc_bytes", "cc_lens", "block_table", "block_flags",
                                               "tx_table", "tx_flags", "wd_table", "public_inputs", "raw_bytes", "raw_lens")]


# ZK_ERR_PI_* (include/zkevm_hip.h): why zk_pi_assign* rejected its inputs
ERR_PI_TXS, ERR_PI_WITHDRAWALS, ERR_PI_CALLDATA, ERR_PI_FIELD, ERR_PI_ROWS = -50, -51, -52, -53, -54
ERR_EXP_CELL, ERR_EXP_ORDER, ERR_EXP_ROWS = -40, -41, -42  # ZK_ERR_EXP_* (include/zkevm_hip.h): why zk_exp_assign* rejected its events
ERR_BTB_ID, ERR_BTB_OFFSETS, ERR_BTB_HISTORY, ERR_BTB_ROWS = -60, -61, -62, -63  # ZK_ERR_BTB_*: why zk_evm_tables_from_block* rejected its inputs
ERR_TRC_HEAD, ERR_TRC_ORDER, ERR_TRC_POOL, ERR_TRC_ROWS = -70, -71, -72, -73  # ZK_ERR_TRC_*: why zk_evm_witness_from_trace* rejected its records
ERR_ECL_OFFSETS, ERR_ECL_ROWS, ERR_ECL_RANDOMNESS = -80, -81, -82  # ZK_ERR_ECL_*: why zk_ecc_from_calls* rejected its calls
ERR_CPS_OFFSETS, ERR_CPS_ROWS = -90, -91  # ZK_ERR_CPS_*: why zk_copy_assign_from_sources* rejected its sources
ERR_TEV_OFFSETS, ERR_TEV_ROWS = -100, -101  # ZK_ERR_TEV_*: why zk_events_from_trace* rejected its code set or its counts
ERR_TS3_ROWS, ERR_TS3_BYTES = -110, -111  # ZK_ERR_TS3_*: why zk_sha3_from_trace* rejected its counts


class ZkBlock(ctypes.Structure):
    """zk_block (include/zkevm_hip.h): the raw device-resident inputs of zk_block_verify"""
    _fields_ = [
        ("evm", ZkEvmTables),
        ("hashed_data", ctypes.c_void_p), ("hashed_bytes", ctypes.c_uint64), ("hashed_offsets", ctypes.c_void_p),
        ("n_codes", ctypes.c_uint64), ("n_hashed", ctypes.c_uint64),
        ("randomness", ctypes.c_void_p),
        ("code_offsets", ctypes.c_void_p), ("code_lengths", ctypes.c_void_p), ("n_bytecodes", ctypes.c_uint64), ("k", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
        ("copy_events", ZkCopyEvents),
        ("exp_rows", ctypes.c_void_p), ("n_exp_rows", ctypes.c_uint64),
        ("tx", ZkSignUnits),
        ("exp_events", ZkExpEvents),
    ]


BLOCK_CIRCUITS = ("evm", "state", "bytecode", "tx", "copy", "exp")  # order of zk_block_verify's results (ZK_BLOCK_*)
OPT_NO_STATE_SORT = 2
OPT_GENERIC_INDEX = 4
OPT_SINGLE_PASS = 8
OPT_SIDE_STREAM = 16
OPT_STATE_COMPACT = 32  # State rows without the limb / byte columns (include/zkevm_hip.h ZK_OPT_STATE_COMPACT)
OPT_BLOCK_STATE_ROWS = 64  # zk_block_verify: materialise the State witness instead of the fused form


class EngineError(RuntimeError):
    rc = None  # the C entry's return code, where one call failed (check)


_lib = None
_inited_device = None


def load():
    """Load the shared library (no GPU needed for loading / symbol checks)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EngineError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(zkevm_specs_amd/csrc/build.sh). There is no CPU fallback."
        )
    # torch ships its own libamdhip64.so.7; importing it first makes the dynamic loader bind
    # this library to the SAME HIP runtime instance (one runtime per process: device pointers,
    # streams and events are then interchangeable with torch's).
    if BACKEND == "hip":
        # one hardware queue per concurrent circuit session (csrc/zkevm_hip.hip zk_default_hw_queues): the HIP runtime reads the
        # variable at its first call, which torch makes lazily.  Set here — when the HIP library is actually loaded — and not
        # at package import: a process that only uses the CPU backend, or imports the package for its witness generators, keeps
        # its environment untouched.  A host that sets the variable itself keeps its own choice.
        os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
        import torch  # noqa: F401

    _lib = _bind(ctypes.CDLL(LIB_PATH))
    return _lib


_cpu_lib = None


def load_cpu():
    """The CPU backend's library next to the default one (same C ABI; bench.py's optimised-CPU legs call it with
    `device="cpu"` on the one-shot entries).  Never a fallback: only explicit callers get it."""
    global _cpu_lib
    if _cpu_lib is None:
        if not os.path.exists(CPU_LIB_PATH):
            raise EngineError(f"{CPU_LIB_PATH} is missing: build it with zkevm_specs_amd/csrc/build.sh")
        _cpu_lib = _bind(ctypes.CDLL(CPU_LIB_PATH))
    return _cpu_lib


def set_cpu_threads(n):
    """OpenMP threads of the CPU backend's passes (libgomp's omp_set_num_threads)"""
    ctypes.CDLL("libgomp.so.1").omp_set_num_threads(int(n))


def _bind(lib):
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    lib.zk_init.argtypes = [ctypes.c_int]
    lib.zk_set_stream.argtypes = [vp]
    lib.zk_session_set_stream.argtypes = [vp, vp]
    lib.zk_last_error.restype = ctypes.c_char_p
    lib.zk_fr_op.argtypes = [ctypes.c_int, vp, vp, vp, u64, u32]
    lib.zk_state_open.argtypes = [vp, vp, u64, vp, u64, u32, ctypes.POINTER(vp)]
    lib.zk_state_set_range.argtypes = [vp, u64, u64]
    lib.zk_set_range.argtypes = [vp, u64, u64]
    lib.zk_state_verify.argtypes = [vp, vp, u64, vp, u64, u32, vp, ctypes.POINTER(ZkResult)]
    lib.zk_evm_open.argtypes = [ctypes.POINTER(ZkEvmTables), u32, ctypes.POINTER(vp)]
    lib.zk_evm_verify.argtypes = [ctypes.POINTER(ZkEvmTables), u32, vp, ctypes.POINTER(ZkResult)]
    lib.zk_evm_verify_batch.argtypes = [ctypes.POINTER(ctypes.POINTER(ZkEvmTables)), u64, u32, ctypes.POINTER(ZkResult)]
    lib.zk_bytecode_open.argtypes = [vp, u64, vp, u64, vp, u32, ctypes.POINTER(vp)]
    lib.zk_bytecode_verify.argtypes = [vp, u64, vp, u64, vp, u32, vp, ctypes.POINTER(ZkResult)]
    lib.zk_exp_open.argtypes = [vp, u64, u32, ctypes.POINTER(vp)]
    lib.zk_exp_verify.argtypes = [vp, u64, u32, vp, ctypes.POINTER(ZkResult)]
    lib.zk_copy_open.argtypes = [ctypes.POINTER(ZkCopyTables), u32, ctypes.POINTER(vp)]
    lib.zk_copy_verify.argtypes = [ctypes.POINTER(ZkCopyTables), u32, vp, ctypes.POINTER(ZkResult)]
    lib.zk_sign_open.argtypes = [ctypes.POINTER(ZkSignUnits), u32, ctypes.POINTER(vp)]
    lib.zk_sign_verify.argtypes = [ctypes.POINTER(ZkSignUnits), u32, vp, ctypes.POINTER(ZkResult)]
    lib.zk_ecc_assign.argtypes = [ctypes.POINTER(ZkEccOps), u32, vp]
    lib.zk_ecc_verify.argtypes = [ctypes.POINTER(ZkEccOps), vp, u32, vp, ctypes.POINTER(ZkResult)]
    lib.zk_ecc_open.argtypes = [ctypes.POINTER(ZkEccOps), vp, u32, ctypes.POINTER(vp)]
    lib.zk_ecc_assign_open.argtypes = [ctypes.POINTER(ZkEccOps), vp, u32, ctypes.POINTER(vp)]
    lib.zk_ecc_assign_read.argtypes = [vp, vp]
    lib.zk_withdrawal_open.argtypes = [ctypes.POINTER(ZkWithdrawalWitness), u32, ctypes.POINTER(vp)]
    lib.zk_withdrawal_verify.argtypes = [ctypes.POINTER(ZkWithdrawalWitness), u32, vp, ctypes.POINTER(ZkResult)]
    lib.zk_withdrawal_assign.argtypes = [vp, u64, u64, vp, u32, vp, vp]
    lib.zk_tx_assign_open.argtypes = [ctypes.POINTER(ZkTxInputs), ctypes.POINTER(ZkTxWire), u32, ctypes.POINTER(vp)]
    lib.zk_tx_assign_read.argtypes = [vp, ctypes.POINTER(ZkTxWire), ctypes.POINTER(u64)]
    lib.zk_tx_assign.argtypes = [ctypes.POINTER(ZkTxInputs), ctypes.POINTER(ZkTxWire), u32, vp, ctypes.POINTER(u64), ctypes.POINTER(ZkResult)]
    lib.zk_keccak_open.argtypes = [vp, u64, vp, u64, vp, u32, vp, u32, ctypes.POINTER(vp)]
    lib.zk_keccak_read_rows.argtypes = [vp, vp]
    lib.zk_keccak_table.argtypes = [vp, u64, vp, u64, vp, u32, vp, u32, vp, ctypes.POINTER(ZkResult)]
    lib.zk_state_assign_open.argtypes = [vp, vp, u64, vp, vp, vp, u32, ctypes.POINTER(vp)]
    lib.zk_state_assign_read.argtypes = [vp, vp, vp, vp, u64, ctypes.POINTER(u64)]
    lib.zk_state_assign.argtypes = [vp, vp, u64, vp, vp, vp, ctypes.POINTER(u64), u32, vp, ctypes.POINTER(ZkResult)]
    lib.zk_state_ops_from_rw_open.argtypes = [vp, vp, u64, vp, vp, u32, ctypes.POINTER(u64), ctypes.POINTER(vp)]
    lib.zk_state_ops_from_rw_read.argtypes = [vp, vp, vp, ctypes.POINTER(u64)]
    lib.zk_state_assign_from_rw_open.argtypes = [vp, vp, u64, vp, vp, vp, u32, ctypes.POINTER(u64), ctypes.POINTER(vp)]
    lib.zk_state_verify_from_rw_open.argtypes = [vp, vp, u64, u32, ctypes.POINTER(u64), ctypes.POINTER(vp)]
    lib.zk_state_verify_from_rw.argtypes = [vp, vp, u64, u32, vp, ctypes.POINTER(u64), ctypes.POINTER(ZkResult)]
    lib.zk_block_verify.argtypes = [vp, u32, vp, vp]
    lib.zk_state_ops_from_rw.argtypes = [vp, vp, u64, vp, vp, ctypes.POINTER(u64), u32, vp, ctypes.POINTER(ZkResult)]
    lib.zk_ecdsa_open.argtypes = [vp, u32, vp, u32, u64, vp, u32, u32, ctypes.POINTER(vp)]
    lib.zk_ecdsa_verify.argtypes = [vp, u32, vp, u32, u64, u32, vp, ctypes.POINTER(ZkResult)]
    lib.zk_ecdsa_open_batches.argtypes = [ctypes.POINTER(ZkEcdsaBatch), u32, u32, ctypes.POINTER(vp)]
    lib.zk_bytecode_assign_open.argtypes = [vp, u64, vp, vp, u64, u32, vp, vp, u32, ctypes.POINTER(vp)]
    lib.zk_bytecode_assign_read.argtypes = [vp, vp]
    lib.zk_bytecode_assign.argtypes = [vp, u64, vp, vp, u64, u32, vp, vp, u32, ctypes.POINTER(ZkResult)]
    lib.zk_pi_open.argtypes = [vp, u64, vp, u64, vp, u64, u64, vp, vp, u32, ctypes.POINTER(vp)]
    lib.zk_pi_verify.argtypes = [vp, u64, vp, u64, vp, u64, u64, vp, vp, u32, vp, ctypes.POINTER(ZkResult)]
    lib.zk_pi_copy_open.argtypes = [vp, vp, vp, u64, u32, ctypes.POINTER(vp)]
    lib.zk_pi_copy_verify.argtypes = [vp, vp, vp, u64, u32, vp, ctypes.POINTER(ZkResult)]
    lib.zk_copy_assign_sizes.argtypes = [ctypes.POINTER(ZkCopyEvents), u32, ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.zk_copy_assign_open.argtypes = [ctypes.POINTER(ZkCopyEvents), vp, vp, vp, vp, vp, u32, ctypes.POINTER(vp)]
    lib.zk_copy_assign_read.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.zk_copy_assign.argtypes = [ctypes.POINTER(ZkCopyEvents), vp, vp, vp, vp, vp, u32, ctypes.POINTER(ZkResult)]
    lib.zk_exp_assign_sizes.argtypes = [ctypes.POINTER(ZkExpEvents), u32, ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.zk_exp_assign_open.argtypes = [ctypes.POINTER(ZkExpEvents), vp, vp, u32, ctypes.POINTER(vp)]
    lib.zk_exp_assign_read.argtypes = [vp, vp, vp]
    lib.zk_exp_assign_counts.argtypes = [vp, ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.zk_exp_assign.argtypes = [ctypes.POINTER(ZkExpEvents), vp, vp, u32, ctypes.POINTER(ZkResult)]
    lib.zk_pi_assign_sizes.argtypes = [ctypes.POINTER(ZkPiInputs), u32, ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.zk_pi_assign_open.argtypes = [ctypes.POINTER(ZkPiInputs), ctypes.POINTER(ZkPiWire), u32, ctypes.POINTER(vp)]
    lib.zk_pi_assign_read.argtypes = [vp, ctypes.POINTER(ZkPiWire)]
    lib.zk_pi_assign.argtypes = [ctypes.POINTER(ZkPiInputs), ctypes.POINTER(ZkPiWire), u32, ctypes.POINTER(ZkResult)]
    lib.zk_sig_assign_open.argtypes = [ctypes.POINTER(ZkSigInputs), ctypes.POINTER(ZkSigWire), u32, ctypes.POINTER(vp)]
    lib.zk_sig_assign_read.argtypes = [vp, ctypes.POINTER(ZkSigWire), ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.zk_sig_assign.argtypes = [ctypes.POINTER(ZkSigInputs), ctypes.POINTER(ZkSigWire), u32, vp, ctypes.POINTER(u64), ctypes.POINTER(u64),
                                  ctypes.POINTER(ZkResult)]
    lib.zk_bytecode_from_code_open.argtypes = [ctypes.POINTER(ZkCodeSet), ctypes.POINTER(ZkCodeWire), u32, ctypes.POINTER(vp)]
    lib.zk_bytecode_from_code_read.argtypes = [vp, ctypes.POINTER(ZkCodeWire)]
    lib.zk_bytecode_from_code.argtypes = [ctypes.POINTER(ZkCodeSet), ctypes.POINTER(ZkCodeWire), u32, ctypes.POINTER(ZkResult)]
    lib.zk_evm_tables_from_block_sizes.argtypes = [ctypes.POINTER(ZkBlockData), u32, ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.zk_evm_tables_from_block_open.argtypes = [ctypes.POINTER(ZkBlockData), ctypes.POINTER(ZkBlockTables), u32, ctypes.POINTER(vp)]
    lib.zk_evm_tables_from_block_read.argtypes = [vp, ctypes.POINTER(ZkBlockTables)]
    lib.zk_evm_tables_from_block.argtypes = [ctypes.POINTER(ZkBlockData), ctypes.POINTER(ZkBlockTables), u32, ctypes.POINTER(ZkResult)]
    lib.zk_evm_witness_from_trace_sizes.argtypes = [ctypes.POINTER(ZkTrace), u32, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.zk_evm_witness_from_trace_open.argtypes = [ctypes.POINTER(ZkTrace), ctypes.POINTER(ZkTraceWitness), u32, ctypes.POINTER(vp)]
    lib.zk_evm_witness_from_trace_read.argtypes = [vp, ctypes.POINTER(ZkTraceWitness)]
    lib.zk_evm_witness_from_trace.argtypes = [ctypes.POINTER(ZkTrace), ctypes.POINTER(ZkTraceWitness), u32, ctypes.POINTER(ZkResult)]
    lib.zk_state_verify_from_trace_open.argtypes = [ctypes.POINTER(ZkTrace), u32, ctypes.POINTER(u64), ctypes.POINTER(vp)]
    lib.zk_state_verify_from_trace.argtypes = [ctypes.POINTER(ZkTrace), u32, vp, ctypes.POINTER(u64), ctypes.POINTER(ZkResult)]
    lib.zk_state_ops_from_trace_open.argtypes = [ctypes.POINTER(ZkTrace), vp, vp, u32, ctypes.POINTER(u64), ctypes.POINTER(vp)]
    lib.zk_state_ops_from_trace_read.argtypes = [vp, vp, vp, ctypes.POINTER(u64)]
    lib.zk_state_ops_from_trace.argtypes = [ctypes.POINTER(ZkTrace), vp, vp, ctypes.POINTER(u64), u32, vp, ctypes.POINTER(ZkResult)]
    lib.zk_state_assign_from_trace_open.argtypes = [ctypes.POINTER(ZkTrace), vp, vp, vp, u32, ctypes.POINTER(u64), ctypes.POINTER(vp)]
    lib.zk_state_assign_from_trace.argtypes = [ctypes.POINTER(ZkTrace), vp, vp, vp, ctypes.POINTER(u64), ctypes.POINTER(u64), u32, vp, ctypes.POINTER(ZkResult)]
    lib.zk_ecc_from_calls_open.argtypes = [ctypes.POINTER(ZkEccCalls), ctypes.POINTER(ZkEccCallWire), u32, ctypes.POINTER(vp)]
    lib.zk_ecc_from_calls_read.argtypes = [vp, ctypes.POINTER(ZkEccCallWire), ctypes.POINTER(u64)]
    lib.zk_ecc_from_calls.argtypes = [ctypes.POINTER(ZkEccCalls), ctypes.POINTER(ZkEccCallWire), u32, vp, ctypes.POINTER(u64),
                                      ctypes.POINTER(ZkResult)]
    lib.zk_copy_assign_from_sources_sizes.argtypes = [ctypes.POINTER(ZkCopySources), u32] + [ctypes.POINTER(u64)] * 4
    lib.zk_copy_assign_from_sources_open.argtypes = [ctypes.POINTER(ZkCopySources), vp, vp, vp, vp, vp, vp, u32, ctypes.POINTER(vp)]
    lib.zk_copy_assign_from_sources_read.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    lib.zk_copy_assign_from_sources.argtypes = [ctypes.POINTER(ZkCopySources), vp, vp, vp, vp, vp, vp, vp, u32, vp, ctypes.POINTER(ZkResult)]
    lib.zk_events_from_trace_sizes.argtypes = [ctypes.POINTER(ZkTraceSources), u32, ctypes.POINTER(u64)]
    lib.zk_events_from_trace_open.argtypes = [ctypes.POINTER(ZkTraceSources), ctypes.POINTER(ZkTraceEvents), u32, ctypes.POINTER(vp)]
    lib.zk_events_from_trace_read.argtypes = [vp, ctypes.POINTER(ZkTraceEvents), ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.zk_events_from_trace_counts.argtypes = [vp, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.zk_events_from_trace.argtypes = [ctypes.POINTER(ZkTraceSources), ctypes.POINTER(ZkTraceEvents), u32, vp, ctypes.POINTER(u64),
                                         ctypes.POINTER(u64), ctypes.POINTER(ZkResult)]
    lib.zk_events_from_trace_ext_sizes.argtypes = [ctypes.POINTER(ZkTraceSources), u32, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.zk_events_from_trace_ext_open.argtypes = [ctypes.POINTER(ZkTraceSources), ctypes.POINTER(ZkTraceEventsExt), u32, ctypes.POINTER(vp)]
    lib.zk_events_from_trace_ext_read.argtypes = [vp, ctypes.POINTER(ZkTraceEventsExt), ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.zk_events_from_trace_ext_counts.argtypes = [vp, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.zk_events_from_trace_ext.argtypes = [ctypes.POINTER(ZkTraceSources), ctypes.POINTER(ZkTraceEventsExt), u32, vp, ctypes.POINTER(u64),
                                             ctypes.POINTER(u64), ctypes.POINTER(ZkResult)]
    lib.zk_sha3_from_trace_sizes.argtypes = [ctypes.POINTER(ZkTrace), u32, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.zk_sha3_from_trace_open.argtypes = [ctypes.POINTER(ZkTrace), vp, ctypes.POINTER(ZkTraceSha3), u32, ctypes.POINTER(vp)]
    lib.zk_sha3_from_trace_read.argtypes = [vp, ctypes.POINTER(ZkTraceSha3), ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.zk_sha3_from_trace.argtypes = [ctypes.POINTER(ZkTrace), vp, ctypes.POINTER(ZkTraceSha3), u32, vp, ctypes.POINTER(u64), ctypes.POINTER(u64),
                                       ctypes.POINTER(ZkResult)]
    lib.zk_launch.argtypes = [vp, vp]
    lib.zk_collect.argtypes = [vp, ctypes.POINTER(ZkResult)]
    lib.zk_read_status.argtypes = [vp, vp]
    lib.zk_close.argtypes = [vp]
    dp = ctypes.POINTER(ctypes.c_double)
    lib.zk_session_timing.argtypes = [vp, dp, dp]
    lib.zk_last_timing.argtypes = [dp, dp, dp]
    lib.zk_last_host_phases.argtypes = [dp]
    lib.zk_timing_sums.argtypes = [dp, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]
    lib.zk_dist_unique_id.argtypes = [ctypes.c_void_p]
    lib.zk_dist_init.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    lib.zk_dist_tally.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    lib.zk_dist_close.argtypes = [ctypes.c_void_p]
    return lib


def check(rc, what, lib=None):
    """`lib`: the library the failing call was made on (a Session passes its own: an error of the CPU backend must not make
    this process load torch + the HIP library just to format it)."""
    if rc != 0:
        owner = lib if lib is not None else (_lib if _lib is not None else (_cpu_lib if _cpu_lib is not None else load()))
        msg = owner.zk_last_error().decode(errors="replace")
        if not msg and lib is None and _cpu_lib is not None and owner is not _cpu_lib:
            msg = _cpu_lib.zk_last_error().decode(errors="replace")
        err = EngineError(f"{what} failed (rc={rc}): {msg}")
        err.rc = int(rc)
        raise err


def init(device=None):
    """Initialise the engine on a HIP device (default: the device an earlier init() of this process selected, else
    LOCAL_RANK, else 0)."""
    global _inited_device
    if device == "cpu":  # the CPU backend's library, explicitly (see load_cpu)
        return load_cpu()
    lib = load()
    if device is None:
        device = _inited_device if _inited_device is not None else int(os.environ.get("LOCAL_RANK", "0"))
    # zk_init is idempotent and its selection is per thread: always forward it (a cached "already initialised" flag would
    # be wrong for a second thread or after another device was selected in between)
    check(lib.zk_init(int(device)), "zk_init")
    _inited_device = device
    return lib


def ptr(x, n=1):
    """void* of a numpy array (host) or a torch tensor (device / host); None (a null pointer) for no array, or when its count
    `n` is 0."""
    if x is None or not n:
        return None
    if hasattr(x, "data_ptr"):
        return ctypes.c_void_p(x.data_ptr())
    return ctypes.c_void_p(x.ctypes.data)
