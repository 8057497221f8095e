"""The one-shot C entries (`zk_*_verify`, `zk_keccak_table`, `zk_state_assign`, `zk_bytecode_assign`, `zk_ecdsa_verify`):
host buffers in, tally + per-row status out — exactly the calls INTEGRATION.md's reference-side stub makes.  The host
mirrors (`evm_circuit.verify_steps`, `state_circuit.verify_state_rows`, ...) go through these; `engine.py` is the session
form (upload once, many passes) for benchmarks and device-resident pipelines.  Both forms check and marshal their arguments
with the same builders (engine._*_args and kin); a one-shot first makes its inputs host arrays of the wire dtype.  The seven
"input struct + wire struct of outputs" families (tx, sig, ecc calls, pi, code, block tables, trace: engine.WireFamily) share one
body here, _wire_oneshot; the from-RW and from-trace State one-shots share _state_verify_from and _state_ops_from.
"""
import ctypes

import numpy as np

from . import _lib, engine
from ._lib import ZkResult, check, ptr
from .engine import Result, _expect, _host, _randomness_cells, withdrawal_arrays  # noqa: F401 (withdrawal_arrays: kept importable here)


def _verify(lib, fn, n, *args):
    """one `fn(*args, status, &result)` call of a zk_*_verify entry of `lib` -> (Result, status uint32[n])"""
    status, r = np.zeros(n, dtype=np.uint32), ZkResult()
    check(fn(*args, ptr(status), ctypes.byref(r)), fn.__name__, lib)
    return Result(r), status


def _host_inputs(fam, x):
    """the input dict `x` of a wire-struct family (engine.WireFamily) with its arrays made C-contiguous host arrays"""
    return {k: (_host(v) if k in fam.inputs else v) for k, v in x.items()}


def _wire_oneshot(fam, lib, p):
    """The one-shot entry of a wire-struct family over a prepared call `p` (engine._wire_args): allocate the host outputs, one
    `<stem>(&inputs, &wire, opts, [status,] &count..., &result)` call, cut the family's `cut` outputs to the counts -> (Result,
    [status uint32[n],] dict of the outputs)"""
    out, w = engine._wire_host_outputs(fam, p.shapes)
    status = np.zeros(max(p.n, 1), dtype=np.uint32) if fam.status else None
    counts, r = [ctypes.c_uint64() for _ in fam.cut], ZkResult()
    check(getattr(lib, fam.stem)(ctypes.byref(p.t), ctypes.byref(w), p.opts, *([ptr(status)] if fam.status else []),
                                 *(ctypes.byref(c) for c in counts), ctypes.byref(r)), fam.stem, lib)
    for k, c in zip(fam.cut, counts):
        out[k] = out[k][: c.value]
    return (Result(r), status[: p.n], out) if fam.status else (Result(r), out)


def state_verify(rows, flags, mpt, device=None):
    """zk_state_verify -> (Result, status uint32[n])"""
    lib = _lib.init(device)
    args, opts, keep = engine._state_args(_host(rows), _host(flags), _host(mpt))
    return _verify(lib, lib.zk_state_verify, args[2], *args, opts)


def evm_verify(wire, begin_with_first_step=False, end_with_last_step=False, opts=0, device=None):
    """zk_evm_verify over a wire dict (flatten.flatten_evm) -> (Result, status uint32[n_steps - 1])"""
    lib = _lib.init(device)
    t, o, keep, n_pairs = engine._evm_tables({k: _host(wire.get(k)) for k in engine._EVM_WIRE}, begin_with_first_step, end_with_last_step)
    status, r = np.zeros(max(n_pairs, 1), dtype=np.uint32), ZkResult()
    check(lib.zk_evm_verify(ctypes.byref(t), o | int(opts), ptr(status), ctypes.byref(r)), "zk_evm_verify", lib)
    return Result(r), status[:n_pairs]


def bytecode_verify(rows, keccak, randomness, device=None):
    lib = _lib.init(device)
    args, opts, keep = engine._bytecode_args(_host(rows), _host(keccak), randomness)
    return _verify(lib, lib.zk_bytecode_verify, args[1], *args, opts)


def exp_verify(rows, device=None):
    lib = _lib.init(device)
    args, opts, keep = engine._exp_args(_host(rows))
    return _verify(lib, lib.zk_exp_verify, args[1], *args, opts)


def copy_verify(rows, row_flags, randomness, rw, rw_flags, bytecode, tx, tx_flags, opts=0, device=None):
    lib = _lib.init(device)
    rows, row_flags, rw, rw_flags, bytecode, tx, tx_flags = (_host(x) for x in (rows, row_flags, rw, rw_flags, bytecode, tx, tx_flags))
    t, o, keep = engine._copy_tables(rows, row_flags, randomness, rw, rw_flags, bytecode, tx, tx_flags)
    return _verify(lib, lib.zk_copy_verify, t.n_rows, ctypes.byref(t), o | int(opts))


def sign_verify(wire, randomness, is_sig, device=None):
    lib = _lib.init(device)
    t, opts, keep = engine._sign_units({k: _host(wire.get(k)) for k in engine._SIGN_WIRE}, randomness, is_sig)
    return _verify(lib, lib.zk_sign_verify, t.n_units, ctypes.byref(t), opts)


def keccak_table(data, offsets, randomness, mode=0, device=None):
    """zk_keccak_table -> (Result, status, rows uint64[n, 5, 4])"""
    lib = _lib.init(device)
    data, offsets = _host(data, np.uint8), _host(offsets, np.uint64)
    rows = np.zeros((int(offsets.shape[0]) - 1, 5, 4), dtype=np.uint64)
    args, opts, keep = engine._keccak_args(data, offsets, randomness, mode, rows)
    return (*_verify(lib, lib.zk_keccak_table, args[3], *args, opts), rows)


def state_assign(ops, op_flags, device=None):
    """zk_state_assign -> (Result, status, rows uint64[57, n, 4], row_flags uint32[n], mpt uint64[m, 12, 4])"""
    lib = _lib.init(device)
    args, opts, keep = engine._state_assign_args(_host(ops), _host(op_flags))
    n = args[2]
    rows, rflags = np.zeros((57, n, 4), dtype=np.uint64), np.zeros(n, dtype=np.uint32)
    mpt, n_mpt = np.zeros((n, 12, 4), dtype=np.uint64), ctypes.c_uint64()
    status, r = np.zeros(n, dtype=np.uint32), ZkResult()
    check(lib.zk_state_assign(*args, ptr(rows), ptr(rflags), ptr(mpt), ctypes.byref(n_mpt), opts, ptr(status), ctypes.byref(r)), "zk_state_assign", lib)
    return Result(r), status, rows, rflags, mpt[: int(n_mpt.value)]


def _state_ops_from(lib, fn, n, opts, *source):
    """one `fn(*source, ops, op_flags, &n_ops, opts, status, &result)` call over n RW rows or ops (the from-RW and the from-trace form)
    -> (Result, status uint32[n], ops uint64[12, n_ops, 4], op_flags uint32[n_ops])"""
    ops, flags = np.zeros(12 * (n + 1) * 4, dtype=np.uint64), np.zeros(n + 1, dtype=np.uint32)
    status, r, n_ops = np.zeros(n, dtype=np.uint32), ZkResult(), ctypes.c_uint64()
    check(fn(*source, ptr(ops), ptr(flags), ctypes.byref(n_ops), opts, ptr(status), ctypes.byref(r)), fn.__name__, lib)
    m = int(n_ops.value)
    return Result(r), status, ops[: 48 * m].reshape(12, m, 4), flags[:m]


def _state_verify_from(lib, fn, n, opts, *source):
    """one `fn(*source, opts, status, &n_ops, &result)` call over n RW rows or ops -> (Result of the State circuit, status uint32[n_ops])"""
    status, r, n_ops = np.zeros(n + 1, dtype=np.uint32), ZkResult(), ctypes.c_uint64()
    check(fn(*source, opts, ptr(status), ctypes.byref(n_ops), ctypes.byref(r)), fn.__name__, lib)
    return Result(r), status[: int(n_ops.value)]


def state_ops_from_rw(rw, rw_flags, device=None):
    """zk_state_ops_from_rw -> (Result, status uint32[n] per RW row, ops uint64[12, n_ops, 4], op_flags uint32[n_ops])"""
    lib = _lib.init(device)
    args, opts, keep = engine._rw_args(_host(rw), _host(rw_flags, np.uint32))
    return _state_ops_from(lib, lib.zk_state_ops_from_rw, args[2], opts, *args)


def state_verify_from_rw(rw, rw_flags, device=None):
    """zk_state_verify_from_rw -> (Result of the State circuit, status uint32[n_ops] per State row)"""
    lib = _lib.init(device)
    args, opts, keep = engine._rw_args(_host(rw), _host(rw_flags, np.uint32))
    return _state_verify_from(lib, lib.zk_state_verify_from_rw, args[2], opts, *args)


def bytecode_assign(in_rows, offsets, lengths, k, randomness, device=None):
    """zk_bytecode_assign -> (Result, rows uint64[12, 2^k, 4])"""
    lib = _lib.init(device)
    rows, r = np.zeros((12, 1 << int(k), 4), dtype=np.uint64), ZkResult()
    args, opts, keep = engine._bytecode_assign_args(_host(in_rows), _host(offsets, np.uint64), _host(lengths, np.uint64), k, randomness, rows)
    check(lib.zk_bytecode_assign(*args, opts, ctypes.byref(r)), "zk_bytecode_assign", lib)
    return Result(r), rows


def bytecode_from_code(code, offsets, k, randomness, device=None):
    """zk_bytecode_from_code over raw contract code (engine._bytecode_from_code_args) -> (Result, table uint64[n_bytes + n_codes, 6, 4],
    rows uint64[12, 2^k, 4] (None when k == 0), keccak uint64[n_codes, 5, 4])"""
    lib = _lib.init(device)
    x = {"code": _host(code, np.uint8), "offsets": _host(offsets, np.uint64), "k": k}
    res, out = _wire_oneshot(engine.CODE, lib, engine._wire_args(engine.CODE, x, (randomness,)))
    return (res, *(out[name] for name in engine.CODE_OUTPUTS))


def evm_tables_from_block(raw, device=None):
    """zk_evm_tables_from_block over raw block data of host arrays (engine._evm_tables_from_block_args) -> (Result, dict of tx uint64[12 n +
    b, 5, 4], tx_flags, block uint64[8 + h, 4, 4] (no rows without a block), block_flags, withdrawals uint64[m, 4, 4])"""
    lib = _lib.init(device)
    dtypes = {"calldata": np.uint8, "to_is_none": np.uint32, "access_list": np.uint32}
    raw = {k: _host(raw.get(k), dtypes.get(k, np.uint64)) for k in engine.BLOCK_TABLES_INPUTS}
    p = engine._wire_args(engine.BLOCK_TABLES, raw)
    engine._check_block_table_sizes(engine._wire_sizes(engine.BLOCK_TABLES, lib, p), p.shapes)
    return _wire_oneshot(engine.BLOCK_TABLES, lib, p)


def evm_witness_from_trace(trace, device=None):
    """zk_evm_witness_from_trace over trace records of host arrays (engine._evm_witness_from_trace_args, trace.py) -> (Result, dict of rw
    uint64[n, 14, 4], rw_flags uint32[n], steps uint64[k, 13, 4])"""
    lib = _lib.init(device)
    rec = {k: _host(trace.get(k), np.uint32 if k == "head" else np.uint64) for k in engine.TRACE_INPUTS}
    rec["rw_base"] = trace.get("rw_base", 1)
    return _wire_oneshot(engine.TRACE, lib, engine._wire_args(engine.TRACE, rec))


def events_from_trace(trace, codes, code_hashes, device=None):
    """zk_events_from_trace over trace records of host arrays, the code set `codes` and its hashes (engine.trace_event_sources) ->
    (Result over the STEPS, status uint32[n_steps], dict of copy_events uint64[n_copy, 12, 4], copy_flags, copy_src_ref, copy_step
    uint32[n_copy], exp_events uint64[n_exp, 5, 4], exp_step uint32[n_exp])"""
    lib = _lib.init(device)
    x = engine.trace_event_sources(trace, codes, code_hashes)
    dtypes = {"head": np.uint32, "code": np.uint8}
    x = {k: (_host(v, dtypes.get(k, np.uint64)) if k in engine.TRACE_EVENTS_INPUTS else v) for k, v in x.items()}
    res, status, out = _wire_oneshot(engine.TRACE_EVENTS, lib, engine._wire_args(engine.TRACE_EVENTS, x))
    return res, status, engine.cut_trace_events(out, len(out["copy_events"]), len(out["exp_events"]))


def events_from_trace_ext(trace, codes, code_hashes, device=None):
    """zk_events_from_trace_ext: events_from_trace with the copy events of BeginTx, RETURN / REVERT and DATACOPY steps and the extra
    output copy_dst_ref uint32[n_copy]; the copy outputs are sized by one zk_events_from_trace_ext_sizes call in front"""
    lib = _lib.init(device)
    x = engine.trace_event_sources(trace, codes, code_hashes)
    dtypes = {"head": np.uint32, "code": np.uint8}
    x = {k: (_host(v, dtypes.get(k, np.uint64)) if k in engine.TRACE_EVENTS_INPUTS else v) for k, v in x.items()}
    fam = engine.TRACE_EVENTS_EXT
    res, status, out = _wire_oneshot(fam, lib, engine._wire_args(fam, engine._trace_events_ext_sized(lib, x)))
    return res, status, engine.cut_trace_events(out, len(out["copy_events"]), len(out["exp_events"]))


def sha3_from_trace(trace, randomness, device=None):
    """zk_sha3_from_trace over trace records of host arrays -> (Result over the STEPS, status uint32[n_steps], dict of rows
    uint64[n_msgs, 5, 4], step uint32[n_msgs], data uint8[n_bytes], data_offsets uint64[n_msgs + 1]); the outputs are sized by one
    zk_sha3_from_trace_sizes call in front"""
    lib = _lib.init(device)
    fam = engine.TRACE_SHA3
    x = engine._trace_sha3_records(trace)
    x = {k: (_host(v, np.uint32 if k == "head" else np.uint64) if k in engine.TRACE_SHA3_INPUTS else v) for k, v in x.items()}
    x["counts"] = engine._wire_sizes(fam, lib, engine._wire_args(fam, x))
    p = engine._wire_args(fam, x, (int(randomness),))
    out, w = engine._wire_host_outputs(fam, p.shapes)
    status, r = np.zeros(max(p.n, 1), dtype=np.uint32), ZkResult()
    counts = [ctypes.c_uint64(), ctypes.c_uint64()]
    check(lib.zk_sha3_from_trace(ctypes.byref(p.t), ptr(p.keep[-1]), ctypes.byref(w), p.opts, ptr(status), ctypes.byref(counts[0]),
                                 ctypes.byref(counts[1]), ctypes.byref(r)), "zk_sha3_from_trace", lib)
    return Result(r), status[: p.n], out


def _state_trace_records(trace):
    rec = {k: _host(trace.get(k), np.uint32 if k == "head" else np.uint64) for k in engine.TRACE_INPUTS if k != "steps"}
    rec["rw_base"] = trace.get("rw_base", 1)
    return rec


def state_verify_from_trace(trace, device=None):
    """zk_state_verify_from_trace over trace records of host arrays -> (Result of the State circuit, status uint32[n_ops] per State row):
    what state_verify_from_rw returns over evm_witness_from_trace's rw / rw_flags"""
    lib = _lib.init(device)
    t, opts, keep, n = engine._state_from_trace_args(_state_trace_records(trace))
    return _state_verify_from(lib, lib.zk_state_verify_from_trace, n, opts, ctypes.byref(t))


def state_ops_from_trace(trace, device=None):
    """zk_state_ops_from_trace -> (Result, status uint32[n] per RW op, ops uint64[12, n_ops, 4], op_flags uint32[n_ops]): what
    state_ops_from_rw returns over evm_witness_from_trace's rw / rw_flags"""
    lib = _lib.init(device)
    t, opts, keep, n = engine._state_from_trace_args(_state_trace_records(trace))
    return _state_ops_from(lib, lib.zk_state_ops_from_trace, n, opts, ctypes.byref(t))


def state_assign_from_trace(trace, device=None, compact=False):
    """zk_state_assign_from_trace over trace records of host arrays -> (Result, status uint32[n_ops] per op, rows uint64[57, n_ops, 4] (15
    with compact), row_flags uint32[n_ops], mpt uint64[n_mpt, 12, 4]): what a zk_state_assign_from_rw_open session returns over
    evm_witness_from_trace's rw / rw_flags"""
    lib = _lib.init(device)
    t, opts, keep, n = engine._state_from_trace_args(_state_trace_records(trace))
    if compact:
        opts |= _lib.OPT_STATE_COMPACT
    nc = 15 if compact else 57
    rows, rflags = np.zeros(nc * (n + 1) * 4, dtype=np.uint64), np.zeros(n + 1, dtype=np.uint32)
    mpt, n_mpt, n_ops = np.zeros((n + 1, 12, 4), dtype=np.uint64), ctypes.c_uint64(), ctypes.c_uint64()
    status, r = np.zeros(n + 1, dtype=np.uint32), ZkResult()
    check(lib.zk_state_assign_from_trace(ctypes.byref(t), ptr(rows), ptr(rflags), ptr(mpt), ctypes.byref(n_mpt), ctypes.byref(n_ops), opts,
                                         ptr(status), ctypes.byref(r)), "zk_state_assign_from_trace", lib)
    m = int(n_ops.value)
    return Result(r), status[:m], rows[: nc * m * 4].reshape(nc, m, 4), rflags[:m], mpt[: int(n_mpt.value)]


def ecdsa_verify(sig_bytes, v=None, layout=0, v_stride=1, device=None):
    """zk_ecdsa_verify -> (Result, status uint32[n])"""
    lib = _lib.init(device)
    args, opts, keep = engine._ecdsa_args(_host(sig_bytes, np.uint8), _host(v, np.uint32), layout, v_stride)
    return _verify(lib, lib.zk_ecdsa_verify, args[4], *args, opts)


def copy_assign(events, flags, data, offsets, randomness, device=None):
    """zk_copy_assign -> (Result, rows uint64[20, n, 4], row_flags uint32[n], table uint64[m, 14, 4], rw uint64[k, 14, 4], rw_flags)"""
    lib = _lib.init(device)
    t, opts, keep, (n_rows, n_table, n_rw) = engine._copy_assign_args(_host(events), _host(flags, np.uint32), _host(data, np.uint16),
                                                                      _host(offsets, np.uint64), randomness, device)
    rows, rf = np.zeros((20, n_rows, 4), dtype=np.uint64), np.zeros(n_rows, dtype=np.uint32)
    table = np.zeros((n_table, 14, 4), dtype=np.uint64)
    rw, rwf = np.zeros((n_rw, 14, 4), dtype=np.uint64), np.zeros(n_rw, dtype=np.uint32)
    r = ZkResult()
    check(lib.zk_copy_assign(ctypes.byref(t), ptr(rows), ptr(rf), ptr(table, n_table), ptr(rw, n_rw), ptr(rwf, n_rw), opts, ctypes.byref(r)), "zk_copy_assign", lib)
    return Result(r), rows, rf, table, rw, rwf


def copy_assign_from_sources(events, flags, src_ref, dst_ref, sources, randomness, device=None):
    """zk_copy_assign_from_sources over copy events, their refs and `sources` (engine._copy_sources_args) -> (Result over the EVENTS,
    status uint32[n_events], rows, row_flags, table, rw, rw_flags as copy_assign returns them, data uint16[n_data], data_offsets
    uint64[n_events + 1])"""
    lib = _lib.init(device)
    src = {k: _host(sources.get(k)) for k in engine.COPY_SOURCE_KEYS}
    tr = sources.get("trace")
    src["trace"] = None if tr is None else {k: (_host(v) if hasattr(v, "shape") else v) for k, v in tr.items()}
    prepared = engine._copy_sources_args(_host(events), _host(flags, np.uint32), _host(src_ref, np.uint32), _host(dst_ref, np.uint32), src, randomness)
    n_rows, n_table, n_rw, n_data = engine.copy_assign_from_sources_sizes(None, None, None, None, None, device, _prepared=prepared)
    t, opts, keep = prepared
    n = int(t.n_events)
    rows, rf = np.zeros((20, n_rows, 4), dtype=np.uint64), np.zeros(n_rows + 1, dtype=np.uint32)
    table = np.zeros((n_table, 14, 4), dtype=np.uint64)
    rw, rwf = np.zeros((n_rw, 14, 4), dtype=np.uint64), np.zeros(n_rw, dtype=np.uint32)
    data, offsets, status, r = np.zeros(n_data, dtype=np.uint16), np.zeros(n + 1, dtype=np.uint64), np.zeros(n, dtype=np.uint32), ZkResult()
    rows_buf = rows if n_rows else np.zeros((20, 1, 4), dtype=np.uint64)  # (events that copy nothing: the entry still wants its row pointers)
    check(lib.zk_copy_assign_from_sources(ctypes.byref(t), ptr(rows_buf), ptr(rf), ptr(table, n_table), ptr(rw, n_rw), ptr(rwf, n_rw), ptr(data, n_data),
                                          ptr(offsets), opts, ptr(status), ctypes.byref(r)), "zk_copy_assign_from_sources", lib)
    return Result(r), status, rows, rf[:n_rows], table, rw, rwf, data, offsets


def exp_assign(events, max_exp_steps=0, device=None):
    """zk_exp_assign over EXP events uint64[n, 5, 4] -> (Result or None, rows uint64[21, n_rows, 4], table uint64[n_table, 11, 4]);
    events that expand to no row at all give empty arrays without a pass (Result None).  The host buffers of a one-shot have to be
    sized before the call (zk_exp_assign_sizes); a session (engine.open_exp_assign) sizes once."""
    lib = _lib.init(device)
    events = _host(events, np.uint64)
    n_rows, _, n_table = engine.exp_assign_sizes(events, max_exp_steps, device)
    rows, table, r = np.zeros((21, n_rows, 4), dtype=np.uint64), np.zeros((n_table, 11, 4), dtype=np.uint64), ZkResult()
    if n_rows == 0:
        return None, rows, table
    t, opts, keep, _ = engine._exp_assign_args(events, max_exp_steps, device)
    check(lib.zk_exp_assign(ctypes.byref(t), ptr(rows), ptr(table, n_table), opts, ctypes.byref(r)), "zk_exp_assign", lib)
    return Result(r), rows, table


def pi_verify(rows, keccak, gas, circuit_len, keccak_rand=255, byte_pow_base=255, device=None):
    """zk_pi_verify -> (Result, status uint32[n])"""
    lib = _lib.init(device)
    args, opts, keep = engine._pi_args(_host(rows), _host(keccak), _host(gas), circuit_len, keccak_rand, byte_pow_base)
    return _verify(lib, lib.zk_pi_verify, args[1], *args, opts)


def pi_copy_verify(cells, data, lens, device=None):
    """zk_pi_copy_verify over cells uint64[n, 4], data uint8[n, 32], lens uint32[n] -> (Result, status uint32[n])"""
    lib = _lib.init(device)
    args, opts, keep = engine._pi_copy_args(_host(cells), _host(data), _host(lens))
    return _verify(lib, lib.zk_pi_copy_verify, args[3], *args, opts)


def ecc_assign(w, randomness, device=None):
    """zk_ecc_assign over flatten_ecc_ops output -> EccTableRow wire rows uint64[n, 13, 4] (circuit2rows order)"""
    lib = _lib.init(device)
    ops, opts, keep = engine._ecc_ops(w, randomness)
    rows = np.zeros((ops.n_add + ops.n_mul + ops.n_pairing, 13, 4), dtype=np.uint64)
    if rows.shape[0]:
        check(lib.zk_ecc_assign(ctypes.byref(ops), opts, ptr(rows)), "zk_ecc_assign", lib)
    return rows


def ecc_verify(w, rows, randomness, device=None):
    """zk_ecc_verify: the rows against the ops' chips -> (Result, status uint32[n])"""
    lib = _lib.init(device)
    ops, opts, keep = engine._ecc_ops(w, randomness)
    rows = _host(rows)
    _expect(rows, "ecc rows", 8, (ops.n_add + ops.n_mul + ops.n_pairing, 13, 4))
    return _verify(lib, lib.zk_ecc_verify, rows.shape[0], ctypes.byref(ops), ptr(rows), opts)


def withdrawal_verify(w, randomness, device=None):
    """zk_withdrawal_verify over flatten_withdrawal_witness output -> (Result, status uint32[n]); status[j] is global row row_base + j"""
    lib = _lib.init(device)
    ww, opts, keep = engine._withdrawal_witness(w, randomness)
    return _verify(lib, lib.zk_withdrawal_verify, engine._withdrawal_eval_rows(w), ctypes.byref(ww), opts)


def withdrawal_assign(withdrawals, max_withdrawals, randomness, keccak_rows=True, device=None):
    """zk_withdrawal_assign: withdrawals uint64[n, 5, 4] (id, validator_id, address, amount, root) -> (rows uint64[max(n, MAX), 8, 4],
    keccak rows uint64[n, 5, 4] or None)"""
    lib = _lib.init(device)
    wd = _host(withdrawals, np.uint64)
    _expect(wd, "withdrawals", 8, (None, 5, 4))
    n, m = int(wd.shape[0]), int(max_withdrawals)
    rc = _host(_randomness_cells(int(randomness), None))
    rows = np.zeros((max(n, m), 8, 4), dtype=np.uint64)
    kr = np.zeros((n, 5, 4), dtype=np.uint64) if keccak_rows else None
    check(lib.zk_withdrawal_assign(ptr(wd, n), n, m, ptr(rc), 0, ptr(rows, rows.shape[0]), ptr(kr, n)), "zk_withdrawal_assign", lib)
    return rows, kr


def tx_assign(tx, randomness, device=None):
    """zk_tx_assign over raw txs (engine._tx_assign_args) -> (Result, status uint32[n], wire dict: tx_rows, tx_flags, bytes, cells,
    meta, keccak — the arrays flatten_tx_witness makes)"""
    lib = _lib.init(device)
    return _wire_oneshot(engine.TX_ASSIGN, lib, engine._wire_args(engine.TX_ASSIGN, _host_inputs(engine.TX_ASSIGN, tx), (randomness,)))


def sig_assign(sig, randomness, device=None):
    """zk_sig_assign over signed data (engine._sig_assign_args) -> (Result, status uint32[n], wire dict: bytes, cells, meta, keccak,
    sig_table, aux — the units as flatten_sig_witness makes them, the EVM circuit's sig table and its aux rows of kind 5)"""
    lib = _lib.init(device)
    return _wire_oneshot(engine.SIG_ASSIGN, lib, engine._wire_args(engine.SIG_ASSIGN, _host_inputs(engine.SIG_ASSIGN, sig), (randomness,)))


def ecc_from_calls(calls, randomness, device=None):
    """zk_ecc_from_calls over the input words of ecAdd / ecMul / ecPairing calls (engine._ecc_calls_args) -> (Result, status uint32[n],
    wire dict: points, pair_out, rows, ecc_table (cut to its rows), aux, aux_kind)"""
    lib = _lib.init(device)
    return _wire_oneshot(engine.ECC_CALLS, lib, engine._wire_args(engine.ECC_CALLS, _host_inputs(engine.ECC_CALLS, calls), (randomness,)))


def pi_assign(pd, keccak_rand=255, byte_pow_base=255, device=None):
    """zk_pi_assign over raw public data (engine._pi_assign_args) -> (Result, wire dict of engine.PI_ASSIGN_OUTPUTS)"""
    lib = _lib.init(device)
    return _wire_oneshot(engine.PI_ASSIGN, lib, engine._wire_args(engine.PI_ASSIGN, _host_inputs(engine.PI_ASSIGN, pd), (int(keccak_rand), int(byte_pow_base))))
