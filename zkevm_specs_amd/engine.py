"""Session objects over the C ABI: upload once, launch many passes, collect the tally."""
import ctypes
from collections import namedtuple

import numpy as np

from . import _lib
from ._lib import OPT_DEVICE_PTRS, ZkResult, check, ptr
from .errors import exception_for_code


class Result:
    """Outcome of one evaluation pass over all rows (mirrors zk_result)."""

    def __init__(self, r: ZkResult):
        self.fail_count = int(r.fail_count)
        self.first_fail_row = None if r.first_fail_row == 0xFFFFFFFFFFFFFFFF else int(r.first_fail_row)
        self.first_fail_code = int(r.first_fail_code)
        self.first_fail_kind = self.first_fail_code >> 24
        self.first_fail_site = self.first_fail_code & 0xFFFFFF
        self.launches = int(r.launches)
        self.rows_evaluated = int(r.rows_evaluated)
        self.kernel_ms = float(r.kernel_ms)

    @property
    def ok(self):
        return self.fail_count == 0

    def __repr__(self):
        return (f"Result(ok={self.ok}, fail_count={self.fail_count}, first_fail_row={self.first_fail_row}, "
                f"kind={self.first_fail_kind}, site={self.first_fail_site}, kernel_ms={self.kernel_ms:.4f})")


def _is_device(x):
    return hasattr(x, "is_cuda") and x.is_cuda


class Session:
    """RAII wrapper of zk_session*.  Inputs may be numpy arrays (staged to HBM by the library)
    or torch CUDA tensors (used in place; the caller keeps them alive)."""

    def __init__(self, handle, n, keepalive, lib=None):
        self._h = handle
        self.n = n
        self._keep = keepalive
        self._lib = lib if lib is not None else _lib.load()  # the library that opened the session (HIP, or the CPU backend's)

    def launch(self, status_dev=None):
        if status_dev is not None:
            _expect(status_dev, "status_dev", 4, (self.n,))
            if not _is_contiguous(status_dev):
                raise ValueError("status_dev must be contiguous")
        check(self._lib.zk_launch(self._h, ptr(status_dev)), "zk_launch", self._lib)

    def collect(self):
        r = ZkResult()
        check(self._lib.zk_collect(self._h, ctypes.byref(r)), "zk_collect", self._lib)
        return Result(r)

    def run(self):
        self.launch()
        return self.collect()

    def set_stream(self, stream):
        """Bind the session to another HIP stream of its device (a torch.cuda.Stream, a raw handle, or None = the
        engine's own stream); passes already enqueued are waited for first."""
        h = getattr(stream, "cuda_stream", stream)
        check(self._lib.zk_session_set_stream(self._h, ctypes.c_void_p(h) if h else None), "zk_session_set_stream", self._lib)

    def set_range(self, row_lo, row_hi):
        """Row-circuit sessions: evaluate rows [row_lo, row_hi) only (the rest is a read-only halo)."""
        check(self._lib.zk_set_range(self._h, int(row_lo), int(row_hi)), "zk_set_range", self._lib)

    def timing(self):
        """EVM sessions, after a collect: (open_ms, span_ms) — device spans of the open's kernels and of open + first pass"""
        a, b = ctypes.c_double(), ctypes.c_double()
        check(self._lib.zk_session_timing(self._h, ctypes.byref(a), ctypes.byref(b)), "zk_session_timing", self._lib)
        return a.value, b.value

    def read_status(self):
        out = np.empty(self.n, dtype=np.uint32)
        check(self._lib.zk_read_status(self._h, ptr(out)), "zk_read_status", self._lib)
        return out

    def close(self):
        if self._h:
            self._lib.zk_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def _open(lib, fn, n, keep, *args, cls=Session):
    """one `fn(*args, &handle)` call of a zk_*_open entry -> a `cls` session over n rows that keeps the arrays `keep` alive"""
    h = ctypes.c_void_p()
    check(fn(*args, ctypes.byref(h)), fn.__name__, lib)
    return cls(h, n, keep, lib=lib)


def _is_contiguous(a):
    return a.is_contiguous() if hasattr(a, "is_contiguous") else a.flags["C_CONTIGUOUS"]


def _itemsize(a):
    return a.element_size() if hasattr(a, "element_size") else a.dtype.itemsize


def _expect(a, name, itemsize, shape):
    """Wire-format check of one argument: element size (uint64 cells travel as int64 tensors on the device, so the size
    is what is checked, plus 'integer') and shape (None = any extent).  The kernels index these buffers blindly."""
    if a is None:
        return
    kind_ok = (not a.dtype.is_floating_point and not a.dtype.is_complex) if hasattr(a, "is_cuda") else a.dtype.kind in "iu"
    if not kind_ok or _itemsize(a) != itemsize:
        raise TypeError(f"{name}: expected {itemsize}-byte integers, got {a.dtype}")
    if len(a.shape) != len(shape) or any(e is not None and int(d) != e for d, e in zip(a.shape, shape)):
        raise ValueError(f"{name}: expected shape {tuple('n' if e is None else e for e in shape)}, got {tuple(a.shape)}")


def _prep(arrs, outputs=()):
    """Host arrays are made C-contiguous (a copy is fine: they are staged anyway); device tensors are used in place.
    `outputs`: indices of buffers the device WRITES — those must already be contiguous (a silent copy would swallow
    the results)."""
    dev = [_is_device(a) for a in arrs if a is not None]
    if any(dev) and not all(dev):
        raise ValueError("mix of host and device buffers")
    is_dev = bool(dev) and all(dev)
    out = []
    for k, a in enumerate(arrs):
        if a is None:
            out.append(None)
        elif k in outputs:
            if not _is_contiguous(a):
                raise ValueError("output buffer must be contiguous")
            out.append(a)
        elif is_dev:
            out.append(a.contiguous())
        else:
            out.append(np.ascontiguousarray(a))
    return out, (OPT_DEVICE_PTRS if is_dev else 0)


def _randomness_cells(randomness, like):
    """int -> one canonical cell (uint64[4]), on the device when `like` is a CUDA tensor"""
    if not isinstance(randomness, int):
        return randomness
    cells = np.frombuffer(int(randomness).to_bytes(32, "little"), dtype="<u8").copy()
    if _is_device(like):
        import torch

        return torch.from_numpy(cells.view(np.int64)).to(like.device)
    return cells


def _host(x, dtype=None):
    """a C-contiguous host array of `x` (None stays None): the one-shot entries and the host-only argument blocks"""
    return None if x is None else np.ascontiguousarray(x, dtype=dtype)


def _rows(x):
    return 0 if x is None else int(x.shape[0])


def _state_args(rows, flags, mpt, compact=False):
    """zk_state_open / zk_state_verify -> ((rows, flags, n, mpt, m), opts, kept arrays)"""
    _expect(rows, "state rows", 8, (15 if compact else 57, None, 4))
    _expect(flags, "state flags", 4, (rows.shape[1],))
    _expect(mpt, "mpt", 8, (None, 12, 4))
    keep, opts = _prep([rows, flags, mpt])
    rows, flags, mpt = keep
    if compact:
        opts |= _lib.OPT_STATE_COMPACT
    m = _rows(mpt)
    return (ptr(rows), ptr(flags), int(rows.shape[1]), ptr(mpt, m), m), opts, keep


def open_state(rows, flags, mpt, device=None, compact=False):
    """rows uint64[57, n, 4], flags uint32[n], mpt uint64[m, 12, 4] -> Session.  compact: rows uint64[15, n, 4], a device-assigned
    witness without the limb / byte columns (ZK_OPT_STATE_COMPACT, include/zkevm_hip.h)"""
    lib = _lib.init(device)
    args, opts, keep = _state_args(rows, flags, mpt, compact)
    return _open(lib, lib.zk_state_open, args[2], keep, *args, opts)


# cells per row of each zk_evm_tables table (aux: 2 or 12), and the per-row words that go with a table
_EVM_CELLS = {"steps": 13, "rw": 14, "bytecode": 6, "tx": 5, "block": 4, "copy": 14, "keccak": 5, "exp": 11, "withdrawals": 4,
              "sig": 9, "ecc": 13, "aux": None}
_EVM_FLAGS = {"rw_flags": "rw", "tx_flags": "tx", "block_flags": "block", "aux_kind": "steps"}
_EVM_WIRE = list(_EVM_CELLS) + list(_EVM_FLAGS)


def _evm_tables(wire, begin_with_first_step, end_with_last_step):
    """wire dict -> (ZkEvmTables, opts, kept arrays, n_pairs); host arrays are made contiguous, device tensors are used in place"""
    for k, nc in _EVM_CELLS.items():
        _expect(wire.get(k), k, 8, (None, nc, 4))
    for k, of in _EVM_FLAGS.items():
        if wire.get(k) is not None and wire.get(of) is not None:
            _expect(wire[k], k, 4, (wire[of].shape[0],))
    arrs, opts = _prep([wire.get(k) for k in _EVM_WIRE])
    a = dict(zip(_EVM_WIRE, arrs))
    return _evm_struct(a, begin_with_first_step, end_with_last_step), opts, arrs, int(a["steps"].shape[0]) - 1


def _evm_struct(a, begin_with_first_step=False, end_with_last_step=False):
    """the ZkEvmTables block over prepared wire arrays `a`: a table that is missing from the dict or empty is a null pointer"""
    n = {k: _rows(a.get(k)) for k in _EVM_CELLS}
    return _lib.ZkEvmTables(
        ptr(a["steps"]), n["steps"], ptr(a.get("rw"), n["rw"]), ptr(a.get("rw_flags"), n["rw"]), n["rw"],
        ptr(a.get("bytecode"), n["bytecode"]), n["bytecode"], ptr(a.get("tx"), n["tx"]), ptr(a.get("tx_flags"), n["tx"]), n["tx"],
        ptr(a.get("block"), n["block"]), ptr(a.get("block_flags"), n["block"]), n["block"],
        int(bool(begin_with_first_step)), int(bool(end_with_last_step)),
        ptr(a.get("copy"), n["copy"]), n["copy"], ptr(a.get("keccak"), n["keccak"]), n["keccak"], ptr(a.get("exp"), n["exp"]), n["exp"],
        ptr(a.get("aux"), n["aux"]), ptr(a.get("aux_kind"), n["aux"]),
        ptr(a.get("withdrawals"), n["withdrawals"]), n["withdrawals"], ptr(a.get("sig"), n["sig"]), n["sig"],
        ptr(a.get("ecc"), n["ecc"]), n["ecc"], int(a["aux"].shape[1]) if n["aux"] else 0, 0)


def open_evm(wire, begin_with_first_step=False, end_with_last_step=False, device=None, state_sort=True,
             generic_index=False, side_stream=False, single_pass=False):
    """wire: dict with steps uint64[n, 13, 4] (row-major), rw/rw_flags, bytecode, tx/tx_flags, block/block_flags
    and optionally copy uint64[m, 14, 4], keccak uint64[m, 5, 4], exp uint64[m, 11, 4], sig uint64[m, 9, 4], ecc uint64[m, 13, 4],
    aux uint64[n, 2 or 12, 4] + aux_kind, withdrawals uint64[m, 4, 4]
    (numpy arrays or torch CUDA tensors) -> Session over the n-1 step pairs."""
    lib = _lib.init(device)
    t, opts, arrs, n_pairs = _evm_tables(wire, begin_with_first_step, end_with_last_step)
    if not state_sort:
        opts |= _lib.OPT_NO_STATE_SORT
    if generic_index:
        opts |= _lib.OPT_GENERIC_INDEX
    if single_pass:  # the session will evaluate ONE pass: skip the packed step records (ZK_OPT_SINGLE_PASS, include/zkevm_hip.h)
        opts |= _lib.OPT_SINGLE_PASS
    if side_stream:  # warm / cold launches beside the hot one: pays when other sessions' passes share the device (include/zkevm_hip.h)
        opts |= _lib.OPT_SIDE_STREAM
    return _open(lib, lib.zk_evm_open, n_pairs, arrs, ctypes.byref(t), opts)


def evm_verify(wire, begin_with_first_step=False, end_with_last_step=False, status_dev=None, device=None):
    """The one-shot C entry zk_evm_verify (open + one pass + collect + close) over a wire dict of host arrays or of torch
    CUDA tensors (then status_dev, an optional CUDA uint32[n - 1] tensor, receives the per-pair status) -> Result."""
    call = EvmOneShot(wire, begin_with_first_step, end_with_last_step, status_dev, device)
    call()
    return call.result()


class EvmOneShot:
    """A prepared call of the one-shot C entry `zk_evm_verify` over a resident wire dict: the argument block is marshalled
    once, `__call__` is the C call alone (what a foreign caller of the ABI pays — bench.py's timed region)."""

    def __init__(self, wire, begin_with_first_step=False, end_with_last_step=False, status_dev=None, device=None):
        self._lib = _lib.init(device)
        self._t, self._opts, self._keep, self.n_pairs = _evm_tables(wire, begin_with_first_step, end_with_last_step)
        if status_dev is not None:
            _expect(status_dev, "status_dev", 4, (self.n_pairs,))
        self._status = status_dev
        self._status_ptr = ptr(status_dev)
        self._r = ZkResult()
        self._tref, self._rref = ctypes.byref(self._t), ctypes.byref(self._r)

    def __call__(self):
        rc = self._lib.zk_evm_verify(self._tref, self._opts, self._status_ptr, self._rref)
        if rc:
            check(rc, "zk_evm_verify", self._lib)
        return self._r

    def result(self):
        return Result(self._r)


class EvmBatch:
    """A prepared call of `zk_evm_verify_batch` over resident wire dicts (the witness list may name the same dict several times):
    n independent verifications, software-pipelined two deep by the library."""

    def __init__(self, wires, order, device=None, flags=None):
        """`flags`: per wire, (begin_with_first_step, end_with_last_step) — carried in each witness's own argument block"""
        self._lib = _lib.init(device)
        flags = flags if flags is not None else [(False, False)] * len(wires)
        prepared = [_evm_tables(w, bool(f[0]), bool(f[1])) for w, f in zip(wires, flags)]
        self._keep = prepared
        self._opts = prepared[0][1]
        # one `opts` word goes to the library for the whole batch: host and device wires (ZK_OPT_DEVICE_PTRS) cannot be mixed
        if any(p[1] != self._opts for p in prepared):
            raise ValueError("EvmBatch: every witness must be prepared with the same options (all host arrays or all device tensors)")
        self.n = len(order)
        self.n_pairs = prepared[0][3]                    # of the first witness (kept for callers of the equal-size case)
        self.n_pairs_each = [prepared[k][3] for k in order]  # per witness, in call order
        arr_t = ctypes.POINTER(_lib.ZkEvmTables) * self.n
        self._ptrs = arr_t(*[ctypes.pointer(prepared[k][0]) for k in order])
        self._results = (ZkResult * self.n)()

    def __call__(self):
        rc = self._lib.zk_evm_verify_batch(self._ptrs, self.n, self._opts, self._results)
        if rc:
            check(rc, "zk_evm_verify_batch", self._lib)
        return self._results

    def results(self):
        return [Result(r) for r in self._results]


def last_timing(lib=None):
    """(open_ms, pass_ms, span_ms) of the calling thread's last one-shot zk_evm_verify (device spans by HIP events; -1 = not measured)"""
    lib = lib if lib is not None else _lib.load()
    a, b, c = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    lib.zk_last_timing(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
    return a.value, b.value, c.value


def _bytecode_args(rows, keccak, randomness):
    """zk_bytecode_open / zk_bytecode_verify -> ((rows, n, keccak, m, randomness), opts, kept arrays)"""
    randomness = _randomness_cells(randomness, rows)
    _expect(rows, "bytecode rows", 8, (12, None, 4))
    _expect(keccak, "keccak", 8, (None, 5, 4))
    _expect(randomness, "randomness", 8, (4,))
    keep, opts = _prep([rows, keccak, randomness])
    rows, keccak, randomness = keep
    m = _rows(keccak)
    return (ptr(rows), int(rows.shape[1]), ptr(keccak, m), m, ptr(randomness)), opts, keep


def open_bytecode(rows, keccak, randomness, device=None):
    """rows uint64[12, n, 4], keccak uint64[m, 5, 4], randomness uint64[4] (or an int) -> Session"""
    lib = _lib.init(device)
    args, opts, keep = _bytecode_args(rows, keccak, randomness)
    return _open(lib, lib.zk_bytecode_open, args[1], keep, *args, opts)


def _exp_args(rows):
    """zk_exp_open / zk_exp_verify -> ((rows, n), opts, kept arrays)"""
    _expect(rows, "exp rows", 8, (21, None, 4))
    keep, opts = _prep([rows])
    return (ptr(keep[0]), int(keep[0].shape[1])), opts, keep


def open_exp(rows, device=None):
    """rows uint64[21, n, 4] -> Session"""
    lib = _lib.init(device)
    args, opts, keep = _exp_args(rows)
    return _open(lib, lib.zk_exp_open, args[1], keep, *args, opts)


def _copy_tables(rows, row_flags, randomness, rw, rw_flags, bytecode, tx, tx_flags):
    """zk_copy_open / zk_copy_verify -> (ZkCopyTables, opts, kept arrays)"""
    randomness = _randomness_cells(randomness, rows)
    _expect(rows, "copy rows", 8, (20, None, 4))
    _expect(row_flags, "copy row_flags", 4, (rows.shape[1],))
    _expect(rw, "rw", 8, (None, 14, 4))
    _expect(bytecode, "bytecode", 8, (None, 6, 4))
    _expect(tx, "tx", 8, (None, 5, 4))
    keep, opts = _prep([rows, row_flags, randomness, rw, rw_flags, bytecode, tx, tx_flags])
    rows, row_flags, randomness, rw, rw_flags, bytecode, tx, tx_flags = keep
    n_rw, n_bc, n_tx = _rows(rw), _rows(bytecode), _rows(tx)
    t = _lib.ZkCopyTables(ptr(rows), ptr(row_flags), int(rows.shape[1]), ptr(randomness), ptr(rw, n_rw), ptr(rw_flags, n_rw), n_rw,
                          ptr(bytecode, n_bc), n_bc, ptr(tx, n_tx), ptr(tx_flags, n_tx), n_tx)
    return t, opts, keep


def open_copy(rows, row_flags, randomness, rw, rw_flags, bytecode, tx, tx_flags, device=None, generic_index=False):
    """Copy circuit session: rows uint64[20, n, 4] + flags, randomness (int or uint64[4]), EVM-format tables."""
    lib = _lib.init(device)
    t, opts, keep = _copy_tables(rows, row_flags, randomness, rw, rw_flags, bytecode, tx, tx_flags)
    if generic_index:
        opts |= _lib.OPT_GENERIC_INDEX
    return _open(lib, lib.zk_copy_open, int(t.n_rows), keep, ctypes.byref(t), opts)


_SIGN_WIRE = ("bytes", "cells", "meta", "keccak", "tx_rows", "tx_flags")


def _sign_units(wire, randomness, is_sig):
    """zk_sign_open / zk_sign_verify over `wire` = dict(bytes, cells, meta, keccak, tx_rows, tx_flags) -> (ZkSignUnits, opts, kept arrays)"""
    randomness = _randomness_cells(randomness, wire.get("bytes"))
    _expect(wire.get("bytes"), "sign bytes", 1, (None, 9, 32))
    _expect(wire.get("cells"), "sign cells", 8, (8, wire["bytes"].shape[0], 4))
    _expect(wire.get("meta"), "sign meta", 4, (wire["bytes"].shape[0], 4))
    _expect(wire.get("keccak"), "keccak", 8, (None, 5, 4))
    _expect(wire.get("tx_rows"), "tx_rows", 8, (None, 5, 4))
    keep, opts = _prep([wire.get(k) for k in _SIGN_WIRE] + [randomness])
    return _sign_struct(dict(zip(_SIGN_WIRE, keep)), keep[-1], is_sig), opts, keep


def _sign_struct(a, randomness, is_sig):
    """the ZkSignUnits block over prepared arrays `a` (by _SIGN_WIRE name): an empty keccak or tx table is a null pointer"""
    n_k, n_tx = _rows(a["keccak"]), _rows(a["tx_rows"])
    return _lib.ZkSignUnits(ptr(a["bytes"]), ptr(a["cells"]), ptr(a["meta"]), _rows(a["bytes"]), ptr(randomness), ptr(a["keccak"], n_k), n_k,
                            ptr(a["tx_rows"], n_tx), ptr(a["tx_flags"], n_tx), n_tx, int(bool(is_sig)))


def open_sign(wire, randomness, is_sig, device=None):
    """Tx / Sig circuit session over `wire` = dict(bytes, cells, meta, keccak, tx_rows, tx_flags)."""
    lib = _lib.init(device)
    t, opts, keep = _sign_units(wire, randomness, is_sig)
    return _open(lib, lib.zk_sign_open, int(t.n_units), keep, ctypes.byref(t), opts)


KECCAK_MODE_CIRCUIT = 0  # KeccakCircuit.add rows (EVM / bytecode circuits)
KECCAK_MODE_TABLE = 1    # KeccakTable.add rows (Tx / Sig circuits)


class KeccakSession(Session):
    """Keccak-table generation session: launch()/collect() like the circuits, rows() for the table."""

    def rows(self):
        out = np.empty((self.n, 5, 4), dtype=np.uint64)
        check(self._lib.zk_keccak_read_rows(self._h, ptr(out)), "zk_keccak_read_rows", self._lib)
        return out


def pack_messages(messages):
    """list of bytes -> (data uint8[total], offsets uint64[n + 1])"""
    offsets = np.zeros(len(messages) + 1, dtype=np.uint64)
    if len(messages):
        offsets[1:] = np.cumsum([len(m) for m in messages], dtype=np.uint64)
    data = np.frombuffer(b"".join(bytes(m) for m in messages), dtype=np.uint8).copy()
    return data, offsets


def _keccak_args(data, offsets, randomness, mode, rows_out=None):
    """zk_keccak_open / zk_keccak_table -> ((data, n_bytes, offsets, n, randomness, mode, rows_out), opts, kept arrays); rows_out:
    uint64[n, 5, 4] receiving the rows (optional for a session)"""
    randomness = _randomness_cells(randomness, data)
    _expect(data, "keccak data", 1, (None,))
    _expect(offsets, "keccak offsets", 8, (None,))
    _expect(rows_out, "keccak rows_dev", 8, (int(offsets.shape[0]) - 1, 5, 4))
    keep, opts = _prep([data, offsets, randomness, rows_out], outputs=(3,))
    data, offsets, randomness, rows_out = keep
    n_bytes = _rows(data)
    return (ptr(data, n_bytes), n_bytes, ptr(offsets), int(offsets.shape[0]) - 1, ptr(randomness), int(mode), ptr(rows_out)), opts, keep


def open_keccak(data, offsets, randomness, mode=KECCAK_MODE_CIRCUIT, rows_dev=None, device=None):
    """data uint8[total], offsets uint64[n + 1], randomness (int or uint64[4]) -> KeccakSession.
    numpy arrays are staged to HBM; torch CUDA tensors are used in place (rows_dev: optional
    CUDA uint64[n, 5, 4] tensor receiving the rows)."""
    lib = _lib.init(device)
    args, opts, keep = _keccak_args(data, offsets, randomness, mode, rows_dev)
    return _open(lib, lib.zk_keccak_open, args[3], keep, *args, opts, cls=KeccakSession)


def keccak_table(messages, randomness, mode=KECCAK_MODE_CIRCUIT, device=None):
    """Keccak table rows uint64[n, 5, 4] of a list of byte strings, computed on the GPU
    (replaces KeccakCircuit.add / KeccakTable.add loops; see include/zkevm_hip.h).  Raises the
    reference's ValueError for a mode-1 input longer than 64 bytes."""
    if len(messages) == 0:
        return np.zeros((0, 5, 4), dtype=np.uint64)
    data, offsets = pack_messages(messages)
    with open_keccak(data, offsets, randomness, mode, device=device) as s:
        res = s.run()
        if not res.ok:
            raise exception_for_code(res.first_fail_code, f"keccak table: message {res.first_fail_row}")
        return s.rows()


class AssignSession(Session):
    """State-witness assignment session: launch()/collect() like the circuits; n_mpt()/read() for the outputs."""

    def n_mpt(self):
        m = ctypes.c_uint64()
        check(self._lib.zk_state_assign_read(self._h, None, None, None, 0, ctypes.byref(m)), "zk_state_assign_read", self._lib)
        return int(m.value)

    compact = False

    def read(self):
        """-> (rows uint64[57, n, 4] (15 with compact), flags uint32[n], mpt uint64[m, 12, 4]) on the host"""
        m = self.n_mpt()
        rows = np.empty((15 if self.compact else 57, self.n, 4), dtype=np.uint64)
        flags = np.empty(self.n, dtype=np.uint32)
        mpt = np.empty((m, 12, 4), dtype=np.uint64)
        got = ctypes.c_uint64()
        check(self._lib.zk_state_assign_read(self._h, ptr(rows), ptr(flags), ptr(mpt, m), m, ctypes.byref(got)), "zk_state_assign_read", self._lib)
        return rows, flags, mpt


def _state_assign_args(ops, op_flags, outs=(None, None, None), compact=False):
    """zk_state_assign_open / zk_state_assign -> ((ops, op_flags, n), opts, kept arrays); outs: a session's (rows_dev,
    row_flags_dev, mpt_dev), prepared with the inputs (kept arrays 2..4)"""
    _expect(ops, "state ops", 8, (12, None, 4))
    n = int(ops.shape[1])
    _expect(op_flags, "op_flags", 4, (n,))
    rows_dev, row_flags_dev, mpt_dev = outs
    _expect(rows_dev, "rows_dev", 8, (15 if compact else 57, n, 4))
    _expect(row_flags_dev, "row_flags_dev", 4, (n,))
    _expect(mpt_dev, "mpt_dev", 8, (n, 12, 4))
    keep, opts = _prep([ops, op_flags, *outs], outputs=(2, 3, 4))
    if compact:
        opts |= _lib.OPT_STATE_COMPACT
    return (ptr(keep[0]), ptr(keep[1]), n), opts, keep


def open_state_assign(ops, op_flags, rows_dev=None, row_flags_dev=None, mpt_dev=None, device=None, compact=False):
    """ops uint64[12, n, 4] (column-major Operation slots, include/zkevm_hip.h), op_flags uint32[n] -> AssignSession.
    numpy inputs are staged to HBM; torch CUDA tensors are used in place, and rows_dev uint64[57, n, 4] /
    row_flags_dev uint32[n] / mpt_dev uint64[n, 12, 4] (optional CUDA tensors) then receive the outputs, ready
    to be handed to open_state()."""
    lib = _lib.init(device)
    args, opts, keep = _state_assign_args(ops, op_flags, (rows_dev, row_flags_dev, mpt_dev), compact)
    s = _open(lib, lib.zk_state_assign_open, args[2], keep, *args, ptr(keep[2]), ptr(keep[3]), ptr(keep[4]), opts, cls=AssignSession)
    s.compact = bool(compact)
    return s


def _check_flat_outs(outs, n):
    """flat output buffers of a from-RW / from-trace State session, as (buffer or None, name, itemsize, entries per RW row): each holds
    room for the n RW rows + StartOp"""
    for buf, name, size, per_row in outs:
        _expect(buf, name, size, (None,))
        if buf is not None and int(buf.shape[0]) < per_row * (n + 1):
            raise ValueError(f"{name} holds fewer than {per_row * (n + 1)} entries")


def _open_n_ops(lib, fn, keep, *args, cls=Session, n=None, compact=None):
    """one `fn(*args, &n_ops, &handle)` call of a from-RW / from-trace State entry -> a `cls` session over the n_ops = 1 + kept rows State
    rows; with `n` (the op-list sessions, whose status is per RW row) over n rows, n_ops set on it; `compact`: set on an AssignSession"""
    h, n_ops = ctypes.c_void_p(), ctypes.c_uint64()
    check(fn(*args, ctypes.byref(n_ops), ctypes.byref(h)), fn.__name__, lib)
    s = cls(h, int(n_ops.value) if n is None else n, keep, lib=lib)
    if n is not None:
        s.n_ops = int(n_ops.value)
    if compact is not None:
        s.compact = bool(compact)
    return s


def _rw_args(rw, rw_flags, outs=()):
    """zk_state_ops_from_rw* / zk_state_assign_from_rw_open / zk_state_verify_from_rw* -> ((rw, rw_flags, n), opts, kept arrays);
    outs: a session's flat output buffers as (buffer, name, itemsize, entries per RW row + 1), prepared with the inputs"""
    _expect(rw, "rw table", 8, (None, 14, 4))
    n = int(rw.shape[0])
    _expect(rw_flags, "rw_flags", 4, (n,))
    _check_flat_outs(outs, n)
    keep, opts = _prep([rw, rw_flags] + [o[0] for o in outs], outputs=range(2, 2 + len(outs)))
    return (ptr(keep[0]), ptr(keep[1]), n), opts, keep


def open_state_assign_from_rw(rw, rw_flags, rows_dev=None, row_flags_dev=None, mpt_dev=None, device=None, compact=False):
    """rw uint64[n, 14, 4] + rw_flags uint32[n] (the EVM circuit's RW table) -> AssignSession over the n_ops = 1 + kept rows State
    rows (session.n): re-keying + sort + witness assignment in one session, the op list never materialised
    (zk_state_assign_from_rw_open).  With CUDA tensors, rows_dev / row_flags_dev / mpt_dev are FLAT buffers of capacity
    57 * (n + 1) * 4 / n + 1 / (n + 1) * 12 * 4 receiving the outputs packed for n_ops: rows_dev[: 57 * n_ops * 4].view(57, n_ops, 4)
    etc. are what open_state takes."""
    lib = _lib.init(device)
    outs = ((rows_dev, "rows_dev", 8, (15 if compact else 57) * 4), (row_flags_dev, "row_flags_dev", 4, 1), (mpt_dev, "mpt_dev", 8, 48))
    args, opts, keep = _rw_args(rw, rw_flags, outs)
    if compact:
        opts |= _lib.OPT_STATE_COMPACT
    return _open_n_ops(lib, lib.zk_state_assign_from_rw_open, keep, *args, ptr(keep[2]), ptr(keep[3]), ptr(keep[4]), opts, cls=AssignSession,
                       compact=compact)


def open_state_verify_from_rw(rw, rw_flags, device=None):
    """rw uint64[n, 14, 4] + rw_flags uint32[n] (the EVM circuit's RW table) -> Session over the n_ops = 1 + kept rows State rows
    (session.n), which are evaluated where they are computed and never stored (zk_state_verify_from_rw_open): collect() is the State
    circuit's Result; an RW row the re-keying rejects or an op the assignment raises on makes collect() raise EngineError."""
    lib = _lib.init(device)
    args, opts, keep = _rw_args(rw, rw_flags)
    return _open_n_ops(lib, lib.zk_state_verify_from_rw_open, keep, *args, opts)


class RekeySession(Session):
    """RW table -> State-circuit operations (zk_state_ops_from_rw_*): launch()/collect() like the circuits (status = one code per
    RW row); n_ops = StartOp + the rows kept; read() -> (ops uint64[12, n_ops, 4], op_flags uint32[n_ops]) on the host."""

    n_ops = 0

    def read(self):
        ops = np.empty((12, self.n_ops, 4), dtype=np.uint64)
        flags = np.empty(self.n_ops, dtype=np.uint32)
        check(self._lib.zk_state_ops_from_rw_read(self._h, ptr(ops), ptr(flags), None), "zk_state_ops_from_rw_read", self._lib)
        return ops, flags


def open_state_ops_from_rw(rw, rw_flags, ops_dev=None, op_flags_dev=None, device=None):
    """rw uint64[n, 14, 4] + rw_flags uint32[n] (the EVM circuit's RW table) -> RekeySession.  numpy inputs are staged to HBM;
    torch CUDA tensors are used in place, and ops_dev (a flat CUDA buffer of at least 12 * (n + 1) * 4 uint64) / op_flags_dev
    (n + 1 uint32) then receive the op list packed for session.n_ops ops: ops_dev[: 12 * n_ops * 4].view(12, n_ops, 4) is what
    open_state_assign takes."""
    lib = _lib.init(device)
    args, opts, keep = _rw_args(rw, rw_flags, ((ops_dev, "ops_dev", 8, 48), (op_flags_dev, "op_flags_dev", 4, 1)))
    return _open_n_ops(lib, lib.zk_state_ops_from_rw_open, keep, *args, ptr(keep[2]), ptr(keep[3]), opts, cls=RekeySession, n=args[2])


class BytecodeAssignSession(Session):
    """Bytecode-witness assignment session: launch()/collect() like the circuits; rows() for the 2^k circuit rows."""

    def rows(self):
        out = np.empty((12, self.n, 4), dtype=np.uint64)
        check(self._lib.zk_bytecode_assign_read(self._h, ptr(out)), "zk_bytecode_assign_read", self._lib)
        return out


def _bytecode_assign_args(in_rows, offsets, lengths, k, randomness, rows_out=None):
    """zk_bytecode_assign_open / zk_bytecode_assign -> ((in_rows, n_rows, offsets, lengths, n_codes, k, randomness, rows_out), opts,
    kept arrays); rows_out: uint64[12, 2^k, 4] receiving the circuit rows (optional for a session)"""
    randomness = _randomness_cells(randomness, in_rows)
    _expect(in_rows, "unrolled bytecode rows", 8, (None, 6, 4))
    _expect(offsets, "offsets", 8, (int(lengths.shape[0]) + 1,))
    _expect(lengths, "lengths", 8, (None,))
    _expect(rows_out, "rows_dev", 8, (12, 1 << int(k), 4))
    keep, opts = _prep([in_rows, offsets, lengths, randomness, rows_out], outputs=(4,))
    in_rows, offsets, lengths, randomness, rows_out = keep
    n_rows, n_codes = _rows(in_rows), _rows(lengths)
    return (ptr(in_rows, n_rows), n_rows, ptr(offsets), ptr(lengths, n_codes), n_codes, int(k), ptr(randomness), ptr(rows_out)), opts, keep


def open_bytecode_assign(in_rows, offsets, lengths, k, randomness, rows_dev=None, device=None):
    """in_rows uint64[n, 6, 4] (unrolled BytecodeTableRows, input order), offsets uint64[m + 1], lengths uint64[m], k,
    randomness (int or uint64[4]) -> BytecodeAssignSession over the 2^k circuit rows; rows_dev: optional CUDA tensor
    uint64[12, 2^k, 4] receiving them in place (ready for open_bytecode)."""
    lib = _lib.init(device)
    args, opts, keep = _bytecode_assign_args(in_rows, offsets, lengths, k, randomness, rows_dev)
    return _open(lib, lib.zk_bytecode_assign_open, 1 << int(k), keep, *args, opts, cls=BytecodeAssignSession)


def _pi_args(rows, keccak, gas, circuit_len, keccak_rand, byte_pow_base):
    """zk_pi_open / zk_pi_verify -> ((rows, n, keccak, m, gas, k, circuit_len, keccak_rand, byte_pow_base), opts, kept arrays)"""
    kr, bp = _randomness_cells(int(keccak_rand), rows), _randomness_cells(int(byte_pow_base), rows)
    _expect(rows, "pi rows", 8, (24, None, 4))
    _expect(keccak, "keccak", 8, (None, 5, 4))
    _expect(gas, "gas-cost table", 8, (None, 3, 4))
    keep, opts = _prep([rows, keccak, gas, kr, bp])
    rows, keccak, gas, kr, bp = keep
    m, k = _rows(keccak), _rows(gas)
    return (ptr(rows), int(rows.shape[1]), ptr(keccak, m), m, ptr(gas, k), k, int(circuit_len), ptr(kr), ptr(bp)), opts, keep


def open_pi(rows, keccak, gas, circuit_len, keccak_rand=255, byte_pow_base=255, device=None):
    """Public-inputs circuit session: rows uint64[24, n, 4], keccak uint64[m, 5, 4], gas uint64[k, 3, 4] (include/zkevm_hip.h)"""
    lib = _lib.init(device)
    args, opts, keep = _pi_args(rows, keccak, gas, circuit_len, keccak_rand, byte_pow_base)
    return _open(lib, lib.zk_pi_open, args[1], keep, *args, opts)


def _pi_copy_args(cells, data, lens):
    """zk_pi_copy_verify -> ((cells, data, lens, n), opts, kept arrays)"""
    _expect(cells, "pi copy cells", 8, (None, 4))
    _expect(data, "pi copy bytes", 1, (cells.shape[0], 32))
    _expect(lens, "pi copy lens", 4, (cells.shape[0],))
    keep, opts = _prep([cells, data, lens])
    cells, data, lens = keep
    return (ptr(cells), ptr(data), ptr(lens), int(cells.shape[0])), opts, keep


def _copy_events_struct(events, flags, data, offsets, randomness):
    """the ZkCopyEvents block over prepared arrays: empty source data is a null pointer"""
    return _lib.ZkCopyEvents(ptr(events), ptr(flags), int(events.shape[0]), ptr(data, _rows(data)), ptr(offsets), ptr(randomness))


def copy_assign_sizes(events, flags, data, offsets, device=None):
    """(n_rows, n_table, n_rw) a list of copy events expands to (host arithmetic over the events)"""
    lib = _lib.init(device)
    _expect(events, "copy events", 8, (None, 12, 4))
    (events, flags, data, offsets), opts = _prep([events, flags, data, offsets])
    t = _copy_events_struct(events, flags, data, offsets, None)
    a, b, c = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    check(lib.zk_copy_assign_sizes(ctypes.byref(t), opts, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)), "zk_copy_assign_sizes", lib)
    return int(a.value), int(b.value), int(c.value)


def _copy_assign_args(events, flags, data, offsets, randomness, device, outs=(None,) * 5):
    """zk_copy_assign_open / zk_copy_assign -> (ZkCopyEvents, opts, kept arrays, (n_rows, n_table, n_rw)); outs: a session's
    (rows_dev, row_flags_dev, table_dev, rw_dev, rw_flags_dev), checked against the sizes and prepared with the inputs (kept arrays 5..9)"""
    randomness = _randomness_cells(randomness, events)
    _expect(events, "copy events", 8, (None, 12, 4))
    _expect(flags, "copy event flags", 4, (events.shape[0],))
    _expect(data, "copy source data", 2, (None,))
    _expect(offsets, "copy data offsets", 8, (int(events.shape[0]) + 1,))
    sizes = n_rows, n_table, n_rw = copy_assign_sizes(events, flags, data, offsets, device)
    rows_dev, row_flags_dev, table_dev, rw_dev, rw_flags_dev = outs
    _expect(rows_dev, "rows_dev", 8, (20, n_rows, 4))
    _expect(row_flags_dev, "row_flags_dev", 4, (n_rows,))
    _expect(table_dev, "table_dev", 8, (n_table, 14, 4))
    _expect(rw_dev, "rw_dev", 8, (n_rw, 14, 4))
    _expect(rw_flags_dev, "rw_flags_dev", 4, (n_rw,))
    keep, opts = _prep([events, flags, data, offsets, randomness, *outs], outputs=(5, 6, 7, 8, 9))
    return _copy_events_struct(*keep[:5]), opts, keep, sizes


class CopyAssignSession(Session):
    """Copy-circuit witness assignment session: launch()/collect() like the circuits; read() for the outputs."""

    def read(self):
        """-> (rows uint64[20, n, 4], row_flags uint32[n], table uint64[m, 14, 4], rw uint64[k, 14, 4], rw_flags uint32[k]) on the host"""
        rows, rf = np.empty((20, self.n, 4), dtype=np.uint64), np.empty(self.n, dtype=np.uint32)
        table = np.empty((self.n_table, 14, 4), dtype=np.uint64)
        rw, rwf = np.empty((self.n_rw, 14, 4), dtype=np.uint64), np.empty(self.n_rw, dtype=np.uint32)
        check(self._lib.zk_copy_assign_read(self._h, ptr(rows), ptr(rf), ptr(table, self.n_table), ptr(rw, self.n_rw), ptr(rwf, self.n_rw)),
              "zk_copy_assign_read", self._lib)
        return rows, rf, table, rw, rwf


def open_copy_assign(events, flags, data, offsets, randomness, rows_dev=None, row_flags_dev=None, table_dev=None, rw_dev=None,
                     rw_flags_dev=None, device=None):
    """events uint64[n, 12, 4] (row-major copy events, include/zkevm_hip.h), flags uint32[n], data uint16[total], offsets
    uint64[n + 1], randomness (int or uint64[4]) -> CopyAssignSession.  numpy inputs are staged to HBM; torch CUDA tensors are
    used in place and the optional *_dev tensors (sized with copy_assign_sizes) receive the outputs, ready for open_copy /
    open_evm."""
    lib = _lib.init(device)
    t, opts, keep, (n_rows, n_table, n_rw) = _copy_assign_args(events, flags, data, offsets, randomness, device,
                                                               (rows_dev, row_flags_dev, table_dev, rw_dev, rw_flags_dev))
    s = _open(lib, lib.zk_copy_assign_open, n_rows, keep, ctypes.byref(t), *(ptr(x) for x in keep[5:]), opts, cls=CopyAssignSession)
    s.n_table, s.n_rw = n_table, n_rw
    return s


# ---- Copy-circuit witness assignment from raw sources (zk_copy_assign_from_sources*) ---------------------------------------------------
COPY_SOURCE_KEYS = ("code", "code_offsets", "calldata", "calldata_offsets")
_COPY_TRACE_KEYS = ("head", "id", "addr", "val", "rw_counter")


def _copy_sources_args(events, flags, src_ref, dst_ref, sources, randomness, outs=(None,) * 6):
    """zk_copy_assign_from_sources* -> (ZkCopySources, opts, kept arrays).  `sources` = dict(code uint8[], code_offsets uint64[n_codes + 1],
    calldata uint8[], calldata_offsets uint64[n_txs + 1], trace = the RW half of a records dict (head, id, addr, val, rw_counter or None
    with rw_base; see _evm_witness_from_trace_args) or None), each optional: a block without contract code, calldata or memory copies
    leaves it out.  outs: a session's (rows_dev, row_flags_dev, table_dev, rw_dev, rw_flags_dev, data_dev), prepared with the inputs."""
    randomness = _randomness_cells(randomness, events)
    n = int(events.shape[0])
    _expect(events, "copy events", 8, (None, 12, 4))
    _expect(flags, "copy event flags", 4, (n,))
    _expect(src_ref, "src_ref", 4, (n,))
    _expect(dst_ref, "dst_ref", 4, (n,))
    if src_ref is None:
        raise ValueError("src_ref: missing")
    _expect(sources.get("code"), "code", 1, (None,))
    _expect(sources.get("calldata"), "calldata", 1, (None,))
    _expect(sources.get("code_offsets"), "code_offsets", 8, (None,))
    _expect(sources.get("calldata_offsets"), "calldata_offsets", 8, (None,))
    trace = sources.get("trace") or {}
    n_rw = _rows(trace.get("head"))
    _expect(trace.get("head"), "head", 4, (None,))
    for name in _COPY_TRACE_KEYS[1:]:
        _expect(trace.get(name), name, 8, (n_rw,))
        if n_rw and name != "rw_counter" and trace.get(name) is None:
            raise ValueError(f"{name}: missing")
    n_code_bytes, n_codes = _rows(sources.get("code")), max(_rows(sources.get("code_offsets")) - 1, 0)
    n_txs = max(_rows(sources.get("calldata_offsets")) - 1, 0)
    ins = [events, flags, src_ref, dst_ref, randomness, *(sources.get(k) for k in COPY_SOURCE_KEYS), *(trace.get(k) for k in _COPY_TRACE_KEYS)]
    keep, opts = _prep(ins + list(outs), outputs=range(len(ins), len(ins) + len(outs)))
    if any(o is not None for o in outs) and not opts:
        raise ValueError("output buffers need device inputs (ZK_OPT_DEVICE_PTRS)")
    k = keep
    tr = _lib.ZkTrace(ptr(k[9], n_rw), ptr(k[10], n_rw), ptr(k[11], n_rw), ptr(k[12], n_rw), None, ptr(k[13], n_rw), int(trace.get("rw_base", 1)),
                      n_rw, None, 0, None, 0)
    t = _lib.ZkCopySources(ptr(k[0]), ptr(k[1]), n, ptr(k[2]), ptr(k[3]), ptr(k[4]), ptr(k[5], n_code_bytes), n_code_bytes,
                           ptr(k[6], n_codes), n_codes, ptr(k[7], _rows(k[7])), ptr(k[8], n_txs), n_txs, tr)
    return t, opts, keep


def copy_assign_from_sources_sizes(events, flags, src_ref, dst_ref, sources, device=None, _prepared=None):
    """(n_rows, n_table, n_rw, n_data) the events expand to over `sources`; raises EngineError (rc = _lib.ERR_CPS_* / ERR_TRC_*) outside
    the domain"""
    lib = _lib.init(device)
    t, opts, keep = _prepared or _copy_sources_args(events, flags, src_ref, dst_ref, sources, None)
    c = [ctypes.c_uint64() for _ in range(4)]
    check(lib.zk_copy_assign_from_sources_sizes(ctypes.byref(t), opts, *(ctypes.byref(x) for x in c)), "zk_copy_assign_from_sources_sizes", lib)
    return tuple(int(x.value) for x in c)


def _check_copy_sources_outs(outs, sizes):
    n_rows, n_table, n_rw, n_data = sizes
    shapes = ((20, n_rows, 4), (n_rows,), (n_table, 14, 4), (n_rw, 14, 4), (n_rw,), (n_data,))
    for o, name, size, shape in zip(outs, ("rows_dev", "row_flags_dev", "table_dev", "rw_dev", "rw_flags_dev", "data_dev"), (8, 4, 8, 8, 4, 2), shapes):
        _expect(o, name, size, shape)


class CopySourcesSession(Session):
    """zk_copy_assign_from_sources_open: launch() / collect() / read_status() over the EVENTS (status per event); read() -> the Copy
    assignment's outputs and the gathered data"""

    def read(self):
        """-> (rows uint64[20, n, 4], row_flags uint32[n], table uint64[m, 14, 4], rw uint64[k, 14, 4], rw_flags uint32[k], data uint16[d],
        data_offsets uint64[n_events + 1]) on the host"""
        n_rows, n_table, n_rw, n_data = self.sizes
        rows, rf = np.empty((20, n_rows, 4), dtype=np.uint64), np.empty(n_rows, dtype=np.uint32)
        table = np.empty((n_table, 14, 4), dtype=np.uint64)
        rw, rwf = np.empty((n_rw, 14, 4), dtype=np.uint64), np.empty(n_rw, dtype=np.uint32)
        data, offsets = np.empty(n_data, dtype=np.uint16), np.empty(self.n + 1, dtype=np.uint64)
        check(self._lib.zk_copy_assign_from_sources_read(self._h, ptr(rows, n_rows), ptr(rf, n_rows), ptr(table, n_table), ptr(rw, n_rw), ptr(rwf, n_rw),
                                                         ptr(data, n_data), ptr(offsets)), "zk_copy_assign_from_sources_read", self._lib)
        return rows, rf, table, rw, rwf, data, offsets


def open_copy_assign_from_sources(events, flags, src_ref, dst_ref, sources, randomness, rows_dev=None, row_flags_dev=None, table_dev=None,
                                  rw_dev=None, rw_flags_dev=None, data_dev=None, device=None):
    """open_copy_assign without its `data` array: events / flags as there, src_ref / dst_ref uint32[n] (dst_ref None when no event writes a
    code) and `sources` (see _copy_sources_args) -> CopySourcesSession over the n events.  The source bytes are gathered on the device
    from the code set, the calldata and the trace records, then the Copy assignment runs over them: its outputs are open_copy_assign's
    for the gathered data.  numpy inputs are staged to HBM; torch CUDA tensors are used in place (code, calldata and the trace's id /
    addr / val are read by every pass) and the optional *_dev tensors (sized with copy_assign_from_sources_sizes) receive the outputs."""
    lib = _lib.init(device)
    outs = (rows_dev, row_flags_dev, table_dev, rw_dev, rw_flags_dev, data_dev)
    prepared = _copy_sources_args(events, flags, src_ref, dst_ref, sources, randomness, outs)
    sizes = copy_assign_from_sources_sizes(events, flags, src_ref, dst_ref, sources, device, _prepared=prepared)
    _check_copy_sources_outs(outs, sizes)
    t, opts, keep = prepared
    s = _open(lib, lib.zk_copy_assign_from_sources_open, int(events.shape[0]), (keep, t), ctypes.byref(t), *(ptr(x) for x in keep[-6:]), opts,
              cls=CopySourcesSession)
    s.sizes = sizes
    return s


ECDSA_LAYOUT_PACKED = 0  # uint8[n, 5, 32]: pk_x LE, pk_y LE, msg_hash BE, sig_r LE, sig_s LE
ECDSA_LAYOUT_TX_UNITS = 1   # uint8[n, 9, 32]: the Tx units' byte rows (open_sign's wire["bytes"]; msg_hash little-endian)
ECDSA_LAYOUT_SIG_UNITS = 2  # the Sig units' byte rows (msg_hash big-endian; v = meta[:, 3])


def _ecdsa_args(sig_bytes, v, layout, v_stride, out_dev=None):
    """zk_ecdsa_open / zk_ecdsa_verify / a ZkEcdsaBatch -> ((sig_bytes, layout, v, v_stride, n), opts, kept arrays); out_dev: a
    session's status buffer, prepared with the inputs (kept array 2)"""
    _expect(sig_bytes, "signature bytes", 1, (None, 5 if layout == ECDSA_LAYOUT_PACKED else 9, 32))
    keep, opts = _prep([sig_bytes, v, out_dev], outputs=(2,))
    sig_bytes, v, _ = keep
    return (ptr(sig_bytes), int(layout), ptr(v), int(v_stride), int(sig_bytes.shape[0])), opts, keep


def open_ecdsa(sig_bytes, v=None, layout=ECDSA_LAYOUT_PACKED, out_dev=None, out_stride=1, device=None, v_stride=1):
    """secp256k1 ECDSA verification session: status per signature = the `ecdsa_status` column of the Tx / Sig units
    (0 verified, 1 not verified, else the exception's code; include/zkevm_hip.h).  out_dev: optional CUDA uint32
    tensor receiving status i at element i * out_stride (e.g. the units' meta tensor with stride 4)."""
    lib = _lib.init(device)
    args, opts, keep = _ecdsa_args(sig_bytes, v, layout, v_stride, out_dev)
    return _open(lib, lib.zk_ecdsa_open, args[4], keep, *args, ptr(keep[2]), int(out_stride), opts)


def open_ecdsa_batches(batches, device=None):
    """One launch over one or two signature arrays (zk_ecdsa_open_batches): `batches` = list of dicts with the arguments of
    open_ecdsa (sig_bytes, v, layout, out_dev, out_stride, v_stride).  Statuses: batch 0's signatures first."""
    lib = _lib.init(device)
    keep, arr, opts_all, n_total = [], (_lib.ZkEcdsaBatch * len(batches))(), None, 0
    for k, b in enumerate(batches):
        args, opts, kb = _ecdsa_args(b["sig_bytes"], b.get("v"), b.get("layout", ECDSA_LAYOUT_PACKED), b.get("v_stride", 1), b.get("out_dev"))
        assert opts_all is None or opts == opts_all, "mix of host and device batches"
        opts_all = opts
        keep += kb
        n_total += args[4]
        arr[k] = _lib.ZkEcdsaBatch(*args, ptr(kb[2]), int(b.get("out_stride", 1)))
    return _open(lib, lib.zk_ecdsa_open_batches, n_total, tuple(keep), arr, len(batches), opts_all)


def ecdsa_status(sig_bytes, v=None, layout=ECDSA_LAYOUT_PACKED, device=None, v_stride=1):
    """-> uint32[n] ecdsa_status computed on the GPU"""
    with open_ecdsa(sig_bytes, v, layout, device=device, v_stride=v_stride) as s:
        s.run()
        return s.read_status()


def fr_op(op, a, b):
    """Vector Fr op on the device (host numpy in/out): a, b uint64[n, 4]."""
    lib = _lib.init()
    a = np.ascontiguousarray(a, dtype=np.uint64)
    b = np.ascontiguousarray(b, dtype=np.uint64)
    out = np.empty_like(a)
    check(lib.zk_fr_op(int(op), ptr(a), ptr(b), ptr(out), a.shape[0], 0), "zk_fr_op", lib)
    return out


def _ecc_ops(w, randomness):
    """zk_ecc_assign / zk_ecc_verify over the arrays of flatten.flatten_ecc_ops (made host arrays) -> (ZkEccOps, opts 0, kept arrays)"""
    w = {k: (_host(v) if isinstance(v, np.ndarray) else v) for k, v in w.items()}
    randomness = _host(_randomness_cells(randomness, None))
    pts, pair_pts, pair_off, pair_out = w["points"], w["pair_pts"], w["pair_off"], w["pair_out"]
    _expect(pts, "ecc points", 8, (None, 6, 4))
    _expect(pair_pts, "ecc pair_pts", 8, (None, 6, 4))
    _expect(pair_out, "ecc pair_out", 8, (None, 4))
    _expect(pair_off, "ecc pair_off", 4, (pair_out.shape[0] + 1,))
    n_add, n_mul, n_pairing = int(w["n_add"]), int(w["n_mul"]), int(pair_out.shape[0])
    if n_add + n_mul != pts.shape[0]:
        raise ValueError("ecc points: n_add + n_mul != rows of points")
    max_ok = w["max_ok"]
    t = _lib.ZkEccOps(ptr(pts, pts.shape[0]), n_add, n_mul, ptr(pair_pts, pair_pts.shape[0]), ptr(pair_off), ptr(pair_out, n_pairing),
                      n_pairing, ptr(randomness), int(max_ok[0]), int(max_ok[1]), int(max_ok[2]))
    return t, 0, (w, randomness)


def _ecc_session_ops(w, randomness, rows=None, rows_out=None):
    """zk_ecc_open / zk_ecc_assign_open over the arrays of flatten.flatten_ecc_ops, numpy (staged at open) or device tensors (used in
    place; all of them then, `rows` / `rows_out` included) -> (ZkEccOps, rows, rows_out, n, opts, kept arrays)"""
    pts, pair_pts, pair_off, pair_out = w["points"], w["pair_pts"], w["pair_off"], w["pair_out"]
    randomness = _randomness_cells(randomness, pts)
    n_add, n_mul, n_pairing = int(w["n_add"]), int(w["n_mul"]), int(pair_out.shape[0])
    n = n_add + n_mul + n_pairing
    _expect(pts, "ecc points", 8, (n_add + n_mul, 6, 4))
    _expect(pair_pts, "ecc pair_pts", 8, (None, 6, 4))
    _expect(pair_out, "ecc pair_out", 8, (None, 4))
    _expect(pair_off, "ecc pair_off", 4, (n_pairing + 1,))
    _expect(randomness, "randomness", 8, (4,))
    _expect(rows, "ecc rows", 8, (n, 13, 4))
    _expect(rows_out, "rows_dev", 8, (n, 13, 4))
    keep, opts = _prep([pts, pair_pts, pair_off, pair_out, randomness, rows, rows_out], outputs=(6,))
    pts, pair_pts, pair_off, pair_out, randomness, rows, rows_out = keep
    max_ok = w["max_ok"]
    max_ok = max_ok.cpu().tolist() if hasattr(max_ok, "is_cuda") else max_ok
    t = _lib.ZkEccOps(ptr(pts, n_add + n_mul), n_add, n_mul, ptr(pair_pts, _rows(pair_pts)), ptr(pair_off), ptr(pair_out, n_pairing),
                      n_pairing, ptr(randomness), int(max_ok[0]), int(max_ok[1]), int(max_ok[2]))
    return t, rows, rows_out, n, opts, keep


def open_ecc(w, rows, randomness, device=None):
    """ECC circuit session: w = the ops wire of flatten.flatten_ecc_ops, rows uint64[n, 13, 4] (EccTableRow cells: ecc_assign's or an
    EccAssignSession's output), randomness (int or uint64[4]) -> Session over the n_add + n_mul + n_pairing rows.  numpy arrays are
    staged at open, device tensors used in place.  set_range(lo, hi) evaluates rows [lo, hi) (distributed.shard_ecc; lo == hi is
    allowed); first_fail_row is always a row of the whole circuit."""
    lib = _lib.init(device)
    t, rows, _, n, opts, keep = _ecc_session_ops(w, randomness, rows=rows)
    return _open(lib, lib.zk_ecc_open, n, (keep, t), ctypes.byref(t), ptr(rows), opts)


class EccAssignSession(Session):
    """ECC witness-assignment session (circuit2rows): launch()/collect() like the circuits; rows() for the EccTableRow cells."""

    def rows(self):
        out = np.empty((self.n, 13, 4), dtype=np.uint64)
        check(self._lib.zk_ecc_assign_read(self._h, ptr(out)), "zk_ecc_assign_read", self._lib)
        return out


def open_ecc_assign(w, randomness, rows_dev=None, device=None):
    """ECC circuit2rows over resident ops (the wire of flatten.flatten_ecc_ops, numpy or device tensors) -> EccAssignSession;
    rows_dev: optional CUDA tensor uint64[n, 13, 4] receiving the rows in place (ready for open_ecc)."""
    lib = _lib.init(device)
    t, _, rows_dev, n, opts, keep = _ecc_session_ops(w, randomness, rows_out=rows_dev)
    return _open(lib, lib.zk_ecc_assign_open, n, (keep, t), ctypes.byref(t), ptr(rows_dev), opts, cls=EccAssignSession)


def _withdrawal_eval_rows(w):
    """rows a session over the wire dict `w` evaluates (withdrawal_circuit.hpp wd_eval_rows)"""
    n_rows, base, total, m = int(w["rows"].shape[0]), int(w.get("row_base", 0)), int(w.get("total_rows", w["rows"].shape[0])), int(w["max_withdrawals"])
    n_eval = max(1, min(m, total))
    return 1 if n_rows == 0 else max(0, min(n_eval - base, n_rows))


def withdrawal_arrays(w, randomness):
    """(rows, mpt, keccak, block, randomness cell) of a withdrawal wire dict, C-contiguous uint64"""
    return (_host(w["rows"], np.uint64), _host(w["mpt"], np.uint64), _host(w["keccak"], np.uint64), _host(w["block"], np.uint64),
            _host(_randomness_cells(int(randomness), None)))


def _withdrawal_witness(w, randomness):
    """zk_withdrawal_open / zk_withdrawal_verify over the arrays of flatten.flatten_withdrawal_witness (made host arrays) ->
    (ZkWithdrawalWitness, opts 0, kept arrays)"""
    keep = rows, mpt, keccak, block, rc = withdrawal_arrays(w, randomness)
    _expect(rows, "withdrawal rows", 8, (None, 8, 4))
    _expect(mpt, "mpt", 8, (None, 12, 4))
    _expect(keccak, "keccak", 8, (None, 5, 4))
    _expect(block, "block", 8, (None, 4, 4))
    n, m, k, b = (int(x.shape[0]) for x in (rows, mpt, keccak, block))
    t = _lib.ZkWithdrawalWitness(ptr(rows, n), n, int(w.get("row_base", 0)), int(w.get("total_rows", n)), int(w["max_withdrawals"]),
                                 ptr(mpt, m), m, ptr(keccak, k), k, ptr(block, b), b, ptr(rc))
    return t, 0, keep


def open_withdrawal(w, randomness, device=None):
    """Withdrawal circuit session over a wire dict (flatten.flatten_withdrawal_witness, or a shard of it: distributed.shard_rows(...,
    "withdrawal") with row_base set) -> Session; zk_set_range applies (1 row before + 1 after, include/zkevm_hip.h)"""
    lib = _lib.init(device)
    ww, opts, keep = _withdrawal_witness(w, randomness)
    return _open(lib, lib.zk_withdrawal_open, _withdrawal_eval_rows(w), (keep, ww), ctypes.byref(ww), opts)


# ---- The wire-struct assignment families ----------------------------------------------------------------------------------------------
# Seven entry families share one ABI shape (include/zkevm_hip.h): `<stem>_open(&inputs, &wire or NULL, opts, &handle)`,
# `<stem>_read(handle, &wire or NULL, &count...)`, the one-shot `<stem>(&inputs, &wire, opts, [status,] &count..., &result)` and, for
# some, `<stem>_sizes(&inputs, opts, &size...)`.  A family is one record, an input check and a struct filler; the rest is written once,
# here.  The record's fields (an eighth family writes those three things; oneshot._wire_oneshot is the one-shot's body):
#   stem, inputs, outputs: the entry stem and the ordered array members of the input struct's dict and of the wire struct
#   wire: the wire struct's ctypes class
#   check(x, **kw) -> (rows of a session, output name -> (shape or None, dtype)): the wire-format check of the inputs
#   fill(x, a, cells) -> the input struct over the prepared input arrays `a` and the randomness cells
#   cut: the outputs that the trailing count out-parameters cut, in ABI order
#   status: the one-shot returns a status per item
#   null_empty: an EMPTY output travels as a null pointer, else as the pointer to its empty array (seen with host arrays: read() and
#     the one-shot; an empty device tensor's own pointer is null already)
#   n_sizes: the out-parameters of `<stem>_sizes` (0: the family has no such entry)
WireFamily = namedtuple("WireFamily", "stem inputs outputs wire check fill cut status null_empty n_sizes", defaults=((), False, False, 0))
Prepared = namedtuple("Prepared", "t w opts keep shapes n")  # one marshalled call: structs, options, kept arrays, output shapes, session rows


def _wire_struct(fam, arrs):
    """the family's wire struct over output arrays in ABI order (None: a null pointer)"""
    return fam.wire(*[ptr(x, int(np.prod(x.shape)) if fam.null_empty and x is not None else 1) for x in arrs])


def _wire_args(fam, x, randomness=(), outs=None, **kw):
    """`<stem>_open` / `<stem>` over the input dict `x` -> Prepared.  `outs` (device tensors only, each optional): buffers of fam.outputs
    the session writes in place; w is None for host inputs (the library then keeps the outputs in its own buffers)."""
    n, shapes = fam.check(x, **kw)
    outs = dict(outs or {})
    for k, v in outs.items():
        if v is not None:
            _expect(v, k, np.dtype(shapes[k][1]).itemsize, shapes[k][0])
    out_list, n_in = [outs.get(k) for k in fam.outputs], len(fam.inputs)
    a, opts = _prep([x.get(k) for k in fam.inputs] + out_list, outputs=range(n_in, n_in + len(out_list)))
    if any(v is not None for v in out_list) and not opts:
        raise ValueError("output buffers need device inputs (ZK_OPT_DEVICE_PTRS)")
    cells = [_randomness_cells(r, a[0]) for r in randomness]
    return Prepared(fam.fill(x, a, cells), _wire_struct(fam, a[n_in:]) if opts else None, opts, a + cells, shapes, n)


def _wire_host_outputs(fam, shapes, names=None):
    """zeroed host arrays for the outputs in `names` (None: all; an output without a shape stays None) -> (dict, wire struct over them)"""
    out = {k: None if shp is None else np.zeros(shp, dtype=dt) for k, (shp, dt) in shapes.items() if names is None or k in names}
    return out, _wire_struct(fam, [out.get(k) for k in fam.outputs])


def _wire_sizes(fam, lib, p):
    """`<stem>_sizes` over a Prepared call -> the library's own counts"""
    c = [ctypes.c_uint64() for _ in range(fam.n_sizes)]
    check(getattr(lib, fam.stem + "_sizes")(ctypes.byref(p.t), p.opts, *(ctypes.byref(x) for x in c)), fam.stem + "_sizes", lib)
    return tuple(int(x.value) for x in c)


class WireSession(Session):
    """A session of one wire-struct family: launch() / collect() / read_status() like the circuits; read(names=None) -> dict of the
    last pass's outputs as host arrays (all, or those named), the family's `cut` outputs cut to the library's counts."""

    family = shapes = None  # the WireFamily and output name -> (shape, dtype): set by _wire_open

    def _read(self, w=None):
        """one `<stem>_read` call (w None: the counts alone) -> the counts, in the order of family.cut"""
        c = [ctypes.c_uint64() for _ in self.family.cut]
        check(getattr(self._lib, self.family.stem + "_read")(self._h, ctypes.byref(w) if w is not None else None, *(ctypes.byref(x) for x in c)),
              self.family.stem + "_read", self._lib)
        return [int(x.value) for x in c]

    def _count(self, name):
        return self._read()[self.family.cut.index(name)]

    def read(self, names=None):
        out, w = _wire_host_outputs(self.family, self.shapes, names)
        for k, c in zip(self.family.cut, self._read(w)):
            if k in out:
                out[k] = out[k][:c]
        return out


def _wire_open(fam, device, x, randomness=(), outs=None, cls=WireSession, agree=None):
    """`<stem>_open` over the input dict `x` -> a `cls` session that keeps its arrays and structs alive and knows its family and output
    shapes.  agree(sizes, shapes): raises where the library's own `<stem>_sizes` counts are not what the buffers are shaped for."""
    lib = _lib.init(device)
    p = _wire_args(fam, x, randomness, outs)
    if agree is not None:
        agree(_wire_sizes(fam, lib, p), p.shapes)
    s = _open(lib, getattr(lib, fam.stem + "_open"), p.n, (p.keep, p.t, p.w), ctypes.byref(p.t), ctypes.byref(p.w) if p.w is not None else None,
              p.opts, cls=cls)
    s.family, s.shapes = fam, p.shapes
    return s


# ---- Tx circuit witness assignment (zk_tx_assign*) --------------------------------------------------------------------------------
TX_ASSIGN_INPUTS = ("fields", "to_is_none", "calldata", "offsets")
TX_ASSIGN_OUTPUTS = ("tx_rows", "tx_flags", "bytes", "cells", "meta", "keccak")


def tx_assign_shapes(n, max_txs, max_calldata_bytes):
    """name -> (shape, dtype) of the outputs of zk_tx_assign* (keccak: its capacity, n + 1 rows)"""
    rows = max_txs * 12 + max_calldata_bytes
    return {"tx_rows": ((rows, 5, 4), np.uint64), "tx_flags": ((rows,), np.uint32), "bytes": ((max_txs, 9, 32), np.uint8),
            "cells": ((8, max_txs, 4), np.uint64), "meta": ((max_txs, 4), np.uint32), "keccak": ((n + 1, 5, 4), np.uint64)}


def _tx_check(tx):
    n = int(tx["fields"].shape[0])
    _expect(tx["fields"], "fields", 8, (None, 8, 4))
    _expect(tx["to_is_none"], "to_is_none", 4, (n,))
    _expect(tx["offsets"], "offsets", 8, (n + 1,))
    _expect(tx["calldata"], "calldata", 1, (None,))
    return n, tx_assign_shapes(n, int(tx["max_txs"]), int(tx["max_calldata_bytes"]))


def _tx_fill(tx, a, cells):
    n = _rows(a[0])
    return _lib.ZkTxInputs(ptr(a[0], n), ptr(a[1], n), n, ptr(a[2], int(a[2].shape[0])), ptr(a[3]), int(tx["chain_id"]), int(tx["max_txs"]),
                           int(tx["max_calldata_bytes"]), ptr(cells[0]))


TX_ASSIGN = WireFamily("zk_tx_assign", TX_ASSIGN_INPUTS, TX_ASSIGN_OUTPUTS, _lib.ZkTxWire, _tx_check, _tx_fill, cut=("keccak",), status=True)


def _tx_assign_args(tx, randomness, outs=None):
    """zk_tx_assign_open / zk_tx_assign over `tx` = dict(fields uint64[n, 8, 4], to_is_none uint32[n], calldata uint8[b], offsets
    uint64[n + 1], chain_id, max_txs, max_calldata_bytes) -> (ZkTxInputs, ZkTxWire of the device outputs or None, opts, kept arrays).
    `outs` (device tensors only, each optional): buffers of TX_ASSIGN_OUTPUTS the session writes in place."""
    return _wire_args(TX_ASSIGN, tx, (randomness,), outs)[:4]


class TxAssignSession(WireSession):
    """zk_tx_assign_open: status per tx; read() -> the wire dict of the last pass (host arrays)"""

    def n_keccak(self):
        return self._count("keccak")


def open_tx_assign(tx, randomness, outs=None, device=None):
    """Tx circuit witness assignment session over the raw txs of `tx` (see _tx_assign_args).  With device tensors the outputs stay
    in HBM: in `outs`' buffers where given (e.g. for zk_ecdsa_open / zk_sign_open on them), else in the session's own."""
    return _wire_open(TX_ASSIGN, device, tx, (randomness,), outs, cls=TxAssignSession)


# ---- Sig circuit witness assignment (zk_sig_assign*) ------------------------------------------------------------------------------
SIG_ASSIGN_INPUTS = ("fields", "addr", "expect_valid")
SIG_ASSIGN_OUTPUTS = ("bytes", "cells", "meta", "keccak", "sig_table", "aux")


def sig_assign_shapes(n):
    """name -> (shape, dtype) of the outputs of zk_sig_assign* (keccak, sig_table: their capacities, n + 1 and n rows)"""
    return {"bytes": ((n, 9, 32), np.uint8), "cells": ((8, n, 4), np.uint64), "meta": ((n, 4), np.uint32),
            "keccak": ((n + 1, 5, 4), np.uint64), "sig_table": ((n, 9, 4), np.uint64), "aux": ((n, 12, 4), np.uint64)}


def _sig_check(sig):
    n = int(sig["fields"].shape[0])
    _expect(sig["fields"], "fields", 8, (None, 4, 4))
    _expect(sig.get("addr"), "addr", 8, (n, 4))
    _expect(sig.get("expect_valid"), "expect_valid", 4, (n,))
    return n, sig_assign_shapes(n)


def _sig_fill(sig, a, cells):
    n = _rows(a[0])
    return _lib.ZkSigInputs(ptr(a[0], n), ptr(a[1], n), ptr(a[2], n), n, int(sig.get("v_offset", 0)), 0, ptr(cells[0]))


SIG_ASSIGN = WireFamily("zk_sig_assign", SIG_ASSIGN_INPUTS, SIG_ASSIGN_OUTPUTS, _lib.ZkSigWire, _sig_check, _sig_fill, cut=("keccak", "sig_table"),
                        status=True)


def _sig_assign_args(sig, randomness, outs=None):
    """zk_sig_assign_open / zk_sig_assign over `sig` = dict(fields uint64[n, 4, 4]: msg_hash, sig_v, sig_r, sig_s; addr uint64[n, 4] or
    None: the claimed addresses; expect_valid uint32[n] or None; v_offset: 0 (v is the parity) or 27 (the precompile's input word))
    -> (ZkSigInputs, ZkSigWire of the device outputs or None, opts, kept arrays).
    `outs` (device tensors only, each optional): buffers of SIG_ASSIGN_OUTPUTS the session writes in place."""
    return _wire_args(SIG_ASSIGN, sig, (randomness,), outs)[:4]


class SigAssignSession(WireSession):
    """zk_sig_assign_open: status per signature; read() -> the wire dict of the last pass (host arrays)"""

    def n_keccak(self):
        return self._count("keccak")

    def n_sig_rows(self):
        return self._count("sig_table")


def open_sig_assign(sig, randomness, outs=None, device=None):
    """Sig circuit witness assignment session over the signed data of `sig` (see _sig_assign_args).  With device tensors the outputs
    stay in HBM: in `outs`' buffers where given (e.g. for zk_ecdsa_open / zk_sign_open on them), else in the session's own."""
    return _wire_open(SIG_ASSIGN, device, sig, (randomness,), outs, cls=SigAssignSession)


# ---- ECC precompile calls (zk_ecc_from_calls*) -------------------------------------------------------------------------------------
ECC_CALLS_INPUTS = ("add_in", "mul_in", "pair_pts", "pair_off")
ECC_CALLS_OUTPUTS = ("points", "pair_out", "rows", "ecc_table", "aux", "aux_kind")


def ecc_calls_shapes(n_add, n_mul, n_pairing):
    """name -> (shape, dtype) of the outputs of zk_ecc_from_calls* (ecc_table: its capacity, one row per call)"""
    n = n_add + n_mul + n_pairing
    return {"points": ((n_add + n_mul, 6, 4), np.uint64), "pair_out": ((n_pairing, 4), np.uint64), "rows": ((n, 13, 4), np.uint64),
            "ecc_table": ((n, 13, 4), np.uint64), "aux": ((n, 12, 4), np.uint64), "aux_kind": ((n,), np.uint32)}


def _ecc_calls_check(calls):
    add_in, mul_in, pair_pts, pair_off = (calls[k] for k in ECC_CALLS_INPUTS)
    n_add, n_mul, n_pairing = int(add_in.shape[0]), int(mul_in.shape[0]), int(pair_off.shape[0]) - 1
    _expect(add_in, "add_in", 8, (None, 4, 4))
    _expect(mul_in, "mul_in", 8, (None, 3, 4))
    _expect(pair_pts, "pair_pts", 8, (None, 6, 4))
    _expect(pair_off, "pair_off", 4, (n_pairing + 1,))
    return n_add + n_mul + n_pairing, ecc_calls_shapes(n_add, n_mul, n_pairing)


def _ecc_calls_fill(calls, a, cells):
    n_add, n_mul, n_pairing = _rows(a[0]), _rows(a[1]), _rows(a[3]) - 1
    return _lib.ZkEccCalls(ptr(a[0], n_add), n_add, ptr(a[1], n_mul), n_mul, ptr(a[2], _rows(a[2])), ptr(a[3], n_pairing), n_pairing, ptr(cells[0]))


ECC_CALLS = WireFamily("zk_ecc_from_calls", ECC_CALLS_INPUTS, ECC_CALLS_OUTPUTS, _lib.ZkEccCallWire, _ecc_calls_check, _ecc_calls_fill,
                       cut=("ecc_table",), status=True)


def _ecc_calls_args(calls, randomness, outs=None):
    """zk_ecc_from_calls_open / zk_ecc_from_calls over `calls` = dict(add_in uint64[n_add, 4, 4]: p.x, p.y, q.x, q.y; mul_in
    uint64[n_mul, 3, 4]: p.x, p.y, s; pair_pts uint64[m, 6, 4] in EIP-197 order + pair_off uint32[n_pairing + 1]) — the arrays of
    ecc_circuit.ecc_calls_wire — -> (ZkEccCalls, ZkEccCallWire of the device outputs or None, opts, kept arrays, output shapes).
    `outs` (device tensors only, each optional): buffers of ECC_CALLS_OUTPUTS the session writes in place."""
    return _wire_args(ECC_CALLS, calls, (randomness,), outs)[:5]


class EccCallsSession(WireSession):
    """zk_ecc_from_calls_open: launch() / collect() like the circuits (every status 0); read() -> the wire dict of the last pass
    (host arrays, ecc_table cut to its rows); n_table_rows() the table's row count alone"""

    def n_table_rows(self):
        return self._count("ecc_table")


def open_ecc_from_calls(calls, randomness, outs=None, device=None):
    """ECC precompile calls session (see _ecc_calls_args): from the calls' input words to the ECC circuit's ops and rows and the EVM
    circuit's ecc table and aux rows.  With device tensors the outputs stay in HBM: in `outs`' buffers where given (ready for
    open_ecc / open_evm), else in the session's own."""
    return _wire_open(ECC_CALLS, device, calls, (randomness,), outs, cls=EccCallsSession)


# ---- PI circuit witness assignment (zk_pi_assign*) ----------------------------------------------------------------------------------
PI_ASSIGN_INPUTS = ("block", "state_root_prev", "block_hashes", "tx_fields", "to_is_none", "calldata", "offsets", "withdrawals")
PI_ASSIGN_OUTPUTS = ("rows", "gas", "keccak", "cc_cells", "cc_bytes", "cc_lens", "block_table", "block_flags", "tx_table", "tx_flags",
                     "wd_table", "public_inputs", "raw_bytes", "raw_lens")


def pi_assign_shapes(max_txs, max_calldata_bytes, max_withdrawals, calldata_bytes):
    """name -> (shape, dtype) of the outputs of zk_pi_assign* (include/zkevm_hip.h)"""
    mt, mc, mw = int(max_txs), int(max_calldata_bytes), int(max_withdrawals)
    n = 8454 + 336 * mt + mc + 56 * mw
    n_cc = 538 + 4 * (10 * mt + 1) + 2 * mc + 5 * mw
    t = 10 * mt + 1 + mc
    return {"rows": ((24, n, 4), np.uint64), "gas": ((1 + int(calldata_bytes), 3, 4), np.uint64), "keccak": ((2, 5, 4), np.uint64),
            "cc_cells": ((n_cc, 4), np.uint64), "cc_bytes": ((n_cc, 32), np.uint8), "cc_lens": ((n_cc,), np.uint32),
            "block_table": ((268, 2, 4), np.uint64), "block_flags": ((268,), np.uint32), "tx_table": ((t, 5, 4), np.uint64),
            "tx_flags": ((t,), np.uint32), "wd_table": ((mw, 5, 4), np.uint64), "public_inputs": ((4, 2, 4), np.uint64),
            "raw_bytes": ((n,), np.uint8), "raw_lens": ((533 + 33 * mt + mc + 5 * mw,), np.uint32)}


def _pi_check(pd):
    n = _rows(pd["tx_fields"])
    _expect(pd["block"], "block", 8, (9, 4))
    _expect(pd["state_root_prev"], "state_root_prev", 8, (4,))
    _expect(pd["block_hashes"], "block_hashes", 8, (256, 4))
    _expect(pd["tx_fields"], "tx_fields", 8, (None, 7, 4))
    _expect(pd["to_is_none"], "to_is_none", 4, (n,))
    _expect(pd["offsets"], "offsets", 8, (n + 1,))
    _expect(pd["calldata"], "calldata", 1, (None,))
    _expect(pd["withdrawals"], "withdrawals", 8, (None, 4, 4))
    shapes = pi_assign_shapes(pd["max_txs"], pd["max_calldata_bytes"], pd["max_withdrawals"], pd["calldata"].shape[0])
    return shapes["rows"][0][1], shapes


def _pi_fill(pd, a, cells):
    n, m = _rows(a[3]), _rows(a[7])
    return _lib.ZkPiInputs(int(pd["chain_id"]), ptr(a[0]), ptr(a[1]), ptr(a[2]), ptr(a[3], n), ptr(a[4], n), n, ptr(a[5], int(a[5].shape[0])),
                           ptr(a[6]), ptr(a[7], m), m, int(pd["max_txs"]), int(pd["max_calldata_bytes"]), int(pd["max_withdrawals"]),
                           ptr(cells[0]), ptr(cells[1]))


PI_ASSIGN = WireFamily("zk_pi_assign", PI_ASSIGN_INPUTS, PI_ASSIGN_OUTPUTS, _lib.ZkPiWire, _pi_check, _pi_fill, n_sizes=3)


def _pi_assign_args(pd, keccak_rand=255, byte_pow_base=255, outs=None):
    """zk_pi_assign_open / zk_pi_assign over `pd` = dict(chain_id, block uint64[9, 4], state_root_prev uint64[4], block_hashes
    uint64[256, 4], tx_fields uint64[n, 7, 4], to_is_none uint32[n], calldata uint8[b], offsets uint64[n + 1], withdrawals
    uint64[m, 4, 4], max_txs, max_calldata_bytes, max_withdrawals) -> (ZkPiInputs, ZkPiWire of the device outputs or None, opts, kept
    arrays, output shapes).  `outs` (device tensors only, each optional): buffers of PI_ASSIGN_OUTPUTS the session writes in place; they
    are sized from pd["calldata"], so its extent must be the offsets' last entry."""
    return _wire_args(PI_ASSIGN, pd, (int(keccak_rand), int(byte_pow_base)), outs)[:5]


def pi_assign_sizes(pd, device=None):
    """(circuit_len, gas-table rows, copy constraints) of the public data `pd`; raises EngineError (rc = _lib.ERR_PI_*) for inputs
    outside the circuit's domain"""
    lib = _lib.init(device)
    return _wire_sizes(PI_ASSIGN, lib, _wire_args(PI_ASSIGN, pd, (255, 255)))


PiAssignSession = WireSession  # zk_pi_assign_open: one status per row

def open_pi_assign(pd, keccak_rand=255, byte_pow_base=255, outs=None, device=None):
    """PI circuit witness assignment session over the public data `pd` (see _pi_assign_args).  With device tensors the outputs stay in
    HBM: in `outs`' buffers where given (rows / keccak / gas for open_pi, cc_cells / cc_bytes / cc_lens for zk_pi_copy_open), else in
    the session's own."""
    return _wire_open(PI_ASSIGN, device, pd, (int(keccak_rand), int(byte_pow_base)), outs)


# ---- Bytecode table + circuit rows + keccak rows from raw contract code (zk_bytecode_from_code*) ----------------------------------
CODE_OUTPUTS = ("table", "rows", "keccak")


def bytecode_from_code_shapes(n_bytes, n_codes, k):
    """name -> shape of the uint64 outputs of zk_bytecode_from_code* (rows: None when k == 0)"""
    return {"table": (n_bytes + n_codes, 6, 4), "rows": (12, 1 << int(k), 4) if int(k) else None, "keccak": (n_codes, 5, 4)}


def _code_check(x):
    _expect(x["code"], "code", 1, (None,))
    _expect(x["offsets"], "offsets", 8, (None,))
    n_bytes, n_codes = int(x["code"].shape[0]), int(x["offsets"].shape[0]) - 1
    if n_codes < 0:
        raise ValueError("offsets: expected n_codes + 1 entries")
    if not int(x["k"]) and x.get("rows_dev") is not None:
        raise ValueError("rows_dev needs k > 0")
    return n_bytes + n_codes, {k: (shp, np.uint64) for k, shp in bytecode_from_code_shapes(n_bytes, n_codes, x["k"]).items()}


def _code_fill(x, a, cells):
    if _is_device(a[0]) and not _is_device(cells[0]):  # (this family alone refuses host randomness beside device inputs)
        raise ValueError("mix of host and device buffers")
    n_bytes, n_codes = _rows(a[0]), _rows(a[1]) - 1
    return _lib.ZkCodeSet(ptr(a[0], n_bytes), n_bytes, ptr(a[1]), n_codes, int(x["k"]), 0, ptr(cells[0]))


CODE = WireFamily("zk_bytecode_from_code", ("code", "offsets"), CODE_OUTPUTS, _lib.ZkCodeWire, _code_check, _code_fill, null_empty=True)


def _bytecode_from_code_args(code, offsets, k, randomness, outs=None):
    """zk_bytecode_from_code_open / zk_bytecode_from_code over code uint8[n_bytes] (the contracts back to back) and offsets
    uint64[n_codes + 1] -> (ZkCodeSet, ZkCodeWire of the device outputs or None, opts, kept arrays).  `outs` (device tensors only,
    each optional): table / rows / keccak buffers the session writes in place."""
    return _wire_args(CODE, {"code": code, "offsets": offsets, "k": k, "rows_dev": (outs or {}).get("rows")}, (randomness,), outs)[:4]


class BytecodeFromCodeSession(WireSession):
    """zk_bytecode_from_code_open: launch() / collect() like the other assignments (status per table row, always 0);
    read() -> (table uint64[n_bytes + n_codes, 6, 4], rows uint64[12, 2^k, 4] or None when k == 0, keccak uint64[n_codes, 5, 4])
    of the last pass, as host arrays"""

    def read(self, names=None):
        out = super().read(names)
        return tuple(out.get(name) for name in CODE_OUTPUTS)


def open_bytecode_from_code(code, offsets, k, randomness, table_dev=None, rows_dev=None, keccak_dev=None, device=None):
    """code uint8[n_bytes] + offsets uint64[n_codes + 1] (raw contract code), k (0: no circuit rows), randomness (int or uint64[4])
    -> BytecodeFromCodeSession.  numpy inputs are staged to HBM; torch CUDA tensors are used in place, and table_dev / rows_dev /
    keccak_dev (CUDA tensors of the shapes read() returns) then receive the outputs in place: rows_dev and keccak_dev are what
    open_bytecode takes, table_dev is zk_evm_tables.bytecode."""
    return _wire_open(CODE, device, {"code": code, "offsets": offsets, "k": k, "rows_dev": rows_dev}, (randomness,),
                      {"table": table_dev, "rows": rows_dev, "keccak": keccak_dev}, cls=BytecodeFromCodeSession)


# ---- EVM circuit tx / block / withdrawal tables from raw block data (zk_evm_tables_from_block*) -------------------------------------
BLOCK_TABLES_INPUTS = ("tx_fields", "to_is_none", "access_list", "calldata", "offsets", "block", "history_hashes", "withdrawals")
BLOCK_TABLES_OUTPUTS = ("tx", "tx_flags", "block", "block_flags", "withdrawals")
CALLDATA_GAS_BLOCK = 256  # bytes of calldata per partial count of the calldata-gas kernel (csrc/block_tables.hpp BTB_GAS_BLOCK)


def evm_tables_from_block_shapes(n_txs, calldata_bytes, n_history, n_withdrawals, has_block=True):
    """name -> (shape, dtype) of the outputs of zk_evm_tables_from_block* (include/zkevm_hip.h)"""
    t, b, m = 12 * int(n_txs) + int(calldata_bytes), (8 + int(n_history)) if has_block else 0, int(n_withdrawals)
    return {"tx": ((t, 5, 4), np.uint64), "tx_flags": ((t,), np.uint32), "block": ((b, 4, 4), np.uint64), "block_flags": ((b,), np.uint32),
            "withdrawals": ((m, 4, 4), np.uint64)}


def _block_tables_check(raw):
    n, h, m = _rows(raw["tx_fields"]), _rows(raw.get("history_hashes")), _rows(raw.get("withdrawals"))
    _expect(raw["tx_fields"], "tx_fields", 8, (None, 9, 4))
    _expect(raw["to_is_none"], "to_is_none", 4, (n,))
    _expect(raw["access_list"], "access_list", 4, (n, 2))
    _expect(raw["calldata"], "calldata", 1, (None,))
    _expect(raw["offsets"], "offsets", 8, (n + 1,))
    _expect(raw.get("block"), "block", 8, (8, 4))
    _expect(raw.get("history_hashes"), "history_hashes", 8, (None, 4))
    _expect(raw.get("withdrawals"), "withdrawals", 8, (None, 4, 4))
    shapes = evm_tables_from_block_shapes(n, raw["calldata"].shape[0], h, m, raw.get("block") is not None)
    return shapes["tx"][0][0], shapes


def _block_tables_fill(raw, a, cells):
    n, h, m = _rows(a[0]), _rows(a[6]), _rows(a[7])
    return _lib.ZkBlockData(ptr(a[0], n), ptr(a[1], n), ptr(a[2], n), n, ptr(a[3], int(a[3].shape[0])), ptr(a[4]), ptr(a[5]), ptr(a[6], h), h,
                            ptr(a[7], m), m)


BLOCK_TABLES = WireFamily("zk_evm_tables_from_block", BLOCK_TABLES_INPUTS, BLOCK_TABLES_OUTPUTS, _lib.ZkBlockTables, _block_tables_check,
                          _block_tables_fill, null_empty=True, n_sizes=3)


def _evm_tables_from_block_args(raw, outs=None):
    """zk_evm_tables_from_block* over `raw` = dict(tx_fields uint64[n, 9, 4], to_is_none uint32[n], access_list uint32[n, 2], calldata
    uint8[b], offsets uint64[n + 1], block uint64[8, 4] or None, history_hashes uint64[h, 4], withdrawals uint64[m, 4, 4]) -> (ZkBlockData,
    ZkBlockTables of the device outputs or None, opts, kept arrays, shapes).  `outs` (device tensors only, each optional): buffers of
    BLOCK_TABLES_OUTPUTS the session writes in place; they are sized from raw["calldata"], whose extent must be the offsets' last entry
    (the opening functions check that against the library's own count)."""
    return _wire_args(BLOCK_TABLES, raw, (), outs)[:5]


def evm_tables_from_block_sizes(raw, device=None, _prepared=None):
    """(tx-table rows, block-table rows, withdrawal rows) of the raw block data `raw`; raises EngineError (rc = _lib.ERR_BTB_*) for inputs
    outside the domain.  _prepared: the Prepared call of _wire_args, where the caller has made it"""
    lib = _lib.init(device)
    return _wire_sizes(BLOCK_TABLES, lib, _prepared or _wire_args(BLOCK_TABLES, raw))


def _check_block_table_sizes(sizes, shapes):
    if sizes != (shapes["tx"][0][0], shapes["block"][0][0], shapes["withdrawals"][0][0]):
        raise ValueError(f"calldata: its extent must be the offsets' last entry (the library counts {sizes[0]} tx-table rows, the buffers "
                         f"are sized for {shapes['tx'][0][0]})")


TablesFromBlockSession = WireSession  # zk_evm_tables_from_block_open: status per tx-table row, always 0

def open_evm_tables_from_block(raw, outs=None, device=None):
    """The EVM circuit's tx, block and withdrawal tables from raw block data `raw` (see _evm_tables_from_block_args) ->
    TablesFromBlockSession.  numpy inputs are staged to HBM; torch CUDA tensors are used in place, and the CUDA tensors of `outs` (tx /
    tx_flags / block / block_flags / withdrawals, shapes of evm_tables_from_block_shapes) then receive the tables in place: what
    open_evm's wire and open_copy's tx / tx_flags take."""
    return _wire_open(BLOCK_TABLES, device, raw, (), outs, agree=_check_block_table_sizes)


# ---- EVM circuit witness from compact trace records (zk_evm_witness_from_trace*) ---------------------------------------------------
TRACE_INPUTS = ("head", "id", "addr", "val", "prev", "rw_counter", "pool", "steps")
TRACE_OUTPUTS = ("rw", "rw_flags", "steps")


def evm_witness_from_trace_shapes(n_rw, n_steps):
    """name -> (shape, dtype) of the outputs of zk_evm_witness_from_trace* (include/zkevm_hip.h)"""
    return {"rw": ((int(n_rw), 14, 4), np.uint64), "rw_flags": ((int(n_rw),), np.uint32), "steps": ((int(n_steps), 13, 4), np.uint64)}


def _trace_check(trace, optional=()):
    n = _rows(trace.get("head"))
    _expect(trace.get("head"), "head", 4, (None,))
    for name in ("id", "addr", "val", "prev", "rw_counter"):
        _expect(trace.get(name), name, 8, (n,))
        if n and name != "rw_counter" and name not in optional and trace.get(name) is None:
            raise ValueError(f"{name}: missing")
    _expect(trace.get("pool"), "pool", 8, (None, 4))
    _expect(trace.get("steps"), "steps", 8, (None, 13))
    return n, evm_witness_from_trace_shapes(n, _rows(trace.get("steps")))


def _trace_fill(trace, a, cells):
    n, m, k = _rows(a[0]), _rows(a[6]), _rows(a[7])
    return _lib.ZkTrace(ptr(a[0], n), ptr(a[1], n), ptr(a[2], n), ptr(a[3], n), ptr(a[4], n), ptr(a[5], n), int(trace.get("rw_base", 1)), n,
                        ptr(a[6], m), m, ptr(a[7], k), k)


TRACE = WireFamily("zk_evm_witness_from_trace", TRACE_INPUTS, TRACE_OUTPUTS, _lib.ZkTraceWitness, _trace_check, _trace_fill,
                   null_empty=True, n_sizes=2)


def _evm_witness_from_trace_args(trace, outs=None, optional=()):
    """zk_evm_witness_from_trace* over `trace` = dict(head uint32[n], id / addr / val / prev uint64[n], rw_counter uint64[n] or None (then
    rw_base, default 1: the counter of op i is rw_base + i), pool uint64[m, 4], steps uint64[k, 13]) -> (ZkTrace, ZkTraceWitness of the
    device outputs or None, opts, kept arrays, shapes).  trace.py makes such records.  `outs` (device tensors only, each optional):
    buffers of TRACE_OUTPUTS the session writes in place.  `optional`: per-op arrays the entry does not read and that may be missing."""
    return _wire_args(TRACE, trace, (), outs, optional=optional)[:5]


def evm_witness_from_trace_sizes(trace, device=None, _prepared=None):
    """(RW rows, step rows) of the trace records `trace`; raises EngineError (rc = _lib.ERR_TRC_*) for records outside the domain"""
    lib = _lib.init(device)
    return _wire_sizes(TRACE, lib, _prepared or _wire_args(TRACE, trace))


WitnessFromTraceSession = WireSession  # zk_evm_witness_from_trace_open: status per RW row, always 0

def open_evm_witness_from_trace(trace, outs=None, device=None):
    """The EVM circuit's RW table, its flags and its step table from compact trace records `trace` (see _evm_witness_from_trace_args) ->
    WitnessFromTraceSession.  numpy inputs are staged to HBM (the CPU backend reads id / addr / val / prev / pool / steps in place, every
    pass); torch CUDA tensors are used in place, and the CUDA tensors of `outs` (rw / rw_flags / steps, shapes of
    evm_witness_from_trace_shapes) then receive the rows in place: what open_evm's wire and the from-RW State sessions take."""
    return _wire_open(TRACE, device, trace, (), outs)


# ---- Copy and EXP events from compact trace records (zk_events_from_trace*) ---------------------------------------------------------
TRACE_EVENTS_INPUTS = ("head", "id", "addr", "val", "rw_counter", "pool", "steps", "code", "code_offsets", "code_hashes")
TRACE_EVENTS_OUTPUTS = ("copy_events", "copy_flags", "copy_src_ref", "copy_step", "exp_events", "exp_step")


def events_from_trace_shapes(n_steps):
    """name -> (shape, dtype) of the outputs of zk_events_from_trace*: each has the capacity n_steps (include/zkevm_hip.h)"""
    n = int(n_steps)
    return {"copy_events": ((n, 12, 4), np.uint64), "copy_flags": ((n,), np.uint32), "copy_src_ref": ((n,), np.uint32),
            "copy_step": ((n,), np.uint32), "exp_events": ((n, 5, 4), np.uint64), "exp_step": ((n,), np.uint32)}


def trace_event_sources(trace, codes, code_hashes):
    """The input dict of the family: the records of `trace` (trace.py; prev is not read) with the code set.  codes: a list of byte
    strings, or dict(code uint8[b], code_offsets uint64[n + 1]) of arrays or CUDA tensors; code_hashes: a list of ints, or uint64[n, 4]."""
    x = {k: trace.get(k) for k in TRACE_EVENTS_INPUTS[:7]}
    x["rw_base"] = trace.get("rw_base", 1)
    if isinstance(codes, dict):
        x["code"], x["code_offsets"] = codes.get("code"), codes.get("code_offsets")
    else:
        codes = [bytes(c) for c in codes]
        x["code"] = np.frombuffer(b"".join(codes), dtype=np.uint8).copy()
        x["code_offsets"] = np.cumsum([0] + [len(c) for c in codes]).astype(np.uint64)
    if isinstance(code_hashes, (list, tuple)):
        code_hashes = np.frombuffer(b"".join(int(h).to_bytes(32, "little") for h in code_hashes), dtype="<u8").astype(np.uint64).reshape(-1, 4)
    x["code_hashes"] = code_hashes
    return x


def _trace_events_check(x):
    n = _rows(x.get("head"))
    _expect(x.get("head"), "head", 4, (None,))
    for name in ("id", "addr", "val", "rw_counter"):
        _expect(x.get(name), name, 8, (n,))
        if n and name != "rw_counter" and x.get(name) is None:
            raise ValueError(f"{name}: missing")
    _expect(x.get("pool"), "pool", 8, (None, 4))
    _expect(x.get("steps"), "steps", 8, (None, 13))
    nc = _rows(x.get("code_hashes"))
    _expect(x.get("code"), "code", 1, (None,))
    _expect(x.get("code_hashes"), "code_hashes", 8, (None, 4))
    _expect(x.get("code_offsets"), "code_offsets", 8, (None,))
    if nc and _rows(x.get("code_offsets")) != nc + 1:
        raise ValueError(f"code_offsets: expected {nc + 1} entries for {nc} code hashes, got {_rows(x.get('code_offsets'))}")
    ns = _rows(x.get("steps"))
    return ns, events_from_trace_shapes(ns)


def _trace_events_fill(x, a, cells):
    n, m, k, nb, nc = _rows(a[0]), _rows(a[5]), _rows(a[6]), _rows(a[7]), _rows(a[9])
    t = _lib.ZkTrace(ptr(a[0], n), ptr(a[1], n), ptr(a[2], n), ptr(a[3], n), None, ptr(a[4], n), int(x.get("rw_base", 1)), n, ptr(a[5], m), m,
                     ptr(a[6], k), k)
    return _lib.ZkTraceSources(t, ptr(a[7], nb), nb, ptr(a[8], nc), nc, ptr(a[9], nc))


TRACE_EVENTS = WireFamily("zk_events_from_trace", TRACE_EVENTS_INPUTS, TRACE_EVENTS_OUTPUTS, _lib.ZkTraceEvents, _trace_events_check,
                          _trace_events_fill, cut=("copy_events", "exp_events"), status=True, null_empty=True, n_sizes=1)


def cut_trace_events(out, n_copy, n_exp):
    """the outputs of the family cut to the pass's counts: the copy_* arrays to n_copy, the exp_* arrays to n_exp"""
    return {k: (v if v is None else v[: n_copy if k.startswith("copy") else n_exp]) for k, v in out.items()}


def events_from_trace_sizes(trace, codes, code_hashes, device=None, _prepared=None):
    """the capacity every output of zk_events_from_trace* needs (n_steps); raises EngineError (rc = _lib.ERR_TRC_* / ERR_TEV_*) for
    inputs outside the domain"""
    lib = _lib.init(device)
    return _wire_sizes(TRACE_EVENTS, lib, _prepared or _wire_args(TRACE_EVENTS, trace_event_sources(trace, codes, code_hashes)))[0]


class EventsFromTraceSession(WireSession):
    """zk_events_from_trace_open: a status per step; counts() -> (n_copy, n_exp) of the last pass; read(names=None) -> dict of the
    outputs cut to those counts (copy_events / copy_flags / copy_src_ref: what open_copy_assign_from_sources takes; exp_events: what
    open_exp_assign takes; copy_step / exp_step: the step of each event)"""

    def counts(self):
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        check(self._lib.zk_events_from_trace_counts(self._h, ctypes.byref(a), ctypes.byref(b)), "zk_events_from_trace_counts", self._lib)
        return int(a.value), int(b.value)

    def read(self, names=None):
        out, w = _wire_host_outputs(self.family, self.shapes, names)
        return cut_trace_events(out, *self._read(w))


def open_events_from_trace(trace, codes, code_hashes, outs=None, device=None):
    """The copy and EXP events of the steps of compact trace records `trace` (see trace_event_sources) -> EventsFromTraceSession over the
    steps.  numpy inputs are staged to HBM (the CPU backend reads id / addr / val / pool / steps / code in place, every pass); torch CUDA
    tensors are used in place, and the CUDA tensors of `outs` (TRACE_EVENTS_OUTPUTS, shapes of events_from_trace_shapes: capacity
    n_steps each) then receive the packed lists in place."""
    return _wire_open(TRACE_EVENTS, device, trace_event_sources(trace, codes, code_hashes), (), outs, cls=EventsFromTraceSession)


# ---- The same with the events of BeginTx, RETURN / REVERT and DATACOPY (zk_events_from_trace_ext*) ----------------------------------
TRACE_EVENTS_EXT_OUTPUTS = ("copy_events", "copy_flags", "copy_src_ref", "copy_dst_ref", "copy_step", "exp_events", "exp_step")


def events_from_trace_ext_shapes(copy_capacity, n_steps):
    """name -> (shape, dtype) of the outputs of zk_events_from_trace_ext* for the capacities of events_from_trace_ext_sizes"""
    c, n = int(copy_capacity), int(n_steps)
    return {"copy_events": ((c, 12, 4), np.uint64), "copy_flags": ((c,), np.uint32), "copy_src_ref": ((c,), np.uint32),
            "copy_dst_ref": ((c,), np.uint32), "copy_step": ((c,), np.uint32), "exp_events": ((n, 5, 4), np.uint64), "exp_step": ((n,), np.uint32)}


def _trace_events_ext_check(x):
    ns, _ = _trace_events_check(x)
    return ns, events_from_trace_ext_shapes(x.get("copy_capacity", ns), ns)  # (no capacity yet: the `_sizes` call, which shapes nothing)


TRACE_EVENTS_EXT = WireFamily("zk_events_from_trace_ext", TRACE_EVENTS_INPUTS, TRACE_EVENTS_EXT_OUTPUTS, _lib.ZkTraceEventsExt,
                              _trace_events_ext_check, _trace_events_fill, cut=("copy_events", "exp_events"), status=True, null_empty=True, n_sizes=2)


def _trace_events_ext_sized(lib, x):
    """the input dict `x` with the library's own copy capacity (one `_sizes` call)"""
    x = dict(x)
    x["copy_capacity"] = _wire_sizes(TRACE_EVENTS_EXT, lib, _wire_args(TRACE_EVENTS_EXT, x))[0]
    return x


def events_from_trace_ext_sizes(trace, codes, code_hashes, device=None):
    """(copy capacity, EXP capacity) of zk_events_from_trace_ext*: n_steps + the BeginTx and DATACOPY steps, and n_steps; raises
    EngineError (rc = _lib.ERR_TRC_* / ERR_TEV_*) for inputs outside the domain"""
    lib = _lib.init(device)
    return _wire_sizes(TRACE_EVENTS_EXT, lib, _wire_args(TRACE_EVENTS_EXT, trace_event_sources(trace, codes, code_hashes)))


class EventsFromTraceExtSession(WireSession):
    """zk_events_from_trace_ext_open: a status per step; counts() -> (n_copy, n_exp) of the last pass; read(names=None) -> dict of the
    outputs cut to those counts (copy_events / copy_flags / copy_src_ref / copy_dst_ref: what open_copy_assign_from_sources takes)"""

    def counts(self):
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        check(self._lib.zk_events_from_trace_ext_counts(self._h, ctypes.byref(a), ctypes.byref(b)), "zk_events_from_trace_ext_counts", self._lib)
        return int(a.value), int(b.value)

    def read(self, names=None):
        out, w = _wire_host_outputs(self.family, self.shapes, names)
        return cut_trace_events(out, *self._read(w))


def open_events_from_trace_ext(trace, codes, code_hashes, outs=None, device=None):
    """open_events_from_trace with the copy events of BeginTx, RETURN / REVERT and DATACOPY steps -> EventsFromTraceExtSession.  The CUDA
    tensors of `outs` (TRACE_EVENTS_EXT_OUTPUTS, shapes of events_from_trace_ext_shapes over events_from_trace_ext_sizes) receive the
    packed lists in place."""
    lib = _lib.init(device)
    x = _trace_events_ext_sized(lib, trace_event_sources(trace, codes, code_hashes))
    return _wire_open(TRACE_EVENTS_EXT, device, x, (), outs, cls=EventsFromTraceExtSession)


# ---- SHA3 inputs and keccak rows from compact trace records (zk_sha3_from_trace*) ----------------------------------------------------
TRACE_SHA3_INPUTS = ("head", "id", "addr", "val", "rw_counter", "pool", "steps")
TRACE_SHA3_OUTPUTS = ("rows", "step", "data", "data_offsets")


def sha3_from_trace_shapes(n_msgs, n_bytes):
    """name -> (shape, dtype) of the outputs of zk_sha3_from_trace* for the counts of sha3_from_trace_sizes (include/zkevm_hip.h)"""
    m, b = int(n_msgs), int(n_bytes)
    return {"rows": ((m, 5, 4), np.uint64), "step": ((m,), np.uint32), "data": ((b,), np.uint8), "data_offsets": ((m + 1,), np.uint64)}


def _trace_sha3_check(x):
    n = _rows(x.get("head"))
    _expect(x.get("head"), "head", 4, (None,))
    for name in ("id", "addr", "val", "rw_counter"):
        _expect(x.get(name), name, 8, (n,))
        if n and name != "rw_counter" and x.get(name) is None:
            raise ValueError(f"{name}: missing")
    _expect(x.get("pool"), "pool", 8, (None, 4))
    _expect(x.get("steps"), "steps", 8, (None, 13))
    return _rows(x.get("steps")), sha3_from_trace_shapes(*x.get("counts", (0, 0)))


def _trace_sha3_fill(x, a, cells):
    n, m, k = _rows(a[0]), _rows(a[5]), _rows(a[6])
    return _lib.ZkTrace(ptr(a[0], n), ptr(a[1], n), ptr(a[2], n), ptr(a[3], n), None, ptr(a[4], n), int(x.get("rw_base", 1)), n, ptr(a[5], m), m,
                        ptr(a[6], k), k)


# (the randomness travels as an argument of its own behind the inputs: the open and the one-shot below make the call themselves)
TRACE_SHA3 = WireFamily("zk_sha3_from_trace", TRACE_SHA3_INPUTS, TRACE_SHA3_OUTPUTS, _lib.ZkTraceSha3, _trace_sha3_check, _trace_sha3_fill,
                        cut=("rows", "data"), status=True, null_empty=True, n_sizes=2)


def _trace_sha3_records(trace, counts=None):
    x = {k: trace.get(k) for k in TRACE_SHA3_INPUTS}
    x["rw_base"] = trace.get("rw_base", 1)
    if counts is not None:
        x["counts"] = counts
    return x


def sha3_from_trace_sizes(trace, device=None):
    """(n_msgs, n_bytes) of the SHA3 steps of the trace records `trace`: what sizes the outputs of zk_sha3_from_trace*; raises
    EngineError (rc = _lib.ERR_TRC_* / ERR_TS3_*) for records outside the domain"""
    lib = _lib.init(device)
    return _wire_sizes(TRACE_SHA3, lib, _wire_args(TRACE_SHA3, _trace_sha3_records(trace)))


class Sha3FromTraceSession(WireSession):
    """zk_sha3_from_trace_open: a status per step; counts() -> (n_msgs, n_bytes); read(names=None) -> dict of rows uint64[n_msgs, 5, 4]
    (what zk_evm_tables' keccak table takes), step uint32[n_msgs], data uint8[n_bytes], data_offsets uint64[n_msgs + 1] of the last pass"""

    def counts(self):
        return tuple(self._read())


def open_sha3_from_trace(trace, randomness, outs=None, device=None):
    """The SHA3 steps' messages and keccak rows of compact trace records `trace` (trace.py; prev is not read) -> Sha3FromTraceSession
    over the steps.  numpy inputs are staged to HBM (the CPU backend reads id / addr / val / pool in place, every pass); torch CUDA
    tensors are used in place, and the CUDA tensors of `outs` (TRACE_SHA3_OUTPUTS, shapes of sha3_from_trace_shapes over
    sha3_from_trace_sizes) then receive the outputs in place, every pass."""
    lib = _lib.init(device)
    fam = TRACE_SHA3
    counts = _wire_sizes(fam, lib, _wire_args(fam, _trace_sha3_records(trace)))
    p = _wire_args(fam, _trace_sha3_records(trace, counts), (int(randomness),), outs)
    s = _open(lib, lib.zk_sha3_from_trace_open, p.n, (p.keep, p.t, p.w), ctypes.byref(p.t), ptr(p.keep[-1]),
              ctypes.byref(p.w) if p.w is not None else None, p.opts, cls=Sha3FromTraceSession)
    s.family, s.shapes = fam, p.shapes
    return s


# ---- State circuit from compact trace records (zk_state_verify_from_trace* / zk_state_ops_from_trace* / zk_state_assign_from_trace*) ---------------------------------
def _state_from_trace_args(trace, outs=()):
    """The RW half of `trace` (see _evm_witness_from_trace_args; prev and steps are not read and may be missing) -> (ZkTrace, opts, kept
    arrays, n_rw); outs: flat output buffers as for _rw_args, prepared with the inputs"""
    rec = {k: trace.get(k) for k in TRACE_INPUTS if k != "steps"}
    rec["rw_base"] = trace.get("rw_base", 1)
    n = _rows(rec.get("head"))
    _check_flat_outs(outs, n)
    t, _, opts, keep, _ = _evm_witness_from_trace_args(rec, optional=("prev",))
    bufs = [o[0] for o in outs]
    if any(b is not None for b in bufs):
        if not opts or not all(_is_device(b) for b in bufs if b is not None):
            raise ValueError("output buffers need device inputs (ZK_OPT_DEVICE_PTRS)")
        if not all(_is_contiguous(b) for b in bufs if b is not None):
            raise ValueError("output buffer must be contiguous")
    return t, opts, (keep, t, bufs), n


def open_state_verify_from_trace(trace, device=None):
    """The State circuit's verdict over the RW ops of compact trace records (zk_state_verify_from_trace_open) -> Session over the n_ops =
    1 + kept ops State rows, exactly open_state_verify_from_rw over the rw / rw_flags open_evm_witness_from_trace writes for the same
    records, without those rows.  CUDA tensors are used in place: id / addr / val / pool must stay unchanged while the session lives."""
    lib = _lib.init(device)
    t, opts, keep, _ = _state_from_trace_args(trace)
    return _open_n_ops(lib, lib.zk_state_verify_from_trace_open, keep, ctypes.byref(t), opts)


def open_state_ops_from_trace(trace, ops_dev=None, op_flags_dev=None, device=None):
    """The State op list of the RW ops of compact trace records (zk_state_ops_from_trace_open) -> RekeySession, exactly
    open_state_ops_from_rw over the expanded rows; ops_dev / op_flags_dev as there (capacity n_rw + 1 ops)."""
    lib = _lib.init(device)
    t, opts, keep, n = _state_from_trace_args(trace, ((ops_dev, "ops_dev", 8, 48), (op_flags_dev, "op_flags_dev", 4, 1)))
    return _open_n_ops(lib, lib.zk_state_ops_from_trace_open, keep, ctypes.byref(t), ptr(ops_dev), ptr(op_flags_dev), opts, cls=RekeySession, n=n)


def open_state_assign_from_trace(trace, rows_dev=None, row_flags_dev=None, mpt_dev=None, device=None, compact=False):
    """The State witness of the RW ops of compact trace records (zk_state_assign_from_trace_open) -> AssignSession over the n_ops = 1 +
    kept ops State rows (session.n), exactly open_state_assign_from_rw over the rw / rw_flags open_evm_witness_from_trace writes for the
    same records, without those rows; rows_dev / row_flags_dev / mpt_dev as there (flat CUDA buffers of capacity n_rw + 1 rows, packed
    for n_ops).  CUDA tensors are used in place: id / addr / val / pool must stay unchanged while the session lives."""
    lib = _lib.init(device)
    outs = ((rows_dev, "rows_dev", 8, (15 if compact else 57) * 4), (row_flags_dev, "row_flags_dev", 4, 1), (mpt_dev, "mpt_dev", 8, 48))
    t, opts, keep, _ = _state_from_trace_args(trace, outs)
    if compact:
        opts |= _lib.OPT_STATE_COMPACT
    return _open_n_ops(lib, lib.zk_state_assign_from_trace_open, keep, ctypes.byref(t), ptr(rows_dev), ptr(row_flags_dev), ptr(mpt_dev), opts,
                       cls=AssignSession, compact=compact)


# ---- Exp circuit witness assignment (zk_exp_assign*) ------------------------------------------------------------------------------
def _exp_events_struct(events, max_exp_steps):
    """the ZkExpEvents block over a prepared event array (None or empty: a null pointer, dummy rows only)"""
    n = _rows(events)
    return _lib.ZkExpEvents(ptr(events, n), n, int(max_exp_steps))


def exp_assign_sizes(events, max_exp_steps=0, device=None):
    """(n_rows, n_step_rows, n_table) a list of EXP events expands to; with device tensors the counts come back from the device.
    Raises EngineError (rc = _lib.ERR_EXP_*) for events outside the wire's domain."""
    lib = _lib.init(device)
    _expect(events, "exp events", 8, (None, 5, 4))
    (events,), opts = _prep([events])
    t = _exp_events_struct(events, max_exp_steps)
    a, b, c = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    check(lib.zk_exp_assign_sizes(ctypes.byref(t), opts, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)), "zk_exp_assign_sizes", lib)
    return int(a.value), int(b.value), int(c.value)


def _exp_assign_args(events, max_exp_steps, device, outs=(None, None)):
    """zk_exp_assign_open / zk_exp_assign -> (ZkExpEvents, opts, kept arrays, sizes or None); outs: (rows_out, table_out), checked
    against the sizes (one size pass of their own: zk_exp_assign_sizes) and prepared with the input (kept arrays 1..2).  Without
    output buffers nothing is sized here: the open's own size pass is the only one (ExpAssignSession reads its counts back)."""
    _expect(events, "exp events", 8, (None, 5, 4))
    sizes = None
    if any(o is not None for o in outs):
        sizes = n_rows, _, n_table = exp_assign_sizes(events, max_exp_steps, device)
        _expect(outs[0], "rows", 8, (21, n_rows, 4))
        _expect(outs[1], "table", 8, (n_table, 11, 4))
    keep, opts = _prep([events, *outs], outputs=(1, 2))
    return _exp_events_struct(keep[0], max_exp_steps), opts, keep, sizes


class ExpAssignSession(Session):
    """Exp-circuit witness assignment session: launch()/collect() like the circuits; read() for the outputs."""

    def read(self):
        """-> (rows uint64[21, n, 4], table uint64[m, 11, 4]) on the host"""
        rows, table = np.empty((21, self.n, 4), dtype=np.uint64), np.empty((self.n_table, 11, 4), dtype=np.uint64)
        check(self._lib.zk_exp_assign_read(self._h, ptr(rows), ptr(table, self.n_table)), "zk_exp_assign_read", self._lib)
        return rows, table


def open_exp_assign(events, max_exp_steps=0, rows_dev=None, table_dev=None, device=None):
    """events uint64[n, 5, 4] (row-major EXP events: identifier, base lo / hi, exponent lo / hi; include/zkevm_hip.h) ->
    ExpAssignSession over the n_rows circuit rows (n, n_step, n_table: the open's counts).  numpy inputs are staged to HBM; torch CUDA
    tensors are used in place and the optional rows_dev uint64[21, n_rows, 4] / table_dev uint64[n_table, 11, 4] (sized with
    exp_assign_sizes) receive the outputs, ready for open_exp / open_evm."""
    lib = _lib.init(device)
    t, opts, keep, _ = _exp_assign_args(events, max_exp_steps, device, (rows_dev, table_dev))
    if (rows_dev is not None or table_dev is not None) and not opts:
        raise ValueError("output buffers need device inputs (ZK_OPT_DEVICE_PTRS)")
    s = _open(lib, lib.zk_exp_assign_open, 0, keep, ctypes.byref(t), ptr(keep[1]), ptr(keep[2]), opts, cls=ExpAssignSession)
    a, b, c = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    check(lib.zk_exp_assign_counts(s._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)), "zk_exp_assign_counts", lib)
    s.n, s.n_step, s.n_table = int(a.value), int(b.value), int(c.value)
    return s
