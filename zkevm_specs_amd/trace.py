"""Compact trace records for zk_evm_witness_from_trace (include/zkevm_hip.h): RW ops and step records in their natural widths.

An RW op is a head word, four 64-bit integers and the 256-bit pool words its head names; a step is thirteen 64-bit words.  The device
blows them up to the wire rows (`rw` / `rw_flags` / `steps` of zk_evm_tables), so a producer of traces uploads 40-odd bytes per RW row
instead of 452.

  RWDictionary            the reference's builder (evm_circuit/typing.py:464-845: same constructor and method signatures, its Word / FQ
                          sanity asserts, the reversion rows of its state writes, the TxLog address packing), appending integers to a list
                          instead of building RWTableRow objects; .ops() -> records
  step_records(steps)     step objects (StepState attributes) -> uint64[n, 13]
  rw_ops_from_wire, step_records_from_wire   the inverses of the device's expansion, for wires that exist already
  trace_records(ops, steps)                  one dict for engine.open_evm_witness_from_trace / oneshot.evm_witness_from_trace

The encoder is canonical: a value below 2^64 is narrow, a zero Word is absent, consecutive counters travel as rw_base.  What the records
cannot hold raises UnsupportedOnDevice, never a guess.
"""
import numpy as np

from .arithmetic import FQ, Word
from .errors import UnsupportedOnDevice
from .evm_tables import RW, CallContextFieldTag, Target
from .flatten import step_cells
from .wire import FR_MODULUS

# head bits (csrc/trace_witness.hpp)
H_WRITE, H_TAG_SHIFT, H_FIELD_SHIFT, H_VALUE_WORD, H_PREV_WORD = 1, 1, 8, 1 << 16, 1 << 17
H_ADDR_POOL, H_KEY, H_VALUE_POOL, H_PREV_POOL, H_AUX = 1 << 20, 1 << 21, 1 << 22, 1 << 23, 1 << 24
HEAD_MASK = 0x1 | (0xF << 1) | (0xFF << 8) | (0x3 << 16) | (0x1F << 20)
RW_NCELLS, STEP_NCELLS, STEP_WORDS = 14, 13, 13
_P_LIMBS = [(FR_MODULUS >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)]
_WORD_CONTEXT_FIELDS = {int(CallContextFieldTag[k]) for k in ("CallerAddress", "CalleeAddress", "Value", "CodeHash")}


# ---- the canonical encoder, on wire-shaped arrays ------------------------------------------------------------------------------------
def _below_p(cells):
    """bool[n]: the cells uint64[n, 4] are canonical (< p)"""
    ok = np.ones(cells.shape[0], dtype=bool)
    for i in np.nonzero(cells[:, 3] >= np.uint64(_P_LIMBS[3]))[0]:
        ok[i] = int.from_bytes(cells[i].tobytes(), "little") < FR_MODULUS
    return ok


def _narrow(c):
    return (c[:, 1] == 0) & (c[:, 2] == 0) & (c[:, 3] == 0)


def _half(c):
    return (c[:, 2] == 0) & (c[:, 3] == 0)


def _need(ok, what):
    if not bool(np.all(ok)):
        raise UnsupportedOnDevice(f"trace records: {what} (row {int(np.argmin(ok))})")


def _word_of(lo, hi):
    """uint64[n, 4] of the Words with halves lo / hi (each below 2^128)"""
    return np.stack([lo[:, 0], lo[:, 1], hi[:, 0], hi[:, 1]], axis=1)


def rw_ops_from_wire(rw, rw_flags):
    """RW ops of the wire arrays rw uint64[n, 14, 4] / rw_flags uint32[n] (flatten_rw_table's result) -> dict(head uint32[n], id, addr, val,
    prev uint64[n], rw_counter uint64[n] or None with rw_base, pool uint64[m, 4]); raises UnsupportedOnDevice where the records cannot
    hold the table: counters or ids of 2^64 or more, rw above 1, tag above 15, field_tag above 255, key / aux / word-flagged halves of
    2^128 or more, an unflagged value with a non-zero hi cell, a non-canonical cell, counters that are not strictly ascending."""
    rw = np.ascontiguousarray(rw, dtype=np.uint64)
    flags = np.ascontiguousarray(rw_flags, dtype=np.uint32)
    n = rw.shape[0]
    if rw.shape != (n, RW_NCELLS, 4) or flags.shape != (n,):
        raise ValueError(f"rw / rw_flags: expected shapes (n, 14, 4) and (n,), got {rw.shape} and {flags.shape}")
    c = [rw[:, k] for k in range(RW_NCELLS)]
    for k, what in ((0, "an rw_counter"), (3, "an id")):
        _need(_narrow(c[k]), f"{what} of 2^64 or more")
    _need(_narrow(c[1]) & (c[1][:, 0] <= 1), "is_write above 1")
    _need(_narrow(c[2]) & (c[2][:, 0] <= 15), "a tag above 15")
    _need(_narrow(c[5]) & (c[5][:, 0] <= 255), "a field_tag above 255")
    _need(flags <= 3, "a flag word above 3")
    ctr = c[0][:, 0]
    _need(np.concatenate([[True], ctr[1:] > ctr[:-1]]), "rw_counters that are not strictly ascending")
    head = (c[1][:, 0] | (c[2][:, 0] << np.uint64(H_TAG_SHIFT)) | (c[5][:, 0] << np.uint64(H_FIELD_SHIFT))).astype(np.uint32) | (flags << np.uint32(16))
    words = np.zeros((n, 5, 4), dtype=np.uint64)
    used = np.zeros((n, 5), dtype=bool)
    # address: FQ
    _need(_below_p(c[4]), "an address cell of p or more")
    used[:, 0] = ~_narrow(c[4])
    words[:, 0] = c[4]
    narrow = {"addr": c[4][:, 0].copy()}
    narrow["addr"][used[:, 0]] = 0
    # storage_key, aux0: Words
    for slot, lo, hi, what in ((1, 6, 7, "storage_key"), (4, 12, 13, "aux0")):
        _need(_half(c[lo]) & _half(c[hi]), f"a {what} half of 2^128 or more")
        words[:, slot] = _word_of(c[lo], c[hi])
        used[:, slot] = words[:, slot].any(axis=1)
    # value, value_prev: Word (flagged) or FQ
    for slot, lo, hi, bit, name in ((2, 8, 9, 1, "val"), (3, 10, 11, 2, "prev")):
        word = (flags & bit) != 0
        _need(~word | (_half(c[lo]) & _half(c[hi])), "a word-flagged value half of 2^128 or more")
        _need(word | ~c[hi].any(axis=1), "an unflagged value with a non-zero hi cell")
        _need(word | _below_p(c[lo]), "an unflagged value of p or more")
        w = np.where(word[:, None], _word_of(c[lo], c[hi]), c[lo])
        used[:, slot] = ~_narrow(w)
        words[:, slot] = w
        narrow[name] = np.where(used[:, slot], np.uint64(0), w[:, 0])
    head |= (used.astype(np.uint32) << np.arange(20, 25, dtype=np.uint32)).sum(axis=1, dtype=np.uint32)
    dense = n > 0 and bool(np.all(ctr[1:] - ctr[:-1] == 1))
    return {"head": head, "id": c[3][:, 0].copy(), "addr": narrow["addr"], "val": np.ascontiguousarray(narrow["val"]),
            "prev": np.ascontiguousarray(narrow["prev"]), "rw_counter": None if dense or n == 0 else ctr.copy(),
            "rw_base": int(ctr[0]) if dense else 1, "pool": np.ascontiguousarray(words[used])}


def step_records_from_wire(steps):
    """step records uint64[n, 13] of the wire array steps uint64[n, 13, 4] (flatten_steps' result); raises UnsupportedOnDevice for an
    integer of 2^64 or more, an execution_state above 255, an is_root / is_create above 1 or a code-hash half of 2^128 or more"""
    steps = np.ascontiguousarray(steps, dtype=np.uint64)
    n = steps.shape[0]
    if steps.shape != (n, STEP_NCELLS, 4):
        raise ValueError(f"steps: expected shape (n, 13, 4), got {steps.shape}")
    c = [steps[:, k] for k in range(STEP_NCELLS)]
    for k in (0, 1, 2, 3, 4, 7, 8, 9, 10, 11, 12):
        _need(_narrow(c[k]), "a step integer of 2^64 or more")
    _need(c[0][:, 0] <= 255, "an execution_state above 255")
    _need((c[3][:, 0] <= 1) & (c[4][:, 0] <= 1), "an is_root / is_create above 1")
    _need(_half(c[5]) & _half(c[6]), "a code-hash half of 2^128 or more")
    out = np.zeros((n, STEP_WORDS), dtype=np.uint64)
    out[:, 0] = c[0][:, 0] | (c[3][:, 0] << np.uint64(8)) | (c[4][:, 0] << np.uint64(9))
    out[:, 1], out[:, 2] = c[1][:, 0], c[2][:, 0]
    for k in range(7, 13):
        out[:, k - 4] = c[k][:, 0]
    out[:, 9:13] = _word_of(c[5], c[6])
    return out


def _cells(rows, ncells, what):
    """list of int rows -> uint64[n, ncells, 4]; an int outside [0, 2^256) cannot travel"""
    try:
        raw = b"".join(int(v).to_bytes(32, "little") for r in rows for v in r)
    except OverflowError:
        raise UnsupportedOnDevice(f"trace records: {what} outside [0, 2^256)") from None
    return np.frombuffer(raw, dtype="<u8").reshape(len(rows), ncells, 4).astype(np.uint64)


def step_records(steps):
    """step objects (execution_state, rw_counter, call_id, is_root, is_create, code_hash, program_counter, stack_pointer, gas_left,
    memory_word_size, reversible_write_counter, log_id: the reference's StepState or a stand-in) -> uint64[n, 13]"""
    return step_records_from_wire(_cells([step_cells(s) for s in steps], STEP_NCELLS, "a step cell"))


def trace_records(ops=None, steps=None):
    """one records dict of RW ops (rw_ops_from_wire / RWDictionary.ops) and step records (uint64[n, 13])"""
    rec = dict(ops) if ops is not None else {"head": np.zeros(0, np.uint32), **{k: np.zeros(0, np.uint64) for k in ("id", "addr", "val", "prev")},
                                             "rw_counter": None, "rw_base": 1, "pool": np.zeros((0, 4), np.uint64)}
    rec["steps"] = np.zeros((0, STEP_WORDS), np.uint64) if steps is None else steps
    return rec


def record_bytes(rec):
    """bytes the records dict `rec` uploads"""
    return sum(int(v.nbytes) for v in rec.values() if hasattr(v, "nbytes"))


# ---- the reference's RWDictionary over integer rows ------------------------------------------------------------------------------------
def _is_word(v):
    return hasattr(v, "lo") and hasattr(v, "hi") and bool(getattr(v, "is_word", True))


def _fq(v):
    return v.n if isinstance(v, FQ) else FQ(v).n


def _halves(w):
    return FQ(w.lo).n, FQ(w.hi).n


def _value(v):
    """(lo, hi, is_word) of a Word or of anything FQ takes"""
    if _is_word(v):
        return (*_halves(v), 1)
    return _fq(v.lo) if hasattr(v, "lo") else _fq(v), 0, 0


_ZERO = Word(0)


class RWDictionary:
    """The reference's RWDictionary (evm_circuit/typing.py:464-845) appending integer rows; .ops() -> the records of rw_ops_from_wire.
    self.rows holds (rw_counter, rw, tag, id, address, field_tag, key lo, key hi, value lo, hi, prev lo, hi, aux lo, hi, flags)."""

    def __init__(self, rw_counter: int) -> None:
        self.rw_counter = rw_counter
        self.rows = []

    # -- stack, memory, call context
    def stack_read(self, call_id, stack_pointer, value):
        return self._append(RW.Read, Target.Stack, id=call_id, address=stack_pointer, value=value)

    def stack_write(self, call_id, stack_pointer, value):
        return self._append(RW.Write, Target.Stack, id=call_id, address=stack_pointer, value=value)

    def memory_read(self, call_id, memory_address, byte):
        return self._append(RW.Read, Target.Memory, id=call_id, address=memory_address, value=FQ(byte))

    def memory_write(self, call_id, memory_address, byte):
        return self._append(RW.Write, Target.Memory, id=call_id, address=memory_address, value=FQ(byte))

    def _call_context(self, rw, call_id, field_tag, value):
        if isinstance(value, int):
            value = FQ(value)
        wide = int(field_tag) in _WORD_CONTEXT_FIELDS
        assert _is_word(value) if wide else not _is_word(value)  # the reference's sanity checks
        return self._append(rw, Target.CallContext, id=call_id, address=int(field_tag), value=value)

    def call_context_read(self, call_id, field_tag, value):
        return self._call_context(RW.Read, call_id, field_tag, value)

    def call_context_write(self, call_id, field_tag, value):
        return self._call_context(RW.Write, call_id, field_tag, value)

    # -- tx log, receipt, refund
    def tx_log_write(self, tx_id, log_id, field_tag, index, value):
        if isinstance(value, int):
            value = FQ(value)
        assert _is_word(value) if int(field_tag) in (1, 2) else not _is_word(value)  # Address and Topic are Words
        return self._append(RW.Write, Target.TxLog, id=tx_id, address=FQ(index + (int(field_tag) << 32) + (log_id << 48)), value=value)

    def tx_receipt_read(self, tx_id, field_tag, value):
        return self._append(RW.Read, Target.TxReceipt, id=tx_id, field_tag=field_tag, value=FQ(value))

    def tx_receipt_write(self, tx_id, field_tag, value):
        return self._append(RW.Write, Target.TxReceipt, id=tx_id, field_tag=field_tag, value=FQ(value))

    def tx_refund_read(self, tx_id, refund):
        return self._append(RW.Read, Target.TxRefund, id=tx_id, value=FQ(refund), value_prev=FQ(refund))

    def tx_refund_write(self, tx_id, refund, refund_prev, rw_counter_of_reversion=None):
        return self._state_write(Target.TxRefund, id=tx_id, value=FQ(refund), value_prev=FQ(refund_prev), rw_counter_of_reversion=rw_counter_of_reversion)

    # -- access lists
    def tx_access_list_account_write(self, tx_id, account_address, value, value_prev, rw_counter_of_reversion=None):
        return self._state_write(Target.TxAccessListAccount, id=tx_id, address=account_address, value=FQ(value), value_prev=FQ(value_prev),
                                 rw_counter_of_reversion=rw_counter_of_reversion)

    def tx_access_list_account_read(self, tx_id, account_address, value):
        return self._append(RW.Read, Target.TxAccessListAccount, id=tx_id, address=account_address, value=FQ(value), value_prev=FQ(value))

    def tx_access_list_account_storage_write(self, tx_id, account_address, storage_key, value, value_prev, rw_counter_of_reversion=None):
        return self._state_write(Target.TxAccessListAccountStorage, id=tx_id, address=account_address, storage_key=storage_key, value=FQ(value),
                                 value_prev=FQ(value_prev), rw_counter_of_reversion=rw_counter_of_reversion)

    def tx_access_list_account_storage_read(self, tx_id, account_address, storage_key, value):
        return self._append(RW.Read, Target.TxAccessListAccountStorage, id=tx_id, address=account_address, storage_key=storage_key, value=FQ(value),
                            value_prev=FQ(value))

    # -- accounts and storage
    def account_read(self, account_address, field_tag, value):
        if isinstance(value, int):
            value = FQ(value)
        return self._append(RW.Read, Target.Account, address=account_address, field_tag=field_tag, value=value, value_prev=value)

    def account_write(self, account_address, field_tag, value, value_prev, rw_counter_of_reversion=None):
        value, value_prev = (FQ(v) if isinstance(v, int) else v for v in (value, value_prev))
        return self._state_write(Target.Account, address=account_address, field_tag=field_tag, value=value, value_prev=value_prev,
                                 rw_counter_of_reversion=rw_counter_of_reversion)

    def account_storage_read(self, account_address, storage_key, value, tx_id, value_committed):
        return self._append(RW.Read, Target.AccountStorage, id=tx_id, address=account_address, storage_key=storage_key, value=value,
                            value_prev=value, aux0=value_committed)

    def account_storage_write(self, account_address, storage_key, value, value_prev, tx_id, value_committed, rw_counter_of_reversion=None):
        return self._state_write(Target.AccountStorage, id=tx_id, address=account_address, storage_key=storage_key, value=value,
                                 value_prev=value_prev, aux0=value_committed, rw_counter_of_reversion=rw_counter_of_reversion)

    # -- rows
    def _state_write(self, tag, rw_counter_of_reversion=None, value=_ZERO, value_prev=_ZERO, **keys):
        """a write, and with rw_counter_of_reversion the row that undoes it at that counter (value and value_prev swapped)"""
        self._append(RW.Write, tag, value=value, value_prev=value_prev, **keys)
        if rw_counter_of_reversion is None:
            return self
        return self._append(RW.Write, tag, value=value_prev, value_prev=value, rw_counter=rw_counter_of_reversion, **keys)

    def _append(self, rw, tag, id=0, address=0, field_tag=0, storage_key=_ZERO, value=_ZERO, value_prev=_ZERO, aux0=_ZERO, rw_counter=None):
        if rw_counter is None:
            rw_counter = self.rw_counter
            self.rw_counter += 1
        vlo, vhi, vw = _value(value)
        plo, phi, pw = _value(value_prev)
        self.rows.append((_fq(rw_counter), int(rw), int(tag), _fq(id), _fq(address), _fq(field_tag), *_halves(storage_key), vlo, vhi, plo, phi,
                          *_halves(aux0), vw | (pw << 1)))
        return self

    def ops(self):
        """the rows as records, in the RW table's order: sorted by rw_counter, exact duplicates dropped (the table is a set; the first
        occurrence's type bits stay).  Two different rows with one rw_counter, or a value outside the records' widths, raise
        UnsupportedOnDevice."""
        seen = {}
        for r in self.rows:
            seen.setdefault(r[:RW_NCELLS], r[RW_NCELLS])
        rows = sorted(seen)
        return rw_ops_from_wire(_cells(rows, RW_NCELLS, "an RW cell"), np.array([seen[r] for r in rows], dtype=np.uint32))
