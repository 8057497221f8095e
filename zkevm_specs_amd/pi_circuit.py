"""Host-side mirror of `zkevm_specs.pi_circuit.verify_circuit(witness, MAX_TXS, MAX_CALLDATA_BYTES, MAX_WITHDRAWALS)`
(pi_circuit.py:338-459).  Both halves run on the device: the copy constraints in front of the gates (:355-445) — block / tx /
withdrawal table cells and the public inputs' words against the byte strings of `witness.copy_constrains` — are listed here in
the reference's statement order (it consumes `witness.copy_constrains` with pop(0); so does this) and evaluated by one launch of
`zk_pi_copy_verify` (csrc/pi_circuit.hpp pi_copy_check: bytes_to_fq's length assert and the equality, per entry); the per-row
gates and lookups (`check_row`, :150-322) by one launch of `zk_pi_verify`.  Every copy-constraint failure is an AssertionError
in the reference; the gate pass reports the exception class of its first failing row."""
from dataclasses import dataclass
from types import SimpleNamespace
from typing import List, Optional

import numpy as np

from . import oneshot
from .errors import raise_for_code
from .flatten import _n, flatten_keccak_tuples, flatten_pi_gas_table, flatten_pi_rows

BLOCK_LEN = (8 + 256) * 2   # PUBLIC_INPUTS_BLOCK_LEN (util/param.py:126)
TX_LEN = 10                 # PUBLIC_INPUTS_TX_LEN (util/param.py:128)
MAX_N_BYTES = 31            # util/param.py: bytes_to_fq asserts len(value) <= MAX_N_BYTES (on the device: pi_copy_check site 1)
KECCAK_RAND = BYTE_POW_BASE = 255  # pi_circuit.py:834-836


PI_COPY_CELL = 0xFFFFFFFF  # csrc/pi_circuit.hpp: the 32 bytes are a canonical cell compared as is


class _Constraints:
    """the copy constraints of one witness, in the reference's statement order"""

    def __init__(self, cc):
        self.cc, self.cells, self.entries = cc, [], []

    def cell_eq(self, cell, other):       # `Word.__eq__`: lo / hi expressions compared (util/arithmetic.py:138-140)
        self.cells.append(_n(cell))
        self.entries.append((PI_COPY_CELL, int(_n(other)).to_bytes(32, "little")))

    def pop(self):                        # copy_constrains.pop(0)[::-1]: kept as popped, the device reads it big-endian
        return bytes(self.cc.pop(0))

    def eq(self, cell, entry):            # assert cell == bytes_to_fq(entry[::-1])
        self.cells.append(_n(cell))
        self.entries.append((len(entry), entry))

    def lo_hi(self, lo, hi, is_word):     # lo_le = pop; hi_le = pop if is_word else b""; then the two asserts (pops come first)
        lo_e = self.pop()
        hi_e = self.pop() if is_word else b""
        self.eq(lo, lo_e)
        self.eq(hi, hi_e)

    def wire(self):
        n = len(self.cells)
        cells = np.zeros((n, 4), dtype=np.uint64)
        data = np.zeros((n, 32), dtype=np.uint8)
        lens = np.zeros(n, dtype=np.uint32)
        for i, (c, (ln, e)) in enumerate(zip(self.cells, self.entries)):
            cells[i] = np.frombuffer(int(c).to_bytes(32, "little"), dtype="<u8")
            lens[i] = ln
            k = min(len(e), 32)  # an entry longer than its slot fails bytes_to_fq's length assert whatever its bytes
            data[i, :k] = np.frombuffer(e[:k], dtype=np.uint8)
        return cells, data, lens


def list_copy_constraints(witness, MAX_TXS, MAX_CALLDATA_BYTES, MAX_WITHDRAWALS):
    """-> (_Constraints, pending): the constraints listed until `witness.copy_constrains` ran out (`pending` = the IndexError the
    reference's pop(0) raises at that statement, raised after the constraints in front of it have passed), else all of them"""
    rows, public_inputs = witness.rows, witness.public_inputs
    block_table, tx_table, withdrawal_table = witness.block_table, witness.tx_table, witness.withdrawal_table
    C = _Constraints(witness.copy_constrains)
    try:
        # constrain witness rpi digest lo/hi equals pi input keccak lo/hi (:358)
        C.cell_eq(rows[0].rpi_digest_word.lo, public_inputs.pi_keccak.lo)
        C.cell_eq(rows[0].rpi_digest_word.hi, public_inputs.pi_keccak.hi)
        # block table word_or_value equals witness rpi bytes in vertical order (:361-372)
        for i in range(BLOCK_LEN // 2 + 1):
            block_row = block_table.table[i]
            C.lo_hi(block_row.lo, block_row.hi, block_row.is_word)
        # block_hash, state_root, state_root_prev (:374-393)
        for w in (public_inputs.block_hash, public_inputs.state_root, public_inputs.state_root_prev):
            C.lo_hi(w.lo, w.hi, True)
        # tx table id, index, value per row (:395-410)
        tx_len = TX_LEN * MAX_TXS + 1
        for i in range(tx_len):
            tx_row = tx_table.table[i]
            C.eq(tx_row.tx_id, C.pop())
            C.eq(tx_row.index, C.pop())
            C.lo_hi(tx_row.value.lo, tx_row.value.hi, tx_row.value.is_word)
        # tx calldata values (:412-423)
        for i in range(MAX_CALLDATA_BYTES):
            value = tx_table.table[tx_len + i].value
            C.lo_hi(value.lo, value.hi, value.is_word)
        # withdrawal table (:425-444)
        for i in range(MAX_WITHDRAWALS):
            wd = withdrawal_table.table[i]
            C.eq(wd.id, C.pop())
            C.eq(wd.validator_id, C.pop())
            C.lo_hi(wd.address.lo, wd.address.hi, True)
            C.eq(wd.amount, C.pop())
    except IndexError as e:  # pop(0) from an exhausted list / a table shorter than the circuit's shape
        return C, e
    return C, None


def verify_circuit(witness, MAX_TXS, MAX_CALLDATA_BYTES, MAX_WITHDRAWALS):
    rows = witness.rows
    C, pending = list_copy_constraints(witness, MAX_TXS, MAX_CALLDATA_BYTES, MAX_WITHDRAWALS)
    if C.cells:
        res, _ = oneshot.pi_copy_verify(*C.wire())  # zk_pi_copy_verify
        raise_for_code(res.first_fail_code, f"PI circuit copy constraint {res.first_fail_row}")
    if pending is not None:
        raise pending
    # gates (:447-459): one device pass over all rows
    res, _ = oneshot.pi_verify(flatten_pi_rows(rows), flatten_keccak_tuples(witness.keccak_table.table),
                               flatten_pi_gas_table(witness.calldata_gas_cost_table), int(witness.circuit_len), KECCAK_RAND, BYTE_POW_BASE)
    raise_for_code(res.first_fail_code, f"PI circuit row {res.first_fail_row}")
    return res


# ---- public_data2witness on the device (pi_circuit.py:461-1073) ------------------------------------------------------------------------
@dataclass
class Block:
    """Block header (pi_circuit.py:461-482); public_data2witness reads hash, coinbase, state_root, prev_randao, number, gas_limit, time,
    base_fee and withdrawals_root"""
    hash: int = 0
    parent_hash: int = 0
    uncle_hash: int = 0
    coinbase: int = 0
    state_root: int = 0
    tx_hash: int = 0
    receipt_hash: int = 0
    bloom: bytes = bytes(256)
    prev_randao: int = 0
    number: int = 0
    gas_limit: int = 0
    gas_used: int = 0
    time: int = 0
    extra: bytes = b""
    mix_digest: int = 0
    nonce: int = 0
    base_fee: int = 0
    withdrawals_root: int = 0


@dataclass
class Transaction:
    nonce: int
    gas_price: int
    gas: int
    from_addr: int
    to_addr: Optional[int]
    value: int
    data: bytes
    tx_sign_hash: int

    @classmethod
    def default(cls):
        return cls(0, 0, 0, 0, 0, 0, b"", 0)


@dataclass
class Withdrawal:
    id: int
    validator_id: int
    address: int
    amount: int

    @classmethod
    def default(cls):
        return cls(0, 0, 0, 0)


@dataclass
class PublicData:
    chain_id: int
    block: Block
    state_root_prev: int
    block_hashes: List[int]
    txs: List[Transaction]
    withdrawals: List[Withdrawal]


@dataclass(frozen=True)
class TxCallDataGasCostAccRow:
    """pi_circuit.TxCallDataGasCostAccRow (:66-70): hashable, the gas-cost table is a set"""
    tx_id: object
    is_final: object
    gas_cost_acc: object


@dataclass
class Witness:
    """pi_circuit.Witness (:324-334) over the device's wire"""
    rows: list
    public_inputs: object
    calldata_gas_cost_table: set
    keccak_table: object
    block_table: object
    tx_table: object
    withdrawal_table: object
    circuit_len: int
    copy_constrains: list


def _word_check(v):
    """Word(int) (util/arithmetic.py:99-123): the assert, then to_bytes"""
    assert v < 256**32
    v.to_bytes(32, "little")


def _classify(pd, MAX_TXS, MAX_CALLDATA_BYTES, MAX_WITHDRAWALS):
    """Raises what the reference's public_data2witness raises for inputs outside its domain, in its statement order (:861-907):
    AssertionError for the counts, len(block_hashes) and ints of 2^256 and more in a Word; OverflowError from to_bytes."""
    b = pd.block
    # block_table_value_column (:639-654), block_table_raw_byte_values (:656-680)
    for v in (b.prev_randao, b.base_fee, b.withdrawals_root):
        _word_check(v)
    assert len(pd.block_hashes) == 256
    for h in pd.block_hashes:
        _word_check(h)
    b.coinbase.to_bytes(20, "big")
    for v in (b.gas_limit, b.number, b.time):
        v.to_bytes(8, "big")
    pd.chain_id.to_bytes(8, "big")
    # the extra fields (:866-874)
    for v in (b.hash, b.state_root, pd.state_root_prev):
        _word_check(v)
    # tx_table_cols (:802-812): the value columns, then the calldata columns
    assert len(pd.txs) <= MAX_TXS
    for tx in pd.txs:
        for v in (tx.gas_price, tx.value, tx.tx_sign_hash):
            _word_check(v)
    total = sum(len(tx.data) for tx in pd.txs)
    assert total <= MAX_CALLDATA_BYTES
    # tx_table_raw_bytes (:717-730)
    assert len(pd.txs) > 0
    for tx in pd.txs:
        tx.nonce.to_bytes(8, "big")
        tx.gas.to_bytes(8, "big")
        tx.from_addr.to_bytes(20, "big")
        (tx.to_addr or 0).to_bytes(20, "big")
    # withdrawal_table_cols (:696-715), withdrawal_table_raw_bytes (:682-694)
    assert len(pd.withdrawals) <= MAX_WITHDRAWALS
    for w in pd.withdrawals:
        _word_check(w.address)
    assert len(pd.withdrawals) > 0
    for w in pd.withdrawals:
        w.validator_id.to_bytes(8, "big")
        w.amount.to_bytes(8, "big")


def _words(vals):
    """ints below 2^256 -> uint64[len, 4]"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype="<u8").reshape(len(vals), 4).copy()


def public_data_inputs(pd, MAX_TXS, MAX_CALLDATA_BYTES, MAX_WITHDRAWALS):
    """the `pd` dict of engine._pi_assign_args for a PublicData (this module's or the reference's); call _classify first"""
    b = pd.block
    txs, wds = list(pd.txs), list(pd.withdrawals)
    datas = [bytes(tx.data) for tx in txs]
    offsets = np.zeros(len(txs) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(d) for d in datas], dtype=np.uint64) if txs else []
    from .flatten import FR_MODULUS

    return {
        "chain_id": int(pd.chain_id),
        "block": _words([b.hash, b.coinbase, b.state_root, b.prev_randao, b.number, b.gas_limit, b.time, b.base_fee, b.withdrawals_root]),
        "state_root_prev": _words([pd.state_root_prev])[0], "block_hashes": _words(list(pd.block_hashes)),
        "tx_fields": _words([v for tx in txs for v in (tx.nonce, tx.gas_price, tx.gas, tx.from_addr, tx.to_addr or 0, tx.value,
                                                       tx.tx_sign_hash)]).reshape(len(txs), 7, 4),
        "to_is_none": np.array([1 if tx.to_addr is None else 0 for tx in txs], dtype=np.uint32),
        "calldata": np.frombuffer(b"".join(datas), dtype=np.uint8).copy(), "offsets": offsets,
        # the table's FQ(withdrawal.id): the cell, whatever the integer's width
        "withdrawals": _words([v for w in wds for v in (int(w.id) % FR_MODULUS, w.validator_id, w.address, w.amount)]).reshape(len(wds), 4, 4),
        "max_txs": int(MAX_TXS), "max_calldata_bytes": int(MAX_CALLDATA_BYTES), "max_withdrawals": int(MAX_WITHDRAWALS),
    }


def witness_from_wire(wire, mod=None):
    """the Witness over the arrays of zk_pi_assign; `mod`: the reference's pi_circuit module, for its own Row / table classes (whose
    fields do field arithmetic), else this package's stand-ins"""
    from .objects import FQ as _FQ, Word as _Word, WordOrValue as _WoV, _cols, _rows
    from .wire import cells_to_ints

    if mod is not None:
        from zkevm_specs.util import FQ, Word, WordOrValue

        word = lambda lo, hi: Word((FQ(lo), FQ(hi)))  # noqa: E731
        wov = lambda lo, hi, f: WordOrValue(word(lo, hi)) if f else WordOrValue(FQ(lo))  # noqa: E731
        TxRow, WdRow, Row, Gas = mod.TxTableRow, mod.WithdrawalTableRow, mod.Row, mod.TxCallDataGasCostAccRow
        kt, bt, tt, wt = mod.KeccakTable(), mod.BlockTable(), mod.TxTable(), mod.WithdrawalTable()
        PI = mod.PublicInputs
    else:
        FQ, word, wov = _FQ, _Word, _WoV
        TxRow = lambda a, b, c, d: SimpleNamespace(tx_id=a, tag=b, index=c, value=d)  # noqa: E731
        WdRow = lambda a, b, c, d: SimpleNamespace(id=a, validator_id=b, address=c, amount=d)  # noqa: E731
        Row = None
        Gas = TxCallDataGasCostAccRow
        kt, bt, tt, wt = SimpleNamespace(table=set()), SimpleNamespace(table=[]), SimpleNamespace(table=[]), SimpleNamespace(table=[])
        kt.table.add((FQ(0), FQ(0), FQ(0), word(0, 0)))
        PI = lambda a, b, c, d: SimpleNamespace(pi_keccak=a, block_hash=b, state_root=c, state_root_prev=d)  # noqa: E731
    k = cells_to_ints(wire["keccak"][1])
    kt.table.add((FQ(k[0]), FQ(k[1]), FQ(k[2]), word(k[3], k[4])))
    for (lo, hi), f in zip(_rows(wire["block_table"]), wire["block_flags"]):
        bt.table.append(wov(lo, hi, int(f)))
    tx_rows = [TxRow(FQ(c[0]), FQ(c[1]), FQ(c[2]), wov(c[3], c[4], int(f))) for c, f in zip(_rows(wire["tx_table"]), wire["tx_flags"])]
    tt.table.extend(tx_rows)
    wd_rows = [WdRow(FQ(c[0]), FQ(c[1]), word(c[2], c[3]), FQ(c[4])) for c in _rows(wire["wd_table"])]
    wt.table.extend(wd_rows)
    zero_tx, zero_wd = TxRow(FQ(0), FQ(0), FQ(0), wov(0, 0, 0)), WdRow(FQ(0), FQ(0), word(0, 0), FQ(0))
    rows = []
    n_tx, n_wd = len(tx_rows), len(wd_rows)
    for i, c in enumerate(_cols(wire["rows"])):
        txr = tx_rows[i] if i < n_tx else zero_tx
        wdr = wd_rows[i - n_tx] if n_tx <= i < n_tx + n_wd else zero_wd
        cells = [FQ(x) for x in c[0:15]] + [word(c[15], c[16]), FQ(c[17]), kt, txr, wdr]
        if Row is not None:
            rows.append(Row(*cells))
        else:
            names = ("q_bytes_last", "q_tx_table", "q_tx_calldata", "q_tx_calldata_start", "q_rpi_keccak_lookup", "q_rpi_value_start", "tx_id_inv",
                     "tx_value_lo_inv", "tx_id_diff_inv", "calldata_gas_cost", "is_final", "q_withdrawal_table", "rpi_bytes", "rpi_bytes_keccakrlc",
                     "rpi_value_lc", "rpi_digest_word", "q_rpi_byte_enable", "keccak_table", "tx_table", "withdrawal_table")
            rows.append(SimpleNamespace(**dict(zip(names, cells))))
    gas = set(Gas(FQ(a), FQ(b), FQ(c)) for a, b, c in _rows(wire["gas"]))
    p = _rows(wire["public_inputs"])
    raw, cc, at = wire["raw_bytes"].tobytes(), [], 0
    for ln in wire["raw_lens"].tolist():
        cc.append(raw[at:at + ln])
        at += ln
    pub = PI(*[word(lo, hi) for lo, hi in p])
    if mod is not None:  # (the reference's tests tell a witness from public data by its class)
        return mod.Witness(rows, pub, gas, kt, bt, tt, wt, int(wire["rows"].shape[1]), cc)
    return Witness(rows, pub, gas, kt, bt, tt, wt, int(wire["rows"].shape[1]), cc)


def public_data2witness(public_data, MAX_TXS, MAX_CALLDATA_BYTES, MAX_WITHDRAWALS, device=None, reference=None):
    """Mirror of `zkevm_specs.pi_circuit.public_data2witness` (pi_circuit.py:839-1073): rows, tables and copy constraints computed by
    zk_pi_assign.  Raises the reference's exception class for every input it refuses, classified on the host in its statement order.
    Returns this module's Witness over stand-in objects; with `reference` = the reference's pi_circuit module, that module's own
    Witness / Row / table objects (its tests edit them and its verify_circuit does field arithmetic on them).  This package's
    verify_circuit takes either."""
    _classify(public_data, MAX_TXS, MAX_CALLDATA_BYTES, MAX_WITHDRAWALS)
    _, wire = oneshot.pi_assign(public_data_inputs(public_data, MAX_TXS, MAX_CALLDATA_BYTES, MAX_WITHDRAWALS), KECCAK_RAND, BYTE_POW_BASE,
                                device=device)
    return witness_from_wire(wire, reference)


def public_data2witness_reference(public_data, MAX_TXS, MAX_CALLDATA_BYTES, MAX_WITHDRAWALS, device=None):
    """public_data2witness returning the reference's own objects: the entry tools/run_reference_suite.py binds in the reference's tests
    (the reference must be importable)"""
    import zkevm_specs.pi_circuit as ref

    return public_data2witness(public_data, MAX_TXS, MAX_CALLDATA_BYTES, MAX_WITHDRAWALS, device=device, reference=ref)


def verify_public_data(pd, device=None):
    """The whole PI circuit from raw public data without a host copy of the rows: assign -> copy constraints -> gates, each session on
    the device pointers of the one before.  `pd`: the dict of engine._pi_assign_args with torch CUDA tensors.
    -> (copy-constraint Result, gate Result)"""
    import torch

    from . import engine

    dev = pd["block"].device
    shapes = engine.pi_assign_shapes(pd["max_txs"], pd["max_calldata_bytes"], pd["max_withdrawals"], pd["calldata"].shape[0])
    outs = {k: torch.zeros(shapes[k][0], dtype={8: torch.int64, 4: torch.int32, 1: torch.uint8}[np.dtype(shapes[k][1]).itemsize], device=dev)
            for k in ("rows", "gas", "keccak", "cc_cells", "cc_bytes", "cc_lens")}
    with engine.open_pi_assign(pd, KECCAK_RAND, BYTE_POW_BASE, outs=outs, device=device) as asg:
        asg.run()
        lib = asg._lib
        args, opts, keep = engine._pi_copy_args(outs["cc_cells"], outs["cc_bytes"], outs["cc_lens"])
        with engine._open(lib, lib.zk_pi_copy_open, args[3], keep, *args, opts) as cs:
            copy_res = cs.run()
        with engine.open_pi(outs["rows"], outs["keccak"], outs["gas"], shapes["rows"][0][1], KECCAK_RAND, BYTE_POW_BASE, device=device) as ps:
            gate_res = ps.run()
    return copy_res, gate_res
