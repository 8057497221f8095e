"""The EVM circuit's tx, block and withdrawal tables from a block's objects, built on the device (zk_evm_tables_from_block).

`Transaction`, `Block` and `Withdrawal` carry the constructor signatures of the reference's witness builders
(`evm_circuit/typing.py:92-103, 157-169, 290-296`); `tables_from_block` takes them — or the reference's own objects, it only reads
attributes — and returns what `flatten_tx_table`, `flatten_block_table` and `flatten_withdrawal_table` return for
`Tables(block_table=set(block.table_assignments()), tx_table=set(chain(*[tx.table_assignments() for tx in txs])),
withdrawal_table=set(chain(*[w.table_assignments() for w in withdrawals])), ...)`, without running those loops: the host packs the raw
fields (288 bytes per tx, the calldata as it is) and the device unrolls them.

What stays on the host, because it is about Python values and not about rows:
  * txs and withdrawals are sorted by `FQ(id)`, exact duplicates are dropped (the reference's tables are sets); two different objects
    with one id raise `UnsupportedOnDevice` (their rows would interleave);
  * ints outside [0, 2^256) that feed `FQ(...)` cells are reduced mod p (exact: that is what FQ does);
  * `Word(int)`'s outcomes (`util/arithmetic.py:115-118`): `AssertionError` for a value of 2^256 or more, `OverflowError` for a negative
    one, in the reference's order of evaluation.
"""
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

from . import engine, oneshot
from .errors import UnsupportedOnDevice
from .objects import FQ, WordOrValue

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
TX_SIGN_HASH_MOCK = 1234  # typing.py:265 ("Mock value for TxSignHash"); an object may carry its own `tx_sign_hash`
GAS_COST_ACCESS_LIST_ADDRESS, GAS_COST_ACCESS_LIST_STORAGE = 2400, 1900  # util/param.py:80-82 (applied on the device)

AccessTuple = namedtuple("AccessTuple", "address storage_keys")


class Block:
    """evm_circuit/typing.py:92-114"""

    def __init__(self, coinbase=0x10, gas_limit=int(15e6), number=0, timestamp=0, prev_randao=0, base_fee=int(1e9), chainid=0x01,
                 withdrawal_root=0, history_hashes=[]):  # noqa: B006 (the reference's signature)
        assert len(history_hashes) <= min(256, number)
        self.coinbase = coinbase
        self.gas_limit = gas_limit
        self.number = number
        self.timestamp = timestamp
        self.prev_randao = prev_randao
        self.base_fee = base_fee
        self.chainid = chainid
        self.history_hashes = history_hashes
        self.withdrawal_root = withdrawal_root

    def table_assignments(self):
        """the host loop (typing.py:116-137), as row stand-ins flatten_block_table reads"""
        row = lambda tag, number, v: SimpleNamespace(field_tag=FQ(tag), block_number_or_zero=FQ(number), value=v)  # noqa: E731
        return [row(1, 0, _word_cell(self.coinbase)), row(2, 0, _value_cell(self.gas_limit)), row(3, 0, _value_cell(self.number)),
                row(4, 0, _value_cell(self.timestamp)), row(5, 0, _word_cell(self.prev_randao)), row(6, 0, _word_cell(self.base_fee)),
                row(7, 0, _value_cell(self.chainid)), row(9, 0, _value_cell(self.withdrawal_root))] + [
                    row(8, (self.number - idx - 1) % P, _word_cell(h)) for idx, h in enumerate(reversed(self.history_hashes))]


class Transaction:
    """evm_circuit/typing.py:157-179"""

    def __init__(self, id=1, nonce=0, gas=21000, gas_price=int(2e9), caller_address=0xCAFE, callee_address=None, value=0,
                 call_data=bytes(), invalid_tx=0, access_list=list()):  # noqa: B006, B008 (the reference's signature)
        self.id = id
        self.nonce = nonce
        self.gas = gas
        self.gas_price = gas_price
        self.caller_address = caller_address
        self.callee_address = callee_address
        self.value = value
        self.call_data = call_data
        self.invalid_tx = invalid_tx
        self.access_list = access_list

    @classmethod
    def padding(cls, id):
        return cls(id, 0, 0, 0, 0, 0, 0, bytes(), 0, list())

    def table_assignments(self):
        """the host loop (typing.py:186-281), as row stand-ins flatten_tx_table reads: what zk_evm_tables_from_block replaces"""
        tid = FQ(self.id % P)
        row = lambda tag, index, v: SimpleNamespace(tx_id=tid, field_tag=FQ(tag), call_data_index_or_zero=FQ(index), value=v)  # noqa: E731
        gas = sum(4 if b == 0 else 16 for b in self.call_data)
        access = sum(GAS_COST_ACCESS_LIST_ADDRESS + len(t.storage_keys) * GAS_COST_ACCESS_LIST_STORAGE for t in self.access_list)
        to_none = self.callee_address is None
        fixed = [_value_cell(self.nonce), _value_cell(self.gas), _word_cell(self.gas_price), _word_cell(self.caller_address),
                 _word_cell(0 if to_none else self.callee_address), _value_cell(int(to_none)), _word_cell(self.value),
                 _value_cell(len(self.call_data)), _value_cell(gas), _value_cell(self.invalid_tx), _value_cell(access),
                 _value_cell(getattr(self, "tx_sign_hash", TX_SIGN_HASH_MOCK))]
        return [row(k + 1, 0, v) for k, v in enumerate(fixed)] + [row(13, i, WordOrValue(b, 0, False)) for i, b in enumerate(self.call_data)]


class Withdrawal:
    """evm_circuit/typing.py:290-300"""

    def __init__(self, id=0, validator_id=0, address=0xCAFE, amount=int(1e9)):
        self.id = id
        self.validator_id = validator_id
        self.address = address
        self.amount = amount

    @classmethod
    def padding(cls, id):
        return cls(id, 0, 0, 0)

    def table_assignments(self):
        return [SimpleNamespace(id=FQ(self.id % P), validator_id=FQ(self.validator_id % P), address=FQ(self.address % P), amount=FQ(self.amount % P))]


def _int(v, what):
    if isinstance(v, bool) or not isinstance(v, int):
        if hasattr(v, "n") and isinstance(v.n, int):  # an FQ
            return int(v.n)
        raise UnsupportedOnDevice(f"{what}: a {type(v).__name__} where the wire carries an int")
    return int(v)


def _fq(v, what):
    """FQ(v).n"""
    return _int(v, what) % P


def _word(v, what):
    """the int behind Word(v), with Word(int)'s own failures (util/arithmetic.py:115-118)"""
    v = _int(v, what)
    assert v < 256**32
    if v < 0:
        raise OverflowError("can't convert negative int to unsigned")
    return v


def _value_cell(v):
    """WordOrValue(FQ(v))"""
    return WordOrValue(_fq(v, "value"), 0, False)


def _word_cell(v):
    """WordOrValue(Word(v))"""
    v = _word(v, "word")
    return WordOrValue(v & ((1 << 128) - 1), v >> 128, True)


def _cells(ints):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in ints), dtype="<u8").reshape(-1, 4).astype(np.uint64)


def _tx_record(tx):
    """the normalised fields of one tx, evaluated in table_fixed's order (typing.py:209-267)"""
    tid, nonce, gas = _fq(tx.id, "tx.id"), _fq(tx.nonce, "tx.nonce"), _fq(tx.gas, "tx.gas")
    gas_price = _word(tx.gas_price, "tx.gas_price")
    caller = _word(tx.caller_address, "tx.caller_address")
    to_none = tx.callee_address is None
    callee = _word(0 if to_none else tx.callee_address, "tx.callee_address")
    value = _word(tx.value, "tx.value")
    data = bytes(tx.call_data)
    invalid = _fq(tx.invalid_tx, "tx.invalid_tx")
    acc = list(tx.access_list)
    a, k = len(acc), sum(len(t.storage_keys) for t in acc)
    if a >= 1 << 32 or k >= 1 << 32:
        raise UnsupportedOnDevice("tx.access_list: more than 2^32 - 1 entries")
    sign_hash = _fq(getattr(tx, "tx_sign_hash", TX_SIGN_HASH_MOCK), "tx.tx_sign_hash")
    return (tid, nonce, gas, gas_price, caller, callee, value, invalid, sign_hash, int(to_none), a, k, data)


def _by_id(records, what):
    """sorted by id, exact duplicates dropped; two different records with one id cannot be expressed"""
    out = {}
    for r in records:
        if out.setdefault(r[0], r) != r:
            raise UnsupportedOnDevice(f"two different {what} with id {r[0]}: their table rows would interleave")
    return [out[k] for k in sorted(out)]


def raw_block_data(block, txs, withdrawals):
    """`Block` (or None: no block table), sequences of `Transaction` and `Withdrawal` (these classes or the reference's: only attributes
    are read) -> the raw input dict of engine.open_evm_tables_from_block / oneshot.evm_tables_from_block (host arrays)"""
    recs = _by_id([_tx_record(tx) for tx in txs], "transactions")
    n = len(recs)
    raw = {"tx_fields": _cells([v for r in recs for v in r[:9]]).reshape(n, 9, 4),
           "to_is_none": np.array([r[9] for r in recs], dtype=np.uint32),
           "access_list": np.array([r[10:12] for r in recs], dtype=np.uint32).reshape(n, 2),
           "calldata": np.frombuffer(b"".join(r[12] for r in recs), dtype=np.uint8).copy(),
           "offsets": np.concatenate([[0], np.cumsum([len(r[12]) for r in recs])]).astype(np.uint64),
           "block": None, "history_hashes": np.zeros((0, 4), dtype=np.uint64)}
    if block is not None:
        hist = list(block.history_hashes)
        coinbase = _word(block.coinbase, "block.coinbase")
        gas_limit = _fq(block.gas_limit, "block.gas_limit")
        number = _int(block.number, "block.number")
        if hist and not 0 <= number < 1 << 256:
            raise UnsupportedOnDevice("block.number outside [0, 2^256) with history hashes")
        timestamp = _fq(block.timestamp, "block.timestamp")
        prev_randao, base_fee = _word(block.prev_randao, "block.prev_randao"), _word(block.base_fee, "block.base_fee")
        chainid, root = _fq(block.chainid, "block.chainid"), _fq(block.withdrawal_root, "block.withdrawal_root")
        hashes = [_word(h, "block.history_hashes") for h in reversed(hist)][::-1]
        raw["block"] = _cells([coinbase, gas_limit, number if hist else number % P, timestamp, prev_randao, base_fee, chainid, root])
        raw["history_hashes"] = _cells(hashes)
    wds = _by_id([(_fq(w.id, "withdrawal.id"), _fq(w.validator_id, "withdrawal.validator_id"), _fq(w.address, "withdrawal.address"),
                   _fq(w.amount, "withdrawal.amount")) for w in withdrawals], "withdrawals")
    raw["withdrawals"] = _cells([v for w in wds for v in w]).reshape(len(wds), 4, 4)
    return raw


def tables_from_block(block, txs, withdrawals, device=None, resident=False):
    """-> ((tx uint64[12 n + b, 5, 4], tx_flags uint32[..]), (block uint64[8 + h, 4, 4], block_flags uint32[..]), withdrawals uint64[m, 4, 4]):
    the wire arrays of flatten_tx_table / flatten_block_table / flatten_withdrawal_table over the objects' table_assignments(), built
    on the device from the raw fields (zk_evm_tables_from_block).  resident=True: the raw fields are uploaded and the tables come back
    as CUDA tensors (int64 views of the same cells) that never visited the host — what engine.open_evm / open_copy take in place."""
    raw = raw_block_data(block, txs, withdrawals)
    if not resident:
        res, out = oneshot.evm_tables_from_block(raw, device=device)
    else:
        import torch

        dev = torch.device("cuda", 0 if device is None else int(device))
        up = {k: None if v is None else torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v.view(np.int32) if v.dtype == np.uint32 else v).to(dev)
              for k, v in raw.items()}
        shapes = engine.evm_tables_from_block_shapes(len(raw["to_is_none"]), len(raw["calldata"]), len(raw["history_hashes"]),
                                                     len(raw["withdrawals"]), raw["block"] is not None)
        out = {k: torch.empty(shp, dtype=torch.int64 if dt == np.uint64 else torch.int32, device=dev) for k, (shp, dt) in shapes.items()}
        with engine.open_evm_tables_from_block(up, outs=out, device=device) as s:
            res = s.run()
    assert res.ok  # (the assignment has no failing case)
    return (out["tx"], out["tx_flags"]), (out["block"], out["block_flags"]), out["withdrawals"]
