"""A plain-Python model of the EVM circuit's tx, block and withdrawal tables, written from the reference's statements
(evm_circuit/typing.py:116-137 Block.table_assignments, :186-281 Transaction.call_data_gas_cost / access_list_gas_cost / table_fixed /
table_assignments, :306-314 Withdrawal.table_assignments; util/arithmetic.py:107-123 Word(int); util/param.py:80-82) and of what
flatten_tx_table / flatten_block_table / flatten_withdrawal_table make of the sets built from them: rows keyed on their cells, the first
flag kept, sorted ascending.  It reads attributes only, so it runs over the mirror's objects and the reference's alike."""
import numpy as np

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
MASK128 = (1 << 128) - 1
(NONCE, GAS, GAS_PRICE, CALLER_ADDRESS, CALLEE_ADDRESS, IS_CREATE, VALUE, CALL_DATA_LENGTH, CALL_DATA_GAS_COST, TX_INVALID,
 ACCESS_LIST_GAS_COST, TX_SIGN_HASH, CALL_DATA) = range(1, 14)
COINBASE, GAS_LIMIT, NUMBER, TIMESTAMP, PREV_RANDAO, BASE_FEE, CHAIN_ID, HISTORY_HASH, WITHDRAWAL_ROOT = range(1, 10)


def fq(v):
    return int(v) % P


def value(v):
    """WordOrValue(FQ(v)) -> (lo, hi, is_word)"""
    return fq(v), 0, 0


def word(w):
    """WordOrValue(Word(w)) for an int w -> (lo, hi, is_word)"""
    w = int(w)
    assert w < 256**32
    b = w.to_bytes(32, "little")  # (OverflowError for a negative int)
    return int.from_bytes(b[:16], "little"), int.from_bytes(b[16:], "little"), 1


def tx_assignments(tx):
    data = bytes(tx.call_data)
    gas_cost = sum(4 if b == 0 else 16 for b in data)
    access_cost = sum(2400 + len(t.storage_keys) * 1900 for t in tx.access_list)
    to_none = tx.callee_address is None
    fixed = [(NONCE, value(tx.nonce)), (GAS, value(tx.gas)), (GAS_PRICE, word(tx.gas_price)), (CALLER_ADDRESS, word(tx.caller_address)),
             (CALLEE_ADDRESS, word(0 if to_none else tx.callee_address)), (IS_CREATE, value(to_none)), (VALUE, word(tx.value)),
             (CALL_DATA_LENGTH, value(len(data))), (CALL_DATA_GAS_COST, value(gas_cost)), (TX_INVALID, value(tx.invalid_tx)),
             (ACCESS_LIST_GAS_COST, value(access_cost)), (TX_SIGN_HASH, value(getattr(tx, "tx_sign_hash", 1234)))]
    rows = [((fq(tx.id), tag, 0, v[0], v[1]), v[2]) for tag, v in fixed]
    rows += [((fq(tx.id), CALL_DATA, i, b, 0), 0) for i, b in enumerate(data)]
    return rows


def block_assignments(block):
    rows = [(COINBASE, 0, word(block.coinbase)), (GAS_LIMIT, 0, value(block.gas_limit)), (NUMBER, 0, value(block.number)),
            (TIMESTAMP, 0, value(block.timestamp)), (PREV_RANDAO, 0, word(block.prev_randao)), (BASE_FEE, 0, word(block.base_fee)),
            (CHAIN_ID, 0, value(block.chainid)), (WITHDRAWAL_ROOT, 0, value(block.withdrawal_root))]
    rows += [(HISTORY_HASH, fq(block.number - idx - 1), word(h)) for idx, h in enumerate(reversed(block.history_hashes))]
    return [((tag, num, v[0], v[1]), v[2]) for tag, num, v in rows]


def withdrawal_assignments(w):
    return [((fq(w.id), fq(w.validator_id), fq(w.address), fq(w.amount)), 0)]


def _table(pairs, ncells):
    """the set keyed on the cells (first flag kept), sorted -> (uint64[n, ncells, 4], uint32[n])"""
    seen = {}
    for cells, flag in pairs:
        seen.setdefault(cells, flag)
    keys = sorted(seen)
    buf = b"".join(int(v).to_bytes(32, "little") for k in keys for v in k)
    return (np.frombuffer(buf, dtype="<u8").reshape(len(keys), ncells, 4).astype(np.uint64),
            np.array([seen[k] for k in keys], dtype=np.uint32))


def model(block, txs, withdrawals):
    """-> dict(tx, tx_flags, block, block_flags, withdrawals): the wire arrays (block=None: an empty block table)"""
    tx, tx_flags = _table([r for t in txs for r in tx_assignments(t)], 5)
    blk, blk_flags = _table(block_assignments(block) if block is not None else [], 4)
    wd, _ = _table([r for w in withdrawals for r in withdrawal_assignments(w)], 4)
    return {"tx": tx, "tx_flags": tx_flags, "block": blk, "block_flags": blk_flags, "withdrawals": wd}
