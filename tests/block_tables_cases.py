"""zk_evm_tables_from_block: the directed case builders, shared by the CPU and GPU tests.  Every case is (name, block or None, txs,
withdrawals) over the mirror's objects (zkevm_specs_amd.block_tables); the expected tables come from the plain-Python model of
tests/block_tables_ref.py, computed once per case and shared read-only."""
import functools
import random
from itertools import chain

import numpy as np

from tests import block_tables_ref as ref
from zkevm_specs_amd import block_tables as bt
from zkevm_specs_amd.engine import CALLDATA_GAS_BLOCK as B

P = ref.P
U64, U256 = (1 << 64) - 1, (1 << 256) - 1
OUTPUTS = ("tx", "tx_flags", "block", "block_flags", "withdrawals")


def _data(rng, n, zero=0.35):
    return bytes(0 if rng.random() < zero else rng.randrange(1, 256) for _ in range(n))


def _tx(rng, tid, data, **kw):
    kw.setdefault("nonce", rng.getrandbits(64))
    kw.setdefault("gas", rng.getrandbits(64))
    kw.setdefault("gas_price", rng.getrandbits(256))
    kw.setdefault("caller_address", rng.getrandbits(160))
    kw.setdefault("callee_address", None if rng.random() < 0.3 else rng.getrandbits(160))
    kw.setdefault("value", rng.getrandbits(256))
    kw.setdefault("invalid_tx", rng.randrange(2))
    kw.setdefault("access_list", [bt.AccessTuple(rng.getrandbits(160), [rng.getrandbits(256) for _ in range(rng.randrange(4))])
                                  for _ in range(rng.randrange(3))])
    return bt.Transaction(id=tid, call_data=data, **kw)


def _block(rng, n_history=0, number=None, **kw):
    number = n_history if number is None else number
    return bt.Block(coinbase=rng.getrandbits(160), gas_limit=rng.getrandbits(64), number=number, timestamp=rng.getrandbits(64),
                    prev_randao=rng.getrandbits(256), base_fee=rng.getrandbits(256), chainid=rng.getrandbits(64),
                    withdrawal_root=kw.pop("withdrawal_root", rng.getrandbits(256)), history_hashes=[rng.getrandbits(256) for _ in range(n_history)])


def _withdrawals(rng, n, first=0, step=1):
    return [bt.Withdrawal(id=first + step * i, validator_id=rng.getrandbits(64), address=rng.getrandbits(160), amount=rng.getrandbits(64)) for i in range(n)]


@functools.lru_cache(maxsize=None)
def directed_cases(seed=20261020):
    """-> tuple of (name, block, txs, withdrawals).  Every case is one call."""
    rng = random.Random(seed)
    cases = []
    # calldata lengths around the 64-row wavefront edges, the 256-row workgroup edges and the gas kernel's block B: every tx but the
    # first starts in the middle of a block
    lengths = [0, 1, 63, 64, 65, 255, 256, 257, B - 1, B, B + 1, 3 * B + 1]
    cases.append(("lengths", _block(rng, 3, number=1000), [_tx(rng, 1 + i, _data(rng, n)) for i, n in enumerate(lengths)], _withdrawals(rng, 1)))
    for n in (1, B - 1, B, B + 1, 3 * B + 1):  # ... and each alone, starting at the buffer's first byte
        cases.append((f"single_{n}", None, [_tx(rng, 7, _data(rng, n))], []))
    cases.append(("short_txs_in_one_block", None, [_tx(rng, 10 + i, _data(rng, rng.randrange(1, 10))) for i in range(20)], []))
    cases.append(("one_tx_holds_all", _block(rng), [_tx(rng, 1, b""), _tx(rng, 2, b""), _tx(rng, 3, _data(rng, 2000)), _tx(rng, 4, b""), _tx(rng, 5, b"")], []))
    cases.append(("only_empty_txs", None, [_tx(rng, i, b"") for i in (1, 2, 3)], _withdrawals(rng, 2)))
    cases.append(("no_txs", _block(rng, 1), [], _withdrawals(rng, 65, first=5, step=3)))
    cases.append(("nothing", None, [], []))
    cases.append(("zero_and_zero_free", None, [_tx(rng, 1, bytes(700)), _tx(rng, 2, bytes(rng.randrange(1, 256) for _ in range(700))),
                                               _tx(rng, 3, bytes(B)), _tx(rng, 4, b"\xff" * (2 * B))], []))
    # tx boundaries on rows 63 | 64 and 255 | 256 of the tx table: 12 + 52 = 64 rows, then 12 + 180 = 192
    cases.append(("row_boundaries", None, [_tx(rng, 1, _data(rng, 52)), _tx(rng, 2, _data(rng, 180)), _tx(rng, 3, _data(rng, 9))], []))
    cases.append(("ids_with_gaps_and_p_minus_1", None, [_tx(rng, 1, _data(rng, 5)), _tx(rng, 1000, _data(rng, 70)), _tx(rng, 1 << 200, b"\x01"),
                                                        _tx(rng, P - 1, _data(rng, 33))], []))
    fields = []
    for i, (price, value, invalid) in enumerate([(U256, 1 << 128, 0), (1 << 128, U256, 1), (0, 0, 0), ((1 << 128) - 1, (1 << 255) + 1, 1)]):
        fields.append(_tx(rng, 1 + i, _data(rng, 3), nonce=U64, gas=U64, gas_price=price, value=value, invalid_tx=invalid,
                          caller_address=(1 << 160) - 1, callee_address=None if i % 2 else (1 << 160) - 1))
    cases.append(("tx_fields", None, fields, []))
    # FQ(...) cells of 256-bit inputs at and above p: reduced on the device
    wide = _tx(rng, 3, _data(rng, 4), nonce=U256, gas=P, invalid_tx=P + 1)
    wide.tx_sign_hash = 5 * P + 7
    cases.append(("fq_cells_at_and_above_p", None, [wide, _tx(rng, 4, b"", nonce=P - 1, gas=2 * P + 1, invalid_tx=4 * P)], []))
    for root in (P - 1, P, P + 1, U256):
        cases.append((f"withdrawal_root_{root - P if root < U256 else 'max'}", _block(rng, withdrawal_root=root), [], []))
    for n in (0, 1, 255, 256):
        cases.append((f"history_{n}", _block(rng, n), [], []))
    cases.append(("history_number_crosses_p", _block(rng, 8, number=P + 3), [], []))
    cases.append(("history_number_max", _block(rng, 5, number=U256), [], []))
    for n in (0, 1, 65):
        cases.append((f"withdrawals_{n}", None, [], _withdrawals(rng, n, first=0)))
    cases.append(("withdrawal_cells_above_p", None, [], [bt.Withdrawal(id=P - 1, validator_id=P, address=U256, amount=P + 1)]))
    return tuple((name, blk, tuple(txs), tuple(wds)) for name, blk, txs, wds in cases)


NAMES = [c[0] for c in directed_cases()]


def case(name):
    return next(c for c in directed_cases() if c[0] == name)


@functools.lru_cache(maxsize=None)
def directed_raw(name):
    """the raw input arrays of one directed case (treat as read-only)"""
    _, blk, txs, wds = case(name)
    raw = bt.raw_block_data(blk, txs, wds)
    for a in raw.values():
        if a is not None:
            a.setflags(write=False)
    return raw


@functools.lru_cache(maxsize=None)
def directed_expected(name):
    """the model's tables for one directed case: computed once, shared (treat as read-only)"""
    _, blk, txs, wds = case(name)
    out = ref.model(blk, txs, wds)
    for a in out.values():
        a.setflags(write=False)
    return out


def same(got, exp):
    return all(got[k].shape == exp[k].shape and got[k].dtype == exp[k].dtype and (got[k] == exp[k]).all() for k in OUTPUTS)


def _ints(cells):
    """uint64[n, c, 4] -> list of rows of python ints"""
    return [[int.from_bytes(c.tobytes(), "little") for c in row] for row in cells]


def cells(ints):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in ints), dtype="<u8").reshape(-1, 4).astype(np.uint64)


# ---- raw data recovered from the wires of a golden case of tests/golden/evm_*.npz (the reference's recorded tables)
def recover_txs(tx):
    """the golden's _tx wire -> the raw tx arrays.  Every golden tx table is a whole-object image: per id the twelve fixed tags once
    each and the CallData rows 0..len-1 (asserted)."""
    by_id = {}
    for tid, tag, index, lo, hi in _ints(tx):
        by_id.setdefault(tid, {}).setdefault(tag, {})[index] = lo + (hi << 128)
    fields, to_none, access, data = [], [], [], []
    for tid in sorted(by_id):
        t = by_id[tid]
        assert sorted(k for k in t if k != 13) == list(range(1, 13)) and all(list(t[k]) == [0] for k in range(1, 13)), tid
        f = {k: t[k][0] for k in range(1, 13)}
        cd = t.get(13, {})
        assert sorted(cd) == list(range(len(cd))) and f[8] == len(cd) and f[11] in (0, 6200), tid
        fields.append([tid, f[1], f[2], f[3], f[4], f[5], f[7], f[10], f[12]])
        to_none.append(f[6])
        access.append([1, 2] if f[11] else [0, 0])  # 6200 = 2400 + 2 * 1900: one address with two storage keys
        data.append(bytes(cd[i] for i in range(len(cd))))
    n = len(fields)
    return {"tx_fields": cells(list(chain(*fields))).reshape(n, 9, 4), "to_is_none": np.array(to_none, dtype=np.uint32),
            "access_list": np.array(access, dtype=np.uint32).reshape(n, 2), "calldata": np.frombuffer(b"".join(data), dtype=np.uint8).copy(),
            "offsets": np.concatenate([[0], np.cumsum([len(d) for d in data])]).astype(np.uint64)}, [len(d) for d in data]


def recover_block(block):
    rows = _ints(block)
    if not rows:
        return None, np.zeros((0, 4), dtype=np.uint64)
    single = {tag: lo + (hi << 128) for tag, num, lo, hi in rows if tag != 8}
    assert sorted(single) == [1, 2, 3, 4, 5, 6, 7, 9] and len(rows) - 8 == sum(1 for r in rows if r[0] == 8)
    hist = sorted((num, lo + (hi << 128)) for tag, num, lo, hi in rows if tag == 8)
    assert [num for num, _ in hist] == list(range(single[3] - len(hist), single[3]))
    return cells([single[k] for k in (1, 2, 3, 4, 5, 6, 7, 9)]), cells([h for _, h in hist])


def recover_raw(tx, block, withdrawals):
    """the _tx / _block / _withdrawals wires of a golden case -> (the raw input dict that must reproduce them, the txs' calldata lengths)"""
    raw, lengths = recover_txs(tx)
    raw["block"], raw["history_hashes"] = recover_block(block)
    raw["withdrawals"] = withdrawals
    return raw, lengths


@functools.lru_cache(maxsize=None)
def random_block(seed=11, n_txs=300, total=1 << 16):
    """a seeded skewed block: n_txs txs with `total` calldata bytes — many empty and tiny ones, three of 8..24 KiB; 256 history hashes,
    40 withdrawals -> (block, txs, withdrawals)"""
    rng = random.Random(seed)
    while True:
        lengths = [rng.randrange(8 << 10, 24 << 10) for _ in range(2)] + [rng.choice([0, 0, rng.randrange(1, 40), rng.randrange(40, 300)]) for _ in range(n_txs - 3)]
        rest = total - sum(lengths)
        if (8 << 10) <= rest <= (24 << 10):
            break
    lengths.append(rest)
    rng.shuffle(lengths)
    ids = sorted(rng.sample(range(1, 1 << 20), n_txs))
    return (_block(rng, 256, number=1 << 40), tuple(_tx(rng, i, rng.randbytes(n) if n % 3 else _data(rng, n, 0.6)) for i, n in zip(ids, lengths)),
            tuple(_withdrawals(rng, 40, first=9, step=2)))
