"""Independent plain-Python model of the Withdrawal circuit, written from the spec (zkevm_specs/withdrawal_circuit.py verify_circuit,
Ethereum RLP of integers, keccak-256 from oracle/keccak.py), with no code of the package or the reference.

Rows are tuples of 8 ints (id, validator_id, address, amount, hash lo, hi, root lo, hi); the MPT table a set of 12-tuples, the
keccak table a set of 5-tuples, the block table a list of 4-tuples (field_tag, block_number, value lo, hi).  Status codes are the
backend's: (kind << 24) | site, kinds 1 AssertionError, 3 LookupUnsatFailure, 4 LookupAmbiguousFailure, 12 IndexError; sites 0 row,
1 id chain, 2 keccak, 3 MPT, 4 block lookup."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.keccak import keccak256  # noqa: E402

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
M128 = (1 << 128) - 1
ASSERT, UNSAT, AMBIGUOUS, INDEX = 1, 3, 4, 12
WITHDRAWAL_ROOT_TAG, WITHDRAWAL_MOD, NON_EXISTING_ACCOUNT = 9, 8, 4


def code(kind, site):
    return (kind << 24) | site


def rlp_int(v):
    """RLP of a non-negative integer: big-endian bytes without leading zeros; a single byte below 0x80 is itself"""
    b = v.to_bytes((v.bit_length() + 7) // 8, "big")
    if len(b) == 1 and b[0] < 0x80:
        return b
    return bytes([0x80 + len(b)]) + b


def rlp_list(items):
    payload = b"".join(rlp_int(v) for v in items)
    n = len(payload)
    header = bytes([0xC0 + n]) if n < 56 else bytes([0xF7 + 1, n])  # payload <= 132 bytes: one length byte
    return header + payload


def rlc(data, r):
    """sum data[k] * r^(len - 1 - k): RLC of the reversed bytes, the first byte weighted highest"""
    acc = 0
    for b in data:
        acc = (acc * r + b) % P
    return acc


def split(v):
    return v & M128, v >> 128


def digest_word(data):
    """Word(keccak(data)): the digest read as a little-endian 256-bit integer, split into lo / hi"""
    return split(int.from_bytes(keccak256(data), "little"))


def keccak_row(fields, r):
    data = rlp_list(fields)
    lo, hi = digest_word(data)
    return (1, rlc(data, r), len(data), lo, hi)


def assign(withdrawals, roots, max_withdrawals, r):
    """withdrawals2witness's rows and the keccak rows KeccakTable.add makes (the (0, 0, 0, 0, 0) row is NOT added here)"""
    rows, krows, last = [], [], 0
    for wd, root in zip(withdrawals, roots):
        data = rlp_list(wd)
        rows.append(tuple(wd) + digest_word(data) + split(root))
        krows.append(keccak_row(wd, r))
        last = root
    for _ in range(len(rows), max_withdrawals):
        rows.append((0, 0, 0, 0, 0, 0) + split(last))
    return rows, krows


def mpt_row(address, proof_type, key, root, root_prev, value, value_prev=0):
    """MPTTableRow cells in table order: address, proof_type, storage_key, root, root_prev, value, value_prev (Words as lo, hi)"""
    return (address, proof_type) + split(key) + split(root) + split(root_prev) + split(value) + split(value_prev)


def mock_mpt(withdrawals, roots):
    """the MPT rows the reference test's mock_mpt_update makes for consecutive roots"""
    out, prev = set(), 0
    for wd, root in zip(withdrawals, roots):
        h = int.from_bytes(keccak256(rlp_list(wd)), "little")
        out.add(mpt_row(wd[2], WITHDRAWAL_MOD, wd[0], root, prev, h))
        prev = root
    return out


def _block(block, lo, hi):
    m = [b for b in set(block) if b[0] == WITHDRAWAL_ROOT_TAG and b[2] == lo and b[3] == hi]
    return code(UNSAT, 4) if not m else (code(AMBIGUOUS, 4) if len(m) > 1 else 0)


def verify_status(rows, mpt, keccak, block, max_withdrawals, r, total_rows=None):
    """per-row status of verify_circuit over `rows` (rows[:MAX] held; len(rows) == total_rows): one entry per evaluated row,
    max(1, min(MAX, total_rows)) of them"""
    total = len(rows) if total_rows is None else total_rows
    m = max_withdrawals
    mpt, keccak = set(mpt), set(keccak)
    if m == 0:
        return [code(INDEX, 4) if total == 0 else _block(block, rows[total - 1][6], rows[total - 1][7])]
    out = []
    for i in range(max(1, min(m, total))):
        if i >= total:
            out.append(code(INDEX, 0))
            continue
        row = rows[i]
        if i != m - 1:
            if i + 1 >= total:
                out.append(code(INDEX, 1))
                continue
            if rows[i + 1][0] != (row[0] + 1) % P:
                out.append(code(ASSERT, 1))
                continue
        pad = 1 if row[3] != 0 else 0
        data = rlp_list(row[:4])
        q = (pad, pad * rlc(data, r), pad * len(data), pad * row[4], pad * row[5])
        if q not in keccak:
            out.append(code(ASSERT, 2))
            continue
        prev = (0, 0) if i == 0 else (rows[i - 1][6], rows[i - 1][7])
        qm = (row[2], WITHDRAWAL_MOD if pad else NON_EXISTING_ACCOUNT) + split(row[0]) + (row[6], row[7]) + prev + (row[4], row[5], 0, 0)
        if qm not in mpt:
            out.append(code(UNSAT, 3))
            continue
        out.append(_block(block, row[6], row[7]) if i == m - 1 else 0)
    return out


def first_failure(status):
    for i, c in enumerate(status):
        if c:
            return i, c
    return None, 0
