"""Host-side mirror of `zkevm_specs.withdrawal_circuit.verify_circuit` (withdrawal_circuit.py:128-201): the rows are checked behind
the C ABI (`zk_withdrawal_verify`: id chain, keccak-table membership of the RLP's RLC, MPT lookup, WithdrawalRoot block lookup), and
`withdrawals2witness`'s rows and keccak rows are assigned there (`zk_withdrawal_assign`, digests computed by the backend).

The reference's own exception classes come back through errors.raise_for_code.  Some outcomes depend on the Python types of a row's
cells, not on their values, and are classified here before the wire is read (the reference tests write plain ints into fields):
* a plain-int withdrawal_id: `Word(row.withdrawal_id.n)` raises AttributeError at the MPT lookup, and `rows[i + 1].withdrawal_id ==
  row.withdrawal_id + 1` compares the UNREDUCED sum, which fails for p - 1;
* a plain-int address: TableRow.match asserts its query cells are Expressions (AssertionError), as soon as the MPT table has a row;
* a root that is a plain int (padding_withdrawal stores one): TableRow.match asserts at the MPT / block lookups that read it;
* a row that is not a Row at all (the reference test's padding_withdrawal returns a one-element list, which withdrawals2witness
  appends as it is): AttributeError at the previous row's id chain, or at the row's own first read of `amount`.
"""
from . import oneshot
from .errors import KIND_ASSERT, raise_for_code
from .flatten import flatten_withdrawal_witness
from .wire import FR_MODULUS

KIND_ATTRIBUTE_ERROR = 13
SITE_ID, SITE_KECCAK, SITE_MPT, SITE_BLOCK = 1, 2, 3, 4


def _code(kind, site):
    return (kind << 24) | site


def _is_plain_int(x):
    return not (hasattr(x, "n") or hasattr(x, "expr"))


def type_quirks(witness, max_withdrawals):
    """{row: status code} of the failures the types of the rows' cells raise in the reference (see the module docstring)"""
    rows, m = list(witness.rows), int(max_withdrawals)
    mpt_rows = len(getattr(witness.mpt_table, "table", witness.mpt_table))
    out = {}
    if m == 0 and rows and not hasattr(rows[-1], "root"):
        return {0: _code(KIND_ATTRIBUTE_ERROR, SITE_BLOCK)}  # rows[-1].root
    for i in range(min(m, len(rows))):
        row = rows[i]
        if not hasattr(row, "withdrawal_id"):
            out[i] = _code(KIND_ATTRIBUTE_ERROR, 0)  # row.amount, before anything else of the row
            continue
        if i != m - 1 and i + 1 < len(rows) and not hasattr(rows[i + 1], "withdrawal_id"):
            out[i] = _code(KIND_ATTRIBUTE_ERROR, SITE_ID)  # rows[i + 1].withdrawal_id
        elif i != m - 1 and i + 1 < len(rows) and _is_plain_int(row.withdrawal_id) and int(row.withdrawal_id) + 1 >= FR_MODULUS:
            out[i] = _code(KIND_ASSERT, SITE_ID)
        elif _is_plain_int(row.withdrawal_id):
            out[i] = _code(KIND_ATTRIBUTE_ERROR, SITE_MPT)
        elif _is_plain_int(row.address) and mpt_rows:
            out[i] = _code(KIND_ASSERT, SITE_MPT)
        elif mpt_rows and (not hasattr(row.root, "lo") or (i > 0 and hasattr(rows[i - 1], "root") and not hasattr(rows[i - 1].root, "lo"))):
            out[i] = _code(KIND_ASSERT, SITE_MPT)  # a root (or root_prev) that is not a Word: TableRow.match asserts
        elif i == m - 1 and not hasattr(row.root, "lo") and len(getattr(witness.block_table, "table", witness.block_table) or ()):
            out[i] = _code(KIND_ASSERT, SITE_BLOCK)
    return out


def first_failure(status, quirks=None, row_base=0):
    """(row, code) of the first failure — per row the earlier site of the backend's status and the type quirk — or (None, 0)"""
    quirks = quirks or {}
    eff = {}
    for j, c in enumerate(status.tolist()):
        c = int(c)
        q = quirks.get(row_base + j)
        if q is not None and (c == 0 or (c & 0xFFFFFF) >= (q & 0xFFFFFF)):
            c = q
        if c:
            eff[row_base + j] = c
    if not eff:
        return None, 0
    row = min(eff)
    return row, eff[row]


def verify_circuit(witness, MAX_WITHDRAWALS, keccak_randomness):
    """The reference's verify_circuit: raises the exception of the first failing row (AssertionError / LookupUnsatFailure /
    LookupAmbiguousFailure / IndexError / AttributeError)."""
    r = int(keccak_randomness.n if hasattr(keccak_randomness, "n") else keccak_randomness)
    w = flatten_withdrawal_witness(witness, MAX_WITHDRAWALS)
    _, status = oneshot.withdrawal_verify(w, r)
    row, code = first_failure(status, type_quirks(witness, MAX_WITHDRAWALS))
    raise_for_code(code, f"Withdrawal circuit row {row}")


def withdrawals_assign(withdrawals, roots, max_withdrawals, keccak_randomness):
    """withdrawals2witness's assignment through the backend: withdrawals — (id, validator_id, address, amount) tuples or objects with
    those attributes — and their MPT roots -> (rows uint64[max(n, MAX), 8, 4], keccak rows uint64[n, 5, 4])"""
    import numpy as np

    from .flatten import _word_limbs

    def fields(wd):
        if hasattr(wd, "validator_id"):
            return (wd.id, wd.validator_id, wd.address, wd.amount)
        return tuple(wd)

    cells = [[_word_limbs(int(x) % FR_MODULUS) for x in fields(wd)] + [_word_limbs(root)] for wd, root in zip(withdrawals, roots)]
    arr = np.array(cells, dtype=np.uint64).reshape(len(cells), 5, 4)
    r = int(keccak_randomness.n if hasattr(keccak_randomness, "n") else keccak_randomness)
    return oneshot.withdrawal_assign(arr, max_withdrawals, r)
