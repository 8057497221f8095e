#!/usr/bin/env python3
"""Write tests/golden/withdrawal_cases.npz: Withdrawal-circuit cases on the zk_withdrawal_witness wire (include/zkevm_hip.h) with
their expected outcome.

Runs where the reference is (it imports the reference's tests/test_withdrawal_circuit.py through oracle/refshim's rlp / eth_utils
stand-ins).  Every case is a witness in wire form — rows uint64[n, 8, 4], mpt uint64[m, 12, 4], keccak uint64[k, 5, 4], block
uint64[b, 4, 4] — plus max_withdrawals, total_rows, the rows' cells that are plain ints in the reference's objects (`int_fields`),
the per-row status of tests/withdrawal_ref.py (`status`, what the backend must return), and the first failure as the mirror must
raise it (`first_row`, `first_kind`).  Each case is also run through the UNMODIFIED reference's verify_circuit, rebuilt from the
wire cells (plain ints where `int_fields` says so), and its exception class is recorded (`ref_outcome`, "" for none); the script
checks that it names the same kind as `first_kind`.
* `ref_*`: the reference test file's witnesses (gen_withdrawals / withdrawals2witness, mutated as its tests mutate them);
* `trap_*`: RLP edge values, padding rows, MAX_WITHDRAWALS against len(rows), block-lookup ambiguity, id wrap-around mod p;
* `tamper_*`: one cell of every row and field changed.
Run: python tools/gen_golden_withdrawal.py [--ref-root <reference checkout>] [--out tests/golden/withdrawal_cases.npz]
"""
import argparse
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import withdrawal_ref as W  # noqa: E402

RANDOMNESS = 0x1D2C3B4A59687786A5B4C3D2E1F00F1E2D3C4B5A69788796A5B4C3D2E1F0  # < p
P = W.P
KIND_NAMES = {0: "", 1: "AssertionError", 3: "LookupUnsatFailure", 4: "LookupAmbiguousFailure", 12: "IndexError", 13: "AttributeError"}


def cells(rows, nc):
    return np.array([[[(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in r] for r in rows], dtype=np.uint64).reshape(
        len(rows), nc, 4)


def expected_first(status, rows, int_fields, m, n_mpt):
    """first (row, kind) as the reference raises it: the model's per-row status with the type quirks of plain-int cells folded in
    (an int id: `Word(id.n)` -> AttributeError at the MPT lookup, its unreduced `id + 1` fails the chain for p - 1; an int address:
    TableRow.match asserts at the MPT lookup when the table has rows)"""
    eff = list(status)
    for (i, f) in int_fields:
        if i >= len(eff) or i >= min(m, len(rows)):
            continue
        q = None
        if f == 0 and i != m - 1 and i + 1 < len(rows) and rows[i][0] + 1 >= P:
            q = W.code(1, 1)
        elif f == 0:
            q = W.code(13, 3)
        elif f == 2 and n_mpt:
            q = W.code(1, 3)
        if q is not None and (eff[i] == 0 or (eff[i] & 0xFFFFFF) >= (q & 0xFFFFFF)):
            eff[i] = q
    for i, c in enumerate(eff):
        if c:
            return i, c >> 24
    return -1, 0


class Ref:
    """the unmodified reference, loaded through the shims"""

    def __init__(self, ref_root):
        for p in (os.path.join(ROOT, "oracle", "refshim"), os.path.join(ref_root, "src"), os.path.join(ref_root, "tests")):
            sys.path.insert(0, p)
        import test_withdrawal_circuit as t
        from zkevm_specs import withdrawal_circuit as wc
        from zkevm_specs.evm_circuit.table import BlockTableRow, MPTTableRow
        from zkevm_specs.util import FQ, Word

        self.t, self.wc, self.FQ, self.Word, self.MPTTableRow, self.BlockTableRow = t, wc, FQ, Word, MPTTableRow, BlockTableRow

    def word(self, lo, hi):
        return self.Word((self.FQ(lo), self.FQ(hi)))

    def witness(self, rows, mpt, keccak, block, int_fields):
        FQ, wd = self.FQ, self.word
        ints = set(int_fields)
        objs = []
        for i, r in enumerate(rows):
            f = [r[k] if (i, k) in ints else FQ(r[k]) for k in range(4)]
            objs.append(self.wc.Row(f[0], f[1], f[2], f[3], wd(r[4], r[5]), wd(r[6], r[7])))
        mt = set(self.MPTTableRow(FQ(m[0]), FQ(m[1]), wd(m[2], m[3]), wd(m[4], m[5]), wd(m[6], m[7]), wd(m[8], m[9]), wd(m[10], m[11]))
                 for m in mpt)
        kt = self.wc.KeccakTable()
        kt.table = set((FQ(k[0]), FQ(k[1]), FQ(k[2]), wd(k[3], k[4])) for k in keccak)
        bt = set(self.BlockTableRow(FQ(b[0]), FQ(b[1]), wd(b[2], b[3])) for b in block)
        return self.wc.Witness(objs, self.wc.MPTTable(mt), kt, self.wc.BlockTable(bt))

    def outcome(self, rows, mpt, keccak, block, m, int_fields):
        try:
            self.wc.verify_circuit(self.witness(rows, mpt, keccak, block, int_fields), m, self.FQ(RANDOMNESS))
            return ""
        except Exception as e:  # the reference's own outcome, recorded as it is
            return type(e).__name__


def build(name, rows, mpt, keccak, block, m, ref, int_fields=()):
    held = rows if m == 0 else rows[:m]
    status = W.verify_status(held, mpt, keccak, block, m, RANDOMNESS, total_rows=len(rows))
    first_row, first_kind = expected_first(status, rows, list(int_fields), m, len(set(mpt)))
    ref_outcome = ref.outcome(rows, mpt, keccak, block, m, int_fields)
    assert ref_outcome == KIND_NAMES[first_kind], (name, ref_outcome, first_row, first_kind, status)
    meta = {"name": name, "max_withdrawals": m, "total_rows": len(rows), "int_fields": [list(x) for x in int_fields],
            "first_row": first_row, "first_kind": first_kind, "ref_outcome": ref_outcome}
    arrays = {"rows": cells(held, 8), "mpt": cells(sorted(set(mpt)), 12), "keccak": cells(sorted(set(keccak)), 5),
              "block": cells(sorted(set(block)), 4), "status": np.array(status, dtype=np.uint32)}
    return meta, arrays


def honest(withdrawals, roots, m, zero_row=True):
    """withdrawals2witness's witness in model form: rows, MPT (mock updates), keccak (with KeccakTable()'s zero row), block"""
    rows, krows = W.assign(withdrawals, roots, m, RANDOMNESS)
    keccak = set(krows) | ({(0, 0, 0, 0, 0)} if zero_row else set())
    last = roots[len(withdrawals) - 1] if withdrawals else 0
    block = [(W.WITHDRAWAL_ROOT_TAG, 0) + W.split(last)]
    return rows, W.mock_mpt(withdrawals, roots), keccak, block


def gen(rng, n, id0=None):
    id0 = rng.randrange(0, 2**64) if id0 is None else id0
    wds, roots, prev = [], [], 0
    for i in range(n):
        wds.append(((id0 + i) % P, rng.randrange(0, 2**64), rng.randrange(1, 2**160), rng.randrange(1, 2**64)))
        prev += 5
        roots.append(prev)
    return wds, roots


def cases(ref):
    rng = random.Random(20261015)
    out = []
    # ---- the reference test file's witnesses ------------------------------------------------------------------------------
    for name, m, mutate in (("basic", 5, None), ("id_not_incremental", 5, ("sub1", 1, 0)), ("inconsistent_id", 5, ("int", 0, 0, 999)),
                            ("inconsistent_validator_id", 5, ("int", 0, 1, 999)), ("inconsistent_address", 5, ("int", 0, 2, 0xDEADBEEF)),
                            ("inconsistent_amount", 2, ("int", 0, 3, 10)), ("withdrawals2witness", 20, None)):
        wds, roots = gen(rng, m)
        rows, mpt, keccak, block = honest(wds, roots, m)
        rows = [list(r) for r in rows]
        ints = []
        if mutate and mutate[0] == "sub1":
            rows[mutate[1]][mutate[2]] = (rows[mutate[1]][mutate[2]] - 1) % P
        elif mutate:
            rows[mutate[1]][mutate[2]] = mutate[3]
            ints.append((mutate[1], mutate[2]))
        out.append(build(f"ref_{name}", [tuple(r) for r in rows], mpt, keccak, block, m, ref, ints))
    # ---- RLP edge values: 0, 1, 127, 128, 2^64 - 1, p - 1, 20-byte and short addresses; payloads above 55 bytes ---------------
    edge = [(P - 3, 0, 0, 1), (P - 2, 1, 1, 127), (P - 1, 127, (1 << 160) - 1, 128), (0, 128, 0x80, 2**64 - 1), (1, 2**64 - 1, 5, P - 1),
            (2, P - 1, P - 1, P - 1), (3, 2**127, 2**159 + 1, 2**64), (4, 0x7F, 0xFF, 0x100)]
    roots = [5 * (k + 1) for k in range(len(edge))]
    out.append(build("trap_rlp_edges", *honest(edge, roots, len(edge)), len(edge), ref))
    # ---- padding rows ---------------------------------------------------------------------------------------------------------
    wds, roots = gen(rng, 3)
    out.append(build("trap_padding_id_chain", *honest(wds, roots, 5), 5, ref))  # padding id 0 breaks the chain at the last real row
    wds, roots = gen(rng, 3, id0=P - 3)  # ids p-3, p-2, p-1: the padding id 0 continues the chain mod p
    rows, mpt, keccak, block = honest(wds, roots, 4)
    out.append(build("trap_padding_nonexisting_missing", rows, mpt, keccak, block, 4, ref))  # its MPT query finds no row
    nonexist = W.mpt_row(0, W.NON_EXISTING_ACCOUNT, 0, roots[-1], roots[-1], 0)
    out.append(build("trap_padding_nonexisting_present", rows, mpt | {nonexist}, keccak, block, 4, ref))
    out.append(build("trap_padding_no_zero_row", rows, mpt | {nonexist}, keccak - {(0, 0, 0, 0, 0)}, block, 4, ref))
    # ---- MAX_WITHDRAWALS against len(rows) ------------------------------------------------------------------------------------
    wds, roots = gen(rng, 6)
    rows, mpt, keccak, block = honest(wds, roots, 6)
    out.append(build("trap_max_below_rows", rows, mpt, keccak, block, 4, ref))  # rows[3].root is not the block's root
    out.append(build("trap_max_below_rows_block_ok", rows, mpt, keccak, [(9, 0) + W.split(roots[3])], 4, ref))
    out.append(build("trap_max_above_rows", rows, mpt, keccak, block, 8, ref))  # rows[6] missing: IndexError on row 5's id chain
    out.append(build("trap_max_zero", rows, mpt, keccak, block, 0, ref))  # the block lookup reads rows[-1]
    out.append(build("trap_max_zero_block_missing", rows, mpt, keccak, [(9, 0, 1, 0)], 0, ref))
    out.append(build("trap_max_zero_no_rows", [], set(), set(), block, 0, ref))
    out.append(build("trap_max_one_no_rows", [], set(), set(), block, 1, ref))
    # ---- block lookup ---------------------------------------------------------------------------------------------------------
    out.append(build("trap_block_ambiguous", rows, mpt, keccak, block + [(9, 7) + block[0][2:]], 6, ref))
    out.append(build("trap_block_other_tag", rows, mpt, keccak, [(8, 0) + block[0][2:]], 6, ref))
    out.append(build("trap_block_duplicate_rows", rows, mpt, keccak, block + block, 6, ref))
    # ---- plain-int cells (host-classified) --------------------------------------------------------------------------------------
    wds, roots = gen(rng, 4)
    rows, mpt, keccak, block = honest(wds, roots, 4)
    out.append(build("trap_int_id_same_value", rows, mpt, keccak, block, 4, ref, [(2, 0)]))  # AttributeError at row 2's MPT lookup
    out.append(build("trap_int_address_same_value", rows, mpt, keccak, block, 4, ref, [(1, 2)]))  # AssertionError in TableRow.match
    out.append(build("trap_int_amount_same_value", rows, mpt, keccak, block, 4, ref, [(0, 3), (3, 1)]))  # no effect
    wds, roots = gen(rng, 3, id0=P - 2)
    rows, mpt, keccak, block = honest(wds, roots, 3)
    out.append(build("trap_int_id_p_minus_1", rows, mpt, keccak, block, 3, ref, [(1, 0)]))  # int p - 1: the unreduced p != 0
    # ---- tampered cells: every row, every field -------------------------------------------------------------------------------
    wds, roots = gen(rng, 5)
    rows, mpt, keccak, block = honest(wds, roots, 5)
    for i in range(5):
        for f in range(8):
            t = [list(r) for r in rows]
            t[i][f] = (t[i][f] + 1 + rng.randrange(0, 1 << 16)) % (P if f < 4 else 1 << 128)
            out.append(build(f"tamper_r{i}_f{f}", [tuple(r) for r in t], mpt, keccak, block, 5, ref))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-root", default=os.path.join(ROOT, "oracle", "_ref"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "withdrawal_cases.npz"))
    args = ap.parse_args()
    cs = cases(Ref(args.ref_root))
    arrays, metas = {}, []
    for i, (meta, a) in enumerate(cs):
        metas.append(meta)
        for k, v in a.items():
            arrays[f"{i}_{k}"] = v
    arrays["meta"] = np.array(json.dumps({"randomness": hex(RANDOMNESS), "cases": metas}))
    np.savez_compressed(args.out, **arrays)
    fails = sum(1 for m in metas if m["first_kind"])
    print(f"{len(cs)} cases ({fails} failing) -> {args.out}")


if __name__ == "__main__":
    main()
