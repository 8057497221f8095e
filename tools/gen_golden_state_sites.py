#!/usr/bin/env python3
"""Generate tests/golden/state_site_cases.npz: directed cases that make each numbered check of csrc/state_circuit.hpp the first
failure of one chosen row, recorded against the UNMODIFIED reference (needs the reference checkout; same recipe as oracle/gen_golden.py):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=oracle/refshim:<reference>/src:<reference>/tests python3 tools/gen_golden_state_sites.py

One valid base witness is built from an Operation list through the reference's assign_state_circuit and checked with its
check_state_row loop.  Candidate patches — directed ones per check, then a seeded random fill — are classified by oracle/state_oracle.py:
a candidate is a case of the site the oracle reports on its target row.  For every case the reference itself is run on the patched rows:
its exception class on the target row and the line of its state_circuit.py it raises at are stored (the first line of the innermost
statement of that file in the traceback — a statement's first line, so that the record does not depend on how an interpreter
attributes the lines of a multi-line call).  The oracle's kind of EVERY row must equal the reference's, and two cases of one site must
raise at one line, or the run fails.  Every (truncation, k) shift tests/state_site_cases.py applies is checked against the reference
on the unpatched base and recorded.  The file holds recorded results only: rows, patches, codes, kinds, line numbers.
"""
import ast
import dataclasses
import io
import os
import random
import sys
import traceback
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from oracle import codes, state_oracle as so, wire  # noqa: E402
from oracle.gen_golden import kind_of_exception  # noqa: E402
from tests import state_site_cases as ssc  # noqa: E402

SEED = 20261018
P = wire.P
PER_SITE = 4      # cases kept per site before the ones kept for their width, form or row
B64, B128, B160 = 1 << 64, 1 << 128, 1 << 160
C, F, M = ssc.PATCH_CELL, ssc.PATCH_FLAGS, ssc.PATCH_MPT
A1, A2 = 0x1234567890ABCDEF1234567890ABCDEF12345678, 0xFEDCBA9876543210FEDCBA9876543210FEDCBA98
K1, K2 = (0xAABBCCDD << 200) | 0x1516, (1 << 255) | (7 << 128) | 0x4959


# --------------------------------------------------------------------------------------------------------------------------------
# base
# --------------------------------------------------------------------------------------------------------------------------------
def base_ops():
    from zkevm_specs.evm_circuit import RW, AccountFieldTag, CallContextFieldTag, TxLogFieldTag, TxReceiptFieldTag
    from zkevm_specs.state_circuit import (AccountOp, CallContextOp, MemoryOp, StackOp, StartOp, StorageOp, TxAccessListAccountOp,
                                           TxAccessListAccountStorageOp, TxLogOp, TxReceiptOp, TxRefundOp)
    from zkevm_specs.util import FQ, Word

    R, W = RW.Read, RW.Write
    ops = []
    # Memory: first-access reads and writes, read-after-write, the address bound 2^32 - 1, two call ids
    for call in (1, 2):
        for a in range(12 if call == 1 else 4):
            addr = [0, 1, 2, 31, 32, 33, 255, 256, 65535, 65536, 2**32 - 2, 2**32 - 1][a]
            if a % 3 == 0:
                ops += [MemoryOp(0, R, call, addr, FQ(0)), MemoryOp(0, W, call, addr, FQ(200 + a)), MemoryOp(0, R, call, addr, FQ(200 + a))]
            elif a % 3 == 1:
                ops += [MemoryOp(0, W, call, addr, FQ(255)), MemoryOp(0, R, call, addr, FQ(255)), MemoryOp(0, W, call, addr, FQ(0))]
            else:
                ops += [MemoryOp(0, R, call, addr, FQ(0))]
    # Stack: id changes, pointer steps of 0 and 1, the pointer bound 1023, values with high limbs
    for call, top in ((1, 1023), (2, 1010), (2**28 - 1, 900)):
        for d in range(6):
            ptr = top - 5 + d
            v = [4321, B64 + 5, B128 + 9, (1 << 255) + 3, 0, 1][d]
            ops += [StackOp(0, W, call, ptr, Word(v)), StackOp(0, R, call, ptr, Word(v))]
            if d % 2:
                ops += [StackOp(0, W, call, ptr, Word(v + 1))]
    # Storage: an all-zero (non-existing) leaf and modified ones, more than one access per key (the last access carries the first's
    # value: the reference's mock MPT updates are made from the first op of a key)
    for tx in (1, 2):
        for addr in (A1 + tx, A2 + tx):  # (the mock MPT updates are keyed by address and key alone: one key group per pair)
            for key in (0x1516, K1, K2):
                if key == 0x1516:
                    ops += [StorageOp(0, R, tx, addr, key, Word(0), Word(0)), StorageOp(0, R, tx, addr, key, Word(0), Word(0))]
                elif key == K1:
                    v, c = Word(B128 + 789 + tx), Word(B64 + 98765)
                    ops += [StorageOp(0, W, tx, addr, key, v, c), StorageOp(0, W, tx, addr, key, Word(5), c), StorageOp(0, W, tx, addr, key, v, c),
                            StorageOp(0, R, tx, addr, key, v, c)]
                else:
                    ops += [StorageOp(0, W, tx, addr, key, Word(38491), Word(38491))]
    # CallContext: first-access reads (value 0) and writes, field tags up to 24 (the bound), word values
    for call in (1, 2, 2**28 - 1):
        for ft in (1, 2, 7, 24):
            if ft % 2:
                ops += [CallContextOp(0, R, call, ft, FQ(0)), CallContextOp(0, R, call, ft, FQ(0))]
            else:
                ops += [CallContextOp(0, W, call, ft, Word(B128 + ft)), CallContextOp(0, R, call, ft, Word(B128 + ft))]
    # Account: every field tag 1..4, the non-existing CodeHash case (0 -> 0), more than one access per key
    for addr in (A1, A2, 0x77):
        ops += [AccountOp(0, W, addr, AccountFieldTag.Nonce, FQ(1), FQ(0)), AccountOp(0, R, addr, AccountFieldTag.Nonce, FQ(1), FQ(0)),
                AccountOp(0, W, addr, AccountFieldTag.Balance, Word(B128 + 3), Word(B64)), AccountOp(0, W, addr, AccountFieldTag.Balance, Word(9), Word(B64)),
                AccountOp(0, R, addr, AccountFieldTag.Balance, Word(9), Word(B64)), AccountOp(0, W, addr, AccountFieldTag.Balance, Word(B128 + 3), Word(B64))]
        if addr == 0x77:
            ops += [AccountOp(0, R, addr, AccountFieldTag.CodeHash, Word(0), Word(0)), AccountOp(0, R, addr, AccountFieldTag.CodeHash, Word(0), Word(0))]
        else:
            ops += [AccountOp(0, R, addr, AccountFieldTag.CodeHash, Word((1 << 250) + addr % 1000), Word((1 << 250) + addr % 1000))]
        ops += [AccountOp(0, R, addr, AccountFieldTag.NonExisting, Word(0), Word(0))]
    # TxRefund, TxAccessListAccount, TxAccessListAccountStorage: first-access reads and writes
    for tx in (1, 2, 3):
        if tx != 2:
            ops += [TxRefundOp(0, R, tx, FQ(0))]
        ops += [TxRefundOp(0, W, tx, FQ(B64 + tx)), TxRefundOp(0, R, tx, FQ(B64 + tx)), TxRefundOp(0, W, tx, Word(B128 + tx))]
        for addr in (A1, A2):
            ops += [TxAccessListAccountOp(0, R, tx, addr, FQ(0)), TxAccessListAccountOp(0, W, tx, addr, FQ(1)), TxAccessListAccountOp(0, R, tx, addr, FQ(1))]
            for key in (0x1516, K2):
                if tx == 3:
                    ops += [TxAccessListAccountStorageOp(0, W, tx, addr, key, FQ(1))]
                else:
                    ops += [TxAccessListAccountStorageOp(0, R, tx, addr, key, FQ(0)), TxAccessListAccountStorageOp(0, W, tx, addr, key, FQ(1))]
    # TxLog: Topic (word values, high half used) and non-Topic rows
    for tx in (1, 2):
        for log in (1, 2):
            ops += [TxLogOp(0, W, tx, log, TxLogFieldTag.Address, 0, FQ(A1 % (1 << 150)))]
            for i in range(3):
                ops += [TxLogOp(0, W, tx, log, TxLogFieldTag.Topic, i, Word((1 << 255) + i))]
            for i in range(2):
                ops += [TxLogOp(0, W, tx, log, TxLogFieldTag.Data, i, FQ(255 - i))]
    # TxReceipt: four ids, both field tags, cumulative gas growing; ids 2 and 4 have the CumulativeGasUsed row alone, so that an id change
    # meets that row
    gas = 0
    for tx in (1, 2, 3, 4):
        if tx % 2:
            ops += [TxReceiptOp(0, R, tx, TxReceiptFieldTag.PostStateOrStatus, FQ(1 if tx == 1 else 0))]
        gas += 21000 + tx
        ops += [TxReceiptOp(0, R, tx, TxReceiptFieldTag.CumulativeGasUsed, FQ(gas))]
    # the State circuit's order; rw_counter counts up in it (insertion order within equal keys)
    # (the order check packs the storage key 32 bits above rw_counter WITHOUT making room for its 256 bits, state_circuit.py:557: a wide
    # key reaches into the field_tag / address limbs, and the order is that of the packed integer, not of the key tuple)
    def packed(o):
        v = int(o.tag)
        v = v * 2**28 + int(o.id)
        v = v * 2**160 + int(o.address)
        v = v * 2**16 + int(o.field_tag)
        return v * 2**32 + int(o.storage_key)

    order = sorted(range(len(ops)), key=lambda j: (packed(ops[j]), j))
    out = [StartOp(1, R, 0), StartOp(2, R), StartOp(3, R)]
    for c, j in enumerate(order):
        out.append(ops[j]._replace(rw_counter=c + 1))
    return out


def base_tables(ops):
    """the reference's mock MPT table, with the proof type of all-zero Storage / CodeHash leaves set to the non-existing proof the
    circuit looks up for them (the mock writes StorageMod / CodeHashMod for every leaf)"""
    from zkevm_specs.evm_circuit.table import MPTProofType
    from zkevm_specs.state_circuit import mpt_table_from_ops
    from zkevm_specs.util import FQ, Word

    out = set()
    for m in mpt_table_from_ops(ops):
        if m.value == Word(0) and m.value_prev == Word(0) and m.proof_type.n in (int(MPTProofType.StorageMod), int(MPTProofType.CodeHashMod)):
            m = dataclasses.replace(m, proof_type=FQ(int(MPTProofType.NonExistingAccountProof)))
        out.add(m)
    return out


# --------------------------------------------------------------------------------------------------------------------------------
# the reference on wire rows
# --------------------------------------------------------------------------------------------------------------------------------
class Ref:
    def __init__(self):
        import zkevm_specs.state_circuit as sc

        self.sc = sc
        self.file = os.path.abspath(sc.__file__)
        tree = ast.parse(open(self.file).read())
        self.stmt_first = {}  # line -> first line of the innermost statement that spans it
        for node in ast.walk(tree):
            if isinstance(node, ast.stmt):
                for ln in range(node.lineno, node.end_lineno + 1):
                    if ln not in self.stmt_first or node.lineno >= self.stmt_first[ln]:
                        self.stmt_first[ln] = node.lineno

    def row(self, r, fl):
        from zkevm_specs.util import FQ, Word, WordOrValue

        def wov(lo, hi, is_word):
            if is_word:
                return WordOrValue(Word((FQ(lo), FQ(hi)), check=False))
            w = WordOrValue(FQ(lo))
            w.hi = FQ(hi)
            return w

        keys = (FQ(r[so.TAG]), FQ(r[so.ID]), FQ(r[so.ADDR]), FQ(r[so.FIELD_TAG]), Word((FQ(r[so.KEY_LO]), FQ(r[so.KEY_HI])), check=False))
        return self.sc.Row(FQ(r[so.RWC]), FQ(r[so.IS_WRITE]), keys, tuple(FQ(x) for x in r[so.LIMB0:so.LIMB0 + 10]),
                           tuple(FQ(x) for x in r[so.BYTE0:so.BYTE0 + 32]), wov(r[so.VAL_LO], r[so.VAL_HI], fl & 1),
                           wov(r[so.INIT_LO], r[so.INIT_HI], fl & 2), Word((FQ(r[so.ROOT_LO]), FQ(r[so.ROOT_HI])), check=False), FQ(r[so.LEX]))

    def tables(self, mpt_rows):
        from zkevm_specs.evm_circuit import MPTTableRow
        from zkevm_specs.util import FQ, Word

        w = lambda lo, hi: Word((FQ(lo), FQ(hi)), check=False)  # noqa: E731
        return self.sc.Tables({MPTTableRow(FQ(m[0]), FQ(m[1]), w(m[2], m[3]), w(m[4], m[5]), w(m[6], m[7]), w(m[8], m[9]), w(m[10], m[11])) for m in mpt_rows})

    def check(self, ref_rows, tables, i):
        """(kind, line | call line << 16) of check_state_row on row i: 0, 0 when it passes.  line: of the innermost frame in state_circuit.py;
        call line: of the innermost frame there that is a check_* function — for a check made by a shared helper (assert_in_range,
        LowerThanGadget.verify, Tables.mpt_lookup) the line it was called from.  Both as the first line of their statement."""
        n = len(ref_rows)
        try:
            self.sc.check_state_row(ref_rows[i], ref_rows[(i - 1) % n], ref_rows[(i + 1) % n], tables)
            return 0, 0
        except Exception as e:  # noqa: BLE001 - the class is the record
            frames = [f for f in traceback.extract_tb(e.__traceback__) if os.path.abspath(f.filename) == self.file]
            checks = [f.lineno for f in frames if f.name.startswith("check_")]  # the innermost check_* frame: where a shared helper was called from
            return kind_of_exception(e), self.stmt_first[frames[-1].lineno] | (self.stmt_first[checks[-1]] << 16)

    def check_all(self, rows, flags, mpt_rows, only=None):
        ref_rows = [self.row(r, int(f)) for r, f in zip(rows, flags)]
        tables = self.tables(mpt_rows)
        return {i: self.check(ref_rows, tables, i) for i in (range(len(rows)) if only is None else only)}


# --------------------------------------------------------------------------------------------------------------------------------
# candidates
# --------------------------------------------------------------------------------------------------------------------------------
def with_limbs(addr):
    """patches (cell, value) that set the address cell and its limbs consistently (addr < 2^160)"""
    return [(so.ADDR, addr)] + [(so.LIMB0 + j, (addr >> (16 * j)) & 0xFFFF) for j in range(10)]


def with_bytes(key):
    return [(so.KEY_LO, key & (B128 - 1)), (so.KEY_HI, key >> 128)] + [(so.BYTE0 + j, (key >> (8 * j)) & 0xFF) for j in range(32)]


def directed(rows, flags, mpt_rows):
    """[(target row, [(kind, row, cell, value)], fixed)] — the ways each check can fail, on rows of every tag, with values below and above
    the ranges and with high limbs set (2^64 + x, 2^128 + x) wherever the cell admits them"""
    n = len(rows)
    out = []
    keys = lambda j: rows[j][so.TAG:so.KEY_HI + 1]  # noqa: E731
    first_of_group = lambda j: keys(j) != keys(j - 1)  # noqa: E731
    last_of_group = lambda j: keys(j) != keys((j + 1) % n)  # noqa: E731

    def add(t, cells, fixed=False, extra=()):
        prev = {(c, v) for c, v in cells if rows[t][c] == v}
        out.append((t, [(C, t, c, v % P) for c, v in cells if (c, v) not in prev] + list(extra), fixed))

    by_tag = {tg: [j for j in range(n) if rows[j][so.TAG] == tg] for tg in range(1, 12)}
    pick = lambda tg, pred: [j for j in by_tag[tg] if pred(j)]  # noqa: E731
    wide = [1, 2, 255, 256, 65535, 65536, 2**32, B64, B64 + 1, B128, B128 + 1, B160 + 1, P - 1]

    # sites 1..13 on a row of every tag (the second row of each tag and a row in the middle)
    for tg in range(2, 12):
        for t in {by_tag[tg][1], by_tag[tg][len(by_tag[tg]) // 2]}:
            r = rows[t]
            for v in (0, 13, 12, B64 + tg, B128 + tg, P - 1):
                add(t, [(so.TAG, v)])
            for v in (2**28, 2**28 - 1, B64 + r[so.ID], B128 + r[so.ID]):
                add(t, [(so.ID, v)])
            for v in (25, 24, B64 + r[so.FIELD_TAG], B128 + r[so.FIELD_TAG], P - 1):
                add(t, [(so.FIELD_TAG, v)])
            for j in (0, 4, 9):
                for v in (65536, B64 + r[so.LIMB0 + j], B128, r[so.LIMB0 + j] ^ 1):
                    add(t, [(so.LIMB0 + j, v)])
            for v in (r[so.ADDR] + B160, r[so.ADDR] + 1, B64 * B128 + r[so.ADDR] % B64):
                add(t, [(so.ADDR, v)])
            for j in (0, 15, 16, 31):
                for v in (256, B64 + r[so.BYTE0 + j], B128 + r[so.BYTE0 + j], r[so.BYTE0 + j] ^ 1):
                    add(t, [(so.BYTE0 + j, v)])
                    add((t + 1) % n, [], extra=[(C, t, so.BYTE0 + j, v)])  # the NEXT row packs this row's bytes: site 9
            for v in (r[so.KEY_LO] + B128, r[so.KEY_LO] + 1):
                add(t, [(so.KEY_LO, v)])
            for v in (r[so.KEY_HI] + B128, r[so.KEY_HI] + 1):
                add(t, [(so.KEY_HI, v)])
            for v in (2, B64, B64 + 1, B128 + 1, P - 1):
                add(t, [(so.IS_WRITE, v)])
            for v in (0, rows[t - 1][so.RWC], rows[t - 1][so.RWC] - 1, 2**32 + 1, B64 + r[so.RWC]):
                add(t, [(so.RWC, v)])
            for v in (r[so.VAL_LO] + 1, r[so.VAL_LO] + B64, r[so.VAL_LO] + B128):
                add(t, [(so.VAL_LO, v)])
            for c in (so.VAL_HI, so.INIT_LO, so.INIT_HI, so.ROOT_LO, so.ROOT_HI):
                for v in (r[c] + 1, r[c] + B64, r[c] + B128):
                    add(t, [(c, v)])
            out.append((t, [(F, t, 0, 1)], False))
            out.append((t, [(F, t, 0, 2)], False))
    # every row of every tag: the cells its per-tag checks read, one at a time
    for tg in range(1, 12):
        for t in by_tag[tg]:
            if t == 0:
                continue
            r = rows[t]
            if not (first_of_group(t) or last_of_group(t) or t % 3 == 0):
                continue
            add(t, [(so.FIELD_TAG, r[so.FIELD_TAG] + 1)])
            add(t, [(so.FIELD_TAG, 0)])
            add(t, [(so.FIELD_TAG, 5)])
            add(t, [(so.ID, r[so.ID] + 1)])
            add(t, [(so.ID, 0)])
            add(t, [(so.IS_WRITE, 1 - r[so.IS_WRITE])])
            add(t, [(so.RWC, 0)])
            for a in (1, 1024, 2**32, B64, B128, r[so.ADDR] + 2, r[so.ADDR] + 1, 1023, 2**32 - 1):
                add(t, with_limbs(a))
            for k in (1, B128, r[so.KEY_LO] + 1):
                add(t, with_bytes(k))
            for c in (so.VAL_LO, so.VAL_HI, so.INIT_LO, so.INIT_HI, so.ROOT_LO, so.ROOT_HI):
                for v in (0, 1, 2, 256, r[c] + 1, B64, B64 + 1, B128 + 1):
                    add(t, [(c, v)])
            out.append((t, [(F, t, 0, 1)], False))
            out.append((t, [(F, t, 0, 2)], False))
            out.append((t, [(F, t - 1, 0, 1)], False))
            for v in (rows[t - 1][so.VAL_LO], rows[t - 1][so.VAL_LO] - 1, rows[t - 1][so.VAL_LO] + 1):
                add(t, [(so.VAL_LO, v)])
            for v in (r[so.VAL_LO], r[so.VAL_LO] + B64, r[so.VAL_LO] + B128):  # the previous row's value grows past this one's
                out.append((t, [(C, t - 1, so.VAL_LO, v % P)], False))
    # Start rows: the rw_counter step and the lexicographic selector
    for t in (1, 2):
        for v in (B64 + 7, rows[t - 1][so.RWC], rows[t][so.RWC] + 1, 0):
            add(t, [(so.RWC, v)])
        for v in (0, 2, B64, B128):
            add(t, [(so.LEX, v)])
            add(t, [(so.LEX, v), (so.ROOT_LO, 77)])
            add(t, [(so.LEX, v), (so.RWC, 9)])
    # Start rows behind a Start row whose keys differ (its id made non-zero: that row fails at site 22): the read-consistency checks 11 / 12
    # do not apply, so the value / initial-value checks of the Start tag are reached on a row that shifts with the padding
    for t in (1, 2):
        for c in (so.VAL_HI, so.INIT_HI, so.VAL_LO, so.INIT_LO):
            for v in (1, B64 + 1, B128 + 1):
                add(t, [(c, v)], extra=[(C, t - 1, so.ID, 1)])
        out.append((t, [(C, t - 1, so.ID, 1), (F, t, 0, 1)], False))
        out.append((t, [(C, t - 1, so.ID, 1), (F, t, 0, 2)], False))
    # row 0 of the unshifted base: its previous row is row n - 1
    last = rows[n - 1]
    for cells in ([(so.FIELD_TAG, 1)], with_limbs(1), with_limbs(B128), [(so.ID, 1)], with_bytes(1), with_bytes(B128), [(so.VAL_HI, 1)], [(so.VAL_HI, B64)],
                  [(so.INIT_HI, B128)], [(so.LEX, 1)], [(so.LEX, B64)], [(so.LEX, B128), (so.RWC, last[so.RWC] + 1)], [(so.LEX, 1), (so.RWC, last[so.RWC] + 1)],
                  [(so.VAL_LO, 1)], [(so.VAL_LO, B128)], [(so.INIT_LO, 1)], [(so.INIT_LO, B64)],
                  [(so.LEX, 1), (so.RWC, last[so.RWC] + 1), (so.ROOT_LO, last[so.ROOT_LO]), (so.ROOT_HI, 1)]):
        add(0, cells, fixed=True)
    out.append((0, [(F, 0, 0, 1)], True))
    out.append((0, [(F, 0, 0, 2)], True))
    out.append((0, [(C, n - 1, so.BYTE0 + 3, 256)], True))  # row n - 1's bytes are packed by row 0
    # TxReceipt: ids 0 / above 2^11 on both rows of an id (the second row keeps the id and reaches the range check), id steps
    rc = by_tag[11]
    for a, b in ((rc[0], rc[1]), (rc[3], rc[4])):
        for v in (0, 2**11 + 1, 2**11, B64 + 1, 2**28 - 1):
            out.append((b, [(C, a, so.ID, v), (C, b, so.ID, v)], False))
    for t in rc:
        for v in (rows[t][so.ID] + 1, rows[t][so.ID] + 2, 0, 2, B64 + 2):
            add(t, [(so.ID, v)])
    # a tag-12 row placed last in the order
    add(n - 1, [(so.TAG, 12)])
    add(n - 2, [(so.TAG, 12)], extra=[(C, n - 1, so.TAG, 12)])
    # the MPT table: every cell of the rows the last accesses look up
    for m in range(len(mpt_rows)):
        users = [j for j in by_tag[4] + by_tag[6] if last_of_group(j) and rows[j][so.ADDR] == mpt_rows[m][0] and rows[j][so.KEY_LO] == mpt_rows[m][2]
                 and rows[j][so.KEY_HI] == mpt_rows[m][3] and rows[j][so.ROOT_LO] == mpt_rows[m][4]]
        if len(users) != 1:
            continue
        for cell in range(12):
            if m % 3 == cell % 3:
                out.append((users[0], [(M, m, cell, (mpt_rows[m][cell] + [1, B64, B128][cell % 3]) % P)], False))
    return out


def random_fill(rows, rng, count):
    n = len(rows)
    pool = [0, 1, 2, 3, 4, 5, 12, 24, 25, 255, 256, 1023, 1024, 2047, 2048, 2049, 65535, 65536, 2**28 - 1, 2**28, 2**32 - 1, 2**32, B64 - 1, B64, B64 + 1,
            B128 - 1, B128, B128 + 1, B160 - 1, B160, P - 1]
    for _ in range(count):
        t = rng.randrange(1, n)
        patches = []
        for _ in range(rng.choice([1, 1, 2])):
            r = t - rng.choice([0, 0, 0, 1])
            if rng.random() < 0.1:
                patches.append((F, r, 0, rng.choice([1, 2, 3])))
                continue
            c = rng.choice([0, 1, 2, 3, 4, 5, 6, 7, 50, 51, 52, 53, 54, 55, 56] * 3 + list(range(8, 50)))
            v = rng.choice(pool) if rng.random() < 0.6 else (rows[r][c] + rng.choice([1, -1, B64, B128])) % P
            patches.append((C, r, c, v))
        yield t, patches, False


def save_npz(path, arrays):
    """np.load-able archive with fixed member times: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, arr in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arr), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


# --------------------------------------------------------------------------------------------------------------------------------
def main():
    from zkevm_specs.state_circuit import assign_state_circuit
    from zkevm_specs_amd.flatten import flatten_mpt_table, flatten_state_rows

    ref = Ref()
    ops = base_ops()
    ref_rows = assign_state_circuit(ops)
    tables_ref = base_tables(ops)
    tables = ref.sc.Tables(tables_ref)
    for i, row in enumerate(ref_rows):  # the reference's own loop (tests/test_state_circuit.py verify)
        ref.sc.check_state_row(row, ref_rows[(i - 1) % len(ref_rows)], ref_rows[(i + 1) % len(ref_rows)], tables)
    cols, flags = flatten_state_rows(ref_rows)
    mpt = flatten_mpt_table(tables_ref)
    rows, mpt_rows = wire.colmajor_to_rows(cols), wire.rowmajor_to_rows(mpt)
    n = len(rows)
    assert n <= ssc.MAX_TARGET + 1, n
    assert not any(so.verify_rows(rows, flags, mpt_rows))
    assert not any(k for k, _ in ref.check_all(rows, flags, mpt_rows).values())  # the wire rows read back are the rows the reference accepts
    tags = sorted({r[so.TAG] for r in rows})
    assert tags == list(range(1, 12)), tags
    data = ssc.Data(cols, flags, mpt, rows, mpt_rows, [], {}, [], [], [], set(), SEED, ssc.n_start(rows))
    print(f"base: {n} rows, {len(mpt_rows)} MPT rows")

    rng = random.Random(SEED)
    cands = directed(rows, flags, mpt_rows) + list(random_fill(rows, rng, 6000))
    per_site, seen, all_cands = {}, set(), {}
    for t, patches, fixed in cands:
        patches = [p for p in patches]
        if not patches or (tuple(patches), t) in seen:
            continue
        seen.add((tuple(patches), t))
        c0 = ssc.Case(0, t, 0, 0, 0, fixed, 0, patches, [])
        _, fl, _, prow, pmpt, _, affected = ssc.build(data, c0, 0, 0)
        mpt_set = set(tuple(m) for m in pmpt)
        code = so.check_row(prow, fl, t, mpt_set)
        site = codes.site_of(code)
        if not code:
            continue
        kinds = tuple(sorted({(p[0], p[2] if p[0] == C else -1) for p in patches}))
        top = max(p[3] for p in patches)
        width = 2 if top >= B128 else 1 if top >= B64 else 0
        dropped_col = any(p[0] == C and 8 <= p[2] < 50 for p in patches)
        all_cands.setdefault(site, []).append((t, patches, fixed, kinds, width, dropped_col))
    # per site, in candidate order: the first case of each value width (below 2^64, 2^64 and above, 2^128 and above), the first the
    # 15-cell form can run, the first two on row 0, then other patched cells up to PER_SITE
    for site, cs in all_cands.items():
        got = []

        def take(pred, limit):
            for c in cs:
                if len([g for g in got if pred(g)]) >= limit:
                    break
                if c not in got and pred(c):
                    got.append(c)

        for w in (0, 1, 2):
            take(lambda c, w=w: c[4] == w and not c[2], 1)
        take(lambda c: not c[5] and not c[2], 1)
        take(lambda c: c[2], 2)
        for c in cs:
            if len(got) >= PER_SITE:
                break
            if c not in got and not c[2] and sum(1 for g in got if g[3] == c[3]) < 2:
                got.append(c)
        per_site[site] = [g[:4] for g in sorted(got, key=cs.index)]

    # the reference on every case: kinds of all rows == the oracle's, one line per site
    out_cases, site_line = [], {}
    for site in sorted(per_site):
        for t, patches, fixed, _ in per_site[site]:
            c0 = ssc.Case(site, t, 0, 0, 0, fixed, 0, patches, [])
            _, fl, _, prow, pmpt, _, affected = ssc.build(data, c0, 0, 0)
            exp = so.verify_rows(prow, fl, pmpt)
            assert exp == ssc.expected(prow, fl, pmpt, affected), ("a status changed outside the patched rows' neighbourhood", site, patches)
            refd = ref.check_all(prow, fl, pmpt)
            for i in range(n):
                assert refd[i][0] == codes.kind_of(exp[i]), ("reference / oracle disagree", site, t, i, patches, refd[i], hex(exp[i]))
            kind, line = refd[t]
            for i, e in enumerate(exp):  # every failing row of every case feeds the site <-> line table
                if e:
                    s = codes.site_of(e)
                    assert site_line.setdefault(s, refd[i][1]) == refd[i][1], ("two lines for one site", s, site_line[s], refd[i][1], patches)
            if ssc.touches_dropped(c0):
                ccode = ssc.EXCLUDED
            else:
                _, cfl, _, crow, cmpt, _, _ = ssc.build(data, c0, 0, 0, compact=True)
                ccode = so.check_row(crow, cfl, t, set(tuple(m) for m in cmpt))
            out_cases.append(ssc.Case(site, t, exp[t], kind, line, fixed, ccode, patches, [(i, e) for i, e in enumerate(exp) if e]))
    have = sorted({c.site for c in out_cases})
    missing = sorted(set(ssc.ALL_SITES) - set(have))
    shared = {}
    for s in have:
        shared.setdefault(site_line[s], []).append(s)
    pairs = [(a, b) for ss in shared.values() for a in ss for b in ss if a < b]

    # every shift the tests apply, against the reference on the unpatched base
    data = data._replace(cases=out_cases)
    checked = set()
    for c in out_cases:
        checked |= set(ssc.variants(rows, c))
    for trunc, k in sorted(checked):
        _, pfl, prow = ssc.padded(data, trunc, k)
        assert not any(kd for kd, _ in ref.check_all(prow, pfl, mpt_rows).values()), ("padded base fails the reference", trunc, k)
        assert not any(so.verify_rows(prow, pfl, mpt_rows)), (trunc, k)

    tried_txt = {82: "field_tag cell > 24 on CallContext rows (25, 2^64 + tag, 2^128 + tag, p - 1): site 3 fails first on all of them"}
    out = {"base_rows": cols, "base_flags": flags, "base_mpt": mpt, "seed": np.int64(SEED),
           "case_site": np.array([c.site for c in out_cases], dtype=np.uint32), "case_target": np.array([c.target for c in out_cases], dtype=np.uint32),
           "case_code": np.array([c.code for c in out_cases], dtype=np.uint32), "case_ref_kind": np.array([c.ref_kind for c in out_cases], dtype=np.uint8),
           "case_ref_line": np.array([c.ref_line for c in out_cases], dtype=np.uint32), "case_fixed": np.array([c.fixed for c in out_cases], dtype=np.uint8),
           "case_compact_code": np.array([c.compact_code for c in out_cases], dtype=np.uint32),
           "case_patch_off": np.cumsum([0] + [len(c.patches) for c in out_cases]).astype(np.uint32),
           "case_fail_off": np.cumsum([0] + [len(c.fails) for c in out_cases]).astype(np.uint32)}
    allp = [p for c in out_cases for p in c.patches]
    out["patch_kind"] = np.array([p[0] for p in allp], dtype=np.uint8)
    out["patch_row"] = np.array([p[1] for p in allp], dtype=np.uint32)
    out["patch_cell"] = np.array([p[2] for p in allp], dtype=np.uint8)
    out["patch_value"] = wire.ints_to_cells([p[3] for p in allp])
    allf = [f for c in out_cases for f in c.fails]
    out["fail_row"] = np.array([f[0] for f in allf], dtype=np.uint32)
    out["fail_code"] = np.array([f[1] for f in allf], dtype=np.uint32)
    out["site"] = np.array(sorted(site_line), dtype=np.uint32)
    out["site_line"] = np.array([site_line[s] for s in sorted(site_line)], dtype=np.uint32)
    out["unreached"] = np.array(missing, dtype=np.uint32)
    assert all(s in tried_txt for s in missing), ("a site without a case needs a written account of what was tried", missing)
    assert all(any(not c.fixed for c in out_cases if c.site == s) for s in have), "a site has row-0 cases only: it would never be shifted"
    out["unreached_tried"] = np.array([tried_txt[s] for s in missing])
    out["shared_lines"] = np.array(pairs, dtype=np.uint32).reshape(-1, 2)
    out["checked_variants"] = np.array(sorted(checked), dtype=np.int32).reshape(-1, 2)
    path = ssc.path(os.path.join(ROOT, "tests", "golden"))
    save_npz(path, out)

    print(f"{len(out_cases)} cases over {len(have)} of {len(ssc.ALL_SITES)} sites ; "
          f"{len(checked)} shifts checked against the reference -> {path} ({os.path.getsize(path)} bytes)")
    print("site: reference line, cases, cases with a 15-cell form")
    for s in have:
        cs = [c for c in out_cases if c.site == s]
        print(f"  {s:3d}: line {site_line[s] & 0xFFFF:3d} (called from {site_line[s] >> 16:3d}), {len(cs)} cases, {sum(1 for c in cs if c.compact_code != ssc.EXCLUDED)} compact")
    print("sites without a case:", missing)
    for s in missing:
        print(f"  {s}: tried {tried_txt[s]}")
    print("reference (line, call line) that serve more than one site:", {(ln & 0xFFFF, ln >> 16): ss for ln, ss in sorted(shared.items()) if len(ss) > 1})
    assert len(missing) <= 3, missing


if __name__ == "__main__":
    main()
