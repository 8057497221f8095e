#!/usr/bin/env python3
"""Write tests/golden/arith_cases.npz: reference labels for the directed arithmetic operands (tests/evm_arith_cases.py).

Runs where the reference is (staged under oracle/_ref/ by oracle/stage_ref.py, or --ref-root).  Per opcode (MUL DIV MOD SDIV SMOD
ADDMOD MULMOD) one passing two-step golden case is the base; every directed and edge operand tuple is written into the value cells of
its stack rows with the word the opcode pushes, and a seeded quarter of them once more with a wrong pushed word (result + 1, - 1,
+ divisor, quotient and remainder swapped, 0).  Each case goes to the oracle and to the unmodified reference's verify_step; the file
records the operand words, the pushed word, the opcode, the oracle's status code and the reference's exception class (`ref_kind`).
No witness is stored: tests/evm_arith_cases.py rebuilds it from the base.  A case on which the oracle's kind is not the reference's
fails the run.
Run: python tools/gen_golden_evm_arith.py [--ref-root oracle/_ref] [--out tests/golden/arith_cases.npz]
"""
import argparse
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gen_golden_evm_checkpoints as ck  # noqa: E402  (ref_kind_of, add_ref_path, save_npz)
from oracle import codes, wire  # noqa: E402
from tests import evm_arith_cases as ac  # noqa: E402
from tests.evm_cases import load_cases, oracle_status  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
INVALID_ONE_IN = 4


def wrong_words(op, t, res, rng):
    """one wrong pushed word for the step, of the kinds tests/evm_arith_cases.py invalid_variant() uses"""
    div = t[-1] if len(t) == 3 else t[1]
    twin = {"DIV": "MOD", "MOD": "DIV", "SDIV": "SMOD", "SMOD": "SDIV"}.get(op)
    swapped = ac.evm_result(twin, t) if twin else ((t[0] * t[1] if op == "MULMOD" else t[0] + t[1]) // div if div else 1)
    v = rng.choice([res + 1, res - 1, res + div, swapped, 0]) & ac.M256
    return v if v != res else (res + 1) & ac.M256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-root", default=os.path.join(ROOT, "oracle", "_ref"))
    ap.add_argument("--out", default=ac.path(GOLDEN))
    a = ap.parse_args()
    ck.add_ref_path(a.ref_root)
    import zkevm_specs  # noqa: F401  (fail early when the reference is not there)

    bases = ac.find_bases(GOLDEN)
    assert set(bases) == set(ac.OPCODES), bases
    gold = {op: list(load_cases(os.path.join(GOLDEN, ac.BASE_FILES[op])))[ci] for op, ci in bases.items()}
    rng = random.Random(f"{ac.SEED}/golden")
    todo = []
    for op, t in ac.all_cases():
        res = ac.evm_result(op, t)
        todo.append((op, t, res))
        if rng.randrange(INVALID_ONE_IN) == 0:
            todo.append((op, t, wrong_words(op, t, res, rng)))
    ops, words, code_l, kind_l, mismatches = [], [], [], [], []
    per_op = {}
    for op, t, pushed in todo:
        _, w, opts, _ = gold[op]
        cw = ac.case_wire(w, t, pushed)
        code = oracle_status(cw, opts)[0]
        rk = ck.ref_kind_of(cw, opts, 0)
        if codes.kind_of(code) != rk:
            mismatches.append((op, t, pushed, hex(code), rk))
        ops.append(ac.OPCODES.index(op))
        words += list(t) + [0] * (3 - len(t)) + [pushed]
        code_l.append(code)
        kind_l.append(rk)
        row = per_op.setdefault(op, [0, 0])
        row[0 if code == 0 else 1] += 1
    files = {
        "op": np.array(ops, dtype=np.uint8), "words": wire.ints_to_cells(words).reshape(-1, 4, 4),
        "code": np.array(code_l, dtype=np.uint32), "ref_kind": np.array(kind_l, dtype=np.uint8),
        "base_case": np.array([bases[op] for op in ac.OPCODES], dtype=np.int32), "seed": np.array(ac.SEED, dtype=np.int64),
    }
    ck.save_npz(a.out, files)
    for op in ac.OPCODES:
        print(f"{op:7s} base {ac.BASE_FILES[op]}[{bases[op]}]  passing {per_op[op][0]:4d}  failing {per_op[op][1]:4d}")
    print(f"{len(ops)} cases -> {os.path.getsize(a.out) // 1024} KiB")
    for mm in mismatches[:40]:
        print("ORACLE / REFERENCE KIND MISMATCH", mm)
    if mismatches:
        sys.exit(f"{len(mismatches)} cases where the oracle's kind is not the reference's: a finding, fix the oracle")


if __name__ == "__main__":
    main()
