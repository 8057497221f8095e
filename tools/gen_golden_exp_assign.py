#!/usr/bin/env python3
"""Golden cases of the Exp circuit's witness assignment: tests/golden/exp_assign_cases.npz.

Runs the unmodified reference's `ExpCircuit` (src/zkevm_specs/evm_circuit/typing.py:868-994) and `Tables` (evm_circuit/table.py:
654-671) over the third-party stand-ins of oracle/refshim and records, per case, the calls made on the circuit (`add_event` arguments
as decimal strings, `fill_dummy_events`), `max_exp_steps`, the flattened rows, the exp table as a sorted row list and, where a call
raised, the exception's class and the index of the call.  Needs the reference checkout (--ref-root); the cases are data, the
generator stays out of the test run.
"""
import argparse
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POW2 = 2**256


def build_cases():
    rng = random.Random(20261016)
    F = "fill"
    cases = []  # (name, max_exp_steps, calls); a call is (base, exponent, identifier) or F
    exps = [0, 1, 2, 3, 4, 2**128 - 1, 2**128, 2**255, POW2 - 1]
    bases = [0, 1, 2, 2**128, POW2 - 1, 2**250, 6 << 200, rng.getrandbits(256), rng.getrandbits(256) | 1]
    for k, e in enumerate(exps):
        cases.append((f"exponent_{k}", 100, [(rng.getrandbits(256), e, 5 + k), F]))
    for k, b in enumerate(bases):
        cases.append((f"base_{k}", 100, [(b, rng.getrandbits(70) | (1 << 69), 9), F]))
    cases.append(("even_base_reaches_zero", 0, [(2**20 * 3, rng.getrandbits(256), 1)]))
    cases.append(("several_events", 100, [(3, 101, 4), (5, 0, 9), (7, 1, 9), (rng.getrandbits(256), 259, 12), (0, 0, 13), (2, 1023, 30), F]))
    cases.append(("empty_events_only", 2, [(3, 0, 4), (5, 1, 9), F]))
    cases.append(("no_fill", 100, [(rng.getrandbits(256), rng.getrandbits(40), 3), (rng.getrandbits(256), rng.getrandbits(256), 2**200 + 1)]))
    cases.append(("pad_left", 5, [(3, 101, 4), F]))           # 9 step rows < 35
    cases.append(("pad_exact", 2, [(7, 255, 4), F]))          # bit_length 8, popcount 8: 14 step rows == 7 * 2
    cases.append(("pad_exceeded", 1, [(3, 101, 4), F]))       # 9 step rows > 7
    cases.append(("default_max", None, [(POW2 - 1, POW2 - 1, 77), F]))
    cases.append(("identifier_reduced", 3, [(2, 5, 21888242871839275222246405745257275088548364400416034343698204186575808495617 + 6), F]))
    for k, (b, e) in enumerate([(0, 0), (0, POW2 - 1), (1, 0), (1, POW2 - 1), (0xCAFE, 0), (POW2 - 1, 0), (0, 1), (1, 1), (0xCAFE, 1),
                                (POW2 - 1, 1), (2, 5), (3, 101), (5, 259), (7, 1023), (POW2 - 1, 2), (POW2 - 1, 3), (POW2 - 1, POW2 - 1)]):
        cases.append((f"ref_test_exp_{k}", None, [(b, e, 6), F]))
    # outcomes Python's own types decide
    cases.append(("exc_base_wide_exp0", 100, [(3, 5, 1), (POW2, 0, 2)]))
    cases.append(("exc_base_wide_exp1", 100, [(POW2, 1, 2)]))
    cases.append(("exc_base_wide", 100, [(POW2 + 5, 7, 2)]))
    cases.append(("exc_base_negative_exp0", 100, [(-1, 0, 2)]))
    cases.append(("exc_base_negative", 100, [(-7, 9, 2)]))
    cases.append(("exc_exponent_wide", 100, [(3, POW2, 2)]))
    cases.append(("exc_exponent_negative", 100, [(3, -1, 2)]))
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-root", required=True, help="checkout of the reference (its src/ is imported unmodified)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "exp_assign_cases.npz"))
    args = ap.parse_args()
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle", "refshim"), os.path.join(args.ref_root, "src")]
    from zkevm_specs.evm_circuit import ExpCircuit, Tables

    from zkevm_specs_amd.flatten import flatten_exp_rows
    from zkevm_specs_amd.wire import rows_to_rowmajor

    out, names, total = {}, [], 0
    for ci, (name, mx, calls) in enumerate(build_cases()):
        names.append(name)
        circuit = ExpCircuit() if mx is None else ExpCircuit(mx)
        exc, at = "", -1
        for k, c in enumerate(calls):
            try:
                circuit.fill_dummy_events() if c == "fill" else circuit.add_event(*c)
            except BaseException as e:  # noqa: BLE001 - the reference's exception is the outcome (RecursionError included)
                exc, at = type(e).__name__, k
                break
        out[f"c{ci}_calls"] = np.array(json.dumps([c if c == "fill" else [str(v) for v in c] for c in calls]))
        out[f"c{ci}_max"] = np.array([circuit.max_exp_steps], dtype=np.int64)
        out[f"c{ci}_exc"] = np.array([exc, str(at)])
        if exc:
            print(f"{name}: raises {exc} at call {at}")
            continue
        rows = circuit.rows
        out[f"c{ci}_rows"] = flatten_exp_rows(rows) if rows else np.zeros((21, 0, 4), dtype=np.uint64)
        table = Tables(set(), set(), set(), set(), set(), exp_circuit=rows).exp_table if rows else set()
        ints = sorted((r.is_step.n, r.identifier.n, r.is_last.n, r.base_limb0.n, r.base_limb1.n, r.base_limb2.n, r.base_limb3.n,
                       r.exponent.lo.n, r.exponent.hi.n, r.exponentiation.lo.n, r.exponentiation.hi.n) for r in table)
        out[f"c{ci}_table"] = rows_to_rowmajor(ints, 11) if ints else np.zeros((0, 11, 4), dtype=np.uint64)
        total += len(rows)
        print(f"{name}: {len(rows)} rows, {len(ints)} table rows")
    out["names"] = np.array(names)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out}: {len(names)} cases, {total} rows, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
