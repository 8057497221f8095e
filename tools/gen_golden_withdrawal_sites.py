#!/usr/bin/env python3
"""Write tests/golden/withdrawal_site_cases.npz: every variant of tests/withdrawal_site_cases.py in its smallest form (the 6-row bases of
`SMALL`, the one-lane and small-table variants as they are where they have at most 8 rows), judged by the UNMODIFIED reference.

Runs where the reference is staged (oracle/_ref, through oracle/refshim), with `Ref` of tools/gen_golden_withdrawal.py.  Per case the file
holds the wire arrays (rows uint64[n, 8, 4], mpt uint64[m, 12, 4], keccak uint64[k, 5, 4], block uint64[b, 4, 4]), max_withdrawals,
total_rows, the per-row status of the model tests/withdrawal_ref.py, its first failure (`first_row`, `first_kind`) and the class of the
exception the reference's verify_circuit raised (`ref_outcome`, "" for none).  The script stops where that class and the model's first
kind disagree: the new ground of these variants (a padding row with hash cells, value_prev, hash twins, the 2^128 key split) is the
reference's verdict before it is the model's.  Only recorded data is written; the file re-creates byte for byte (fixed zip dates).
Run: python tools/gen_golden_withdrawal_sites.py [--ref-root oracle/_ref] [--out tests/golden/withdrawal_site_cases.npz]
"""
import argparse
import io
import json
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gen_golden_withdrawal as g  # noqa: E402
from tests import withdrawal_ref as W  # noqa: E402
from tests import withdrawal_site_cases as sc  # noqa: E402

MAX_ROWS = 8
assert g.RANDOMNESS == sc.R


def small_targets(name):
    """the rows a variant stands on in the small form: an interior row on either side of the carry, the last row for the last-row forms"""
    placements = sc.VARIANTS[name][4]
    if isinstance(placements[0], str):
        return placements
    if name.startswith("4/") and name.endswith("_rows") or name.startswith("1/index"):
        return (sc.SMALL.n - 1,)
    return (sc.SMALL.carry + 1, sc.SMALL.carry - 1)


def small_cases():
    sc.FORM = sc.SMALL
    try:
        out = []
        for name, (_, code, fn, first, _) in sc.VARIANTS.items():
            if name.startswith(("3/mpt_511", "3/mpt_512")):
                continue  # (capacity steps of the full form only)
            for t in small_targets(name):
                made = fn(t)
                if made is None or len(made[0].rows) > MAX_ROWS:
                    continue
                w, target = made
                status = sc.status_of(w)
                assert status[target] == code, (name, t, hex(status[target]), hex(code))
                assert not code or not first or W.first_failure(status) == (target, code), (name, t)
                out.append((f"{name}@{t}", w, status, target))
        return out
    finally:
        sc.FORM = sc.FULL


def write_npz(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, arr in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arr), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-root", default=os.path.join(ROOT, "oracle", "_ref"))
    ap.add_argument("--out", default=sc.GOLDEN)
    args = ap.parse_args()
    ref = g.Ref(args.ref_root)
    arrays, metas = {}, []
    for i, (name, w, status, target) in enumerate(small_cases()):
        row, code = W.first_failure(status)
        outcome = ref.outcome(w.rows, w.mpt, w.keccak, w.block, w.m, ())
        assert outcome == g.KIND_NAMES[code >> 24], (name, outcome, row, hex(code))
        metas.append({"name": name, "max_withdrawals": w.m, "total_rows": len(w.rows), "target": target, "first_row": -1 if row is None else row,
                      "first_kind": code >> 24, "ref_outcome": outcome})
        arrays.update({f"{i}_rows": g.cells(w.rows, 8), f"{i}_mpt": g.cells(w.mpt, 12), f"{i}_keccak": g.cells(w.keccak, 5),
                       f"{i}_block": g.cells(w.block, 4), f"{i}_status": np.array(status, dtype=np.uint32)})
    covered = {m["name"].split("@")[0] for m in metas}
    missing = set(sc.VARIANTS) - covered
    assert missing <= {n for n in sc.VARIANTS if n.startswith(("3/mpt_15", "3/mpt_16", "3/mpt_511", "3/mpt_512"))}, sorted(missing)
    arrays["meta"] = np.array(json.dumps({"randomness": hex(sc.R), "cases": metas, "not_judged": sorted(missing)}, sort_keys=True))
    write_npz(args.out, arrays)
    print(f"{len(metas)} cases ({sum(1 for m in metas if m['first_kind'])} failing), {len(covered)} variants -> {args.out} ({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()
