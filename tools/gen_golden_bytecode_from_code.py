#!/usr/bin/env python3
"""Golden data of the bytecode table from raw code: tests/golden/bytecode_code_cases.npz.

Runs the unmodified reference's `Bytecode` (src/zkevm_specs/evm_circuit/typing.py:317-427) over the third-party stand-ins of
oracle/refshim on every directed code of tests/bytecode_code_cases.py of at most 600 bytes and records, per code, the code bytes,
`Bytecode(bytearray(code)).is_code` as uint8 and `.hash()` as 32 big-endian bytes.  Needs the reference checkout (--ref-root); the
file holds data only, the generator stays out of the test run.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-root", required=True, help="checkout of the reference (its src/ is imported unmodified)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "bytecode_code_cases.npz"))
    args = ap.parse_args()
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle", "refshim"), os.path.join(args.ref_root, "src")]
    from zkevm_specs.evm_circuit import Bytecode

    from tests.bytecode_code_cases import golden_codes

    codes = golden_codes()
    offsets = np.zeros(len(codes) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(c) for c in codes], dtype=np.uint64)
    is_code, hashes = [], []
    for c in codes:
        b = Bytecode(bytearray(c))
        assert len(b.is_code) == len(c)
        is_code.extend(int(bool(x)) for x in b.is_code)
        hashes.append(int(b.hash()).to_bytes(32, "big"))
    out = {"code": np.frombuffer(b"".join(codes), dtype=np.uint8), "offsets": offsets, "is_code": np.array(is_code, dtype=np.uint8),
           "hash": np.frombuffer(b"".join(hashes), dtype=np.uint8).reshape(len(codes), 32)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out}: {len(codes)} codes, {int(offsets[-1])} bytes of code, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
