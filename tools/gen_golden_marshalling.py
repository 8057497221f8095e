#!/usr/bin/env python3
"""Record how the calls of tests/marshalling_cases.py reach the library: tests/golden/marshalling_calls_cpu.json (host arrays through
the CPU backend; no GPU needed) or, with --hip, marshalling_calls_hip.json (device tensors through the HIP library; needs the GPU).
Run at the commit whose marshalling is the reference — the tests replay the list on the code under test and require equal records.

    python tools/gen_golden_marshalling.py [--hip] [--out PATH]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hip", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    from tests import marshalling_cases

    log = marshalling_cases.run(None if a.hip else "cpu")
    path = a.out or os.path.join(ROOT, "tests", "golden", f"marshalling_calls_{'hip' if a.hip else 'cpu'}.json")
    with open(path, "w") as f:
        json.dump(log, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{path}: {len(log)} cases, {sum(len(c['calls']) for c in log.values())} calls, "
          f"{sum('raised' in c for c in log.values())} refusals")


if __name__ == "__main__":
    main()
