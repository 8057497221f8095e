"""Compare two build/resource_usage.txt files kernel by kernel (SGPRs, VGPRs, scratch, occupancy, LDS; source positions ignored):
    python tools/compare_resource_usage.py PARENT NEW
prints the kernels whose figures differ or that are gone, then the new ones; exit status 1 when an existing kernel moved."""
import re
import sys


def load(path):
    out = {}
    for line in open(path):
        m = re.search(r"Name: (\S+)", line)
        if m:
            out[m.group(1)] = " ".join(re.findall(r"(?:TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): \d+", line))
    return out


def main(parent, new):
    a, b = load(parent), load(new)
    moved = [k for k in a if a[k] != b.get(k)]
    for k in moved:
        print(f"MOVED {k}\n  was {a[k]}\n  is  {b.get(k, 'gone')}")
    for k in b:
        if k not in a:
            print(f"NEW   {k}: {b[k]}")
    print(f"{len(a)} kernels before, {len(b)} after, {len(moved)} moved")
    return 1 if moved else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
