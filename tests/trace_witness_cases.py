"""zk_evm_witness_from_trace: the directed case builders, shared by the CPU and GPU tests.  A case is a records dict
(zkevm_specs_amd.trace); the expected wires come from the plain-Python model of tests/trace_witness_ref.py, computed once per case and
shared read-only.  The builders assert their own coverage (test_directed_sets_cover_what_they_claim)."""
import functools
import glob
import os
import random

import numpy as np

from tests import trace_witness_ref as ref
from zkevm_specs_amd import errors, trace

P = ref.P
U64 = (1 << 64) - 1
OUTPUTS = ("rw", "rw_flags", "steps")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RW_SIZES = (1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097)
STEP_SIZES = (1, 2, 31, 32, 33, 64, 65, 1025)
EDGE_WORDS = (0, 1, P - 1, P, P + 1, (1 << 128) - 1, 1 << 128, (1 << 160) - 1, (1 << 256) - 1)
RW_NAMES = tuple(f"rw_{n}_{v}" for n in RW_SIZES for v in "ab")
STEP_NAMES = tuple(f"steps_{n}" for n in STEP_SIZES)
NAMES = RW_NAMES + STEP_NAMES


def limbs(w):
    return [(w >> (64 * k)) & U64 for k in range(4)]


def _u64(rng, i):
    return (0, U64)[i % 2] if i % 7 < 2 else rng.getrandbits(rng.choice((1, 8, 32, 64)))


def _rw_case(n, variant, rng):
    """rows 0, n - 1 and either side of every multiple of 16 (so of 64) are all-wide or all-narrow, swapped between the variants; the
    others walk the 32 combinations of the pool bits.  Each operand position walks EDGE_WORDS (and three random words) over its wide rows, from its own phase."""
    head, pool, uses = np.zeros(n, np.uint32), [], [0, 3, 6, 9, 1]
    for i in range(n):
        edge_row = i in (0, n - 1) or i % 16 in (15, 0)
        combo = (31 if (i + variant) % 2 == 0 else 0) if edge_row else (i * 7 + 3 + variant) % 32
        field_tag = (0, 255)[(i // 5) % 2] if i % 5 < 2 else rng.randrange(256)
        h = (i + variant) % 2 | ((i % 16) << 1) | (field_tag << 8) | (rng.getrandbits(2) << 16) | (combo << 20)
        if n <= 3:
            h = (h & ~(3 << 16)) | (((i + variant) % 4) << 16)
        head[i] = h
        for slot in range(5):
            if (combo >> slot) & 1:
                k = uses[slot] % (len(EDGE_WORDS) + 3)
                uses[slot] += 1
                pool.append(limbs(EDGE_WORDS[k] if k < len(EDGE_WORDS) else rng.getrandbits(256)))
    mode = (RW_SIZES.index(n) + variant) % 3
    rec = {"head": head, "pool": np.array(pool, dtype=np.uint64).reshape(-1, 4), "rw_counter": None, "rw_base": 1,
           "steps": np.zeros((0, 13), np.uint64)}
    for j, k in enumerate(("id", "addr", "val", "prev")):
        rec[k] = np.array([_u64(rng, i + j) for i in range(n)], dtype=np.uint64)
    if mode == 1:
        rec["rw_base"] = (1 << 64) - n  # the last counter is 2^64 - 1
    elif mode == 2:
        rec["rw_counter"] = np.cumsum([rng.randrange(1, 1000) for _ in range(n)]).astype(np.uint64) + np.uint64(rng.getrandbits(40))
    return rec


def _step_case(n, rng):
    steps = np.zeros((n, 13), np.uint64)
    for i in range(n):
        steps[i, 0] = (0, 255, rng.randrange(256))[i % 3] | (((i // 3) % 4) << 8)
        for k in range(1, 9):
            steps[i, k] = (0, U64, rng.getrandbits(64))[(i + k) % 3]
        j = i % (len(EDGE_WORDS) + 2)
        steps[i, 9:13] = limbs(EDGE_WORDS[j] if j < len(EDGE_WORDS) else rng.getrandbits(256))
    return trace.trace_records(None, steps)


@functools.lru_cache(maxsize=None)
def _all(seed=20261021):
    rng = random.Random(seed)
    out = {}
    for n in RW_SIZES:
        for v, tag in enumerate("ab"):
            out[f"rw_{n}_{tag}"] = _rw_case(n, v, rng)
    for n in STEP_SIZES:
        out[f"steps_{n}"] = _step_case(n, rng)
    for rec in out.values():
        for a in rec.values():
            if hasattr(a, "setflags"):
                a.setflags(write=False)
    return out


def directed(name):
    return _all()[name]


@functools.lru_cache(maxsize=None)
def expected(name):
    out = ref.model(directed(name))
    for a in out.values():
        a.setflags(write=False)
    return out


def mutable(name):
    return {k: v.copy() if hasattr(v, "copy") else v for k, v in directed(name).items()}


def same(got, exp):
    return all(np.array_equal(got[k], exp[k]) and got[k].dtype == exp[k].dtype for k in OUTPUTS)


def coverage():
    """what the directed sets hold, for the coverage test"""
    combos, tags, fields, modes, flag_forms = set(), set(), set(), set(), set()
    edge_at = {slot: set() for slot in range(5)}
    ends = {31: set(), 0: set()}
    for name in RW_NAMES:
        rec = directed(name)
        n, at = len(rec["head"]), 0
        modes.add("explicit" if rec["rw_counter"] is not None else rec["rw_base"] == 1)
        for i, h in enumerate(int(x) for x in rec["head"]):
            combo = h >> 20
            combos.add(combo)
            tags.add((h >> 1) & 15)
            fields.add((h >> 8) & 255)
            flag_forms.add(((h >> 16) & 1, (combo >> 2) & 1))
            flag_forms.add(((h >> 17) & 1, (combo >> 3) & 1))
            if combo in ends:
                ends[combo] |= {w for w, hit in (("first", i == 0), ("last", i == n - 1), ("before16", i % 16 == 15), ("at16", i and i % 16 == 0),
                                                 ("before64", i % 64 == 63), ("at64", i and i % 64 == 0)) if hit}
            for slot in range(5):
                if (combo >> slot) & 1:
                    edge_at[slot].add(sum(int(x) << (64 * k) for k, x in enumerate(rec["pool"][at])))
                    at += 1
    return {"combos": combos, "tags": tags, "fields": fields, "modes": modes, "flag_forms": flag_forms, "edge_at": edge_at, "ends": ends}


# ---- the golden corpus ------------------------------------------------------------------------------------------------------------------
def golden_cases():
    """(where, rw, rw_flags, steps) of every case of tests/golden/evm_*.npz"""
    for path in sorted(glob.glob(os.path.join(GOLDEN, "evm_*.npz"))):
        z = np.load(path)
        for c in sorted({k.split("_")[0] for k in z.files if k.startswith("c")}):
            yield f"{os.path.basename(path)} {c}", z[f"{c}_rw"], z[f"{c}_rw_flags"], z[f"{c}_steps"]


@functools.lru_cache(maxsize=None)
def long_table():
    """every golden RW table the records hold, concatenated, each table's counters rebased above the previous table's: (records, rw,
    rw_flags) with about 42,000 rows — every row form the corpus has, at arbitrary phases of the writer's 16-row period"""
    tables, flags, base = [], [], 0
    for _, rw, fl, _ in golden_cases():
        if not rw.shape[0]:
            continue
        try:
            trace.rw_ops_from_wire(rw, fl)
        except errors.UnsupportedOnDevice:
            continue
        rw = rw.copy()
        rw[:, 0, 0] = rw[:, 0, 0] - rw[0, 0, 0] + np.uint64(base + 3)  # (an accepted table's counters span far less than 2^64: no carry)
        base = int(rw[-1, 0, 0])
        tables.append(rw)
        flags.append(fl)
    rw, fl = np.concatenate(tables), np.concatenate(flags)
    rec = trace.trace_records(trace.rw_ops_from_wire(rw, fl))
    for a in (rw, fl, *[v for v in rec.values() if hasattr(v, "setflags")]):
        a.setflags(write=False)
    return rec, rw, fl
