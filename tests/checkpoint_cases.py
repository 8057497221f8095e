"""Directed checkpoint cases of the EVM circuit (tests/golden/checkpoint_cases.npz, written by tools/gen_golden_evm_checkpoints.py).

The file holds no witnesses: a case is a *base* — one passing step pair of a golden case in tests/golden/evm_*.npz — plus a few
patches (one cell of one table row overwritten, or the type bits of a row flipped), the oracle's status code of the patched pair and the
exception class the unmodified reference raises on it (`ref_kind`).  Every case makes one particular checkpoint of
csrc/evm_circuit.hpp the FIRST one that fails, so a checkpoint that is missing or weaker in the kernel shows as a wrong code.

This module rebuilds the wire dicts and carries the census: which checkpoints of the accepted paths are the failing site of some case.
"""
import os
from collections import namedtuple

import numpy as np

from oracle import codes, evm_oracle as eo, wire
from tests.evm_cases import golden_files, load_cases, to_witness

FILE = "checkpoint_cases.npz"
# patch targets: cell tables (a patch overwrites one 32-byte cell) and flag tables (a patch xors the row's type bits)
CELL_TABLES = ("steps", "rw", "bytecode", "tx", "block", "copy", "keccak", "exp", "sig", "ecc", "withdrawals", "aux")
FLAG_TABLES = ("rw_flags", "tx_flags", "block_flags")
TABLES = CELL_TABLES + FLAG_TABLES

Base = namedtuple("Base", "file case pair state count failable unreached tried")
Case = namedtuple("Case", "base code ref_kind patches")  # patches: [(table name, row, cell, value)]; flag tables: cell = 0, value = xor mask


def path(golden_dir):
    return os.path.join(golden_dir, FILE)


def load(golden_dir):
    g = np.load(path(golden_dir))
    bases = []
    fo, uo = g["base_failable_off"], g["base_unreached_off"]
    for b in range(len(g["base_file"])):
        bases.append(Base(str(g["base_file"][b]), int(g["base_case"][b]), int(g["base_pair"][b]), int(g["base_state"][b]),
                          int(g["base_count"][b]), g["base_failable"][fo[b]:fo[b + 1]].tolist(),
                          g["base_unreached"][uo[b]:uo[b + 1]].tolist(), g["base_unreached_tried"][uo[b]:uo[b + 1]].tolist()))
    cases = []
    po = g["case_patch_off"]
    values = wire.cells_to_ints(g["patch_value"]) if len(g["patch_value"]) else []
    for c in range(len(g["case_base"])):
        patches = [(TABLES[int(g["patch_table"][k])], int(g["patch_row"][k]), int(g["patch_cell"][k]), values[k]) for k in range(po[c], po[c + 1])]
        cases.append(Case(int(g["case_base"][c]), int(g["case_code"][c]), int(g["case_ref_kind"][c]), patches))
    return bases, cases, {k: g[k] for k in ("seed", "moves", "values")}


class _Goldens:
    """golden cases by (file name, index), one file decoded at a time (cases are grouped by base, bases by file)"""

    def __init__(self, golden_dir):
        self.dir, self.name, self.cases = golden_dir, None, None

    def get(self, name, idx):
        if name != self.name:
            self.name, self.cases = name, list(load_cases(os.path.join(self.dir, name)))
        return self.cases[idx]


def apply_patches(w, patches):
    """a copy of wire dict `w` with the patches applied"""
    out = dict(w)
    for table, row, cell, value in patches:
        if out[table] is w[table]:
            out[table] = w[table].copy()
        if table in FLAG_TABLES:
            out[table][row] ^= np.uint32(value)
        else:
            out[table][row, cell] = np.frombuffer(int(value).to_bytes(32, "little"), dtype="<u8")
    return out


def is_wide(case):
    """the patch makes a step cell wider than the hot kernel stages (>= 2^64) or a word cell of a table wide (>= 2^128): the pair
    (or a lookup of it) leaves the fast path"""
    return any((t == "steps" and v >= 1 << 64) or (t in CELL_TABLES and t != "steps" and v >= 1 << 128) for t, _, _, v in case.patches)


def iter_cases(golden_dir, loaded=None):
    """(case index, Case, Base, golden name, wire dict, opts) for every case of the file"""
    bases, cases, _ = loaded or load(golden_dir)
    gold = _Goldens(golden_dir)
    for k, c in enumerate(cases):
        b = bases[c.base]
        name, w, opts, _ = gold.get(b.file, b.case)
        yield k, c, b, name, apply_patches(w, c.patches), opts


def pair_flags(opts, n_steps, pair):
    return bool(opts[0]) and pair == 0, bool(opts[1]) and pair == n_steps - 2


def traced_status(w, opts):
    """[(status code, checkpoints evaluated, ordinals reached through require)] for every pair of wire dict `w`"""
    W = to_witness(w)
    n = len(W.steps)
    out = []
    for j in range(n - 1):
        tr = {}
        c = eo.verify_step(W, j, *pair_flags(opts, n, j), trace=tr)
        out.append((c, tr["count"], tr["required"]))
    return out


def census(golden_dir, with_checkpoint_cases=True):
    """The accounting of the corpus: per execution state, the longest passing checkpoint count seen (the checkpoints on its accepted
    path) and the set of ordinals within it that are the failing site of some pair — `corpus` over tests/golden/evm_*.npz alone,
    `all` with the checkpoint cases added.  Returns {state: {"path": L, "corpus": set, "all": set}}."""
    longest, sites = {}, {}
    for fn in golden_files(golden_dir):
        for _, w, opts, _ in load_cases(fn):
            states = [int(x) for x in w["steps"][:-1, 0, 0]]
            for st, (c, count, _) in zip(states, traced_status(w, opts)):
                if c == 0:
                    longest[st] = max(longest.get(st, 0), count)
                else:
                    sites.setdefault(st, set()).add(codes.site_of(c))
    out = {st: {"path": L, "corpus": {s for s in sites.get(st, ()) if 1 <= s <= L}} for st, L in longest.items()}
    for st in out:
        out[st]["all"] = set(out[st]["corpus"])
    if with_checkpoint_cases:
        bases, cases, _ = load(golden_dir)
        for c in cases:
            st = case_state(bases[c.base], c)
            s = codes.site_of(c.code)
            if st in out and 1 <= s <= out[st]["path"] and c.code:
                out[st]["all"].add(s)
    return out


def case_state(base, case):
    """the execution_state cell of the case's pair after its patches"""
    st = base.state
    for t, row, cell, v in case.patches:
        if t == "steps" and row == base.pair and cell == 0:
            st = v
    return st


def base_census(bases, cases):
    """per base: (failable, reached, unreached) ordinal sets, from the file alone"""
    reached = [set() for _ in bases]
    for c in cases:
        reached[c.base].add(codes.site_of(c.code))
    return [(set(b.failable), reached[k] & set(b.failable), set(b.unreached)) for k, b in enumerate(bases)]


def state_name(st):
    try:
        return eo.ES(st).name
    except ValueError:
        return str(st)


# Witnesses the search found that PASS, so they are no cases of the file, though they once separated the evaluators from the reference:
# a block's last EndBlock pair with one RW padding row's rw_counter overwritten so that the row equals its neighbour.  The reference's
# rw_table is a set, the equal rows count once in `max_rws = len(rw_table)`, and it accepts the pair (verify_step returns).
DUPLICATE_RW_ROW_WITNESSES = (("evm_end_block.npz", 8, 1, [("rw", 13, 0, 6)]), ("evm_end_block.npz", 12, 1, [("rw", 31, 0, 31)]))


def duplicate_rw_row_witnesses(golden_dir):
    """(wire dict, opts, pair) of DUPLICATE_RW_ROW_WITNESSES"""
    for f, case, pair, patches in DUPLICATE_RW_ROW_WITNESSES:
        _, w, opts, _ = list(load_cases(os.path.join(golden_dir, f)))[case]
        yield apply_patches(w, patches), opts, pair
