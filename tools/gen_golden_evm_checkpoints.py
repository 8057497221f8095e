#!/usr/bin/env python3
"""Write tests/golden/checkpoint_cases.npz: directed failing cases for the EVM circuit's checkpoints (tests/checkpoint_cases.py).

Runs where the reference is (staged under oracle/_ref/ by oracle/stage_ref.py, or --ref-root).  For every execution state with a
passing pair in tests/golden/evm_*.npz it takes up to four passing, unfuzzed pairs as bases (one per distinct passing checkpoint
count, longest first) and searches, with the oracle alone, for small patches that make each checkpoint 1..L of the base the first one
to fail:
* one cell overwritten — the two step rows of the pair, every row of every table of the case, the pair's aux cells — with each of
  VALUES (a row the passing path never looks up, whose old and new index key no lookup of the path asks for, cannot change the verdict
  and is not evaluated);
* the type bits of every RW / tx / block row flipped;
* two single patches of the above together, sampled, for the bases that still have unreached checkpoints;
* the execution_state cell set to values that are no ExecutionState, as curr and as next.
Per (base, failing ordinal, kind) up to two patches are kept, the second from another table where there is one.  Every kept case is
then put to the unmodified reference (wire -> reference objects as oracle/gen_golden_evm.py's fuzz variants are; verify_step on that
pair) and the exception class is recorded as `ref_kind`; a case where the oracle's kind differs is reported and fails the run.
Run: python tools/gen_golden_evm_checkpoints.py [--ref-root oracle/_ref] [--jobs N] [--out tests/golden/checkpoint_cases.npz]
"""
import argparse
import bisect
import io
import json
import os
import random
import signal
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import codes, evm_oracle as eo, wire  # noqa: E402
from tests import checkpoint_cases as cc  # noqa: E402
from tests.evm_cases import golden_files, load_cases, to_witness  # noqa: E402

P = wire.P
SEED = 20250117
MAX_BASES_PER_STATE = 4
KEEP_PER_SITE = 2
EVAL_LIMIT_S = 5


class Slow(BaseException):
    """the alarm of an evaluation that did not come back in EVAL_LIMIT_S (not an Exception: the evaluators catch those)"""


def _alarm(*_):
    raise Slow

PAIR_SAMPLES = 4000  # two-patch candidates per base that still has unreached checkpoints
VALUE_NAMES = ("old+1", "old-1", "0", "1", "256", "2^64", "2^128", "old+2^128", "P-1", "old^0x80", "old+32", "2^64-1", "2^128-1", "2^255 mod P")
MOVES = ("cell: every step cell of the pair, every cell of every table row, the pair's aux cells <- VALUES",
         "flags: rw_flags ^ 1|2|3, tx_flags ^ 1, block_flags ^ 1, every row",
         f"pairs: {PAIR_SAMPLES} sampled unions of two failing single patches, bases with unreached checkpoints only",
         "states: execution_state <- 0, last+1, 2^64, P-1, 2^32+old as curr (next <- EndTx, BeginTx, EndBlock, PUSH) and as next")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def values_for(old):
    vals = [old + 1, old - 1, 0, 1, 256, 1 << 64, 1 << 128, old + (1 << 128), P - 1, old ^ 0x80, old + 32, (1 << 64) - 1, (1 << 128) - 1, (1 << 255) % P]
    out = []
    for v in vals:
        v %= P
        if v != old and v not in out:
            out.append(v)
    return out


class RecDict(dict):
    """an index of the oracle's witness that remembers which keys the lookups asked for"""

    def __init__(self, *a):
        super().__init__(*a)
        self.asked = None

    def get(self, k, d=None):
        if self.asked is not None:
            self.asked.add(k)
        return super().get(k, d)


# table name -> (rows attribute, index attribute, key function)
INDEXED = {
    "rw": ("rw", "rw_idx", lambda r: r[0]), "bytecode": ("bytecode", "bc_idx", lambda r: r[:4]), "tx": ("tx", "tx_idx", lambda r: r[:3]),
    "block": ("block", "blk_idx", lambda r: r[:2]), "copy": ("copy", "copy_idx", lambda r: r[12]),
    "keccak": ("keccak", "keccak_idx", lambda r: (r[2], r[1])), "exp": ("exp", "exp_idx", lambda r: r[1]),
    "sig": ("sig", "sig_idx", lambda r: r), "ecc": ("ecc", "ecc_idx", lambda r: r),
}
FLAGS_OF = {"rw_flags": "rw", "tx_flags": "tx", "block_flags": "block"}


class Mutable:
    """the oracle's witness of one golden case, patched and restored in place"""

    def __init__(self, w, opts, pair):
        self.W = to_witness(w)
        self.W.steps = [list(r) for r in self.W.steps]
        self.W.aux = list(self.W.aux)
        for _, idx, _ in INDEXED.values():
            setattr(self.W, idx, RecDict(getattr(self.W, idx)))
        self.pair = pair
        self.flags = cc.pair_flags(opts, len(self.W.steps), pair)
        self.evals = 0

    def run(self, trace=None):
        self.evals += 1
        return eo.verify_step(self.W, self.pair, *self.flags, trace=trace)

    def asked(self):
        """evaluate the base with the indices recording: {table: set of keys}"""
        for _, idx, _ in INDEXED.values():
            getattr(self.W, idx).asked = set()
        tr = {}
        c = self.run(tr)
        out = {}
        for t, (_, idx, _) in INDEXED.items():
            out[t] = getattr(self.W, idx).asked
            getattr(self.W, idx).asked = None
        return c, tr, out

    def rows(self, table):
        return self.W.steps if table == "steps" else self.W.aux if table == "aux" else self.W.withdrawals if table == "withdrawals" \
            else getattr(self.W, INDEXED[table][0])

    def get(self, table, row, cell):
        return self.rows(table)[row][cell]

    def apply(self, patch):
        """returns the undo record"""
        table, row, cell, value = patch
        if table in FLAGS_OF:
            fl = getattr(self.W, table)
            old = fl[row]
            fl[row] = int(old) ^ value
            return (table, row, old)
        rows = self.rows(table)
        old = rows[row]
        if table == "steps":
            new = list(old)
            new[cell] = value
        else:
            new = old[:cell] + (value,) + old[cell + 1:]
        self._set(table, row, old, new)
        return (table, row, old)

    def undo(self, rec):
        table, row, old = rec
        if table in FLAGS_OF:
            getattr(self.W, table)[row] = old
        else:
            self._set(table, row, self.rows(table)[row], old)

    def _set(self, table, row, old, new):
        self.rows(table)[row] = new
        if table in INDEXED:
            _, idxn, key = INDEXED[table]
            idx = getattr(self.W, idxn)
            ko, kn = key(old), key(new)
            if ko != kn:
                lst = idx[ko]
                lst.remove(row)
                if not lst:
                    del idx[ko]
                bisect.insort(idx.setdefault(kn, []), row)

    def status_of(self, patches):
        """the status with the patches applied, or None where the oracle's loops over a patched value do not come back in time"""
        recs = [self.apply(p) for p in patches]
        signal.alarm(EVAL_LIMIT_S)
        try:
            c = self.run()
        except Slow:
            c = None
        finally:
            signal.alarm(0)
            for r in reversed(recs):
                self.undo(r)
        return c


def single_moves(m, asked):
    """every single patch of the move list that can change the verdict, in a fixed order"""
    W = m.W
    for row in (m.pair, m.pair + 1):
        for cell in range(13):
            for v in values_for(W.steps[row][cell]):
                yield ("steps", row, cell, v)
    for table in cc.CELL_TABLES[1:]:
        if table == "aux":
            for cell in range(len(W.aux[m.pair])):
                for v in values_for(W.aux[m.pair][cell]):
                    yield ("aux", m.pair, cell, v)
            continue
        rows = m.rows(table)
        key = INDEXED[table][2] if table in INDEXED else None
        for row, r in enumerate(rows):
            live = key is None or key(r) in asked[table]
            for cell in range(len(r)):
                for v in values_for(r[cell]):
                    if live or key(r[:cell] + (v,) + r[cell + 1:]) in asked[table]:
                        yield (table, row, cell, v)
    for table, masks in (("rw_flags", (1, 2, 3)), ("tx_flags", (1,)), ("block_flags", (1,))):
        key = INDEXED[FLAGS_OF[table]][2]
        for row, r in enumerate(m.rows(FLAGS_OF[table])):
            if key(r) in asked[FLAGS_OF[table]]:
                for mask in masks:
                    yield (table, row, 0, mask)


class Keep:
    """per status code (ordinal and kind): the first few patch sets found, in search order"""
    PER_CODE = 6

    def __init__(self):
        self.by_code = {}

    def add(self, code, patches):
        lst = self.by_code.setdefault(code, [])
        tabs = {p[0] for p in patches}
        if len(lst) < self.PER_CODE and (len(lst) < self.PER_CODE // 2 or all(tabs != {p[0] for p in q} for q in lst)):
            lst.append(patches)  # the later places are kept for candidates from other tables

    def sites(self):
        return {codes.site_of(c) for c in self.by_code}


def label(cands, w, opts, pair, code):
    """up to KEEP_PER_SITE of the candidates with the reference's exception class: the first one, then one from another table where
    there is one.  A candidate the reference does not return from within the limit (its loops run over the patched value) cannot be
    labelled and is passed over."""
    out = []
    order = list(cands)
    while order and len(out) < KEEP_PER_SITE:
        if out:
            first_tabs = {p[0] for p in out[0][0]}
            order.sort(key=lambda ps: {p[0] for p in ps} == first_tabs)  # stable: another table first
        patches = order.pop(0)
        pw = cc.apply_patches(w, patches)
        signal.alarm(EVAL_LIMIT_S)
        try:
            st = cc.traced_status(pw, opts)
            assert st[pair][0] == code and code != 0, (patches, code, st[pair][0])  # the in-place evaluation is the rebuilt witness's
            rk = ref_kind_of(pw, opts, pair)
        except Slow:
            continue
        finally:
            signal.alarm(0)
        out.append((patches, rk))
    return out


_REF = {}


def ref_kind_of(w, opts, pair):
    """the exception class of the unmodified reference for that pair of wire dict `w` (0 = verify_step returned)"""
    if not _REF:
        from oracle.gen_golden import kind_of_exception
        from oracle.gen_golden_evm import unflatten
        from zkevm_specs.evm_circuit.instruction import Instruction
        from zkevm_specs.evm_circuit.main import verify_step

        _REF.update(kind=kind_of_exception, unflatten=unflatten, Instruction=Instruction, verify_step=verify_step)
    try:
        tables, steps = _REF["unflatten"](w)
        for s, c in zip(steps, wire.rowmajor_to_rows(w["steps"])):  # unflatten makes bools of is_root / is_create: keep a cell that is neither 0 nor 1
            if c[3] > 1:
                s.is_root = c[3]
            if c[4] > 1:
                s.is_create = c[4]
        first, last = cc.pair_flags(opts, len(steps), pair)
        _REF["verify_step"](_REF["Instruction"](tables=tables, curr=steps[pair], next=steps[pair + 1], is_first_step=first, is_last_step=last))
        return 0
    except Exception as e:  # noqa: BLE001
        return _REF["kind"](e)


def search_base(args):
    """one base: (label jobs, one per status code found; passing count; ordinals reached through require; evaluations)"""
    k, fname, case_idx, pair, ref_root = args
    add_ref_path(ref_root)
    name, w, opts, _ = list(load_cases(os.path.join(GOLDEN, fname)))[case_idx]
    m = Mutable(w, opts, pair)
    c0, tr, asked = m.asked()
    assert c0 == 0, (fname, name, pair)
    L = tr["count"]
    keep = Keep()
    failing = []
    signal.signal(signal.SIGALRM, _alarm)
    for patch in single_moves(m, asked):
        c = m.status_of([patch])
        if c:
            keep.add(c, [patch])
            failing.append(patch)
    # the execution_state cell as no ExecutionState member: directed, whatever the search above kept for ordinal 0
    directed = []
    if not m.flags[1]:
        last = max(int(s) for s in eo.ES)
        for bad in (0, last + 1, 1 << 64, P - 1, (1 << 32) + m.W.steps[pair][0]):  # the last one: a member in its low word
            for nxt in (int(eo.ES.EndTx), int(eo.ES.BeginTx), int(eo.ES.EndBlock), int(eo.ES.PUSH)):
                ps = [("steps", pair, 0, bad)] + ([("steps", pair + 1, 0, nxt)] if nxt != m.W.steps[pair + 1][0] else [])
                directed.append(ps)
            directed.append([("steps", pair + 1, 0, bad)])
    failable = set(tr["required"])
    unreached = sorted(failable - keep.sites())
    if unreached and len(failing) > 1:
        rng = random.Random(SEED * 1000 + k)
        want = set(unreached)
        for _ in range(PAIR_SAMPLES):
            a, b = rng.sample(failing, 2)
            if a[:3] == b[:3]:
                continue
            c = m.status_of([a, b])
            if c and codes.site_of(c) in want:
                keep.add(c, [a, b])
    jobs = [(k, fname, case_idx, pair, ref_root, code, keep.by_code[code]) for code in sorted(keep.by_code)]
    if k % 9 == 0:  # the directed state cases ride on every ninth base (each has its own curr / next states)
        jobs += [(k, fname, case_idx, pair, ref_root, m.status_of(ps), [ps]) for ps in directed]
    return k, jobs, L, sorted(tr["required"]), m.evals


_GOLD = {}


def label_job(args):
    """one status code of one base: [(code, patches, ref_kind)] (a stage of its own: the reference takes seconds on some witnesses)"""
    k, fname, case_idx, pair, ref_root, code, cands = args
    add_ref_path(ref_root)
    signal.signal(signal.SIGALRM, _alarm)
    if _GOLD.get("name") != fname:
        _GOLD.update(name=fname, cases=list(load_cases(os.path.join(GOLDEN, fname))))
    _, w, opts, _ = _GOLD["cases"][case_idx]
    return k, [(code, patches, rk) for patches, rk in label(cands, w, opts, pair, code)]


def add_ref_path(ref_root):
    for p in (os.path.join(ROOT, "oracle", "refshim"), os.path.join(ref_root, "src")):
        if p not in sys.path:
            sys.path.insert(0, p)


def choose_bases():
    """[(file name, case index, pair, state, count)]: per state, one passing unfuzzed pair per distinct passing count, longest first"""
    by_state = {}
    for fn in golden_files(GOLDEN):
        for ci, (name, w, opts, _) in enumerate(load_cases(fn)):
            if "#fuzz" in name:
                continue
            size = sum(int(w[t].shape[0]) * int(w[t].shape[1]) for t in cc.CELL_TABLES)
            for j, (c, count, _) in enumerate(cc.traced_status(w, opts)):
                if c == 0:
                    st = int(w["steps"][j, 0, 0])
                    cand = (size, os.path.basename(fn), ci, j)
                    slot = by_state.setdefault(st, {})
                    if count not in slot or cand < slot[count]:
                        slot[count] = cand  # the smallest witness with that count: the search visits every row
    bases = []
    for st in sorted(by_state):
        for count in sorted(by_state[st], reverse=True)[:MAX_BASES_PER_STATE]:
            _, f, ci, j = by_state[st][count]
            bases.append((f, ci, j, st, count))
    return bases


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-root", default=os.path.join(ROOT, "oracle", "_ref"))
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--out", default=cc.path(GOLDEN))
    ap.add_argument("--states", default="", help="comma-separated state names: a partial run, for inspection (not the committed file)")
    a = ap.parse_args()
    add_ref_path(a.ref_root)
    import zkevm_specs  # noqa: F401  (fail early when the reference is not there)

    bases = choose_bases()
    if a.states:
        bases = [b for b in bases if eo.ES(b[3]).name in a.states.split(",")]
    print(f"{len(bases)} bases over {len({b[3] for b in bases})} states", flush=True)
    jobs = [(k, b[0], b[1], b[2], a.ref_root) for k, b in enumerate(bases)]
    import multiprocessing as mp

    with mp.Pool(a.jobs) as pool:
        found = sorted(pool.imap_unordered(search_base, jobs, chunksize=1))
        label_jobs = [j for _, js, _, _, _ in found for j in js]
        print(f"{len(label_jobs)} (base, status code) pairs to label", flush=True)
        labelled = pool.map(label_job, label_jobs, chunksize=4)  # in job order
    results = []
    for k, _, L, required, evals in found:
        out = [c for kk, cs in labelled if kk == k for c in cs]
        reached = {codes.site_of(c) for c, _, _ in out}
        failable = set(required) | {s for s in reached if 1 <= s <= L}
        results.append((k, out, L, sorted(failable), sorted(failable - reached), evals))
    arr = {k: [] for k in ("base_failable", "base_unreached", "base_unreached_tried", "case_base", "case_code", "case_ref_kind",
                           "patch_table", "patch_row", "patch_cell")}
    f_off, u_off, p_off, values, mismatches = [0], [0], [0], [], []
    for (k, out, L, failable, unreached, evals), b in zip(results, bases):
        assert L == b[4]
        arr["base_failable"] += failable
        arr["base_unreached"] += unreached
        arr["base_unreached_tried"] += [evals] * len(unreached)
        f_off.append(len(arr["base_failable"]))
        u_off.append(len(arr["base_unreached"]))
        for c, patches, rk in out:
            arr["case_base"].append(k)
            arr["case_code"].append(c)
            arr["case_ref_kind"].append(rk)
            for t, row, cell, v in patches:
                arr["patch_table"].append(cc.TABLES.index(t))
                arr["patch_row"].append(row)
                arr["patch_cell"].append(cell)
                values.append(v)
            p_off.append(len(values))
            if codes.kind_of(c) != rk:
                mismatches.append((b[:3], hex(c), rk, patches))
        print(f"{eo.ES(b[3]).name:40s} {b[0]}[{b[1]}].{b[2]} path {L:3d} failable {len(failable):3d} unreached {len(unreached):3d} cases {len(out):4d} evals {evals}", flush=True)
    files = {
        "base_file": np.array([b[0] for b in bases]), "base_case": np.array([b[1] for b in bases], dtype=np.int32),
        "base_pair": np.array([b[2] for b in bases], dtype=np.int32), "base_state": np.array([b[3] for b in bases], dtype=np.int32),
        "base_count": np.array([b[4] for b in bases], dtype=np.int32),
        "base_failable": np.array(arr["base_failable"], dtype=np.int32), "base_failable_off": np.array(f_off, dtype=np.int32),
        "base_unreached": np.array(arr["base_unreached"], dtype=np.int32), "base_unreached_off": np.array(u_off, dtype=np.int32),
        "base_unreached_tried": np.array(arr["base_unreached_tried"], dtype=np.int32),
        "case_base": np.array(arr["case_base"], dtype=np.int32), "case_code": np.array(arr["case_code"], dtype=np.uint32),
        "case_ref_kind": np.array(arr["case_ref_kind"], dtype=np.uint8), "case_patch_off": np.array(p_off, dtype=np.int32),
        "patch_table": np.array(arr["patch_table"], dtype=np.uint8), "patch_row": np.array(arr["patch_row"], dtype=np.int32),
        "patch_cell": np.array(arr["patch_cell"], dtype=np.int32),
        "patch_value": wire.ints_to_cells(values) if values else np.zeros((0, 4), dtype=np.uint64),
        "seed": np.array(SEED, dtype=np.int64), "moves": np.array(json.dumps(MOVES)), "values": np.array(json.dumps(VALUE_NAMES)),
    }
    save_npz(a.out, files)
    nf, nu = len(arr["base_failable"]), len(arr["base_unreached"])
    print(f"{len(arr['case_base'])} cases, {nf} failable checkpoints, {nu} unreached ({100.0 * nu / max(nf, 1):.1f} %) -> {os.path.getsize(a.out) // 1024} KiB")
    for mm in mismatches[:40]:
        print("ORACLE / REFERENCE KIND MISMATCH", mm)
    if mismatches:
        sys.exit(f"{len(mismatches)} cases where the oracle's kind is not the reference's: a finding, fix the oracle")


if __name__ == "__main__":
    main()
