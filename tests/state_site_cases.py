"""Directed failure-site cases of the State circuit (tests/golden/state_site_cases.npz, written by tools/gen_golden_state_sites.py).

The file holds one valid base witness (every tag 1..11, a few hundred rows, assigned by the reference's assign_state_circuit) and, per
case, a few patches — one 32-byte cell of a witness row overwritten, a row's type bits xored, or one cell of the MPT table overwritten —
that make one numbered check of csrc/state_circuit.hpp the FIRST one to fail on one chosen row (the target).  Stored with every case:
the oracle's code of every failing row, the exception class the unmodified reference raises on the target row, and the line of the
reference's state_circuit.py it raises at (`ref_line`: low 16 bits the first line of the innermost statement of that file in the traceback,
high 16 bits the same for the innermost check_* function — where a shared helper such as assert_in_range was called from), so the site
half of a status word is pinned to the reference too and not only to the oracle's numbering.

Positions are made here, at test time: a case is shifted by prepending k Start rows (the reference's own padding: StartOp rows with
rw_counter 1, 2, ...), which moves its target to the first / last lane of a 63-row wavefront, the first / last row of a 252-row block,
slots 1 / 15 of the lane-group kernel's 15-row tiling, and — with the base truncated behind the target — to row n - 1, whose next row
is row 0.  The generator checked every (truncation, k) used here against the reference and recorded them.
"""
import os
from collections import namedtuple

import numpy as np

from oracle import codes, state_oracle as so, wire

FILE = "state_site_cases.npz"
PATCH_CELL, PATCH_FLAGS, PATCH_MPT = 0, 1, 2  # (kind, row, cell, value): a witness cell := value, flags[row] ^= value, an MPT cell := value
EXCLUDED = 0xFFFFFFFF                          # compact_code of a case that has no 15-cell form

# all numbered failure sites of state_check_loaded and the row loaders
ALL_SITES = tuple(list(range(1, 14)) + list(range(20, 32)) + list(range(40, 52)) + list(range(60, 67)) + [70, 71, 73] +
                  list(range(80, 87)) + [90, 91, 92, 93, 94, 95, 97] + list(range(100, 106)) + list(range(110, 117)) +
                  list(range(120, 126)) + list(range(130, 134)) + list(range(140, 153)) + [160])

# where a shifted target lands: 251 = last lane of a wavefront and last row of a 252-row block; 252 = first evaluated lane and first row
# of a block; 314 = last lane of a wavefront (314 % 63 == 62) and slot 15 of the 15-row tiling (314 % 15 == 14); 315 = first evaluated
# lane (315 % 63 == 0) and slot 1 (315 % 15 == 0)
POSITIONS = (251, 252, 314, 315)
LAST_ROW_POSITION = 314  # truncated variants: the target is row n - 1 = 314
MAX_TARGET = 251

Case = namedtuple("Case", "site target code ref_kind ref_line fixed compact_code patches fails")
Data = namedtuple("Data", "cols flags mpt rows mpt_rows cases site_line unreached tried shared checked seed n_start")


def path(golden_dir):
    return os.path.join(golden_dir, FILE)


def load(golden_dir):
    g = np.load(path(golden_dir))
    po, fo = g["case_patch_off"], g["case_fail_off"]
    values = wire.cells_to_ints(g["patch_value"])
    cases = []
    for c in range(len(g["case_site"])):
        patches = [(int(g["patch_kind"][k]), int(g["patch_row"][k]), int(g["patch_cell"][k]), values[k]) for k in range(po[c], po[c + 1])]
        fails = [(int(g["fail_row"][k]), int(g["fail_code"][k])) for k in range(fo[c], fo[c + 1])]
        cases.append(Case(int(g["case_site"][c]), int(g["case_target"][c]), int(g["case_code"][c]), int(g["case_ref_kind"][c]),
                          int(g["case_ref_line"][c]), bool(g["case_fixed"][c]), int(g["case_compact_code"][c]), patches, fails))
    cols, flags, mpt = g["base_rows"], g["base_flags"], g["base_mpt"]
    rows = wire.colmajor_to_rows(cols)
    return Data(cols, flags, mpt, rows, wire.rowmajor_to_rows(mpt), cases,
                dict(zip(g["site"].tolist(), g["site_line"].tolist())), g["unreached"].tolist(), [str(s) for s in g["unreached_tried"]],
                [tuple(p) for p in g["shared_lines"].tolist()], set(map(tuple, g["checked_variants"].tolist())), int(g["seed"]),
                n_start(rows))


def n_start(rows):
    """number of leading Start rows of the base"""
    k = 0
    while k < len(rows) and rows[k][so.TAG] == 1:
        k += 1
    return k


def group_end(rows, t):
    """index behind the last row that has row t's keys"""
    e = t + 1
    while e < len(rows) and rows[e][so.TAG:so.KEY_HI + 1] == rows[t][so.TAG:so.KEY_HI + 1]:
        e += 1
    return e


def truncation(rows, case):
    """rows kept by the variants that make the target row n - 1, or 0 when the case has none: the target must be the last row of its key
    group (then the group's end is the row behind it), no Start row, not already the last row, and no patch may lie behind it"""
    t = case.target
    if case.fixed or rows[t][so.TAG] == 1 or t + 1 >= len(rows) or group_end(rows, t) != t + 1:
        return 0
    if any(kind != PATCH_MPT and row > t for kind, row, _, _ in case.patches):
        return 0
    return t + 1


def variants(rows, case):
    """[(truncation or 0, k)] of a case; a `fixed` case targets row 0 of the unshifted base (its previous row is row n - 1) and has one"""
    if case.fixed:
        return [(0, 0)]
    out = [(0, 0)] + [(0, p - case.target) for p in POSITIONS]
    tr = truncation(rows, case)
    if tr:
        out += [(tr, 0), (tr, LAST_ROW_POSITION - case.target)]
    return out


def _cell(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), dtype="<u8")


def padded(data, trunc, k):
    """(cols, flags, int rows) of the base cut to `trunc` rows (0: all) with k Start rows in front: Start rows count 1, 2, ... in
    rw_counter and all but row 0 carry the lexicographic selector, as the reference's own StartOp padding does"""
    n0 = trunc or len(data.rows)
    cols = np.zeros((so.NCELLS, n0 + k, 4), dtype=np.uint64)
    cols[:, k:] = data.cols[:, :n0]
    cols[:, :k] = data.cols[:, :1]
    flags = np.concatenate([np.zeros(k, dtype=np.uint32), data.flags[:n0]])
    rows = [data.rows[0]] * k + data.rows[:n0]
    for j in range(k + data.n_start):
        r = list(rows[j])
        r[so.RWC], r[so.LEX] = j + 1, 1 if j else 0
        rows[j] = r
        cols[so.RWC, j], cols[so.LEX, j] = _cell(r[so.RWC]), _cell(r[so.LEX])
    return cols, flags, rows


def derive_decompositions(r):
    """the row with its limb / byte cells replaced by what the 15-cell form derives: the address's low 160 bits, the key halves' low 128"""
    r = list(r)
    for j in range(10):
        r[so.LIMB0 + j] = (r[so.ADDR] >> (16 * j)) & 0xFFFF
    for j in range(16):
        r[so.BYTE0 + j] = (r[so.KEY_LO] >> (8 * j)) & 0xFF
        r[so.BYTE0 + 16 + j] = (r[so.KEY_HI] >> (8 * j)) & 0xFF
    return r


def touches_dropped(case):
    return any(kind == PATCH_CELL and 8 <= cell < 50 for kind, _, cell, _ in case.patches)


def build(data, case, trunc, k, compact=False):
    """-> (cols, flags, mpt, int rows, int mpt rows, target row, rows whose status the patches can change) of one variant.  `compact`:
    the int rows are the 57-cell rows the 15-cell form stands for (decompositions derived from the patched cells)."""
    cols, flags, rows = padded(data, trunc, k)
    mpt, mpt_rows = data.mpt, data.mpt_rows
    n = len(rows)
    touched, own, mpt_patched = set(), set(), False
    for kind, row, cell, value in case.patches:
        if kind == PATCH_MPT:
            if not mpt_patched:
                mpt, mpt_rows, mpt_patched = mpt.copy(), [list(m) for m in mpt_rows], True
            mpt[row, cell] = _cell(value)
            mpt_rows[row][cell] = value
            continue
        j = row + k
        assert j < n, "patch behind the truncation"
        touched.add(j)
        if kind == PATCH_FLAGS:
            flags[j] ^= np.uint32(value)
        else:
            cols[cell, j] = _cell(value)
            if j not in own:
                rows[j] = list(rows[j])
                own.add(j)
            rows[j][cell] = value
    if compact:
        for j in touched:
            rows[j] = derive_decompositions(rows[j])
    affected = {(j + d) % n for j in touched for d in (-1, 0, 1)}
    if mpt_patched:
        affected |= {j for j in range(n) if rows[j][so.TAG] in (4, 6)}
    return cols, flags, mpt, rows, mpt_rows, case.target + k, affected


def expected(rows, flags, mpt_rows, affected=None):
    """oracle status of every row; with `affected`, of a witness whose other rows are those of a passing base: a row's status reads
    rows i - 1, i, i + 1, the type bits of i - 1 and i, and the MPT table, nothing else (oracle/state_oracle.py _check)"""
    if affected is None:
        return so.verify_rows(rows, flags, mpt_rows)
    mpt_set = set(tuple(m) for m in mpt_rows)
    exp = [0] * len(rows)
    for j in affected:
        exp[j] = so.check_row(rows, flags, j, mpt_set)
    return exp


def compact_cols(cols):
    return np.ascontiguousarray(np.concatenate([cols[:8], cols[50:]]))


def check_tally(res, exp, lo=0, hi=None):  # as tests/test_state_gpu.py
    fails = [j for j, c in enumerate(exp) if c and lo <= j < (len(exp) if hi is None else hi)]
    assert res.fail_count == len(fails)
    if fails:
        assert res.first_fail_row == fails[0] and res.first_fail_code == exp[fails[0]]
    else:
        assert res.first_fail_row is None


# Sites none of whose cases has a 15-cell form.  4, 6 and 9 do not exist there; the others are "an unused address / key is zero" and
# address-range checks whose cases set the cell together with matching limbs / bytes (alone, the cell fails 5 / 7 first in the 57-cell
# form).  The 15-cell kernel still meets those checks: through the site-5 / site-7 cases that patch the cell alone, which it reads as a
# consistent row (COMPACT_REREAD of them: compact_code != code, no reference record behind that reading; none of them passes).
COMPACT_ABSENT = (4, 6, 9, 23, 41, 46, 61, 63, 64, 81, 92, 100, 102, 111, 141)
COMPACT_REREAD = 2
FORMS = ("full", "compact")
RANGE_SPAN = 70  # rows of a ranged session: more than one wavefront


def census(data):
    """(sites with a case, sites without one) from the file"""
    have = sorted({c.site for c in data.cases})
    return have, sorted(set(ALL_SITES) - set(have))


def compact_excluded(data):
    """indices of the cases that have no 15-cell form: a patch overwrites one of the dropped limb / byte columns 8..49 (sites 4, 6 and 9
    do not exist there; 5 and 7 have cases that patch the address / key cell itself, which do run)"""
    return [k for k, c in enumerate(data.cases) if touches_dropped(c)]


def run_slice(data, device, part, n_parts, form="full"):
    """Runs cases [part / n_parts) of the file in every variant through one form — "full": the 57-cell session, every fifth case also the
    one-shot entry, every fourth also as ranged sessions with the target at `lo` and at `hi - 1`; "compact": the 15-cell session — and
    asserts per variant: every row's status == the oracle's, the tally, the target's code == the stored code, its kind == the stored
    reference kind, its site's reference line == the stored line, and (untruncated variants) the failing rows == the stored ones.
    Returns (cases run, variants run, sites seen, cases excluded)."""
    from zkevm_specs_amd import engine, oneshot

    n_cases = len(data.cases)
    lo_c, hi_c = part * n_cases // n_parts, (part + 1) * n_cases // n_parts
    ran = n_var = excluded = 0
    sites = set()
    compact = form == "compact"
    for idx in range(lo_c, hi_c):
        c = data.cases[idx]
        if compact and touches_dropped(c):
            assert c.compact_code == EXCLUDED
            excluded += 1
            continue
        want = c.compact_code if compact else c.code
        assert want != EXCLUDED and (compact or (want != 0 and codes.site_of(want) == c.site))  # (a patched address / key may pass in the 15-cell form)
        vs = variants(data.rows, c)
        ranged_at = vs[min(1, len(vs) - 1)]  # the first shifted variant (target at the end of a block), or the only one
        for trunc, k in vs:
            assert (trunc, k) in data.checked, ("variant not checked against the reference", trunc, k)
            cols, flags, mpt, rows, mpt_rows, t, affected = build(data, c, trunc, k, compact)
            exp = expected(rows, flags, mpt_rows, affected)
            where = (idx, c.site, trunc, k, form)
            assert exp[t] == want, where + (hex(exp[t]),)
            if not trunc and not compact:
                assert [(j, e) for j, e in enumerate(exp) if e] == [(r + k, e) for r, e in c.fails], where
            with engine.open_state(compact_cols(cols) if compact else cols, flags, mpt, device=device, compact=compact) as s:
                res = s.run()
                st = s.read_status().tolist()
                assert st == exp, where + ([(j, hex(st[j]), hex(exp[j])) for j in range(len(exp)) if st[j] != exp[j]][:4],)
                check_tally(res, exp)
                assert res.rows_evaluated == len(exp)
                if want == c.code:  # (a compact case whose address / key patch reads differently there has no reference record)
                    assert codes.kind_of(st[t]) == c.ref_kind and data.site_line[codes.site_of(st[t])] == c.ref_line, where
                if not compact and idx % 4 == 0 and (trunc, k) == ranged_at:
                    n = len(exp)
                    for lo, hi in ((t, min(n, t + RANGE_SPAN)), (max(0, t + 1 - RANGE_SPAN), t + 1)):
                        s.set_range(lo, hi)
                        rr = s.run()
                        sr = s.read_status().tolist()
                        assert sr[lo:hi] == exp[lo:hi], where + ("range", lo, hi)
                        assert rr.rows_evaluated == hi - lo
                        check_tally(rr, exp, lo, hi)
                        n_var += 1
            if not compact and idx % 5 == 0:
                r1, st1 = oneshot.state_verify(cols, flags, mpt, device=device)
                assert st1.tolist() == exp, where + ("one-shot",)
                check_tally(r1, exp)
                n_var += 1
            n_var += 1
        sites.add(c.site)
        ran += 1
    return ran, n_var, sites, excluded


def expected_variants(data, part, n_parts, form="full"):
    """the number of variants run_slice has to run for its slice: what the file declares, worked out without running anything"""
    n_cases = len(data.cases)
    total = 0
    for idx in range(part * n_cases // n_parts, (part + 1) * n_cases // n_parts):
        c = data.cases[idx]
        if form == "compact":
            total += 0 if touches_dropped(c) else len(variants(data.rows, c))
        else:
            total += len(variants(data.rows, c)) * (2 if idx % 5 == 0 else 1) + (2 if idx % 4 == 0 else 0)
    return total


def run_all(data, device, form="full", n_parts=1):
    """every slice; asserts the guards: cases run == cases in the file (less the compact exclusions), variants run == variants declared,
    sites exercised == the file's census"""
    ran = n_var = excl = 0
    sites = set()
    for part in range(n_parts):
        a, b, s, e = run_slice(data, device, part, n_parts, form)
        assert b == expected_variants(data, part, n_parts, form)
        ran, n_var, excl, sites = ran + a, n_var + b, excl + e, sites | s
    assert excl == (len(compact_excluded(data)) if form == "compact" else 0)
    assert ran == len(data.cases) - excl
    assert sorted(sites) == sorted(set(census(data)[0]) - set(COMPACT_ABSENT if form == "compact" else ()))
    return ran, n_var, sorted(sites), excl


def child_main():
    """the lane-group kernel: the caller starts ONE python process with ZK_STATE_DMA=0 that runs every case through the 57-cell session"""
    golden_dir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    data = load(golden_dir)
    ran, n_var, sites, _ = run_all(data, None, "full", 1)
    print("lane-group ok %d %d %d" % (ran, n_var, len(sites)))
