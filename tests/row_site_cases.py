"""Directed failure-site cases of the Copy, Bytecode and Exp circuits (tests/golden/row_site_cases.npz, written by
tools/gen_golden_row_sites.py), after tests/state_site_cases.py.

Per circuit the file holds one valid base witness with its tables (built through the reference's own assignment and accepted by the
reference's own verification loop) and, per case, a few patches that make one numbered check of csrc/copy_circuit.hpp / row_circuits.hpp
the FIRST one to fail on one chosen row (the target).  A patch is (kind, table, row, cell, value):

    P_CELL    witness cell := value                      P_TCELL   table cell := value
    P_FLAG    witness row's type bits ^= value           P_TFLAG   table row's type bits ^= value
    P_TDUP    table row appended again with cell := value (cell NO_CELL: an identical duplicate)
    P_TEMPTY  the table has no rows at all

Rows and table rows are those of the base: the positions below move them.  Stored with every case: the oracle's code of every failing
row, the exception class the unmodified reference raises on the target row, and the line of the reference's copy_circuit.py /
bytecode_circuit.py / exp_circuit.py it raises at (first line of the innermost statement of that file in the traceback).  A case with
site 0 passes on its target: the value just inside a bound whose other side is a failing case.

Positions are made here, at test time, as (k, cut): k rows of valid filler are prepended, then the witness is rotated left by `cut` rows
(Copy, Exp: their loops are cyclic) or cut down to its first `cut` base rows (Bytecode, whose first and last rows are marked).

  Copy      a wavefront holds 64 rows and evaluates 62; rows i + 1, i + 2 come from lanes + 1, + 2.  The filler is one whole
            TxCalldata -> Memory event of k / 2 steps (k even: a row keeps its lane parity) whose RW rows go in front of the base's, with
            the rw_counters below the base's, so the dense index's base and every RW row index move.  Targets run unshifted; on lanes
            0 / 1 of the first wavefront (rotation); on lanes 60 / 61, whose successors are the read-only lanes 62 / 63; on the first
            lanes of the next wavefront; on rows 246 / 247 and 248 / 249, the last and the first rows of a 248-row block of the 256-thread
            launch shape.  Wrap-around cases (their patches lie in the two rows behind the target) also run rotated so that the target is
            the last row of the witness, with row n - 1 on lane 61 (successors: lanes 62 / 63 of the same wavefront) and on lane 1 (lanes
            2 / 3).
  Bytecode  63 evaluated rows per wavefront.  The filler is one code of k - 1 non-PUSH bytes with its keccak row.  Lane 0, lane 62 (its
            successor is the read-only lane 63), rows 251 / 252 (the edge of a 252-row block), and — cut behind a target whose successor is
            a header — row n - 1, whose successor is row 0.  Wrap-around cases patch row 0 itself (of the padded witness) and target the
            last row.
  Exp       no lane exchange: rows 255 / 256 (a block edge) and, rotated, row n - 1.  The filler is the reference's dummy padding row.

The generator checked every padded base used here against the reference and recorded them (`checked`).
"""
import ctypes
import os
from collections import namedtuple

import numpy as np

from oracle import codes, copy_oracle as co, row_oracles as ro, wire

FILE = "row_site_cases.npz"
CIRCUITS = ("copy", "bytecode", "exp")
P_CELL, P_FLAG, P_TCELL, P_TFLAG, P_TDUP, P_TEMPTY = range(6)
T_ROWS, T_RW, T_BYTECODE, T_TX, T_KECCAK = range(5)
NO_CELL = 255
TABLES = {"copy": (T_RW, T_BYTECODE, T_TX), "bytecode": (T_KECCAK,), "exp": ()}
TABLE_NAME = {T_RW: "rw", T_BYTECODE: "bytecode", T_TX: "tx", T_KECCAK: "keccak"}
TABLE_NCELLS = {T_RW: 14, T_BYTECODE: 6, T_TX: 5, T_KECCAK: 5}
TABLE_HAS_FLAGS = {T_RW: True, T_BYTECODE: False, T_TX: True, T_KECCAK: False}

ALL_SITES = {"copy": tuple(s for s in range(1, 43) if s != 33), "bytecode": tuple(range(1, 24)),
             "exp": tuple(list(range(1, 10)) + [12, 13, 15, 17, 18, 19] + list(range(22, 32)))}
# a site that stands for more than one statement of the reference: the kernel's site 22 is `lt`'s two operand asserts (addr, then src_addr_end)
SITE_N_LINES = {("copy", 22): 2}
MAX_UNREACHED = {"bytecode": 0, "copy+exp": 2}
COPY_LOOKUP_SITES = tuple(range(28, 43))
COPY_ROWS_PER_WAVE, BC_ROWS_PER_WAVE = 62, 63
COPY_BLOCK_EDGE, BC_BLOCK_EDGE, EXP_BLOCK_EDGE = 246, 251, 255  # last row of the first 256-thread block (Copy: + lane parity)
COPY_MAX_ROWS = 246
FILLER_TX_ID, FILLER_CALL_ID = 200, 77
RANGE_SPAN = 70

Case = namedtuple("Case", "site target code ref_kind ref_line wrap patches fails")
Data = namedtuple("Data", "name cols flags tabs tflags r rows trows cases site_line unreached tried shared checked seed")
Built = namedtuple("Built", "cols flags tabs tflags rows trows target affected")


def path(golden_dir):
    return os.path.join(golden_dir, FILE)


def _cell(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), dtype="<u8")


def load(golden_dir, name):
    g = np.load(path(golden_dir))
    p = name + "_"
    po, fo = g[p + "case_patch_off"], g[p + "case_fail_off"]
    values = wire.cells_to_ints(g[p + "patch_value"])
    cases = []
    for c in range(len(g[p + "case_site"])):
        patches = [(int(g[p + "patch_kind"][k]), int(g[p + "patch_table"][k]), int(g[p + "patch_row"][k]), int(g[p + "patch_cell"][k]), values[k])
                   for k in range(po[c], po[c + 1])]
        fails = [(int(g[p + "fail_row"][k]), int(g[p + "fail_code"][k])) for k in range(fo[c], fo[c + 1])]
        cases.append(Case(int(g[p + "case_site"][c]), int(g[p + "case_target"][c]), int(g[p + "case_code"][c]), int(g[p + "case_ref_kind"][c]),
                          int(g[p + "case_ref_line"][c]), bool(g[p + "case_wrap"][c]), patches, fails))
    tabs = {t: g[p + TABLE_NAME[t]] for t in TABLES[name]}
    tflags = {t: (g[p + TABLE_NAME[t] + "_flags"] if TABLE_HAS_FLAGS[t] else None) for t in TABLES[name]}
    return make_data(name, g[p + "rows"], g[p + "flags"] if name == "copy" else None, tabs, tflags, wire.cells_to_ints(g[p + "r"])[0], cases,
                     {s: tuple(ln for s2, ln in zip(g[p + "site"].tolist(), g[p + "site_line"].tolist()) if s2 == s) for s in g[p + "site"].tolist()},
                     g[p + "unreached"].tolist(),
                     [str(s) for s in g[p + "unreached_tried"]], [tuple(x) for x in g[p + "shared_lines"].tolist()],
                     set(map(tuple, g[p + "checked_variants"].tolist())), int(g["seed"]))


def make_data(name, cols, flags, tabs, tflags, r, cases=(), site_line=None, unreached=(), tried=(), shared=(), checked=(), seed=0):
    return Data(name, cols, flags, tabs, tflags, r, wire.colmajor_to_rows(cols), {t: wire.rowmajor_to_rows(a) for t, a in tabs.items()},
                list(cases), site_line or {}, list(unreached), list(tried), list(shared), set(checked), seed)


# --------------------------------------------------------------------------------------------------------------------------------
# filler and padded bases
# --------------------------------------------------------------------------------------------------------------------------------
_pad_cache = {}


def _copy_filler(data, k):
    """(rows, rw rows, tx rows) of one TxCalldata -> Memory event of k / 2 steps whose rw_counters end where the base's begin"""
    assert k % 2 == 0
    steps = k // 2
    rw0 = min(r[0] for r in data.trows[T_RW])
    tmpl = next(r for r in data.trows[T_RW] if r[1] == 1 and r[2] == 9)  # a Memory write of the base
    rows, rw, tx = [], [], []
    for i in range(steps):
        v, rwc = (7 * i + 3) & 0xFF, rw0 - steps + i
        rows.append([1, int(i == 0), 0, FILLER_TX_ID, 0, 3, i, steps, steps - i, v, 0, 0, 0, rwc, steps - i, 0, 0, 1, 0, 0])
        rows.append([0, 0, int(i == steps - 1), FILLER_CALL_ID, 0, 2, i, 0, 0, v, 0, 0, 0, rwc, steps - i, 1, 0, 0, 0, 0])
        m = list(tmpl)
        m[0], m[3], m[4], m[8] = rwc, FILLER_CALL_ID, i, v
        rw.append(m)
        tx.append([FILLER_TX_ID, 13, i, v, 0])
    return rows, rw, tx


def _bytecode_filler(data, k):
    """(rows, keccak row or None) of one code of k - 1 non-PUSH bytes; its hash cells are arbitrary (the circuit looks the triple up)"""
    ln = k - 1
    lo, hi = (ro.EMPTY_HASH_LO, ro.EMPTY_HASH_HI) if ln == 0 else (0x1111111111111111 + k, 0x2222 + k)
    rows = [[0, 0, lo, hi, 1, 0, ln, 0, 0, 0, ln, 0]]
    rlc = 0
    for j in range(ln):
        b = (3 * j + 1) % 0x5F
        rlc = (rlc * data.r + b) % wire.P
        rows.append([0, 0, lo, hi, 2, j, b, 1, 0, rlc, ln, 0])
    return rows, ([2, rlc, ln, lo, hi] if ln else None)


def padded(data, k):
    """the base with k rows of valid filler in front -> dict(cols, flags, tabs, tflags, rows, trows, shift: table -> index of base row 0)"""
    key = (data.name, data.seed, len(data.rows), k)
    if key in _pad_cache:
        return _pad_cache[key]
    tabs, tflags, trows = dict(data.tabs), dict(data.tflags), dict(data.trows)
    shift = {t: 0 for t in tabs}
    rows, flags = data.rows, data.flags
    if k:
        if data.name == "copy":
            f_rows, f_rw, f_tx = _copy_filler(data, k)
            tmpl_flag = data.tflags[T_RW][next(i for i, r in enumerate(data.trows[T_RW]) if r[1] == 1 and r[2] == 9)]
            trows[T_RW], trows[T_TX] = f_rw + data.trows[T_RW], data.trows[T_TX] + f_tx
            tflags[T_RW] = np.concatenate([np.full(len(f_rw), tmpl_flag, dtype=np.uint32), data.tflags[T_RW]])
            tflags[T_TX] = np.concatenate([data.tflags[T_TX], np.zeros(len(f_tx), dtype=np.uint32)])
            tabs[T_RW] = np.concatenate([wire.rows_to_rowmajor(f_rw, 14), data.tabs[T_RW]])
            tabs[T_TX] = np.concatenate([data.tabs[T_TX], wire.rows_to_rowmajor(f_tx, 5)])
            shift[T_RW] = len(f_rw)
            flags = np.concatenate([np.zeros(k, dtype=np.uint32), data.flags])
        elif data.name == "bytecode":
            f_rows, kec = _bytecode_filler(data, k)
            f_rows[0][ro.Q_FIRST] = 1
            if kec:
                trows[T_KECCAK] = data.trows[T_KECCAK] + [kec]
                tabs[T_KECCAK] = np.concatenate([data.tabs[T_KECCAK], wire.rows_to_rowmajor([kec], 5)])
        else:
            dummy = next(r for r in data.rows if r[ro.X_IS_STEP] == 0)
            f_rows = [list(dummy) for _ in range(k)]
        rows = f_rows + data.rows
        if data.name == "bytecode":
            rows[k] = list(rows[k])
            rows[k][ro.Q_FIRST] = 0
        cols = wire.rows_to_colmajor(rows)
    else:
        cols = data.cols
    out = dict(cols=cols, flags=flags, tabs=tabs, tflags=tflags, rows=rows, trows=trows, shift=shift, tables=None)
    if data.name == "copy":
        out["tables"] = co.CopyTables(trows[T_RW], tflags[T_RW], trows[T_BYTECODE], trows[T_TX], tflags[T_TX])
    elif data.name == "bytecode":
        out["tables"] = set(tuple(x) for x in trows[T_KECCAK])
    if len(_pad_cache) > 64:
        _pad_cache.clear()
    _pad_cache[key] = out
    return out


# --------------------------------------------------------------------------------------------------------------------------------
# positions
# --------------------------------------------------------------------------------------------------------------------------------
def _first_at_least(t, lane, per_wave):
    """smallest row >= t on `lane` of a wavefront that evaluates `per_wave` rows"""
    return t + (lane - t) % per_wave


def bytecode_cut(data, case):
    """base rows kept by the variants that make the target row n - 1, or 0: the row behind the target must be a header (row 0 is
    one) and no patch may lie behind the target"""
    t = case.target
    if case.wrap or t + 1 >= len(data.rows) or data.rows[t + 1][ro.TAG] != 1:
        return 0
    if any(kind in (P_CELL, P_FLAG) and row > t for kind, _, row, _, _ in case.patches):
        return 0
    return t + 1


def variants(data, case):
    """[(k, cut)] of a case, the unshifted (0, 0) first"""
    t, n0 = case.target, len(data.rows)
    out = [(0, 0)]
    if data.name == "copy":
        p = t % 2
        assert n0 % 2 == 0 and n0 <= COPY_MAX_ROWS
        out.append((0, t - p))                                                        # lanes 0 / 1 of the first wavefront
        out.append((_first_at_least(t, 60 + p, COPY_ROWS_PER_WAVE) - t, 0))           # lanes 60 / 61
        out.append((_first_at_least(max(t, COPY_ROWS_PER_WAVE), p, COPY_ROWS_PER_WAVE) - t, 0))  # first lanes of a later wavefront
        out += [(COPY_BLOCK_EDGE + p - t, 0), (COPY_BLOCK_EDGE + 2 + p - t, 0)]
        if case.wrap:  # the target as the last row (read rows: the last but one); then n = 0 and n = 2 modulo 62
            last = 1 if p else 2
            for k in (0, (-n0) % COPY_ROWS_PER_WAVE, (2 - n0) % COPY_ROWS_PER_WAVE):
                out.append((k, (t + k + last) % (n0 + k)))
    elif data.name == "bytecode":
        if case.wrap:  # target: the last row; on lane 62 (its successor lane is read-only) and on lane 0
            assert t == n0 - 1
            out += [((62 - t) % BC_ROWS_PER_WAVE, 0), ((-t) % BC_ROWS_PER_WAVE, 0)]
        else:
            out += [(_first_at_least(t, 0, BC_ROWS_PER_WAVE) - t, 0), (_first_at_least(t, 62, BC_ROWS_PER_WAVE) - t, 0),
                    (BC_BLOCK_EDGE - t, 0), (BC_BLOCK_EDGE + 1 - t, 0)]
            cut = bytecode_cut(data, case)
            if cut:
                out += [(0, cut), (BC_BLOCK_EDGE - t, cut)]
    else:
        out += [(EXP_BLOCK_EDGE - t, 0), (EXP_BLOCK_EDGE + 1 - t, 0), (0, (t + 1) % n0)]
    seen, uniq = set(), []
    for v in out:
        assert v[0] >= 0
        if v not in seen:
            seen.add(v)
            uniq.append(v)
    return uniq


def ranged_variant(data, case):
    """index into variants() of the one the ranged sessions run on: the target at the end of a wavefront where the case has it"""
    return min(2 if data.name != "exp" else 1, len(variants(data, case)) - 1)


# --------------------------------------------------------------------------------------------------------------------------------
# one variant
# --------------------------------------------------------------------------------------------------------------------------------
def build(data, case, k, cut):
    pb = padded(data, k)
    cols, rows = pb["cols"].copy(), list(pb["rows"])
    flags = pb["flags"].copy() if pb["flags"] is not None else None
    tabs, tflags, trows = dict(pb["tabs"]), dict(pb["tflags"]), dict(pb["trows"])
    own_t, touched, table_touched = set(), set(), False
    n = len(rows)

    def own_table(t):
        if t not in own_t:
            tabs[t], trows[t] = tabs[t].copy(), [list(x) for x in trows[t]]
            if tflags[t] is not None:
                tflags[t] = tflags[t].copy()
            own_t.add(t)

    for kind, t, row, cell, value in case.patches:
        if kind in (P_CELL, P_FLAG):
            j = 0 if (data.name == "bytecode" and case.wrap and row == 0) else row + k
            touched.add(j)
            if kind == P_FLAG:
                flags[j] ^= np.uint32(value)
            else:
                cols[cell, j] = _cell(value)
                rows[j] = list(rows[j])
                rows[j][cell] = value
            continue
        table_touched = True
        own_table(t)
        j = row + pb["shift"][t]
        if kind == P_TCELL:
            tabs[t][j, cell] = _cell(value)
            trows[t][j][cell] = value
        elif kind == P_TFLAG:
            tflags[t][j] ^= np.uint32(value)
        elif kind == P_TDUP:
            new = list(trows[t][j])
            if cell != NO_CELL:
                new[cell] = value
            trows[t].append(new)
            tabs[t] = np.concatenate([tabs[t], wire.rows_to_rowmajor([new], TABLE_NCELLS[t])])
            if tflags[t] is not None:
                tflags[t] = np.concatenate([tflags[t], tflags[t][j:j + 1]])
        else:
            tabs[t], trows[t] = np.zeros((0, TABLE_NCELLS[t], 4), dtype=np.uint64), []
            if tflags[t] is not None:
                tflags[t] = np.zeros(0, dtype=np.uint32)
    target = case.target + k
    if cut and data.name == "bytecode":
        n = cut + k
        assert all(j < n for j in touched), "patch behind the cut"
        cols, rows = np.ascontiguousarray(cols[:, :n]), rows[:n]
    elif cut:
        cols, rows = np.ascontiguousarray(np.roll(cols, -cut, axis=1)), rows[cut:] + rows[:cut]
        flags = np.roll(flags, -cut) if flags is not None else None
        target, touched = (target - cut) % n, {(j - cut) % n for j in touched}
    reach = 3 if data.name == "copy" else 2
    affected = None if table_touched else {(j - d) % n for j in touched for d in range(reach)}
    tables = pb["tables"] if not table_touched else None
    return Built(np.ascontiguousarray(cols), flags, tabs, tflags, rows, trows, target, affected), tables


def expected(data, b, tables=None):
    """oracle status of every row; b.affected: the rows whose status the patches can change (a row reads itself and the one / two rows
    behind it; a patched table can change any row), the others being rows of a passing base"""
    idx = range(len(b.rows)) if b.affected is None else b.affected
    exp = [0] * len(b.rows)
    if data.name == "copy":
        T = tables or co.CopyTables(b.trows[T_RW], b.tflags[T_RW], b.trows[T_BYTECODE], b.trows[T_TX], b.tflags[T_TX])
        for j in idx:
            exp[j] = co.check_row(b.rows, b.flags, j, T, data.r)
    elif data.name == "bytecode":
        ks = tables if tables is not None else set(tuple(x) for x in b.trows[T_KECCAK])
        for j in idx:
            exp[j] = ro.bytecode_check_row(b.rows, j, ks, data.r)
    else:
        for j in idx:
            exp[j] = ro.exp_check_row(b.rows, j)
    return exp


def base_status(data, k, cut):
    """oracle status of every row of an unpatched padded base (all zero for a valid one)"""
    b, _ = build(data, Case(0, 0, 0, 0, 0, False, [], []), k, cut)
    return expected(data, b._replace(affected=None))


# --------------------------------------------------------------------------------------------------------------------------------
# running
# --------------------------------------------------------------------------------------------------------------------------------
vp = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
u64 = ctypes.c_uint64


def _tab(b, t):
    return np.ascontiguousarray(b.tabs[t])


def sim_status(hostsim, data, b, generic=False):
    """the host logic harness (the kernels' row functions with loaded neighbours)"""
    n = len(b.rows)
    st = np.zeros(n, dtype=np.uint32)
    rc = _cell(data.r).copy()
    if data.name == "copy":
        rw, bc, tx = _tab(b, T_RW), _tab(b, T_BYTECODE), _tab(b, T_TX)
        rwf, txf = np.ascontiguousarray(b.tflags[T_RW]), np.ascontiguousarray(b.tflags[T_TX])
        fl = np.ascontiguousarray(b.flags)
        hostsim.sim_copy_verify(vp(b.cols), vp(fl), u64(n), vp(rc), vp(rw), vp(rwf), u64(rw.shape[0]), vp(bc), u64(bc.shape[0]), vp(tx), vp(txf),
                                u64(tx.shape[0]), ctypes.c_uint32(1 if generic else 0), vp(st))
    elif data.name == "bytecode":
        kt = _tab(b, T_KECCAK)
        hostsim.sim_bytecode_verify(vp(b.cols), u64(n), vp(kt), u64(kt.shape[0]), vp(rc), vp(st))
    else:
        hostsim.sim_exp_verify(vp(b.cols), u64(n), vp(st))
    return st.tolist()


def open_session(data, b, device, generic=False):
    from zkevm_specs_amd import engine

    if data.name == "copy":
        return engine.open_copy(b.cols, np.ascontiguousarray(b.flags), data.r, _tab(b, T_RW), np.ascontiguousarray(b.tflags[T_RW]), _tab(b, T_BYTECODE),
                                _tab(b, T_TX), np.ascontiguousarray(b.tflags[T_TX]), device=device, generic_index=generic)
    if data.name == "bytecode":
        return engine.open_bytecode(b.cols, _tab(b, T_KECCAK), data.r, device=device)
    return engine.open_exp(b.cols, device=device)


def oneshot_status(data, b, device):
    from zkevm_specs_amd import oneshot

    if data.name == "copy":
        return oneshot.copy_verify(b.cols, np.ascontiguousarray(b.flags), data.r, _tab(b, T_RW), np.ascontiguousarray(b.tflags[T_RW]), _tab(b, T_BYTECODE),
                                   _tab(b, T_TX), np.ascontiguousarray(b.tflags[T_TX]), device=device)
    if data.name == "bytecode":
        return oneshot.bytecode_verify(b.cols, _tab(b, T_KECCAK), data.r, device=device)
    return oneshot.exp_verify(b.cols, device=device)


def check_tally(res, exp, lo=0, hi=None):
    fails = [j for j, c in enumerate(exp) if c and lo <= j < (len(exp) if hi is None else hi)]
    assert res.fail_count == len(fails)
    if fails:
        assert res.first_fail_row == fails[0] and res.first_fail_code == exp[fails[0]]
    else:
        assert res.first_fail_row is None


def is_ambiguity_case(case):
    return case.ref_kind == codes.LOOKUP_AMBIGUOUS or any(p[0] == P_TDUP for p in case.patches)


def is_dense_edge_case(case):
    """a Copy case that drives the dense RW index's own bounds: the target's rw_counter cell patched, failing the RW lookup"""
    return case.site in (29, 40) and all(p[0] == P_CELL for p in case.patches) and any(p[3] == co.RWC for p in case.patches)


def index_modes(data, idx, case):
    """the RW-index modes a Copy case runs with (False: dense where the table allows it, True: the generic index)"""
    if data.name != "copy":
        return [False]
    if is_ambiguity_case(case):
        return [True]
    if is_dense_edge_case(case):
        return [False]
    return [False, True] if (idx % 3 == 0 or case.site in COPY_LOOKUP_SITES) else [False]


def forms(data, idx, case, vi):
    """names of the runs of variant number vi of case idx (run_slice runs exactly these; expected_variants counts them)"""
    out = ["session-generic" if g else "session" for g in index_modes(data, idx, case)]
    if idx % 4 == 0 and vi == ranged_variant(data, case):
        out.append("ranged")
    if idx % 5 == 0:
        out.append("oneshot")
    return out


def run_slice(data, device, part, n_parts, hostsim=None):
    """Runs cases [part / n_parts) of one circuit in every variant and form — through the engine on `device` (None: the GPU, "cpu": the
    host build), and through the host logic harness when `hostsim` is given — and asserts per variant: every row's status == the
    oracle's, the tally, the target's code == the stored code, its kind == the stored reference kind, its site's reference line == the
    stored line, and (unshifted variant) the failing rows == the stored ones.  Returns (cases run, runs, sites seen)."""
    n_cases = len(data.cases)
    lo_c, hi_c = part * n_cases // n_parts, (part + 1) * n_cases // n_parts
    ran = n_run = 0
    sites = set()
    for idx in range(lo_c, hi_c):
        c = data.cases[idx]
        assert codes.site_of(c.code) == c.site and (c.code != 0) == (c.site != 0)
        for vi, (k, cut) in enumerate(variants(data, c)):
            assert (k, cut) in data.checked, ("variant not checked against the reference", data.name, k, cut)
            b, tables = build(data, c, k, cut)
            exp = expected(data, b, tables)
            t, n = b.target, len(exp)
            where = (data.name, idx, c.site, k, cut)
            assert exp[t] == c.code, where + (hex(exp[t]),)
            assert codes.kind_of(exp[t]) == c.ref_kind and (c.site == 0 or c.ref_line in data.site_line[c.site]), where
            if (k, cut) == (0, 0):
                assert [(j, e) for j, e in enumerate(exp) if e] == c.fails, where
            if hostsim is not None:
                for g in index_modes(data, idx, c):
                    st = sim_status(hostsim, data, b, g)
                    assert st == exp, where + ("hostsim", g, [(j, hex(st[j]), hex(exp[j])) for j in range(n) if st[j] != exp[j]][:4])
            for form in forms(data, idx, c, vi):
                if form.startswith("session"):
                    with open_session(data, b, device, form == "session-generic") as s:
                        res = s.run()
                        st = s.read_status().tolist()
                    assert st == exp, where + (form, [(j, hex(st[j]), hex(exp[j])) for j in range(n) if st[j] != exp[j]][:4])
                    check_tally(res, exp)
                    assert res.rows_evaluated == n
                elif form == "ranged":
                    with open_session(data, b, device, index_modes(data, idx, c)[0]) as s:
                        for lo, hi in ((t, t + 1), (max(0, t + 1 - RANGE_SPAN), t + 1), (max(0, n - RANGE_SPAN), n)):
                            s.set_range(lo, hi)
                            rr = s.run()
                            sr = s.read_status().tolist()
                            assert sr[lo:hi] == exp[lo:hi], where + ("range", lo, hi)
                            assert rr.rows_evaluated == hi - lo
                            check_tally(rr, exp, lo, hi)
                else:
                    r1, st1 = oneshot_status(data, b, device)
                    assert st1.tolist() == exp, where + ("one-shot",)
                    check_tally(r1, exp)
                n_run += 1
        if c.site:
            sites.add(c.site)
        ran += 1
    return ran, n_run, sites


def expected_variants(data, part, n_parts):
    """the number of runs run_slice has to make for its slice: what the file declares, worked out without running anything"""
    n_cases = len(data.cases)
    return sum(len(forms(data, idx, data.cases[idx], vi)) for idx in range(part * n_cases // n_parts, (part + 1) * n_cases // n_parts)
               for vi in range(len(variants(data, data.cases[idx]))))


def census(data):
    """(sites with a failing case, sites without one) from the file"""
    have = sorted({c.site for c in data.cases if c.site})
    return have, sorted(set(ALL_SITES[data.name]) - set(have))


def run_all(data, device, n_parts=1):
    ran = n_run = 0
    sites = set()
    for part in range(n_parts):
        a, b, s = run_slice(data, device, part, n_parts)
        assert b == expected_variants(data, part, n_parts)
        ran, n_run, sites = ran + a, n_run + b, sites | s
    assert ran == len(data.cases) and sorted(sites) == census(data)[0]
    return ran, n_run, sorted(sites)


def child_main():
    """the Copy kernel's launch shape is chosen once per process (ZK_COPY_BLOCK): the caller starts ONE python process per shape that runs
    every Copy case and variant on the device"""
    data = load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"), "copy")
    ran, n_run, sites = run_all(data, None)
    print("copy-block %s ok %d %d %d" % (os.environ.get("ZK_COPY_BLOCK", "-"), ran, n_run, len(sites)))
