"""Directed failure-site cases of the PI circuit's rows, of its copy constraints and of the Tx / Sig units
(tests/golden/pi_sign_site_cases.npz, written by tools/gen_golden_pi_sign_sites.py), after tests/row_site_cases.py, whose patch
encoding, tally check and accounting are reused.

PI rows    one valid witness of the reference's `public_data2witness` (`pifull`, run once per backend) and the same witness cut to its
           first K rows with the cut closed (`pi`: the last row made the last byte row, the keccak-RLC chain recomputed down to row 0,
           the keccak row re-keyed); the reference accepts every row of both.  A case is a few patches (P_CELL on rows, P_TCELL /
           P_TDUP / P_TEMPTY on the keccak table T_KECCAK or the gas-cost table T_GAS) that make one numbered check of
           csrc/pi_circuit.hpp `pi_check_row` the FIRST failure of its target row; site 0: the value just inside a bound.  There is no
           lane exchange: a row reads row i + 1 through memory and the last row reads row 0, and the rows are selector-driven, so a
           rotation keeps every row's successor.  Positions: the target on rows 0, 63 / 64, 255 / 256 (the edge of a 256-thread block)
           and n - 1 (n is no multiple of 64), by rotation.
PI copy    directed entries (cell, 32 bytes, length) put into the valid list of tests/golden/pi_driver.npz at positions 0, 63, 64,
           255, 256 and n - 1.
Tx / Sig   one unit per case, flattened from reference objects that were patched and run through the reference (`verify_circuit` on a
           one-slot Witness / `Row.verify`); a few `wire:` cases hold cells no reference object can (a cell >= p) and carry the
           oracle's verdict only (ref_line 0).  The unit runs alone, with exactly the tables it was recorded with, and embedded in a
           batch of N_UNITS valid units at positions 0, 63, 64, 255, 256 and n - 1; its twelve tx-table rows move with it; the keccak
           table holds the filler's rows too.  Cases that cut the tx table short sit on unit n - 1.

Forms: a session per case and variant; every fourth case four ranged sessions ([t, t + 1); [lo, t + 1), the successor outside; [lo, t), the
target just outside; a range that ends at n); every fifth case the one-shot entry.
"""
import ctypes
import os
from collections import namedtuple

import numpy as np

from oracle import codes, pi_oracle as PO, sign_oracle as SO, wire
from tests.row_site_cases import P_CELL, P_TCELL, P_TDUP, P_TEMPTY, NO_CELL, T_KECCAK, Case, check_tally, _cell, vp, u64  # noqa: F401

FILE = "pi_sign_site_cases.npz"
P = wire.P
T_GAS = 5
PI_TABLE_NCELLS = {T_KECCAK: 5, T_GAS: 3}
PI_SITES = tuple(range(1, 29))
COPY_SITES = (1, 2)
TX_SITES = tuple(range(1, 12))
SIG_SITES = tuple(range(1, 8)) + (12, 13, 14, 15)
# the reference's loops `for cons in ...: assert cons == zero` (one statement each) stand for several sites
# site 5 is two statements: the checked Word that rpi_digest_word.select() builds, and the table's own membership assert
PI_N_LINES = {5: 2}
PI_SHARED = {(a, b) for grp in ((9, 10, 11, 12), tuple(range(14, 21))) for a in grp for b in grp if a < b}
EDGE_ROWS = (0, 63, 64, 255, 256)
N_UNITS = 321
RANGE_SPAN = 70
PI_COPY_CELL = 0xFFFFFFFF

PiData = namedtuple("PiData", "cols gas keccak circuit_len rows gas_rows keccak_rows cases site_line unreached tried checked full")
PiBuilt = namedtuple("PiBuilt", "cols gas keccak rows gas_rows keccak_rows target affected")
CopyCase = namedtuple("CopyCase", "name site code ref_kind ref_line cell data length")
Unit = namedtuple("Unit", "name site code ref_kind ref_line bytes cells meta tx_rows tx_flags keccak r")
SignData = namedtuple("SignData", "is_sig cases site_line unreached tried")


def path(golden_dir):
    return os.path.join(golden_dir, FILE)


# --------------------------------------------------------------------------------------------------------------------------------
# PI rows
# --------------------------------------------------------------------------------------------------------------------------------
def make_pi(cols, gas, keccak, circuit_len, cases=(), site_line=None, unreached=(), tried=(), checked=(), full=None):
    return PiData(cols, gas, keccak, int(circuit_len), wire.colmajor_to_rows(cols), wire.rowmajor_to_rows(gas), wire.rowmajor_to_rows(keccak),
                  list(cases), site_line or {}, list(unreached), list(tried), set(checked), full)


def _arrays(golden_dir, p=""):
    with np.load(path(golden_dir)) as z:
        return {k: z[k] for k in z.files if k.startswith(p) or k == "seed"}


def load_cases(g, p):
    po, fo = g[p + "case_patch_off"], g[p + "case_fail_off"]
    values = wire.cells_to_ints(g[p + "patch_value"])
    cases = []
    for c in range(len(g[p + "case_site"])):
        patches = [(int(g[p + "patch_kind"][k]), int(g[p + "patch_table"][k]), int(g[p + "patch_row"][k]), int(g[p + "patch_cell"][k]), values[k])
                   for k in range(po[c], po[c + 1])]
        fails = [(int(g[p + "fail_row"][k]), int(g[p + "fail_code"][k])) for k in range(fo[c], fo[c + 1])]
        cases.append(Case(int(g[p + "case_site"][c]), int(g[p + "case_target"][c]), int(g[p + "case_code"][c]), int(g[p + "case_ref_kind"][c]),
                          int(g[p + "case_ref_line"][c]), bool(g[p + "case_wrap"][c]), patches, fails))
    return cases


def _site_lines(g, p):
    return {s: tuple(ln for s2, ln in zip(g[p + "site"].tolist(), g[p + "site_line"].tolist()) if s2 == s) for s in g[p + "site"].tolist()}


def load_pi(golden_dir):
    g = _arrays(golden_dir, "pi")
    full = make_pi(g["pifull_rows"], g["pifull_gas"], g["pifull_keccak"], g["pifull_circuit_len"][0])
    return make_pi(g["pi_rows"], g["pi_gas"], g["pi_keccak"], g["pi_circuit_len"][0], load_cases(g, "pi_"), _site_lines(g, "pi_"),
                   g["pi_unreached"].tolist(), [str(s) for s in g["pi_unreached_tried"]][:len(g["pi_unreached"])], g["pi_checked_cuts"].tolist(), full)


def pi_variants(data, case):
    """rotations (`cut`) of a case, the unrotated one first: the target on rows 0, 63, 64, 255, 256 and n - 1"""
    n, t = len(data.rows), case.target
    assert n % 64 and n > 257
    out = [0]
    for pos in EDGE_ROWS + (n - 1,):
        cut = (t - pos) % n
        if cut not in out:
            out.append(cut)
    return out


def pi_build(data, case, cut):
    cols, rows = data.cols.copy(), list(data.rows)
    tabs = {T_KECCAK: data.keccak, T_GAS: data.gas}
    trows = {T_KECCAK: data.keccak_rows, T_GAS: data.gas_rows}
    touched, own, table_touched = set(), set(), False
    n = len(rows)
    for kind, t, row, cell, value in case.patches:
        if kind == P_CELL:
            touched.add(row)
            cols[cell, row] = _cell(value)
            rows[row] = list(rows[row])
            rows[row][cell] = value
            continue
        if t not in own:
            tabs[t], trows[t] = tabs[t].copy(), [list(x) for x in trows[t]]
            own.add(t)
        table_touched = True
        if kind == P_TCELL:
            tabs[t][row, cell] = _cell(value)
            trows[t][row][cell] = value
        elif kind == P_TDUP:
            new = list(trows[t][row])
            if cell != NO_CELL:
                new[cell] = value
            trows[t].append(new)
            tabs[t] = np.concatenate([tabs[t], wire.rows_to_rowmajor([new], PI_TABLE_NCELLS[t])])
        else:
            assert kind == P_TEMPTY
            tabs[t], trows[t] = np.zeros((0, PI_TABLE_NCELLS[t], 4), dtype=np.uint64), []
    target = case.target
    if cut:
        cols, rows = np.roll(cols, -cut, axis=1), rows[cut:] + rows[:cut]
        target, touched = (target - cut) % n, {(j - cut) % n for j in touched}
    affected = None if table_touched else {(j - d) % n for j in touched for d in range(2)}
    return PiBuilt(np.ascontiguousarray(cols), np.ascontiguousarray(tabs[T_GAS]), np.ascontiguousarray(tabs[T_KECCAK]), rows, trows[T_GAS],
                   trows[T_KECCAK], target, affected)


def pi_expected(data, b):
    """oracle status of every row; b.affected: the rows that read a patched cell (a row reads itself and its successor), the others
    being rows of a base that passes (checked per rotation by the tests)"""
    n = len(b.rows)
    gas, kt = set(tuple(x) for x in b.gas_rows), set(tuple(x) for x in b.keccak_rows)
    exp = [0] * n
    for j in (range(n) if b.affected is None else b.affected):
        exp[j] = PO.check_row(b.rows, j, gas, kt, data.circuit_len % P)
    return exp


def pi_base_status(data, cut):
    b = pi_build(data, Case(0, 0, 0, 0, 0, False, [], []), cut)
    return pi_expected(data, b._replace(affected=None))


def pi_sim(hostsim, data, b):
    n = len(b.rows)
    st = np.zeros(n, dtype=np.uint32)
    c255 = _cell(255).copy()
    hostsim.sim_pi_verify(vp(b.cols), u64(n), vp(b.keccak), u64(b.keccak.shape[0]), vp(b.gas), u64(b.gas.shape[0]), u64(data.circuit_len), vp(c255),
                          vp(c255), vp(st))
    return st.tolist()


def pi_ranges(t, n):
    """[t, t + 1); [lo, t + 1): the successor of the last evaluated row lies outside the range; [lo, t): ends in front of the target,
    which must not be counted; a range that ends at n"""
    out = [(t, t + 1), (max(0, t + 1 - RANGE_SPAN), t + 1), (max(0, n - RANGE_SPAN), n)]
    if t > 0:
        out.append((max(0, t - RANGE_SPAN), t))
    return out


def forms(idx):
    return ["session"] + (["ranged"] if idx % 4 == 0 else []) + (["oneshot"] if idx % 5 == 0 else [])


def _assert_status(st, exp, where):
    assert st == exp, where + ([(j, hex(st[j]), hex(exp[j])) for j in range(len(exp)) if st[j] != exp[j]][:4],)


def pi_run_slice(data, device, part, n_parts, hostsim=None):
    """cases [part / n_parts) in every rotation and form, on `device` (None: the GPU, "cpu": the host build) and, when given, through
    the host logic harness.  Per run: every row's status == the oracle's, the tally, the target's code == the stored code, its kind ==
    the reference's, its line == the stored line.  -> (cases run, runs, sites seen)"""
    from zkevm_specs_amd import engine, oneshot

    n_cases = len(data.cases)
    ran = n_run = 0
    sites = set()
    for idx in range(part * n_cases // n_parts, (part + 1) * n_cases // n_parts):
        c = data.cases[idx]
        assert codes.site_of(c.code) == c.site and (c.code != 0) == (c.site != 0)
        for vi, cut in enumerate(pi_variants(data, c)):
            assert cut in data.checked, ("rotation not checked against the reference", cut)
            b = pi_build(data, c, cut)
            exp = pi_expected(data, b)
            t, n = b.target, len(exp)
            where = ("pi", idx, c.site, cut)
            assert exp[t] == c.code, where + (hex(exp[t]),)
            assert codes.kind_of(exp[t]) == c.ref_kind and (c.site == 0 or c.ref_line in data.site_line[c.site]), where
            if cut == 0:
                assert [(j, e) for j, e in enumerate(exp) if e] == c.fails, where
            if hostsim is not None:
                _assert_status(pi_sim(hostsim, data, b), exp, where + ("hostsim",))
            for form in forms(idx):
                if form == "session":
                    with engine.open_pi(b.cols, b.keccak, b.gas, data.circuit_len, device=device) as s:
                        res = s.run()
                        _assert_status(s.read_status().tolist(), exp, where + (form,))
                    check_tally(res, exp)
                    assert res.rows_evaluated == n
                elif form == "ranged":
                    if vi != min(1, len(pi_variants(data, c)) - 1) and vi != len(pi_variants(data, c)) - 1:
                        continue  # ranged: the target on row 0 and on row n - 1
                    with engine.open_pi(b.cols, b.keccak, b.gas, data.circuit_len, device=device) as s:
                        for lo, hi in pi_ranges(t, n):
                            s.set_range(lo, hi)
                            rr = s.run()
                            assert s.read_status().tolist()[lo:hi] == exp[lo:hi], where + ("range", lo, hi)
                            assert rr.rows_evaluated == hi - lo
                            check_tally(rr, exp, lo, hi)
                else:
                    r1, st1 = oneshot.pi_verify(b.cols, b.keccak, b.gas, data.circuit_len, device=device)
                    _assert_status(st1.tolist(), exp, where + (form,))
                    check_tally(r1, exp)
                n_run += 1
        if c.site:
            sites.add(c.site)
        ran += 1
    return ran, n_run, sites


def pi_expected_runs(data, part, n_parts):
    n_cases = len(data.cases)
    total = 0
    for idx in range(part * n_cases // n_parts, (part + 1) * n_cases // n_parts):
        nv = len(pi_variants(data, data.cases[idx]))
        for f in forms(idx):
            total += len({min(1, nv - 1), nv - 1}) if f == "ranged" else nv
    return total


def pi_run_full(data, device, hostsim=None):
    """the full-length witness once: unpatched, and with the first case of every site applied where its rows exist in both"""
    from zkevm_specs_amd import engine

    full = data.full
    n = len(full.rows)
    runs = [Case(0, 0, 0, 0, 0, False, [], [])] + [next(c for c in data.cases if c.site == s and all(p[0] == P_CELL for p in c.patches))
                                                    for s in (2, 8, 16, 27)]
    for c in runs:
        b = pi_build(full, c, 0)
        exp = pi_expected(full, b._replace(affected=None))
        assert exp[c.target] == c.code and (c.code != 0 or not any(exp)), (c.site, hex(exp[c.target]))
        if hostsim is not None:
            _assert_status(pi_sim(hostsim, full, b), exp, ("pifull", c.site, "hostsim"))
        with engine.open_pi(b.cols, b.keccak, b.gas, full.circuit_len, device=device) as s:
            res = s.run()
            _assert_status(s.read_status().tolist(), exp, ("pifull", c.site))
        check_tally(res, exp)
        assert res.rows_evaluated == n
    return len(runs)


def census(cases, all_sites):
    have = sorted({c.site for c in cases if c.site})
    return have, sorted(set(all_sites) - set(have))


# --------------------------------------------------------------------------------------------------------------------------------
# PI copy constraints
# --------------------------------------------------------------------------------------------------------------------------------
_copy_base = []


def copy_base():
    """the valid constraint list of the reference's own PI test witness (tests/golden/pi_driver.npz) as the mirror lists it"""
    if not _copy_base:
        from tests import dropin_cases as D
        from zkevm_specs_amd.pi_circuit import list_copy_constraints

        w0, shape, _, _ = D.pi_witness_from_driver_fixture()
        C, pending = list_copy_constraints(w0, *shape)
        assert pending is None
        _copy_base.append(C.wire())
    return _copy_base[0]


def load_copy(golden_dir):
    g = _arrays(golden_dir, "picopy_")
    cells = wire.cells_to_ints(g["picopy_cell"])
    return [CopyCase(str(g["picopy_name"][i]), int(g["picopy_site"][i]), int(g["picopy_code"][i]), int(g["picopy_ref_kind"][i]), int(g["picopy_ref_line"][i]),
                     cells[i], g["picopy_data"][i].copy(), int(g["picopy_len"][i])) for i in range(len(cells))]


def copy_positions(n):
    return EDGE_ROWS + (n - 1,)


def copy_build(case, pos):
    cells, data, lens = (a.copy() for a in copy_base())
    cells[pos], data[pos], lens[pos] = _cell(case.cell), case.data, case.length
    return cells, data, lens


def copy_run_all(cases, device, hostsim=None):
    """every directed entry at every position through the one-shot entry (the only form the copy constraints have)"""
    from zkevm_specs_amd import oneshot

    n = len(copy_base()[2])
    assert n > 257 and not any(PO.copy_constraints_status(wire.cells_to_ints(copy_base()[0]), copy_base()[1], copy_base()[2].tolist()))
    n_run = 0
    for c in cases:
        for pos in copy_positions(n):
            cells, data, lens = copy_build(c, pos)
            exp = PO.copy_constraints_status([int.from_bytes(cells[i].tobytes(), "little") for i in range(n)], data, lens.tolist())
            assert exp[pos] == c.code and codes.kind_of(exp[pos]) == c.ref_kind and sum(1 for e in exp if e) == (1 if c.code else 0), (c.name, pos)
            if hostsim is not None:
                st = np.zeros(n, dtype=np.uint32)
                hostsim.sim_pi_copy_verify(vp(cells), vp(data), vp(lens), u64(n), vp(st))
                _assert_status(st.tolist(), exp, ("picopy", c.name, pos, "hostsim"))
            res, st = oneshot.pi_copy_verify(cells, data, lens, device=device)
            _assert_status(st.tolist(), exp, ("picopy", c.name, pos))
            check_tally(res, exp)
            n_run += 1
    return len(cases), n_run, {c.site for c in cases if c.site}


# --------------------------------------------------------------------------------------------------------------------------------
# Tx / Sig units
# --------------------------------------------------------------------------------------------------------------------------------
def load_sign(golden_dir, is_sig):
    p = "sig_" if is_sig else "tx_"
    g = _arrays(golden_dir, p)
    to, ko = g[p + "tx_off"], g[p + "keccak_off"]
    rs = wire.cells_to_ints(g[p + "r"])
    cases = [Unit(str(g[p + "name"][i]), int(g[p + "case_site"][i]), int(g[p + "code"][i]), int(g[p + "ref_kind"][i]), int(g[p + "ref_line"][i]),
                  g[p + "bytes"][i], g[p + "cells"][i], g[p + "meta"][i], g[p + "tx_rows"][to[i]:to[i + 1]], g[p + "tx_flags"][to[i]:to[i + 1]],
                  g[p + "keccak"][ko[i]:ko[i + 1]], rs[i]) for i in range(len(rs))]
    return SignData(is_sig, cases, _site_lines(g, p), g[p + "unreached"].tolist(), [str(s) for s in g[p + "unreached_tried"]][:len(g[p + "unreached"])])


def pk_rlc_model(pk_x, pk_y, r):
    """plain-Python model of csrc/sign_circuit.hpp sg_rlc64: the lazy sum of byte_k * (r^k mod p) over pk_y then pk_x
    -> (value mod p, conditional subtractions the low 256 bits need, the ninth 32-bit limb)"""
    acc, pw = 0, 1
    for b in bytes(pk_y) + bytes(pk_x):
        acc += b * pw
        pw = pw * r % P
    assert acc < 1 << 288
    return acc % P, (acc & ((1 << 256) - 1)) // P, acc >> 256


def unit_wire(c):
    return {"bytes": np.ascontiguousarray(c.bytes[None]), "cells": np.ascontiguousarray(c.cells[:, None, :]), "meta": np.ascontiguousarray(c.meta[None]),
            "keccak": np.ascontiguousarray(c.keccak), "tx_rows": np.ascontiguousarray(c.tx_rows), "tx_flags": np.ascontiguousarray(c.tx_flags)}


_filler_cache = {}


def _filler(data, r, n):
    """n valid units under randomness r: Tx — synth_tx_witness; Sig — the file's base units 1 and 2 repeated, their keccak rows re-keyed"""
    key = (data.is_sig, r, n)
    if key not in _filler_cache:
        if not data.is_sig:
            from zkevm_specs_amd.synth import synth_tx_witness

            w = synth_tx_witness(n, r, seed=4)
            w = {k: np.ascontiguousarray(w[k]) for k in ("bytes", "cells", "meta", "keccak", "tx_rows", "tx_flags")}
            # the disabled all-zero row is the target's to bring or to lack (a padding slot looks it up): no filler unit needs it
            w["keccak"] = np.ascontiguousarray(w["keccak"][w["keccak"].reshape(-1, 20).any(axis=1)])
        else:
            base = [c for c in data.cases if c.name in ("base1", "base2")]  # (every case is a patched base0: its keccak row stays its own)
            assert len(base) >= 2
            us = [base[i % len(base)] for i in range(n)]
            kec = []
            for c in base:
                bts = [bytes(c.bytes[k].tolist()) for k in range(9)]
                h = bts[6]
                kec.append([1, pk_rlc_model(bts[0], bts[1], r)[0], 64, int.from_bytes(h[:16], "little"), int.from_bytes(h[16:], "little")])
            w = {"bytes": np.stack([c.bytes for c in us]), "cells": np.ascontiguousarray(np.stack([c.cells for c in us], axis=1)),
                 "meta": np.stack([c.meta for c in us]), "keccak": wire.rows_to_rowmajor(kec, 5), "tx_rows": np.zeros((0, 5, 4), dtype=np.uint64),
                 "tx_flags": np.zeros(0, dtype=np.uint32)}
        if len(_filler_cache) > 16:
            _filler_cache.clear()
        _filler_cache[key] = w
    return _filler_cache[key]


def is_table_cut(data, c):
    return (not data.is_sig) and c.tx_rows.shape[0] != 12


def sign_positions(data, c):
    """None: the unit alone, exactly as recorded; else its index in a batch of N_UNITS"""
    return [None, N_UNITS - 1] if is_table_cut(data, c) else [None] + list(EDGE_ROWS) + [N_UNITS - 1]


def sign_build(data, c, pos):
    if pos is None:
        return unit_wire(c), 0
    f = _filler(data, c.r, N_UNITS - 1)
    ins = lambda a, x, axis=0: np.ascontiguousarray(np.concatenate([a[:pos] if axis == 0 else a[:, :pos], x, a[pos:] if axis == 0 else a[:, pos:]], axis=axis))  # noqa: E731
    w = {"bytes": ins(f["bytes"], c.bytes[None]), "cells": ins(f["cells"], c.cells[:, None, :], 1), "meta": ins(f["meta"], c.meta[None]),
         "keccak": np.ascontiguousarray(np.concatenate([c.keccak, f["keccak"]]))}
    if data.is_sig:
        w["tx_rows"], w["tx_flags"] = f["tx_rows"], f["tx_flags"]
    else:
        w["tx_rows"] = np.ascontiguousarray(np.concatenate([f["tx_rows"][:12 * pos], c.tx_rows, f["tx_rows"][12 * pos:]]))
        w["tx_flags"] = np.ascontiguousarray(np.concatenate([f["tx_flags"][:12 * pos], c.tx_flags, f["tx_flags"][12 * pos:]]))
    return w, pos


def sign_expected(data, w, r):
    return SO.verify_units(w["bytes"], w["cells"], w["meta"], wire.rowmajor_to_rows(w["keccak"]), r, int(data.is_sig), wire.rowmajor_to_rows(w["tx_rows"]),
                           w["tx_flags"])


def sign_sim(hostsim, data, w, r):
    n = w["bytes"].shape[0]
    st = np.zeros(n, dtype=np.uint32)
    rc = _cell(r).copy()
    hostsim.sim_sign_verify(vp(w["bytes"]), vp(w["cells"]), vp(w["meta"]), u64(n), vp(w["keccak"]), u64(w["keccak"].shape[0]), vp(w["tx_rows"]), vp(w["tx_flags"]),
                            u64(w["tx_rows"].shape[0]), vp(rc), ctypes.c_uint32(int(data.is_sig)), vp(st))
    return st.tolist()


def sign_ranges(t, n):
    out = [(t, t + 1), (max(0, t + 1 - RANGE_SPAN), t + 1), (max(0, n - RANGE_SPAN), n)]
    if t > 0:
        out.append((max(0, t - RANGE_SPAN), t))
    return out


def sign_run_slice(data, device, part, n_parts, hostsim=None):
    """as pi_run_slice, over the Tx (or Sig) units"""
    from zkevm_specs_amd import engine, oneshot

    n_cases = len(data.cases)
    name = "sig" if data.is_sig else "tx"
    ran = n_run = 0
    sites = set()
    for idx in range(part * n_cases // n_parts, (part + 1) * n_cases // n_parts):
        c = data.cases[idx]
        assert codes.site_of(c.code) == c.site and (c.code != 0) == (c.site != 0) and codes.kind_of(c.code) == c.ref_kind
        assert c.site == 0 or c.ref_line == 0 or c.ref_line in data.site_line[c.site], (name, c.name)
        for pos in sign_positions(data, c):
            w, t = sign_build(data, c, pos)
            exp = sign_expected(data, w, c.r)
            n = len(exp)
            where = (name, idx, c.name, pos)
            assert exp[t] == c.code, where + (hex(exp[t]),)
            assert sum(1 for e in exp if e) == (1 if c.code else 0), where
            if hostsim is not None:
                _assert_status(sign_sim(hostsim, data, w, c.r), exp, where + ("hostsim",))
            for form in forms(idx):
                if form == "session":
                    with engine.open_sign(w, c.r, data.is_sig, device=device) as s:
                        res = s.run()
                        _assert_status(s.read_status().tolist(), exp, where + (form,))
                    check_tally(res, exp)
                    assert res.rows_evaluated == n
                elif form == "ranged":
                    if pos is None:
                        continue
                    with engine.open_sign(w, c.r, data.is_sig, device=device) as s:
                        for lo, hi in sign_ranges(t, n):
                            s.set_range(lo, hi)
                            rr = s.run()
                            assert s.read_status().tolist()[lo:hi] == exp[lo:hi], where + ("range", lo, hi)
                            assert rr.rows_evaluated == hi - lo
                            check_tally(rr, exp, lo, hi)
                else:
                    r1, st1 = oneshot.sign_verify(w, c.r, data.is_sig, device=device)
                    _assert_status(st1.tolist(), exp, where + (form,))
                    check_tally(r1, exp)
                n_run += 1
        if c.site:
            sites.add(c.site)
        ran += 1
    return ran, n_run, sites


def sign_expected_runs(data, part, n_parts):
    n_cases = len(data.cases)
    total = 0
    for idx in range(part * n_cases // n_parts, (part + 1) * n_cases // n_parts):
        npos = len(sign_positions(data, data.cases[idx]))
        for f in forms(idx):
            total += npos - 1 if f == "ranged" else npos
    return total
