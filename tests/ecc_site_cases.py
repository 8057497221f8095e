"""Directed ECC-circuit sites (tests/test_ecc_sites_cpu.py, tests/test_ecc_sites_gpu.py): the sheets of tests/golden/ecc_site_cases.npz
(tools/gen_golden_ecc_sites.py) and the checks both backends run over them.  Every expected value is what the plain-Python model
tests/bn254_ref.py gave when the file was generated; nothing here is computed by the code under test.

A sheet is one circuit of 131 add / mul rows (65 + 66, or 64 + 67 so that the add / mul boundary is a wavefront edge) and 67 pairing
ops that carries several target rows, each the first failure of its row at a chosen site (csrc/ecc_circuit.hpp, EccSite), the targets
standing on the slot rows below; everything else is a clean filler."""
import functools
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ecc_site_cases.npz")
KEYS = ("points", "pair_pts", "pair_off", "pair_out", "max_ok")
N_POINT, N_PAIRING = 131, 67
PAIR_SLOTS = {"op0": 0, "op63": 63, "op64": 64, "op66": 66}
PAIR_SITES = (23, 25)       # the checks made per pair: the slot of a target is then also where its offending PAIR stands
PAIR_INDEX_CLASSES = ("pair0", "pair63", "pair64", "pair_last")
ALL_SITES = tuple(range(1, 27))
A, ATTR = 1 << 24, 13 << 24
# (site, slot class) a point row cannot stand in: a mul op's qy word is 0, so a qy cell that is not zero fails the copy (site 6) first
UNREACHABLE = {(19, s) for s in ("first_mul", "row127", "row128", "row130")}


# site 20 variants whose base leaves the group law ((x, 0): the y = 0 step at once, the aff_mul_slow fallback; (0, y): order 3) with
# s = r, p - 1, r + 1 or a 190-bit scalar, and the mul slot classes each must stand in ("first_mul_row64": the first mul as row 64)
SLOW_PREFIXES = ("20/x0_", "20/order3_")
SLOW_CLASSES = ("first_mul", "first_mul_row64", "row127", "row128", "row130")


def point_slots(n_add):
    """slot class -> row, for the add / mul rows of a sheet with n_add adds"""
    return {"row0": 0, "row63": 63, "row64": 64, "last_add": n_add - 1, "first_mul": n_add, "row127": 127, "row128": 128, "row130": 130}


def slot_classes(row, n_add):
    """the slot classes row stands in (a row may stand in two: with 65 adds, row 64 is also the last add)"""
    if row < N_POINT:
        return sorted(k for k, v in point_slots(n_add).items() if v == row)
    return sorted(k for k, v in PAIR_SLOTS.items() if v == row - N_POINT)


def pair_index_class(t, n_pairs):
    return {0: "pair0", 63: "pair63", 64: "pair64"}.get(t, "pair_last" if t == n_pairs - 1 else None)


def range_cases(n=N_POINT + N_PAIRING, np_=N_POINT):
    """(lo, hi) of the ranged passes, both ends taken from {63, 64, np - 1, np, np + 1, np + 63, np + 64, n - 1, n}"""
    return [(63, np_ + 1), (64, np_ + 64), (np_ - 1, np_ + 63), (np_, n - 1), (np_ + 1, n), (np_ + 1, np_ + 64), (np_ + 63, n), (np_ + 64, n),
            (np_ + 63, np_ + 64), (n - 1, n)]


def stage1_lane(pair_off, lo, hi, t, np_=N_POINT):
    """the lane of stage 1 that judges pair t in a pass over rows [lo, hi), with the first pair of that launch, or None when the
    pass does not reach the pair"""
    k_lo, k_hi = max(lo, np_) - np_, max(hi, np_) - np_
    t_lo, t_hi = int(pair_off[k_lo]), int(pair_off[k_hi])
    return (t - t_lo, t_lo) if t_lo <= t < t_hi else None


class Sheet:
    def __init__(self, g, i, m, r):
        self.name, self.r, self.meta = m["name"], r, m
        self.w = {k: g[f"{i}_{k}"] for k in KEYS}
        self.w["n_add"], self.w["n_mul"] = m["n_add"], m["n_mul"]
        self.rows, self.assigned, self.status = g[f"{i}_rows"], g[f"{i}_assigned"], g[f"{i}_status"]
        # (row, code, variant, offending pair of the points array or -1)
        self.targets = [(t[0], t[1], t[2], t[3]) for t in m["targets"]]
        self.n = int(self.rows.shape[0])
        self.n_add = m["n_add"]


@functools.lru_cache(maxsize=None)
def load():
    g = np.load(GOLDEN)
    meta = json.loads(str(g["meta"]))
    r = int(meta["randomness"], 16)
    return meta, [Sheet(g, i, m, r) for i, m in enumerate(meta["sheets"])]


def sheets():
    return load()[1]


def sheet_ids():
    return [s.name for s in sheets()]


def tally_of(status, lo=0, hi=None):
    """(fail_count, first_fail_row, first_fail_code) of status[lo:hi], rows numbered globally"""
    hi = len(status) if hi is None else hi
    fails = [i for i in range(lo, hi) if status[i]]
    return (len(fails), fails[0], int(status[fails[0]])) if fails else (0, None, 0)


def result_tally(res):
    return (res.fail_count, res.first_fail_row, res.first_fail_code)


def check_pass(sheet, res, st, lo=0, hi=None):
    """one pass over rows [lo, hi) against the recorded statuses: in-range codes, zeros outside, rows_evaluated and the tally"""
    exp = sheet.status
    hi = sheet.n if hi is None else hi
    bad = [(i, hex(int(st[i])), hex(int(exp[i]))) for i in range(lo, hi) if st[i] != exp[i]]
    assert not bad, (sheet.name, (lo, hi), bad[:8])
    assert not st[:lo].any() and not st[hi:].any(), (sheet.name, lo, hi)
    assert res.rows_evaluated == hi - lo, (sheet.name, lo, hi)
    assert result_tally(res) == tally_of(exp.tolist(), lo, hi), (sheet.name, lo, hi)


def coverage_of(sheet_list, status_of):
    """site x slot class -> sheets, the per-pair sites' pair-index classes and the (kind, site) pairs seen, from the statuses
    `status_of(sheet)` returned: a target counts only where the returned code is the recorded one"""
    table, pairs, seen = {}, {}, set()
    for s in sheet_list:
        st = status_of(s)
        n_pairs = int(s.w["pair_off"][-1])
        for row, code, variant, t in s.targets:
            if int(st[row]) != code or not code:
                continue
            site = code & 0xFFFFFF
            seen.add((code >> 24, site))
            for cl in slot_classes(row, s.n_add):
                table.setdefault(f"{site}:{cl}", []).append(s.name)
            if site in PAIR_SITES and t >= 0 and pair_index_class(t, n_pairs):
                pairs.setdefault(f"{site}:{pair_index_class(t, n_pairs)}", []).append(s.name)
    return table, pairs, seen


def slow_path_cells(sheet_list, status_of):
    """mul slot class -> [[variant, sheet]] of the slow-path site 20 targets whose returned code is the recorded one"""
    out = {}
    for s in sheet_list:
        st = status_of(s)
        for row, code, variant, t in s.targets:
            if variant.startswith(SLOW_PREFIXES) and code and int(st[row]) == code and row >= s.n_add:
                classes = slot_classes(row, s.n_add)
                for cl in classes + (["first_mul_row64"] if row == 64 and "first_mul" in classes else []):
                    out.setdefault(cl, []).append([variant, s.name])
    return out


def required_cells():
    """every (site, slot class) the file must cover: each site in every slot class of its row kind that it can reach"""
    point_sites = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 14, 15, 16, 18, 19, 20, 21]
    pairing_sites = [1, 2, 10, 11, 12, 13, 14, 17, 21, 22, 23, 24, 25, 26]
    req = {f"{s}:{c}" for s in point_sites for c in point_slots(65) if (s, c) not in UNREACHABLE}
    req |= {f"{s}:{c}" for s in pairing_sites for c in PAIR_SLOTS}
    return req


def ranged_lane_hits(sheet_list):
    """(site, lane) of the per-pair targets' offending pairs over the ranged passes whose stage 1 starts past pair 0"""
    hits = set()
    for s in sheet_list:
        for row, code, variant, t in s.targets:
            if (code & 0xFFFFFF) in PAIR_SITES and t >= 0:
                for lo, hi in range_cases():
                    if lo <= row < hi:
                        lane = stage1_lane(s.w["pair_off"], lo, hi, t)
                        if lane and lane[1] != 0:
                            hits.add((code & 0xFFFFFF, lane[0]))
    return hits


# ---- the runs (device=None: the HIP library; "cpu": libzkevm_cpu.so) -----------------------------------------------------------------
def to_dev(x):
    import torch

    return torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x.view(np.int32) if x.dtype == np.uint32 else x).cuda()


def wire_to_dev(w):
    return {k: (to_dev(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) and k != "max_ok" else v) for k, v in w.items()}


def check_assignment(sheet, device):
    from zkevm_specs_amd import engine, oneshot

    got = oneshot.ecc_assign(sheet.w, sheet.r, device=device)
    assert np.array_equal(got, sheet.assigned), (sheet.name, np.argwhere((got != sheet.assigned).any(axis=(1, 2))).ravel()[:8])
    with engine.open_ecc_assign(sheet.w, sheet.r, device=device) as s:
        res = s.run()
        assert res.ok and res.rows_evaluated == sheet.n
        assert np.array_equal(s.rows(), sheet.assigned), sheet.name


def oneshot_status(sheet, device):
    from zkevm_specs_amd import oneshot

    res, st = oneshot.ecc_verify(sheet.w, sheet.rows, sheet.r, device=device)
    check_pass(sheet, res, st)
    return st


def open_session(sheet, device, on_device=False):
    from zkevm_specs_amd import engine

    w, rows = (wire_to_dev(sheet.w), to_dev(np.ascontiguousarray(sheet.rows))) if on_device else (sheet.w, sheet.rows)
    return engine.open_ecc(w, rows, sheet.r, device=device)


def session_status(sheet, device, on_device=False):
    with open_session(sheet, device, on_device) as s:
        res = s.run()
        st = s.read_status()
    check_pass(sheet, res, st)
    return st


def check_ranges(sheet, device, on_device=False):
    with open_session(sheet, device, on_device) as s:  # one resident session, range after range
        for lo, hi in range_cases():
            s.set_range(lo, hi)
            check_pass(sheet, s.run(), s.read_status(), lo, hi)


def check_single_rows(sheet, device, on_device=False):
    with open_session(sheet, device, on_device) as s:
        for row, code, variant, t in sheet.targets:
            s.set_range(row, row + 1)
            res = s.run()
            check_pass(sheet, res, s.read_status(), row, row + 1)
            assert result_tally(res) == ((1, row, code) if code else (0, None, 0)), (sheet.name, row, variant)


def check_range_changes(sheet, device, on_device=False):
    np_ = N_POINT
    with open_session(sheet, device, on_device) as s:
        first = s.run()
        st1 = s.read_status().copy()
        check_pass(sheet, first, st1)
        s.set_range(np_ + 63, np_ + 64)
        check_pass(sheet, s.run(), s.read_status(), np_ + 63, np_ + 64)
        s.set_range(0, sheet.n)
        third = s.run()
        st3 = s.read_status()
        assert st3.tolist() == st1.tolist() and result_tally(third) == result_tally(first) and third.rows_evaluated == first.rows_evaluated


def check_coverage(status_of):
    """the coverage table recomputed from returned statuses equals the file's, covers every required cell, and every site was a first
    failure somewhere, both AttributeError forms included"""
    meta, sh = load()
    table, pairs, seen = coverage_of(sh, status_of)
    assert {k: sorted(v) for k, v in table.items()} == {k: sorted(v) for k, v in meta["coverage"].items()}
    assert {k: sorted(v) for k, v in pairs.items()} == {k: sorted(v) for k, v in meta["pair_coverage"].items()}
    assert not required_cells() - set(table), sorted(required_cells() - set(table))
    assert {f"{s}:{c}" for s in PAIR_SITES for c in PAIR_INDEX_CLASSES} <= set(pairs)
    slow = slow_path_cells(sh, status_of)
    assert {k: sorted(v) for k, v in slow.items()} == meta["slow_path_coverage"]
    assert all(any(v.startswith("20/x0_") for v, _ in slow.get(cl, ())) for cl in SLOW_CLASSES), slow
    assert seen >= {(1, s) for s in ALL_SITES if s != 2} | {(13, 2)}
    forms = {v.split("/")[1] for s in sh for row, code, v, t in s.targets if code == (ATTR | 2) and int(status_of(s)[row]) == code}
    assert forms >= {"pairing_as_add", "pairing_as_mul", "none_as_pairing"}, forms
    n_targets = sum(1 for s in sh for t in s.targets)
    n_seen = sum(1 for s in sh for row, code, v, t in s.targets if int(status_of(s)[row]) == code)
    assert n_seen == n_targets == meta["n_targets"]  # no case skipped
    assert set(meta["variants"]) == {v for s in sh for _, _, v, _ in s.targets}
    assert {(s, l) for s in PAIR_SITES for l in (0, 63, 64)} <= ranged_lane_hits(sh)
    # the reference's own outcome of the add / mul sites: AssertionError <-> kind 1, AttributeError <-> kind 13
    kinds = {"AssertionError": 1, "AttributeError": 13}
    for v, (code, exc) in meta["ref_outcomes"].items():
        assert kinds[exc] == code >> 24, v
    assert {c & 0xFFFFFF for c, _ in meta["ref_outcomes"].values()} >= {1, 2, 3, 4, 5, 6, 7, 8, 9, 14, 15, 16, 18, 19, 20}
