"""Cases of tests/test_evm_oneshot_tail_gpu.py: the one-shot entries (zk_evm_verify, zk_evm_verify_batch) with the RW key pack split
between the open's two launches (ZK_P2_RW_TAIL, include/zkevm_hip.h) and without a status array when the caller passes no buffer.
The knob is read once per process, so `child_main` runs every case of ONE setting; the parent builds what does not depend on the
setting (traces that need the device to synthesise, their oracle statuses) once and hands it over in an .npz file."""
import os
import random
import sys

import numpy as np

from tests.evm_cases import FIELDS, fuzz_wire, oracle_status

KEY_CELLS = (1, 2, 3, 4, 5)  # rw, tag, id, address, field_tag: the cells of a packed key record besides rw_counter
SEAM_PM_WHEN_OFF = 500       # setting 0 has no seam: its cases use the rows setting 500 would split at


def n_head(n_rw, pm):
    """rows phase 1 packs: the head ends on a 64-row boundary and keeps row 0 (include/zkevm_hip.h, zk_evm_verify)"""
    pm = max(0, min(int(pm), 999))
    h = (n_rw - n_rw * pm // 1000 + 63) & ~63
    return h if h < n_rw else n_rw


def plain(w):
    return {k: v for k, v in w.items() if k in FIELDS}


def check_tally(res, exp, what):
    fails = [j for j, c in enumerate(exp) if c]
    assert res.fail_count == len(fails), (what, res.fail_count, len(fails))
    if fails:
        assert (res.first_fail_row, res.first_fail_code) == (fails[0], exp[fails[0]]), what
    else:
        assert res.first_fail_row is None, what


# ---- the four ways into the one-shot path -------------------------------------------------------------------------------------
def run_host(w, flags=(False, False), opts=0):
    from zkevm_specs_amd import oneshot

    res, st = oneshot.evm_verify(w, bool(flags[0]), bool(flags[1]), opts=opts)
    return res, st.tolist()


def run_null(w, flags=(False, False)):
    from zkevm_specs_amd import engine

    call = engine.EvmOneShot(w, bool(flags[0]), bool(flags[1]))
    call()
    return call.result()


def run_dev(w, flags=(False, False)):
    import torch

    from zkevm_specs_amd import engine

    def dev(x):
        return torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x.view(np.int32)).cuda()

    wd = {k: dev(np.ascontiguousarray(v)) for k, v in w.items() if v is not None and v.size}
    buf = torch.full((w["steps"].shape[0] - 1,), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
    res = engine.evm_verify(wd, bool(flags[0]), bool(flags[1]), status_dev=buf)
    return res, buf.cpu().numpy().view(np.uint32).tolist()


def run_batch(wires, flags=None):
    from zkevm_specs_amd import engine

    b = engine.EvmBatch(wires, list(range(len(wires))), flags=flags)
    b()
    return b.results()


def every_path(w, exp, what, flags=(False, False), calls=1):
    """null / host / device status and the batch entry: the oracle's tally on each, its statuses where the path returns them"""
    for k in range(calls):
        check_tally(run_null(w, flags), exp, (what, "null", k))
        res, st = run_host(w, flags)
        assert st == exp, (what, "host", k)
        check_tally(res, exp, (what, "host", k))
    res, st = run_dev(w, flags)
    assert st == exp, (what, "device")
    check_tally(res, exp, (what, "device"))
    for r in run_batch([w, w, w], [flags] * 3):
        check_tally(r, exp, (what, "batch"))


# ---- witnesses ----------------------------------------------------------------------------------------------------------------
def synth(log_n, seed):
    from zkevm_specs_amd.synth_evm import synth_evm_trace

    return plain(synth_evm_trace(1 << log_n, seed=seed))


def damaged(w, rows_cells):
    """one key cell of each named row changed to another value that still fits its record field"""
    w = dict(w, rw=w["rw"].copy())
    for row, cell in rows_cells:
        w["rw"][row, cell, 0] ^= np.uint64(1) if cell == 1 else np.uint64(2)
    return w


def seam_rows(n_rw, h):
    """row 0, the last phase-1 row, the first tail row, a row in the middle of a tail block, the last row"""
    return sorted({0, h - 1, h, h + min(100, (n_rw - h) // 2), n_rw - 1})


def window(w, n_rw, n_steps=192):
    """the RW table cut to n_rw rows and the last n_steps steps whose rw_counter still lies in it (they look up its last rows)"""
    rwc = w["steps"][:, 1, 0].astype(np.int64)
    end = int(np.searchsorted(rwc, int(w["rw"][0, 0, 0]) + n_rw))
    lo = max(0, end - n_steps)
    return dict(w, steps=np.ascontiguousarray(w["steps"][lo : end + 1]), rw=np.ascontiguousarray(w["rw"][:n_rw]), rw_flags=np.ascontiguousarray(w["rw_flags"][:n_rw]))


def with_gap(w, lo, hi):
    """rw_counters of rows [lo, hi) moved out of the consecutive run"""
    w = dict(w, rw=w["rw"].copy())
    w["rw"][lo:hi, 0, 0] += np.uint64(1_000_000)
    return w


def shared_build(path):
    """(parent, once) the witnesses of the status-path cases and their oracle statuses"""
    from oracle import copy_assign_oracle, wire
    from zkevm_specs_amd.super_circuit import synth_super_block
    from zkevm_specs_amd.wire import rows_to_rowmajor

    out = {}
    # a tampered mixed-opcode trace with pairs the fast kernel defers: step cells wider than their record fields
    w = synth(10, 23)
    rng = random.Random(7)
    for _ in range(15):
        w = fuzz_wire(w, rng, copy=False)
    for i in (5, 300, 301, 1000):
        w["steps"][i, 7, 2] = np.uint64(1)  # pc >= 2^128
    out["tampered"] = w
    # the warm-gadget trace of tests/test_evm_gpu.py (SHA3 / CODECOPY / EXP steps against their tables), at 2^12 steps, tampered
    p = synth_super_block(17, seed=9, block_ops=400, n_steps=1 << 12)
    ce = p["copy_events"]
    table = copy_assign_oracle.assign(wire.rowmajor_to_rows(ce["events"]), ce["flags"].tolist(), ce["data"], ce["offsets"], ce["r"])[2]
    w = plain(dict(p["evm"], copy=rows_to_rowmajor(table, 14)))
    w = {k: np.array(v) for k, v in w.items() if v is not None}
    rng = random.Random(31)
    for t, n_cells in (("copy", 14), ("keccak", 5), ("exp", 11), ("rw", 10), ("steps", 12)):
        for _ in range(8):
            w[t][rng.randrange(w[t].shape[0]), rng.randrange(1, n_cells), 0] ^= np.uint64(1 << rng.randrange(8))
    out["warm"] = w
    flat = {}
    for name, w in out.items():
        exp = oracle_status(w)
        assert sum(1 for c in exp if c) >= 8, name
        flat[name + "__oracle"] = np.array(exp, dtype=np.uint32)
        for k, v in w.items():
            flat[name + "__" + k] = v
    np.savez(path, **flat)


def shared_load(path):
    g = np.load(path)
    names = sorted({k.split("__")[0] for k in g.files})
    return {n: ({k.split("__")[1]: g[k] for k in g.files if k.startswith(n + "__") and not k.endswith("__oracle")}, g[n + "__oracle"].tolist()) for n in names}


# ---- one setting ----------------------------------------------------------------------------------------------------------------
def run_setting(pm, shared_path, single_block):
    from zkevm_specs_amd import _lib

    seam_pm = pm if pm else SEAM_PM_WHEN_OFF
    n_cases = 0
    base = synth(10, 5)
    n_rw = base["rw"].shape[0]
    h = n_head(n_rw, seam_pm)
    assert 64 <= h < n_rw
    if single_block:
        assert n_rw - h <= 256, "this setting is meant to put ONE block in phase 2"
    # 1. every row packed exactly once, across the seam: the clean witness first (a stale record of it would hide the damage)
    exp0 = oracle_status(base)
    assert not any(exp0)
    res, st = run_host(base)
    assert st == exp0 and res.ok
    rows = seam_rows(n_rw, h)
    assert len(rows) == 5
    for k in range(5):
        w = damaged(base, [(r, KEY_CELLS[(j + k) % 5]) for j, r in enumerate(rows)])
        exp = oracle_status(w)
        assert any(exp), k
        res, st = run_host(w)
        assert st == exp, ("seam", k, rows)
        check_tally(res, exp, ("seam", k))
        check_tally(run_null(w), exp, ("seam null", k))
        n_cases += 1
    #    tails of 1, 255, 256 and 257 rows, and tables of one and two rows
    big = synth(12, 5)
    n_big = big["rw"].shape[0]
    for tail in (1, 255, 256, 257):
        n = next(n for n in range(n_big, 64, -1) if n - n_head(n, seam_pm) == tail)
        w = window(big, n)
        hh = n_head(n, seam_pm)
        for cut in (w, damaged(w, [(hh, 3), (n - 1, 4)]), damaged(w, [(hh - 1, 5), (hh + tail // 2, 1)])):
            exp = oracle_status(cut)
            res, st = run_host(cut)
            assert st == exp, ("tail rows", tail, n)
            check_tally(res, exp, ("tail rows", tail))
        assert any(exp)
        n_cases += 1
    for n in (1, 2):
        w = dict(base, steps=np.ascontiguousarray(base["steps"][:6]), rw=np.ascontiguousarray(base["rw"][:n]), rw_flags=np.ascontiguousarray(base["rw_flags"][:n]))
        exp = oracle_status(w)
        res, st = run_host(w)
        assert st == exp, ("n_rw", n)
        check_tally(res, exp, ("n_rw", n))
        check_tally(run_null(w), exp, ("n_rw null", n))
        n_cases += 1
    # 2. density: a gap in rw_counter in the head only, in the tail only (verified twice), in both, and on either side of the seam
    mid_tail = h + (n_rw - h) // 2
    gaps = {"head": (h // 2, h // 2 + 1), "tail": (mid_tail, mid_tail + 1), "both": (h // 2, n_rw), "seam, last head row": (h - 1, h), "seam, from the first tail row": (h, n_rw)}
    clean_between = run_null(base)
    assert clean_between.ok
    for name, (lo, hi) in gaps.items():
        w = with_gap(base, lo, hi)
        exp = oracle_status(w)
        assert any(exp), name
        for opts in (0, _lib.OPT_GENERIC_INDEX):
            res, st = run_host(w, opts=opts)
            assert st == exp, ("gap", name, opts)
            check_tally(res, exp, ("gap", name, opts))
        if name in ("tail", "seam, from the first tail row"):
            results = run_batch([w, base, w, w])
            for k in (0, 2, 3):
                check_tally(results[k], exp, ("gap batch", name, k))
            assert results[1].ok
            res, st = run_dev(w)
            assert st == exp, ("gap device status", name)
            check_tally(res, exp, ("gap device status", name))
            check_tally(run_null(w), exp, ("gap null", name))
        n_cases += 1
    # 3. rows whose key cells exceed the record widths sit in the tail: their pairs are deferred and still get the oracle's status
    w = dict(base, rw=base["rw"].copy())
    w["rw"][h + 10, 3, 1] = np.uint64(1)        # id >= 2^64
    w["rw"][n_rw - 5, 4, 2] = np.uint64(1 << 40)  # address >= 2^160
    exp = oracle_status(w)
    assert any(exp)
    res, st = run_host(w)
    assert st == exp, "wide key cells"
    check_tally(res, exp, "wide key cells")
    check_tally(run_null(w), exp, "wide key cells, null")
    n_cases += 1
    # 4. + 5. status paths, three calls in a row
    for name, (w, exp) in shared_load(shared_path).items():
        every_path(w, exp, name, calls=3)
        n_cases += 1
    return n_cases


def child_main():
    pm, shared_path, single_block = int(os.environ["ZK_P2_RW_TAIL"]), sys.argv[1], sys.argv[2] == "1"
    n = run_setting(pm, shared_path, single_block)
    print("oneshot tail ok %d %d" % (pm, n))
