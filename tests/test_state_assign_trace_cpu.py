"""zk_state_assign_from_trace* on the CPU backend: the State WITNESS of compact trace records — rows, row flags, MPT rows, statuses, result
— DEFINED BY COMPOSITION: what a zk_state_assign_from_rw_open session returns over the rw / rw_flags zk_evm_witness_from_trace writes for
the same records.  Every case of tests/state_trace_cases.py and tests/state_assign_trace_cases.py is compared with that composition in the
57-cell and the compact form, the smaller ones also with the plain-Python chain (tests/trace_witness_ref.py records -> wire,
oracle.rw_state_oracle, assign_oracle), and a stand-alone sanitizer build replays the row writer's header functions."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import assign_oracle, rw_state_oracle, wire
from tests import state_assign_trace_cases as ac
from tests import state_trace_cases as sc
from tests import trace_witness_ref as ref
from tests.test_state_trace_cpu import domain_errors, error_of, retitled, verdict
from zkevm_specs_amd import _lib, engine, oneshot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "zk_state_assign_from_trace"
COMPACT_COLS = list(range(8)) + list(range(50, 57))  # the 15 columns of ZK_OPT_STATE_COMPACT among the 57


def records_of(name):
    return ac.case(name) if name in ac.ALL else sc.case(name)


def mutable(name):
    return ac.mutable(name) if name in ac.ALL else sc.mutable(name)


def expand(rec, device):
    res, w = oneshot.evm_witness_from_trace({**rec, "steps": None}, device=device)
    assert res.ok
    return w["rw"], w["rw_flags"]


@pytest.fixture(scope="module")
def expanded():
    """(name, device) -> (rw, rw_flags) of the case's records by that backend's zk_evm_witness_from_trace: computed once, never changed"""
    cache = {}

    def get(name, device="cpu"):
        if (name, device) not in cache:
            cache[name, device] = expand(records_of(name), device)
        return cache[name, device]

    return get


def composition(rw, fl, device, compact):
    """the from-RW session over the expanded rows -> (Result, status, rows, row_flags, mpt)"""
    with engine.open_state_assign_from_rw(rw, fl, device=device, compact=compact) as s:
        r = s.run()
        return (r, s.read_status(), *s.read())


def same_witness(got, want):
    r, st, rows, fl, mpt = got
    r2, st2, rows2, fl2, mpt2 = want
    assert rows.shape == rows2.shape and mpt.shape == mpt2.shape and len(st) == len(st2) == len(fl) == len(fl2) == rows.shape[1]  # n_ops, n_mpt
    assert np.array_equal(rows, rows2), [(int(c), int(j)) for c, j in zip(*np.nonzero((rows != rows2).any(axis=2)))][:5]
    assert np.array_equal(fl, fl2) and np.array_equal(mpt, mpt2)
    assert np.array_equal(st, st2), [(j, hex(st[j]), hex(st2[j])) for j in np.nonzero(st != st2)[0][:5]]
    assert verdict(r) == verdict(r2)


def check_assign(rec, rw, fl, device, with_oracle=False):
    """both forms of the one-shot against the composition on `device`; -> the 57-cell result"""
    full = None
    for compact in (False, True):
        got = oneshot.state_assign_from_trace(rec, device=device, compact=compact)
        same_witness(got, composition(rw, fl, device, compact))
        if compact:
            assert np.array_equal(got[2], full[2][COMPACT_COLS]) and all(np.array_equal(a, b) for a, b in zip(got[3:], full[3:]))
        else:
            full = got
    if with_oracle:
        w = ref.model({**rec, "steps": np.zeros((0, 13), np.uint64)})
        ops, op_flags, _ = rw_state_oracle.rw_to_state_ops(wire.rowmajor_to_rows(w["rw"]), w["rw_flags"].tolist(), strict=True)
        e_rows, e_flags, e_mpt, e_status = assign_oracle.assign(ops, op_flags)
        _, st, rows, flags, mpt = full
        assert st.tolist() == list(e_status) and flags.tolist() == list(e_flags)
        assert wire.colmajor_to_rows(rows) == e_rows and wire.rowmajor_to_rows(mpt) == e_mpt
    return full


def test_cases_are_what_they_claim():
    sc.assert_coverage()
    ac.assert_built()


@pytest.mark.parametrize("name", sc.TAME + sc.VALID + ac.ALL)
def test_witness_equals_the_composition(name, expanded):
    rec = records_of(name)
    r = check_assign(rec, *expanded(name), "cpu", len(rec["head"]) <= sc.ORACLE_MAX)[0]
    assert r.rows_evaluated == (len(rec["head"]) + 1 if name in ac.ALL else r.rows_evaluated)
    if name in sc.VALID + ac.ALL:
        assert r.ok


def test_big_table(expanded):
    check_assign(sc.case(sc.BIG), *expanded(sc.BIG), "cpu")


def failing_ops():
    """(label, records): every row is re-keyed, some ops fail in the assignment — addresses FQ(w) wider than 160 bits, Account field tags
    outside AccountFieldTag on a key's first access (the address and field-tag tables of state_trace_cases.no_witness)"""
    return [(label, rec) for label, rec in sc.no_witness() if not label.startswith("tag nibble")]


@pytest.mark.parametrize("k", range(5))
def test_failing_ops_codes_and_tally(k):
    label, rec = failing_ops()[k]
    r = check_assign(rec, *expand(rec, "cpu"), "cpu", True)[0]
    assert r.fail_count >= 1 and r.first_fail_code >> 24, label


def check_rejected_rows(device):
    """tables with rows the re-keying rejects: the result is the composition's — a tally with the RW row and its code where the backend
    counts them, the from-RW entry's refusal under this entry's name where it refuses at open"""
    for name in sc.WILD[:6]:
        rec = sc.case(name)
        rw, fl = expand(rec, device)
        for compact in (False, True):
            try:
                want = composition(rw, fl, device, compact)
            except _lib.EngineError as e:
                text = (_lib.load_cpu() if device == "cpu" else _lib.init(device)).zk_last_error().decode()  # (the failing library's own text)
                rc, got = error_of(oneshot.state_assign_from_trace, rec, device=device, compact=compact)
                assert rc == e.rc == -1 and got == retitled(text, NAME + "_open"), (name, got, text)
                continue
            got = oneshot.state_assign_from_trace(rec, device=device, compact=compact)
            same_witness(got, want)
            _, st_rw, _, _ = oneshot.state_ops_from_trace(rec, device=device)
            rejected = np.nonzero(st_rw)[0]
            if len(rejected):  # rejected RW rows count in the tally; the first failure names the RW row unless a failed op comes before it
                assert got[0].fail_count == len(rejected) + np.count_nonzero(got[1])


def test_rejected_rows():
    check_rejected_rows("cpu")
    assert any(oneshot.state_ops_from_trace(sc.case(name), device="cpu")[1].any() for name in sc.WILD[:6])


def _raw(lib, rec, entry, n_rw=None, n_pool=None, opts=0, prev=True):
    """one raw call of a from-trace assign entry -> (rc, text)"""
    p = _lib.ptr
    n = rec["head"].shape[0] if n_rw is None else n_rw
    m = rec["pool"].shape[0] if n_pool is None else n_pool
    t = _lib.ZkTrace(p(rec["head"]), p(rec["id"]), p(rec["addr"]), p(rec["val"]), p(rec["prev"]) if prev else None, p(rec["rw_counter"]),
                     int(rec["rw_base"]), n, p(rec["pool"]), m, None, 0)
    n_ops, n_mpt, res, h = ctypes.c_uint64(), ctypes.c_uint64(), _lib.ZkResult(), ctypes.c_void_p()
    if entry == "open":
        rc = lib.zk_state_assign_from_trace_open(ctypes.byref(t), None, None, None, opts, ctypes.byref(n_ops), ctypes.byref(h))
    else:
        rc = lib.zk_state_assign_from_trace(ctypes.byref(t), None, None, None, ctypes.byref(n_mpt), ctypes.byref(n_ops), opts, None, ctypes.byref(res))
    if rc == 0 and h:
        lib.zk_close(h)
    return rc, lib.zk_last_error().decode()


def check_domain_errors(lib, opts=0, to_dev=lambda rec: rec):
    for label, rec, over, code, text in domain_errors():
        rec = to_dev(rec)
        for entry in ("open", "oneshot"):
            rc, msg = _raw(lib, rec, entry, opts=opts, **over)
            assert rc == code and msg.startswith(NAME + ": ") and text in msg, (label, entry, rc, msg)


def test_domain_errors_by_code_and_text():
    lib = _lib.load_cpu()
    check_domain_errors(lib)
    r = sc.mutable("tame_65")
    r["head"][40] |= np.uint32(1 << 6)
    rc, want = error_of(oneshot.evm_witness_from_trace, {**r, "steps": None}, device="cpu")  # the trace session's text
    for call in (oneshot.state_assign_from_trace, engine.open_state_assign_from_trace):
        rc2, got = error_of(call, r, device="cpu")
        assert rc == rc2 == _lib.ERR_TRC_HEAD and got == retitled(want, NAME)
    assert _raw(lib, sc.mutable("tame_65"), "open", opts=_lib.OPT_DEVICE_PTRS)[0] != 0  # no device pointers on this backend


def check_missing_inputs(device, expanded):
    """prev null and steps absent (neither is read); garbage in prev changes nothing"""
    rec = sc.mutable("tame_253")
    want = composition(*expanded("tame_253", device or "cpu"), device, False)
    for change in ({"prev": None}, {"prev": np.full_like(rec["prev"], 0xA5A5A5A5A5A5A5A5)}, {"steps": np.zeros((0, 13), np.uint64)}):
        same_witness(oneshot.state_assign_from_trace({**rec, **change}, device=device), want)


def test_null_prev_and_absent_steps(expanded):
    check_missing_inputs("cpu", expanded)
    lib = _lib.load_cpu()
    for entry in ("open", "oneshot"):
        assert _raw(lib, sc.mutable("tame_65"), entry, prev=False)[0] == 0


def check_two_passes(device, to_dev=lambda rec: rec, zero=lambda a: a.fill(0)):
    """a second pass gives the first one's outputs, also with the caller's heads zeroed after open (the session keeps its own)"""
    for name in ("tame_1025", "block_edge"):
        for compact in (False, True):
            want = oneshot.state_assign_from_trace(records_of(name), device=device, compact=compact)
            for zero_heads in (False, True):
                rec = to_dev(mutable(name))
                with engine.open_state_assign_from_trace(rec, device=device, compact=compact) as s:
                    assert s.compact == compact and s.n == len(want[1])
                    if zero_heads:
                        zero(rec["head"])
                    for _ in range(2):
                        r = s.run()
                        assert s.n_mpt() == len(want[4])
                        same_witness((r, s.read_status(), *s.read()), want)


def test_two_passes_keep_the_heads():
    check_two_passes("cpu")


def check_rows_feed_the_state_circuit(device, names=("valid_block", "valid_directed", "tame_1025")):
    """the assigned rows handed to open_state: the State circuit's verdict over them is state_verify_from_trace's"""
    for name in names:
        rec = records_of(name)
        for compact in (False, True):
            with engine.open_state_assign_from_trace(rec, device=device, compact=compact) as a:
                assert a.run().ok
                rows, flags, mpt = a.read()
            with engine.open_state(rows, flags, mpt, device=device, compact=compact) as s:
                r = s.run()
                st = s.read_status()
            want = oneshot.state_verify_from_trace(rec, device=device)
            assert verdict(r) == verdict(want[0]) and np.array_equal(st, want[1]), (name, compact)
            assert r.ok or name not in sc.VALID


def test_rows_feed_the_state_circuit():
    check_rows_feed_the_state_circuit("cpu")


def test_sanitizer_program(tmp_path):
    """the row writer's header functions and the CPU entries under -fsanitize=address,undefined, as a stand-alone child process"""
    exe = str(tmp_path / "state_assign_trace_asan")
    src = os.path.join(ROOT, "tests", "hostsim", "state_assign_trace_asan.cpp")
    # (-O0 -g1: the program holds the whole CPU backend, whose optimised sanitizer build takes a minute and a half)
    subprocess.check_call(["g++", "-O0", "-g1", "-std=c++17", "-DZK_HOSTSIM", "-fopenmp", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",  # (the runtimes inside the program: nothing to preload)
                           "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-Wno-array-bounds", "-o", exe, src, "-ldl"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "state_assign_trace_asan: ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
