"""ECC circuit sessions on the MI355X (zk_ecc_open: range-aware point rows, one lane per (op, pair), one lane per op; zk_ecc_assign_open)
against the golden file's recorded outcomes, the unchanged one-shot zk_ecc_verify / zk_ecc_assign and the CPU backend, with host and
with device pointers; the "ecc" part of SuperCircuit."""
import ctypes

import numpy as np
import pytest

from tests import ecc_session_cases as c
from tests.ecc_cases import golden_cases
from zkevm_specs_amd import _lib, engine, oneshot

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def geometry():
    """the geometry circuit, valid and tampered, with the expected codes: the HIP one-shot's, which must be the CPU backend's"""
    w, rows = c.geometry_circuit()
    rows_t = c.geometry_tampered_rows()
    _, st_ok = oneshot.ecc_verify(w, rows, c.R_KECCAK)
    _, st_t = oneshot.ecc_verify(w, rows_t, c.R_KECCAK)
    assert st_t.tolist() == oneshot.ecc_verify(w, rows_t, c.R_KECCAK, device="cpu")[1].tolist()
    return w, rows, rows_t, st_ok, st_t


@pytest.mark.parametrize("on_device", [False, True], ids=["host_ptrs", "device_ptrs"])
def test_golden_parity_hip(on_device):
    n = 0
    for m, w, rows, assigned, status, r in golden_cases():
        res, st = c.session_run(w, rows, r, on_device=on_device)
        assert st.tolist() == status.tolist(), m["name"]
        assert c.result_tally(res) == c.tally_of(status.tolist()), m["name"]
        if not on_device:  # (once is enough: the one-shot does not depend on where the session's inputs live)
            res1, st1 = oneshot.ecc_verify(w, rows, r)
            assert st.tolist() == st1.tolist() and c.result_tally(res) == c.result_tally(res1), m["name"]
        assert res.rows_evaluated == len(status), m["name"]
        n += 1
    assert n >= 75


@pytest.mark.parametrize("on_device", [False, True], ids=["host_ptrs", "device_ptrs"])
def test_pair_lane_geometry_hip(geometry, on_device):
    w, rows, rows_t, st_ok, st_t = geometry
    assert not st_ok.any() and np.count_nonzero(st_t) >= 12
    c.check_against(*c.session_run(w, rows, c.R_KECCAK, on_device=on_device), st_ok)
    c.check_against(*c.session_run(w, rows_t, c.R_KECCAK, on_device=on_device), st_t)


def test_first_failure_order_hip():
    w, rows = c.order_circuit()
    _, st1 = oneshot.ecc_verify(w, rows, c.R_KECCAK)
    assert st1.tolist() == oneshot.ecc_verify(w, rows, c.R_KECCAK, device="cpu")[1].tolist()
    assert st1[1] >> 24 == 13 and st1[c.ORDER_NP + 4] >> 24 == 13 and len({int(x) for x in st1 if x}) >= 6
    c.check_against(*c.session_run(w, rows, c.R_KECCAK, on_device=True), st1)


def test_ranges_hip(geometry):
    w, _, rows_t, _, st_t = geometry
    wd, rd = c.wire_to_dev(w), c.to_dev(rows_t)
    with engine.open_ecc(wd, rd, c.R_KECCAK) as s:  # one resident session, range after range
        for lo, hi in c.range_cases():
            s.set_range(lo, hi)
            c.check_against(s.run(), s.read_status(), st_t, lo, hi)


def test_session_protocol_hip(geometry):
    import torch

    w, _, rows_t, _, st_t = geometry
    wd, rd = c.wire_to_dev(w), c.to_dev(rows_t)
    lo, hi = c.NP + 14, c.NP + 23
    with engine.open_ecc(wd, rd, c.R_KECCAK) as s:
        a = s.run()
        b2 = s.run()
        assert c.result_tally(a) == c.result_tally(b2) == c.tally_of(st_t.tolist())
        assert s.read_status().tolist() == st_t.tolist()
        s.set_range(lo, hi)  # only the range changes
        c.check_against(s.run(), s.read_status(), st_t, lo, hi)
        stream = torch.cuda.Stream()
        s.set_stream(stream)
        own = torch.full((c.N,), -1, dtype=torch.int32, device="cuda")
        s.launch(own)
        stream.synchronize()  # no zk_collect: the caller's buffer is final in stream order
        got = own.cpu().numpy().view(np.uint32)
        assert got[lo:hi].tolist() == st_t[lo:hi].tolist() and (got[:lo] == 0xFFFFFFFF).all() and (got[hi:] == 0xFFFFFFFF).all()
        with pytest.raises(_lib.EngineError, match="status_dev"):
            s.read_status()
        assert c.result_tally(s.collect()) == c.tally_of(st_t.tolist(), lo, hi)
        with pytest.raises(_lib.EngineError, match="bad range"):
            s.set_range(0, c.N + 1)
    lib = _lib.init()
    for name, mutate in (("rows", None), ("decreasing", lambda off: off.__setitem__(3, off[5] + 1)), ("first", lambda off: off.__setitem__(0, 1))):
        for on_device in (False, True):
            ww = dict(w, pair_off=w["pair_off"].copy())
            if mutate:
                mutate(ww["pair_off"])
            t, rows, _, n, opts, keep = engine._ecc_session_ops(c.wire_to_dev(ww) if on_device else ww, c.R_KECCAK, rows=rd if on_device else rows_t)
            h = ctypes.c_void_p()
            rc = lib.zk_ecc_open(ctypes.byref(t), None if name == "rows" else _lib.ptr(rows), opts, ctypes.byref(h))
            assert rc != 0 and not h.value and lib.zk_last_error().decode().startswith("zk_ecc_open"), (name, on_device)


@pytest.mark.parametrize("which", ["geometry", "order"])
def test_assign_session_hip(which):
    import torch

    w, _ = c.geometry_circuit() if which == "geometry" else c.order_circuit()
    exp = oneshot.ecc_assign(w, c.R_KECCAK)
    assert np.array_equal(exp, oneshot.ecc_assign(w, c.R_KECCAK, device="cpu"))
    with engine.open_ecc_assign(w, c.R_KECCAK) as s:  # host pointers, the session's own output buffer
        assert s.run().ok
        assert np.array_equal(s.rows(), exp)
    wd = c.wire_to_dev(w)
    rows_dev = torch.zeros((exp.shape[0], 13, 4), dtype=torch.int64, device="cuda")
    with engine.open_ecc_assign(wd, c.R_KECCAK, rows_dev=rows_dev) as s:  # device pointers, the caller's buffer
        assert s.run().ok
    assert np.array_equal(rows_dev.cpu().numpy().view(np.uint64), exp)
    if which == "geometry":  # the device output feeds zk_ecc_open directly and verifies clean
        with engine.open_ecc(wd, rows_dev, c.R_KECCAK) as s:
            res = s.run()
            assert res.ok and res.rows_evaluated == c.N and not s.read_status().any()


def test_super_circuit_ecc_part():
    import torch

    from zkevm_specs_amd.super_circuit import SuperCircuit, synth_super

    p = synth_super(13, seed=7)
    dev = lambda x: torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x.view(np.int32) if x.dtype == np.uint32 else x).cuda()  # noqa: E731
    with SuperCircuit(p, to_device=dev) as sc:
        sc.launch()
        base = sc.collect()
        base_rows = dict(sc.rows)
    assert "ecc" not in base[0] and base[1] == 0
    w, rows = c.order_circuit()
    exp, _ = oneshot.ecc_verify(w, rows, c.R_KECCAK)
    with SuperCircuit(dict(p, ecc=(w, rows, c.R_KECCAK)), to_device=dev) as sc:
        assert {k: v for k, v in sc.rows.items() if k != "ecc"} == base_rows and sc.rows["ecc"] == rows.shape[0]
        sc.launch()
        results, total, first = sc.collect()
    assert c.result_tally(results["ecc"]) == c.result_tally(exp)
    assert total == exp.fail_count and first == ("ecc", exp.first_fail_row, exp.first_fail_code)
    for k, r in base[0].items():  # the other circuits report what they do without the part
        assert c.result_tally(results[k]) == c.result_tally(r) and results[k].rows_evaluated == r.rows_evaluated
    # a sharded ECC range through SuperCircuit: rank 1 of 2 evaluates its shard_ecc rows and reports global rows
    from zkevm_specs_amd import distributed

    lo, hi = distributed.shard_ecc(w["n_add"], w["n_mul"], w["pair_off"], 1, 2)
    with SuperCircuit(dict(p, ecc=(w, rows, c.R_KECCAK)), to_device=dev, shard=(1, 2)) as sc:
        sc.launch()
        results, _, _ = sc.collect()
    _, st1 = oneshot.ecc_verify(w, rows, c.R_KECCAK)
    assert c.result_tally(results["ecc"]) == c.tally_of(st1.tolist(), lo, hi) and results["ecc"].rows_evaluated == hi - lo
