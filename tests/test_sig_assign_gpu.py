"""Sig circuit witness assignment on the MI355X (k_sig_assign.hip): the reference's fixtures, every lane form of the key recovery at
wavefront and block edges, the set builders across their 256-row tile, chunked launches against the CPU backend, and signed data ->
zk_sig_assign_open (HBM) -> ECDSA pass -> zk_sign_open without a read-back in between."""
import numpy as np
import pytest

from tests import sig_assign_cases as C
from tests.test_sig_assign_cpu import directed, ecrecover_fixtures, sig_fixtures
from zkevm_specs_amd import engine, oneshot

pytestmark = pytest.mark.gpu
R = 0x0BADC0FFEE0DDF00D


def test_reference_sig_fixtures_hip():
    sig_fixtures(None)


def test_reference_ecrecover_fixtures_hip():
    ecrecover_fixtures(None)


def test_directed_batch_matches_model_hip():
    directed(None, 27)


@pytest.mark.parametrize("lanes", ["1", "2", "4"])
def test_lane_forms_at_wavefront_and_block_edges(lanes, monkeypatch):
    monkeypatch.setenv("ZK_ECDSA_LANES", lanes)
    sig, fails = C.lanes_batch()
    assert sig["fields"].shape[0] == 130 and fails == [0, 15, 16, 63, 64, 129]
    want_status, want = C.model(sig, R)
    assert [i for i, s in enumerate(want_status) if s] == fails
    res, status, wire = oneshot.sig_assign(sig, R)
    C.compare(status, wire, want_status, want, lanes)
    assert res.fail_count == len(fails) and res.first_fail_row == 0


def test_sets_across_the_tile():
    sig = C.tiles_batch()
    assert sig["fields"].shape[0] == 300
    want_status, want = C.model(sig, R)
    res, status, wire = oneshot.sig_assign(sig, R)
    C.compare(status, wire, want_status, want)
    assert wire["keccak"].shape[0] == 1 + 12 and wire["sig_table"].shape[0] == 40


def test_chunked_launches_hip_vs_cpu(monkeypatch):
    """n = 2^15 + 64 with four lanes per signature: more than 2^17 lanes, two launches over one set of key tables"""
    monkeypatch.setenv("ZK_ECDSA_LANES", "4")
    n = (1 << 15) + 64
    sig = C.random_curve_point_inputs(n, 91)
    sig["fields"][(1 << 15) - 1, 2] = 0   # r = 0 on the first launch's last signature
    sig["fields"][(1 << 15), 1, 0] = 2    # parity 2 on the second launch's first
    res_c, st_c, w_c = oneshot.sig_assign(sig, R, device="cpu")
    res_h, st_h, w_h = oneshot.sig_assign(sig, R)
    assert res_h.fail_count == res_c.fail_count == 2 and np.flatnonzero(st_c).tolist() == [(1 << 15) - 1, 1 << 15]
    C.compare(st_h, w_h, st_c, w_c)
    assert w_h["keccak"].shape[0] == n - 2 + 1 and w_h["sig_table"].shape[0] == n


def _resident(sig, torch):
    """zk_sig_assign_open with device buffers -> ECDSA pass (layout 2, v = meta + 3) into meta[:, 0] -> zk_sign_open(is_sig)"""
    dev = torch.device("cuda")
    to_dev = lambda a: torch.from_numpy(a.view({8: np.int64, 4: np.int32, 1: np.uint8}[a.dtype.itemsize])).to(dev)  # noqa: E731
    sd = {k: (to_dev(np.ascontiguousarray(v)) if k in engine.SIG_ASSIGN_INPUTS and v is not None else v) for k, v in sig.items()}
    tdt = {np.uint64: torch.int64, np.uint32: torch.int32, np.uint8: torch.uint8}
    outs = {k: torch.zeros(shp, dtype=tdt[dt], device=dev) for k, (shp, dt) in engine.sig_assign_shapes(sig["fields"].shape[0]).items()}
    with engine.open_sig_assign(sd, R, outs=outs) as s:
        res = s.run()
        st = s.read_status()
        nk, ns = s.n_keccak(), s.n_sig_rows()
    with engine.open_ecdsa(outs["bytes"], v=outs["meta"].view(-1)[3:], layout=engine.ECDSA_LAYOUT_SIG_UNITS, out_dev=outs["meta"], out_stride=4,
                           v_stride=4) as e:
        e.run()
    wire = {k: outs[k] for k in ("bytes", "cells", "meta")}
    wire["keccak"] = outs["keccak"][:nk].contiguous()
    wire["tx_rows"], wire["tx_flags"] = torch.zeros((0, 5, 4), dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev)
    with engine.open_sign(wire, R, is_sig=True) as sg:
        sres = sg.run()
        sst = sg.read_status()
    torch.cuda.synchronize()
    return res, st, ns, sres, sst


def _cpu_chain(sig):
    res, st, w = oneshot.sig_assign(sig, R, device="cpu")
    _, ecd = oneshot.ecdsa_verify(w["bytes"], np.ascontiguousarray(w["meta"][:, 3]), layout=2, device="cpu")
    w["meta"][:, 0] = ecd
    w["tx_rows"], w["tx_flags"] = np.zeros((0, 5, 4), dtype=np.uint64), np.zeros(0, dtype=np.uint32)
    sres, sst = oneshot.sign_verify(w, R, True, device="cpu")
    return res, st, w["sig_table"].shape[0], sres, sst


def test_resident_chain_signed_data_to_sig_verification():
    torch = pytest.importorskip("torch")
    base = C.tiles_batch()
    sig = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in base.items()}
    sig["fields"][11, 1, 0] += 2          # v
    sig["fields"][75, 2, 3] ^= 1 << 40    # r
    sig["fields"][140, 3] = 0             # s
    sig["addr"][290, 0] ^= 1              # claimed address
    res, st, ns, sres, sst = _resident(sig, torch)
    cres, cst, cns, csres, csst = _cpu_chain(sig)
    assert np.array_equal(st, cst) and res.fail_count == cres.fail_count and ns == cns
    assert np.array_equal(sst, csst) and sres.fail_count == csres.fail_count
    assert st[11] and st[140] and sst[290] and not st[290]
