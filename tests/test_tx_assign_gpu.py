"""Tx circuit witness assignment on the MI355X (k_tx_assign.hip): the golden cases, the CPU backend at 2^14 txs in every lane form
of the key recovery, the new secp256k1 base-field hooks, and raw txs -> zk_tx_assign_open (HBM) -> ECDSA pass -> zk_sign_open."""
import os

import numpy as np
import pytest

from tests import tx_assign_ref as M
from tests.tx_assign_cases import WIRE_KEYS, golden_cases, random_inputs
from zkevm_specs_amd import engine, oneshot
from zkevm_specs_amd.wire import cells_to_ints, ints_to_cells

pytestmark = pytest.mark.gpu
R = 0x0BADC0FFEE0DDF00D


def test_golden_cases_hip():
    n = 0
    for c in golden_cases():
        t = c["tx"]
        if c["host_errors"] or t["fields"].shape[0] > t["max_txs"] or int(t["offsets"][-1]) > t["max_calldata_bytes"]:
            continue
        res, status, wire = oneshot.tx_assign(t, c["randomness"])
        code, fail_tx = c["exc"]
        if code:
            first = int(np.flatnonzero(status)[0])
            assert (first, int(status[first])) == (fail_tx, code), c["name"]
            continue
        assert res.fail_count == 0, c["name"]
        for k in WIRE_KEYS:
            assert np.array_equal(wire[k], c["wire"][k]), (c["name"], k)
        n += 1
    assert n >= 15


@pytest.fixture(scope="module")
def big():
    t = random_inputs(1 << 14, 77, chain_id=10, long_every=5, signed=False)
    t["fields"][100, 6] = 0   # r = 0: site 1
    t["fields"][200, 5, 0] += 2   # parity: site 1
    return t


@pytest.mark.parametrize("lanes", ["1", "2", "4"])
def test_2p14_txs_hip_vs_cpu_every_lane_form(big, lanes, monkeypatch):
    monkeypatch.setenv("ZK_ECDSA_LANES", lanes)
    res_c, st_c, w_c = oneshot.tx_assign(big, R, device="cpu")
    res_h, st_h, w_h = oneshot.tx_assign(big, R)
    assert np.array_equal(st_h, st_c) and res_h.fail_count == res_c.fail_count == 2
    for k in WIRE_KEYS:
        assert np.array_equal(w_h[k], w_c[k]), k


def test_fr_op_sqrt_and_inverse_hooks_hip():
    xs = [0, 1, 2, 7, M.P - 1, M.G[0], M.G[1]] + [pow(3, 1000 + k, M.P) for k in range(57)]
    a = ints_to_cells(xs)
    for op, e in ((26, (M.P + 1) // 4), (27, M.P - 2)):
        assert cells_to_ints(engine.fr_op(op, a, a)) == [pow(x, e, M.P) for x in xs]


def _e2e(t, torch):
    """zk_tx_assign_open with device buffers -> ECDSA pass into meta[:, 0] -> zk_sign_open; -> (assign status, sign status)"""
    dev = torch.device("cuda")
    to_dev = lambda a: torch.from_numpy(a.view({8: np.int64, 4: np.int32, 1: np.uint8}[a.dtype.itemsize])).to(dev)  # noqa: E731
    td = {k: (to_dev(np.ascontiguousarray(v)) if k in engine.TX_ASSIGN_INPUTS else v) for k, v in t.items()}
    shapes = engine.tx_assign_shapes(t["fields"].shape[0], t["max_txs"], t["max_calldata_bytes"])
    tdt = {np.uint64: torch.int64, np.uint32: torch.int32, np.uint8: torch.uint8}
    outs = {k: torch.zeros(shp, dtype=tdt[dt], device=dev) for k, (shp, dt) in shapes.items()}
    with engine.open_tx_assign(td, R, outs=outs) as s:
        res = s.run()
        st = s.read_status()
        nk = s.n_keccak()
    with engine.open_ecdsa(outs["bytes"], layout=engine.ECDSA_LAYOUT_TX_UNITS, out_dev=outs["meta"], out_stride=4) as e:
        e.run()
    wire = {k: outs[k] for k in ("bytes", "cells", "meta", "tx_rows", "tx_flags")}
    wire["keccak"] = outs["keccak"][:nk].contiguous()
    with engine.open_sign(wire, R, is_sig=False) as sg:
        sres = sg.run()
        sst = sg.read_status()
    torch.cuda.synchronize()
    return res, st, sres, sst


def _cpu(t):
    res, st, w = oneshot.tx_assign(t, R, device="cpu")
    _, ecd = oneshot.ecdsa_verify(np.ascontiguousarray(w["bytes"]), None, layout=1, device="cpu")
    w["meta"][:, 0] = ecd
    sres, sst = oneshot.sign_verify(w, R, is_sig=False, device="cpu")
    return res, st, sres, sst


def test_end_to_end_raw_txs_to_sign_verification_on_device(big):
    torch = pytest.importorskip("torch")
    clean = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in big.items()}
    clean["fields"][100] = big["fields"][101]
    clean["fields"][200] = big["fields"][201]
    tampered = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in big.items()}
    tampered["fields"][300, 5, 0] += 4          # v
    tampered["fields"][400, 6, 3] ^= 1 << 40     # r
    tampered["fields"][500, 7] = 0               # s
    tampered["calldata"][7] ^= 0xFF              # calldata: another hash, another (valid) key
    for t, clean_run in ((clean, True), (tampered, False)):
        res, st, sres, sst = _e2e(t, torch)
        cres, cst, csres, csst = _cpu(t)
        assert np.array_equal(st, cst) and res.fail_count == cres.fail_count
        assert np.array_equal(sst, csst) and sres.fail_count == csres.fail_count
        if clean_run:
            assert res.fail_count == 0 and sres.fail_count == 0
        else:
            assert res.fail_count >= 4
