"""zk_sha3_from_trace* on the device: every case of tests/trace_sha3_cases.py through the one-shot and through a session against the
plain-Python model; device pointers with every output and the status in caller tensors, cleared between two passes; passes after the
caller rewrote its resident records; the composition with zk_keccak_table; the reference-recorded goldens; the consistent block; the open
refusals of this entry."""
import ctypes

import numpy as np
import pytest

from tests import test_trace_sha3_cpu as host
from tests import trace_sha3_cases as cc
from zkevm_specs_amd import _lib, engine

pytestmark = pytest.mark.gpu


def dev(x):
    import torch

    if x is None:
        return None
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32, np.dtype(np.uint8): np.uint8}[x.dtype]
    return torch.from_numpy(np.ascontiguousarray(x).view(view)).cuda()


def resident(tr):
    """the records as device tensors"""
    return {k: (dev(v) if hasattr(v, "shape") else v) for k, v in tr.items() if k != "prev"}


@pytest.mark.parametrize("name", cc.NAMES)
def test_one_shot(name):
    cc.check_outputs(name, *host.run(cc.case(name), None))


@pytest.mark.parametrize("name", cc.NAMES)
def test_session(name):
    c, want = cc.case(name), cc.expected(name)
    assert engine.sha3_from_trace_sizes(c["trace"]) == (len(want["step"]), len(want["data"]))
    with engine.open_sha3_from_trace(c["trace"], c["randomness"]) as s:
        res = s.run()
        assert s.counts() == (len(want["step"]), len(want["data"]))
        cc.check_outputs(name, res, s.read_status(), s.read())


def test_sessions_pass_twice_on_two_streams():
    import torch

    host.check_session(None, torch.cuda.Stream())


@pytest.mark.parametrize("name", ["lengths_gaps", "sites", "bytes_edges", "ladder_1025_alt"])
def test_device_pointers_twice(name):
    """inputs resident, every output and the status in place in the caller's tensors; the second pass, into cleared buffers, equals the first"""
    import torch

    c, want = cc.case(name), cc.expected(name)
    tr = resident(c["trace"])
    counts = engine.sha3_from_trace_sizes(tr)
    assert counts == (len(want["step"]), len(want["data"]))
    shapes = engine.sha3_from_trace_shapes(*counts)
    view = {np.uint64: torch.int64, np.uint32: torch.int32, np.uint8: torch.uint8}
    outs = {k: torch.full(shp, 0x55, dtype=view[dt], device="cuda") for k, (shp, dt) in shapes.items()}
    status = torch.full((len(want["status"]),), -1, dtype=torch.int32, device="cuda")
    h = lambda t, dt: t.cpu().numpy().view(dt)  # noqa: E731
    with engine.open_sha3_from_trace(tr, c["randomness"], outs) as s:
        passes = []
        for _ in range(2):
            for t in outs.values():
                t.fill_(0x55)
            status.fill_(-1)
            s.launch(status)
            res = s.collect()
            torch.cuda.synchronize()
            got = {k: h(t, shapes[k][1]) for k, t in outs.items()}
            cc.check_outputs(name, res, h(status, np.uint32), got)
            passes.append((h(status, np.uint32).copy(), {k: v.copy() for k, v in got.items()}))
        assert np.array_equal(passes[0][0], passes[1][0]) and all(np.array_equal(passes[0][1][k], passes[1][1][k]) for k in cc.OUTPUTS)


def test_passes_after_rewrites():
    """the records resident: the caller overwrites val between passes (host.check_rewrites)"""
    def open_session(c):
        tr = resident(c["trace"])
        return engine.open_sha3_from_trace(tr, c["randomness"]), tr

    def poke(tr, name, i, v):
        tr[name][i] = v

    host.check_rewrites(open_session, poke)


def test_rows_are_the_keccak_table_of_the_data():
    host.check_composition(None)


def test_goldens(golden_dir):
    assert host.check_goldens(golden_dir, None) == host.GOLDEN_USED


def test_consistent_block():
    host.check_block(None)


@pytest.mark.parametrize("label,t,rc,text", host.domain_errors(), ids=[d[0] for d in host.domain_errors()])
def test_open_refusals(label, t, rc, text):
    assert host.error_of(engine.sha3_from_trace_sizes, t) == (rc, text)
    assert host.error_of(engine.open_sha3_from_trace, t, cc.RANDOMNESS) == (rc, text)
    tr = resident(t)  # the same verdicts over device-resident records
    assert host.error_of(engine.sha3_from_trace_sizes, tr) == (rc, text)
    assert host.error_of(engine.open_sha3_from_trace, tr, cc.RANDOMNESS) == (rc, text)


def test_refusals_without_arrays():
    host.check_too_many_rows(None)
    import torch

    c = cc.case("single")
    with pytest.raises(ValueError):  # caller buffers beside host inputs
        engine.open_sha3_from_trace(c["trace"], c["randomness"], {"step": torch.zeros(1, dtype=torch.int32, device="cuda")})
    # the library's own refusal of caller buffers without ZK_OPT_DEVICE_PTRS
    p = engine._wire_args(engine.TRACE_SHA3, engine._trace_sha3_records(c["trace"]), (c["randomness"],))
    lib, hnd = _lib.init(None), ctypes.c_void_p()
    w = _lib.ZkTraceSha3()
    assert lib.zk_sha3_from_trace_open(ctypes.byref(p.t), _lib.ptr(p.keep[-1]), ctypes.byref(w), 0, ctypes.byref(hnd)) == -1
    assert lib.zk_last_error().decode() == "zk_sha3_from_trace_open: out_dev needs ZK_OPT_DEVICE_PTRS"


def test_library_exports_the_entries():
    lib = _lib.load()
    for name in ("zk_sha3_from_trace_sizes", "zk_sha3_from_trace_open", "zk_sha3_from_trace_read", "zk_sha3_from_trace"):
        assert hasattr(lib, name)
