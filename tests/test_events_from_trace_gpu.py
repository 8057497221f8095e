"""zk_events_from_trace* on the device: every case of tests/events_from_trace_cases.py through the one-shot and through a session against
the plain-Python model; one case with device pointers and caller buffers, run twice; the reference-recorded goldens; the consistent block;
the open refusals of this entry."""
import numpy as np
import pytest

from tests import events_from_trace_cases as cc
from tests import test_events_from_trace_cpu as host
from zkevm_specs_amd import _lib, engine

pytestmark = pytest.mark.gpu


def dev(x):
    import torch

    if x is None:
        return None
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32, np.dtype(np.uint8): np.uint8}[x.dtype]
    return torch.from_numpy(np.ascontiguousarray(x).view(view)).cuda()


def resident(c):
    """the case's arrays as device tensors: (trace, codes, hashes)"""
    x = engine.trace_event_sources(c["trace"], c["codes"], c["hashes"])
    tr = {k: (dev(v) if hasattr(v, "shape") else v) for k, v in c["trace"].items() if k != "prev"}
    return tr, {"code": dev(x["code"]), "code_offsets": dev(x["code_offsets"])}, dev(x["code_hashes"])


@pytest.mark.parametrize("name", cc.NAMES)
def test_one_shot(name):
    cc.check_outputs(name, *host.run(cc.case(name), None))


@pytest.mark.parametrize("name", cc.NAMES)
def test_session(name):
    c = cc.case(name)
    with engine.open_events_from_trace(c["trace"], c["codes"], c["hashes"]) as s:
        res = s.run()
        want = cc.expected(name)
        assert s.counts() == (len(want["copy_step"]), len(want["exp_step"]))
        cc.check_outputs(name, res, s.read_status(), s.read())


def test_sessions_pass_twice_on_two_streams():
    import torch

    host.check_session(None, torch.cuda.Stream())


@pytest.mark.parametrize("name", ["kinds_gaps", "ladder_1025_alt"])
def test_device_pointers_twice(name):
    """inputs resident, outputs in place in the caller's tensors (status included); the second pass, into cleared buffers, equals the first"""
    import torch

    c, want = cc.case(name), cc.expected(name)
    tr, codes, hashes = resident(c)
    n = len(want["status"])
    assert engine.events_from_trace_sizes(tr, codes, hashes) == n
    shapes = engine.events_from_trace_shapes(n)
    view = {np.uint64: torch.int64, np.uint32: torch.int32}
    outs = {k: torch.full(shp, -1, dtype=view[dt], device="cuda") for k, (shp, dt) in shapes.items()}
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    h = lambda t, dt: t.cpu().numpy().view(dt)  # noqa: E731
    with engine.open_events_from_trace(tr, codes, hashes, outs) as s:
        passes = []
        for _ in range(2):
            for t in (*outs.values(), status):
                t.fill_(-1)
            s.launch(status)
            res = s.collect()
            n_copy, n_exp = s.counts()
            torch.cuda.synchronize()
            got = engine.cut_trace_events({k: h(t, shapes[k][1]) for k, t in outs.items()}, n_copy, n_exp)
            cc.check_outputs(name, res, h(status, np.uint32), got)
            # nothing is written behind the packed lists
            assert all(bool((t[(n_copy if k.startswith("copy") else n_exp):] == -1).all()) for k, t in outs.items())
            passes.append((h(status, np.uint32).copy(), {k: v.copy() for k, v in got.items()}))
        assert np.array_equal(passes[0][0], passes[1][0]) and all(np.array_equal(passes[0][1][k], passes[1][1][k]) for k in cc.OUTPUTS)


def test_goldens(golden_dir):
    used = host.check_goldens(golden_dir, None)
    assert all(used[k] >= n for k, n in host.GOLDEN_KINDS.items()), used


def test_consistent_block():
    host.check_block(None)


@pytest.mark.parametrize("label,c,rc,text", host.domain_errors(), ids=[d[0] for d in host.domain_errors()])
def test_open_refusals(label, c, rc, text):
    args = (c["trace"], c["codes"], c["hashes"])
    assert host.error_of(engine.events_from_trace_sizes, *args) == (rc, text)
    assert host.error_of(engine.open_events_from_trace, *args) == (rc, text)
    tr, codes, hashes = resident(c)  # the same verdicts over device-resident inputs
    assert host.error_of(engine.events_from_trace_sizes, tr, codes, hashes) == (rc, text)
    assert host.error_of(engine.open_events_from_trace, tr, codes, hashes) == (rc, text)


def test_refusals_without_arrays():
    host.check_too_many_rows(None)
    import ctypes

    import torch

    c = cc.case("kinds")
    with pytest.raises(ValueError):  # caller buffers beside host inputs
        engine.open_events_from_trace(c["trace"], c["codes"], c["hashes"], {"copy_step": torch.zeros(len(c["trace"]["steps"]), dtype=torch.int32, device="cuda")})
    # the library's own refusal of caller buffers without ZK_OPT_DEVICE_PTRS
    p = engine._wire_args(engine.TRACE_EVENTS, engine.trace_event_sources(c["trace"], c["codes"], c["hashes"]))
    lib, hnd = _lib.init(None), ctypes.c_void_p()
    w = _lib.ZkTraceEvents()
    assert lib.zk_events_from_trace_open(ctypes.byref(p.t), ctypes.byref(w), 0, ctypes.byref(hnd)) == -1
    assert lib.zk_last_error().decode() == "zk_events_from_trace_open: out_dev needs ZK_OPT_DEVICE_PTRS"


def test_library_exports_the_entries():
    lib = _lib.load()
    for name in ("zk_events_from_trace_sizes", "zk_events_from_trace_open", "zk_events_from_trace_read", "zk_events_from_trace_counts", "zk_events_from_trace"):
        assert hasattr(lib, name)
