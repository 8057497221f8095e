"""zk_events_from_trace_ext* on the device: every case of tests/events_from_trace_ext_cases.py through the one-shot and through a session
against the plain-Python model; sessions passing twice on two streams; device pointers with caller buffers cleared between the passes; the
capacities; the identity with zk_events_from_trace; the reference-recorded goldens; the derived events through
zk_copy_assign_from_sources; the open refusals under this entry's name."""
import ctypes

import numpy as np
import pytest

from tests import events_from_trace_ext_cases as xc
from tests import events_from_trace_ext_ref as xref
from tests import test_events_from_trace_ext_cpu as host
from tests import test_events_from_trace_cpu as old
from tests.test_events_from_trace_gpu import resident
from zkevm_specs_amd import _lib, engine

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", xc.NAMES)
def test_one_shot(name):
    xc.check_outputs(name, *host.run(xc.case(name), None))


@pytest.mark.parametrize("name", xc.NAMES)
def test_session(name):
    c, want = xc.case(name), xc.expected(name)
    with engine.open_events_from_trace_ext(c["trace"], c["codes"], c["hashes"]) as s:
        res = s.run()
        assert s.counts() == (len(want["copy_step"]), len(want["exp_step"]))
        xc.check_outputs(name, res, s.read_status(), s.read())


def test_sizes():
    host.check_sizes(None)


def test_sessions_pass_twice_on_two_streams():
    import torch

    host.check_session(None, torch.cuda.Stream())


@pytest.mark.parametrize("name", ["forms_gaps", "sites", "pairs_257", "ladder_1025_alt", "ladder_1025_all"])
def test_device_pointers_twice(name):
    """inputs resident, outputs in place in the caller's tensors (status included); the second pass, into cleared buffers, equals the first"""
    import torch

    c, want = xc.case(name), xc.expected(name)
    tr, codes, hashes = resident(c)
    n = len(want["status"])
    caps = engine.events_from_trace_ext_sizes(tr, codes, hashes)
    assert caps == xref.capacities(c["trace"])
    shapes = engine.events_from_trace_ext_shapes(*caps)
    view = {np.uint64: torch.int64, np.uint32: torch.int32}
    outs = {k: torch.full(shp, -1, dtype=view[dt], device="cuda") for k, (shp, dt) in shapes.items()}
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    h = lambda t, dt: t.cpu().numpy().view(dt)  # noqa: E731
    with engine.open_events_from_trace_ext(tr, codes, hashes, outs) as s:
        passes = []
        for _ in range(2):
            for t in (*outs.values(), status):
                t.fill_(-1)
            s.launch(status)
            res = s.collect()
            n_copy, n_exp = s.counts()
            torch.cuda.synchronize()
            got = engine.cut_trace_events({k: h(t, shapes[k][1]) for k, t in outs.items()}, n_copy, n_exp)
            xc.check_outputs(name, res, h(status, np.uint32), got)
            # nothing is written behind the packed lists
            assert all(bool((t[(n_copy if k.startswith("copy") else n_exp):] == -1).all()) for k, t in outs.items())
            passes.append((h(status, np.uint32).copy(), {k: v.copy() for k, v in got.items()}))
        assert np.array_equal(passes[0][0], passes[1][0]) and all(np.array_equal(passes[0][1][k], passes[1][1][k]) for k in xc.OUTPUTS)


def test_identity_with_the_old_entry():
    host.check_identity(None)


def test_goldens(golden_dir):
    counts = host.check_goldens(golden_dir, None)
    assert all(counts[k][0] >= u and counts[k][1] >= e for k, (u, e) in host.GOLDEN_KINDS.items()), counts
    seen = host.check_unsupported_goldens(golden_dir, None)
    assert all(n >= 100 for n in seen.values()), seen


def test_pipeline():
    host.check_pipeline(None)


@pytest.mark.parametrize("label,c,rc,text", host.domain_errors(), ids=[d[0] for d in host.domain_errors()])
def test_open_refusals(label, c, rc, text):
    args = (c["trace"], c["codes"], c["hashes"])
    assert old.error_of(engine.events_from_trace_ext_sizes, *args) == (rc, text)
    assert old.error_of(engine.open_events_from_trace_ext, *args) == (rc, text)
    tr, codes, hashes = resident(c)  # the same verdicts over device-resident inputs
    assert old.error_of(engine.events_from_trace_ext_sizes, tr, codes, hashes) == (rc, text)
    assert old.error_of(engine.open_events_from_trace_ext, tr, codes, hashes) == (rc, text)


def test_refusals_without_arrays():
    host.check_too_many_rows(None)
    import torch

    c = xc.case("forms")
    with pytest.raises(ValueError):  # caller buffers beside host inputs
        engine.open_events_from_trace_ext(c["trace"], c["codes"], c["hashes"], {"copy_dst_ref": torch.zeros(xref.capacities(c["trace"])[0], dtype=torch.int32, device="cuda")})
    # the library's own refusal of caller buffers without ZK_OPT_DEVICE_PTRS
    p = engine._wire_args(engine.TRACE_EVENTS_EXT, engine.trace_event_sources(c["trace"], c["codes"], c["hashes"]))
    lib, hnd = _lib.init(None), ctypes.c_void_p()
    w = _lib.ZkTraceEventsExt()
    assert lib.zk_events_from_trace_ext_open(ctypes.byref(p.t), ctypes.byref(w), 0, ctypes.byref(hnd)) == -1
    assert lib.zk_last_error().decode() == "zk_events_from_trace_ext_open: out_dev needs ZK_OPT_DEVICE_PTRS"


def test_library_exports_the_entries():
    lib = _lib.load()
    for name in ("zk_events_from_trace_ext_sizes", "zk_events_from_trace_ext_open", "zk_events_from_trace_ext_read", "zk_events_from_trace_ext_counts",
                 "zk_events_from_trace_ext"):
        assert hasattr(lib, name)
