"""zk_ecc_from_calls on the MI355X (k_ecc_calls.hip): the directed batches through host buffers and through resident inputs with
caller-owned, guarded output buffers, HIP against the CPU backend, every combination of null members of out_dev, two passes with a
word changed in HBM, and the chains — without a host copy in between — into zk_ecc_open and into zk_evm_open on the reference's
ecAdd / ecMul / ecPairing fixtures."""
import itertools
import os

import numpy as np
import pytest

from tests import ecc_calls_cases as C
from tests import ecc_calls_ref as ref
from tests.evm_cases import load_cases
from tests.test_ecc_calls_cpu import RAGGED, _aux_words, domain_errors, evm_fixtures_rebuilt, verify_against_the_oracle
from zkevm_specs_amd import _lib, engine, oneshot
from zkevm_specs_amd import ecc_circuit as mirror

pytestmark = pytest.mark.gpu
BATCHES = ["directed", "n1", "n63", "n64", "n65", "n257", "adds_only", "muls_only", "pairings_only", "dups"]
GUARD = 64  # elements on both sides of every caller-owned output buffer
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _torch():
    return pytest.importorskip("torch")


def to_dev(a):
    torch = _torch()
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])).to(torch.device("cuda"))


def to_host(t, dtype):
    return t.cpu().numpy().view(dtype)


def guarded_outs(shapes, skip=()):
    """name -> (the whole guarded buffer, the view handed to the session); guards hold a pattern on both sides"""
    torch = _torch()
    tdt = {np.uint64: torch.int64, np.uint32: torch.int32}
    out = {}
    for k, (shp, dt) in shapes.items():
        if k in skip:
            continue
        n = int(np.prod(shp))
        whole = torch.full((n + 2 * GUARD,), 0x5A5A5A5A, dtype=tdt[dt], device="cuda")
        out[k] = (whole, whole[GUARD: GUARD + n].view(shp))
    return out


def check_guards(bufs):
    for k, (whole, _) in bufs.items():
        assert bool((whole[:GUARD] == 0x5A5A5A5A).all()) and bool((whole[-GUARD:] == 0x5A5A5A5A).all()), k


def read_outs(bufs, shapes, n_table):
    out = {k: to_host(view, shapes[k][1]).reshape(shapes[k][0]) for k, (_, view) in bufs.items()}
    if "ecc_table" in out:
        out["ecc_table"] = out["ecc_table"][:n_table]
    return out


@pytest.mark.parametrize("name", BATCHES)
def test_directed_batch_host_buffers(name):
    calls = mirror.ecc_calls_wire(*C.batches()[name])
    res, status, out = oneshot.ecc_from_calls(calls, C.RANDOMNESS)
    want = C.expected(name)
    assert res.ok and res.rows_evaluated == want["rows"].shape[0] and not status.any()
    ref.assert_equal(out, want, name)


@pytest.mark.parametrize("name", BATCHES)
def test_directed_batch_resident_with_guards(name):
    torch = _torch()
    calls = {k: to_dev(v) for k, v in mirror.ecc_calls_wire(*C.batches()[name]).items()}
    want = C.expected(name)
    n = want["rows"].shape[0]
    with engine.open_ecc_from_calls(calls, C.RANDOMNESS) as probe:
        shapes = probe.shapes
    bufs = guarded_outs(shapes)
    status = torch.full((n + 2 * GUARD,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    with engine.open_ecc_from_calls(calls, C.RANDOMNESS, outs={k: v for k, (_, v) in bufs.items()}) as s:
        s.launch(status[GUARD: GUARD + n])
        assert s.collect().ok
        nt = s.n_table_rows()
    torch.cuda.synchronize()
    check_guards(bufs)
    assert bool((status[:GUARD] == 0x5A5A5A5A).all()) and bool((status[-GUARD:] == 0x5A5A5A5A).all()) and not bool(status[GUARD: GUARD + n].any())
    ref.assert_equal(read_outs(bufs, shapes, nt), want, name)


def test_hip_equals_cpu_backend():
    for name in ("directed", "n257"):
        calls = mirror.ecc_calls_wire(*C.batches()[name])
        _, st_h, hip = oneshot.ecc_from_calls(calls, C.RANDOMNESS)
        _, st_c, cpu = oneshot.ecc_from_calls(calls, C.RANDOMNESS, device="cpu")
        assert np.array_equal(st_h, st_c)
        ref.assert_equal(hip, cpu, name)


def test_every_combination_of_null_members():
    torch = _torch()
    calls = {k: to_dev(v) for k, v in mirror.ecc_calls_wire(*C.batches()["dups"]).items()}
    want = C.expected("dups")
    with engine.open_ecc_from_calls(calls, C.RANDOMNESS) as probe:
        shapes = probe.shapes
    for r in range(len(ref.OUTPUTS) + 1):
        for skip in itertools.combinations(ref.OUTPUTS, r):
            bufs = guarded_outs(shapes, skip)
            with engine.open_ecc_from_calls(calls, C.RANDOMNESS, outs={k: v for k, (_, v) in bufs.items()}) as s:
                assert s.run().ok
                nt = s.n_table_rows()
                own = s.read()  # the session's own buffers for the null members, the caller's for the others
            torch.cuda.synchronize()
            check_guards(bufs)
            assert nt == want["ecc_table"].shape[0]
            ref.assert_equal(own, want, f"null {skip}")
            got = read_outs(bufs, shapes, nt)
            for k in got:
                assert np.array_equal(got[k], want[k]), (skip, k)


def test_two_passes_with_a_word_changed_in_hbm():
    adds, muls, prs = C.batches()["dups"]
    calls = {k: to_dev(v) for k, v in mirror.ecc_calls_wire(adds, muls, prs).items()}
    with engine.open_ecc_from_calls(calls, C.RANDOMNESS) as s:
        assert s.n_table_rows() == 0
        assert s.run().ok
        ref.assert_equal(s.read(), C.expected("dups"), "first pass")
        calls["add_in"][0, 2:] = calls["add_in"][0, :2].clone()
        calls["mul_in"][1, 2] = calls["mul_in"][2, 2].clone()
        calls["pair_pts"][0, 1, 0] ^= 1
        assert s.run().ok
        g1 = list(prs[0][0])
        g1[0] = (g1[0][0], g1[0][1] ^ 1)
        want = ref.model([(adds[0][0], adds[0][0])] + adds[1:], [muls[0], (muls[1][0], muls[2][1])] + muls[2:], [(g1, prs[0][1])] + prs[1:], C.RANDOMNESS)
        ref.assert_equal(s.read(), want, "second pass")


def test_domain_errors_resident():
    lib = _lib.init()
    domain_errors(lib, to_dev=to_dev, opts=_lib.OPT_DEVICE_PTRS)
    domain_errors(lib)


def test_evm_fixtures_rebuilt_hip():
    evm_fixtures_rebuilt(None)


def test_verify_against_the_oracle_hip():
    verify_against_the_oracle(None)


def test_chain_into_ecc_open():
    """calls (HBM) -> zk_ecc_from_calls_open -> zk_ecc_open over its points / pair_out / rows, nothing copied to the host in between:
    the statuses are those over ops and rows built on the host"""
    torch = _torch()
    adds, muls, prs = C.batches()["n65"]
    host = mirror.ecc_calls_wire(adds, muls, prs)
    calls = {k: to_dev(v) for k, v in host.items()}
    with engine.open_ecc_from_calls(calls, C.RANDOMNESS) as probe:
        shapes = probe.shapes
    tdt = {np.uint64: torch.int64, np.uint32: torch.int32}
    outs = {k: torch.zeros(shp, dtype=tdt[dt], device="cuda") for k, (shp, dt) in shapes.items()}
    with engine.open_ecc_from_calls(calls, C.RANDOMNESS, outs=outs) as s:
        s.launch()
        wire = {"points": outs["points"], "n_add": len(adds), "n_mul": len(muls), "pair_pts": calls["pair_pts"], "pair_off": calls["pair_off"],
                "pair_out": outs["pair_out"], "max_ok": np.ones(3, dtype=np.uint32)}
        with engine.open_ecc(wire, outs["rows"], C.RANDOMNESS) as v:
            res = v.run()
            status = v.read_status()
        assert s.collect().ok
    want = C.expected("n65")
    hw = {"points": want["points"], "n_add": len(adds), "n_mul": len(muls), "pair_pts": host["pair_pts"], "pair_off": host["pair_off"],
          "pair_out": want["pair_out"], "max_ok": np.ones(3, dtype=np.uint32)}
    hres, hstatus = oneshot.ecc_verify(hw, want["rows"], C.RANDOMNESS)
    assert np.array_equal(status, hstatus) and res.fail_count == hres.fail_count
    assert hres.fail_count > 0 and (hstatus == 0).sum() > 100  # the s >= p muls fail (the pinned quirk), everything else passes


def _fixture_call(test, w, k):
    if test == "ecAdd":
        px, py, qx, qy = _aux_words(w["aux"][0], 4)
        return [((px, py), (qx, qy))], [], []
    if test == "ecMul":
        px, py, s = _aux_words(w["aux"][0], 3)
        return [], [((px, py), s)], []
    return [], [], [list(C.REF_PAIRING_VECTORS.values())[k][0]]


def test_chain_into_evm_open():
    """the un-fuzzed ecAdd / ecMul / ecPairing fixtures with `ecc` and the precompile step's aux row taken from the new entry in HBM:
    zk_evm_open's statuses equal those over the fixture's own tables"""
    torch = _torch()
    n = 0
    for test in ("ecAdd", "ecMul", "ecPairing"):
        k = 0
        for name, w, opts, _ in load_cases(os.path.join(GOLDEN, f"evm_{test}.npz")):
            if "#fuzz" in name:
                continue
            k += 1
            if name.split("::")[-1] in RAGGED:
                continue
            _, own = engine_status(w, opts)
            calls = {key: to_dev(v) for key, v in mirror.ecc_calls_wire(*_fixture_call(test, w, k - 1)).items()}
            dev = {key: to_dev(v) for key, v in w.items() if hasattr(v, "dtype") and key not in ("ecc", "aux", "aux_kind")}
            aux = torch.zeros(w["aux"].shape, dtype=torch.int64, device="cuda")
            kind = torch.zeros(w["aux_kind"].shape, dtype=torch.int32, device="cuda")
            ecc = torch.zeros((1, 13, 4), dtype=torch.int64, device="cuda")
            with engine.open_ecc_from_calls(calls, C.RANDOMNESS, outs={"ecc_table": ecc, "aux": aux[:1], "aux_kind": kind[:1]}) as s:
                s.launch()
                dev.update(ecc=ecc, aux=aux, aux_kind=kind)
                with engine.open_evm(dev, bool(opts[0]), bool(opts[1])) as e:
                    res = e.run()
                    status = e.read_status()
                assert s.collect().ok and s.n_table_rows() == 1
            assert status.tolist() == own.tolist() and not status.any(), (test, name)
            n += 1
    assert n == 3 + 5 + 4


def engine_status(w, opts):
    with engine.open_evm({k: v for k, v in w.items() if hasattr(v, "dtype")}, bool(opts[0]), bool(opts[1])) as e:
        res = e.run()
        return res, e.read_status()
