"""zk_bytecode_from_code on the device (csrc/k_bytecode_code.hip): the bytecode table, the Bytecode circuit's rows and the keccak rows
from raw contract code — host buffers, code resident in HBM with caller-owned outputs, sessions, and the chain into the Bytecode
circuit without a host copy — against the plain-Python model of tests/bytecode_code_cases.py and the CPU backend."""
import itertools

import numpy as np
import pytest

from tests import bytecode_code_cases as bc
from zkevm_specs_amd import engine, oneshot

pytestmark = pytest.mark.gpu

R = bc.R_DEFAULT
CASES = bc.directed_cases()
NAMES = [c[0] for c in CASES]
GUARD = 512  # int64 words of -1 on either side of every caller-owned output


def same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a.shape == b.shape and np.array_equal(a, b))


def case(name):
    return next(c for c in CASES if c[0] == name)


def dev(x):
    import torch

    return torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).cuda()


def guarded(shape):
    """(flat tensor of -1 with GUARD words around the output, the output's view) in HBM; (None, None) for no output"""
    import torch

    if shape is None:
        return None, None
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * GUARD,), -1, dtype=torch.int64, device="cuda")
    return flat, flat[GUARD : GUARD + n].view(shape)


def host(t):
    return t.cpu().numpy().view(np.uint64)


def guards_intact(flat):
    return bool((flat[:GUARD] == -1).all()) and bool((flat[-GUARD:] == -1).all())


@pytest.mark.parametrize("name", NAMES)
def test_directed_host_buffers(name):
    _, codes, k = case(name)
    exp = bc.directed_expected(name)
    code, off = bc.pack(list(codes))
    res, table, rows, keccak = oneshot.bytecode_from_code(code, off, k, R)
    assert res.ok and res.fail_count == 0 and res.rows_evaluated == exp[0].shape[0]
    assert same(table, exp[0]) and same(rows, exp[1]) and same(keccak, exp[2])


@pytest.mark.parametrize("name", NAMES)
def test_directed_resident_code_caller_buffers(name):
    import torch

    _, codes, k = case(name)
    exp = bc.directed_expected(name)
    code, off = bc.pack(list(codes))
    shapes = engine.bytecode_from_code_shapes(len(code), len(codes), k)
    bufs = {n: guarded(shapes[n]) for n in engine.CODE_OUTPUTS}
    with engine.open_bytecode_from_code(dev(code), dev(off), k, R, table_dev=bufs["table"][1], rows_dev=bufs["rows"][1],
                                        keccak_dev=bufs["keccak"][1]) as s:
        res = s.run()
        torch.cuda.synchronize()
        assert res.ok and res.rows_evaluated == exp[0].shape[0]
        for n, e in zip(engine.CODE_OUTPUTS, exp):
            flat, out = bufs[n]
            if e is None:
                assert out is None
                continue
            assert same(host(out), e), n  # (no cell of the model is all ones: every cell was written)
            assert guards_intact(flat), n
        assert all(same(a, b) for a, b in zip(s.read(), exp))


def test_hip_equals_cpu_backend_on_a_skewed_random_set():
    codes = bc.random_set()
    assert len(codes) == 200 and sum(len(c) for c in codes) == 1 << 16 and max(len(c) for c in codes) >= 8 << 10
    code, off = bc.pack(codes)
    for k in (17, 15, 0):  # whole, truncated, table only
        cpu = oneshot.bytecode_from_code(code, off, k, R, device="cpu")
        hip = oneshot.bytecode_from_code(code, off, k, R)
        assert hip[0].ok and hip[0].rows_evaluated == cpu[0].rows_evaluated == (1 << 16) + 200
        assert all(same(a, b) for a, b in zip(hip[1:], cpu[1:])), k


def test_two_passes_with_a_byte_changed_in_hbm():
    import torch

    _, codes, k = case("push_misc")
    code, off = bc.pack(list(codes))
    d_code = dev(code)
    with engine.open_bytecode_from_code(d_code, dev(off), k, R) as s:
        assert s.run().ok
        assert all(same(a, b) for a, b in zip(s.read(), bc.directed_expected("push_misc")))
        at = int(off[2]) + 10  # a byte before the third code's PUSH32 becomes a PUSH32 itself: that code's is_code changes, and its hash
        d_code[at] = 0x7F
        torch.cuda.synchronize()
        changed = bytearray(code.tobytes())
        changed[at] = 0x7F
        codes2 = [bytes(changed[int(off[j]) : int(off[j + 1])]) for j in range(len(codes))]
        exp2 = bc.model(codes2, k, R)
        assert not same(exp2[0], bc.directed_expected("push_misc")[0])
        res = s.run()
        assert res.ok and res.launches == 1
        assert all(same(a, b) for a, b in zip(s.read(), exp2))


@pytest.mark.parametrize("name", ["edges", "tiny300", "code_24576"])
def test_chain_into_the_bytecode_circuit_without_a_host_copy(name):
    import torch

    _, codes, k = case(name)
    code, off = bc.pack(list(codes))
    d_rows = torch.full((12, 1 << k, 4), -1, dtype=torch.int64, device="cuda")
    d_keccak = torch.full((len(codes), 5, 4), -1, dtype=torch.int64, device="cuda")
    with engine.open_bytecode_from_code(dev(code), dev(off), k, R, rows_dev=d_rows, keccak_dev=d_keccak) as a:
        a.launch()
        with engine.open_bytecode(d_rows, d_keccak, R) as c:  # (same stream: ordered behind the assignment)
            res = c.run()
        assert res.ok and res.fail_count == 0 and res.rows_evaluated == 1 << k
        assert a.collect().ok
    assert same(host(d_rows), bc.directed_expected(name)[1])


@pytest.mark.parametrize("given", list(itertools.product((False, True), repeat=3)))
def test_null_members_of_out_dev(given):
    _, codes, k = case("truncated_in_push_data")
    exp = bc.directed_expected("truncated_in_push_data")
    code, off = bc.pack(list(codes))
    shapes = engine.bytecode_from_code_shapes(len(code), len(codes), k)
    bufs = {n: guarded(shapes[n]) if g else (None, None) for n, g in zip(engine.CODE_OUTPUTS, given)}
    with engine.open_bytecode_from_code(dev(code), dev(off), k, R, table_dev=bufs["table"][1], rows_dev=bufs["rows"][1],
                                        keccak_dev=bufs["keccak"][1]) as s:
        assert s.run().ok
        got = s.read()  # the session's own buffers, or the caller's: the last pass's outputs either way
    assert all(same(a, b) for a, b in zip(got, exp))
    for n, e in zip(engine.CODE_OUTPUTS, exp):
        flat, out = bufs[n]
        if out is not None:
            assert same(host(out), e) and guards_intact(flat), n
