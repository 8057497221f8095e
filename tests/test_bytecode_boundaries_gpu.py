"""Directed chunk, batch and round edges of the Bytecode-circuit witness assignment on the device: the wavefront forms of
csrc/k_assign.hip (bca_chunk_wave_kernel, bca_prefix_wave_kernel, bca_rows_wave_kernel) and csrc/k_bytecode_code.hip
(bcc_chunk_wave_kernel), which no CPU test runs, against the plain-Python model (the oracle for the wide values), bit for bit.  The
cases and what they reach: tests/bytecode_boundary_cases.py; the same cases on the CPU backend: tests/test_bytecode_boundaries_cpu.py."""
import numpy as np
import pytest

from tests import bytecode_boundary_cases as bb
from tests import bytecode_code_cases as bc
from zkevm_specs_amd import engine, oneshot

pytestmark = pytest.mark.gpu

GUARD = 512  # int64 words of -1 on either side of every caller-owned output
TWICE = ("ladders", "two_rounds")  # a second pass on the same session: more than one round per bytecode


def same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a.shape == b.shape and np.array_equal(a, b))


def dev(x):
    import torch

    x = x if x.flags.writeable else x.copy()  # (the shared expected arrays are read-only)
    return torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).cuda()


def guarded(shape):
    """(flat tensor of -1 with GUARD words around the output, the output's view) in HBM"""
    import torch

    n = int(np.prod(shape))
    flat = torch.full((n + 2 * GUARD,), -1, dtype=torch.int64, device="cuda")
    return flat, flat[GUARD : GUARD + n].view(shape)


def host(t):
    return t.cpu().numpy().view(np.uint64)


def guards_intact(flat):
    return bool((flat[:GUARD] == -1).all()) and bool((flat[-GUARD:] == -1).all())


def resident_assign(in_rows, offsets, lengths, k, r, exp_rows, passes):
    """zk_bytecode_assign over inputs in HBM into a caller-owned, guarded rows buffer; every pass starts from a buffer of -1"""
    import torch

    flat, out = guarded((12, 1 << k, 4))
    with engine.open_bytecode_assign(dev(in_rows), dev(offsets), dev(lengths), k, r, rows_dev=out) as s:
        for p in range(passes):
            out.fill_(-1)
            res = s.run()
            torch.cuda.synchronize()
            assert res.ok and res.fail_count == 0 and res.rows_evaluated == 1 << k, p
            assert same(host(out), exp_rows), p  # (no cell of the expected rows is all ones: every cell was written)
            assert guards_intact(flat), p
        assert same(s.rows(), exp_rows)


# ---- zk_bytecode_assign
@pytest.mark.parametrize("name", bb.case_names("rows"))
def test_assign_host_buffers(name):
    codes, k, r, exp = bb.case("rows", name)
    offsets, lengths = bb.row_offsets(codes)
    res, rows = oneshot.bytecode_assign(exp[0], offsets, lengths, k, r)
    assert res.ok and res.fail_count == 0 and res.rows_evaluated == 1 << k
    assert same(rows, exp[1])


@pytest.mark.parametrize("name", bb.case_names("rows"))
def test_assign_resident_inputs_caller_rows(name):
    codes, k, r, exp = bb.case("rows", name)
    offsets, lengths = bb.row_offsets(codes)
    resident_assign(exp[0], offsets, lengths, k, r, exp[1], 2 if name in TWICE else 1)


def test_assign_wide_values_at_the_far_edges():
    """field elements that are no bytes around the first batch edge and the round edge: the device scan is exact for every canonical
    value (the host forms fall back to the reference's recurrence)"""
    in_rows, offsets, lengths, k, r, exp_rows = bb.wide_case()
    res, rows = oneshot.bytecode_assign(in_rows, offsets, lengths, k, r)
    assert res.ok and res.rows_evaluated == 1 << k
    assert same(rows, exp_rows)
    resident_assign(in_rows, offsets, lengths, k, r, exp_rows, 2)


# ---- zk_bytecode_from_code
@pytest.mark.parametrize("name", bb.case_names("code"))
def test_from_code_host_buffers(name):
    codes, k, r, exp = bb.case("code", name)
    code, off = bc.pack(list(codes))
    res, table, rows, keccak = oneshot.bytecode_from_code(code, off, k, r)
    assert res.ok and res.fail_count == 0 and res.rows_evaluated == exp[0].shape[0]
    assert same(table, exp[0]) and same(rows, exp[1]) and same(keccak, exp[2])  # (the 66,000- and 131,300-byte codes: the keccak lane-group form)


@pytest.mark.parametrize("name", bb.case_names("code"))
def test_from_code_resident_code_caller_buffers(name):
    import torch

    codes, k, r, exp = bb.case("code", name)
    code, off = bc.pack(list(codes))
    shapes = engine.bytecode_from_code_shapes(len(code), len(codes), k)
    bufs = {n: guarded(shapes[n]) for n in engine.CODE_OUTPUTS}
    with engine.open_bytecode_from_code(dev(code), dev(off), k, r, table_dev=bufs["table"][1], rows_dev=bufs["rows"][1],
                                        keccak_dev=bufs["keccak"][1]) as s:
        for p in range(2 if name in TWICE else 1):
            for n in engine.CODE_OUTPUTS:
                bufs[n][1].fill_(-1)
            res = s.run()
            torch.cuda.synchronize()
            assert res.ok and res.rows_evaluated == exp[0].shape[0], p
            for n, e in zip(engine.CODE_OUTPUTS, exp):
                flat, out = bufs[n]
                assert same(host(out), e), (n, p)
                assert guards_intact(flat), (n, p)


# ---- the chain into the Bytecode circuit over the same buffers, one ladder per form
def test_chain_rows_form_into_the_bytecode_circuit():
    import torch

    codes, k, r, exp = bb.case("rows", "ladder_batch_ladder_a")
    offsets, lengths = bb.row_offsets(codes)
    krows = engine.keccak_table(list(codes), r, engine.KECCAK_MODE_CIRCUIT)
    assert same(krows, exp[2])
    d_rows = torch.full((12, 1 << k, 4), -1, dtype=torch.int64, device="cuda")
    with engine.open_bytecode_assign(dev(exp[0]), dev(offsets), dev(lengths), k, r, rows_dev=d_rows) as a:
        assert a.run().ok
        with engine.open_bytecode(d_rows, dev(krows), r) as c:
            res = c.run()
    assert res.ok and res.fail_count == 0 and res.rows_evaluated == 1 << k
    assert same(host(d_rows), exp[1])


def test_chain_code_form_into_the_bytecode_circuit():
    import torch

    codes, k, r, exp = bb.case("code", "ladder_batch_ladder_a")
    code, off = bc.pack(list(codes))
    d_rows = torch.full((12, 1 << k, 4), -1, dtype=torch.int64, device="cuda")
    d_keccak = torch.full((len(codes), 5, 4), -1, dtype=torch.int64, device="cuda")
    with engine.open_bytecode_from_code(dev(code), dev(off), k, r, rows_dev=d_rows, keccak_dev=d_keccak) as a:
        assert a.run().ok
        with engine.open_bytecode(d_rows, d_keccak, r) as c:
            res = c.run()
    assert res.ok and res.fail_count == 0 and res.rows_evaluated == 1 << k
    assert same(host(d_rows), exp[1]) and same(host(d_keccak), exp[2])
