"""zk_evm_tables_from_block on the device (csrc/k_block_tables.hip): the EVM circuit's tx, block and withdrawal tables from raw block data
— host buffers, inputs resident in HBM with guarded caller-owned outputs and the calldata at odd byte alignments, sessions, and the
chain into the EVM circuit without a host copy — against the plain-Python model of tests/block_tables_ref.py and the CPU backend."""
import itertools
import os

import numpy as np
import pytest

from tests import block_tables_cases as bc
from tests import evm_cases
from zkevm_specs_amd import block_tables as bt, engine, oneshot

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GUARD = 512  # words of -1 on either side of every caller-owned output


def dev(x):
    import torch

    if x is None:
        return None
    x = np.array(x)  # (a writable copy: the shared case arrays are read-only)
    return torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x.view(np.int32) if x.dtype == np.uint32 else x).cuda()


def dev_raw(raw, calldata_shift=0):
    """the raw inputs in HBM; the calldata `calldata_shift` bytes past an aligned address"""
    import torch

    up = {k: dev(np.ascontiguousarray(v) if v is not None else None) for k, v in raw.items() if k != "calldata"}
    n = raw["calldata"].shape[0]
    buf = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    at = (-buf.data_ptr()) % 16 + calldata_shift
    buf[at : at + n] = dev(raw["calldata"])
    up["calldata"] = buf[at : at + n]
    assert n == 0 or up["calldata"].data_ptr() % 16 == calldata_shift
    return up


def guarded(shape, dtype):
    """(flat tensor of -1 with GUARD words around the output, the output's view) in HBM"""
    import torch

    n = int(np.prod(shape))
    flat = torch.full((n + 2 * GUARD,), -1, dtype=torch.int64 if dtype == np.uint64 else torch.int32, device="cuda")
    return flat, flat[GUARD : GUARD + n].view(shape)


def guards_intact(flat):
    return bool((flat[:GUARD] == -1).all()) and bool((flat[-GUARD:] == -1).all())


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def shapes_of(raw):
    return engine.evm_tables_from_block_shapes(raw["tx_fields"].shape[0], raw["calldata"].shape[0], raw["history_hashes"].shape[0],
                                               raw["withdrawals"].shape[0], raw["block"] is not None)


@pytest.mark.parametrize("name", bc.NAMES)
def test_directed_host_buffers(name):
    exp = bc.directed_expected(name)
    res, out = oneshot.evm_tables_from_block(bc.directed_raw(name))
    assert res.ok and res.fail_count == 0 and res.rows_evaluated == exp["tx"].shape[0]
    assert bc.same(out, exp)


@pytest.mark.parametrize("name", bc.NAMES)
def test_directed_resident_inputs_caller_buffers(name):
    import torch

    raw, exp = bc.directed_raw(name), bc.directed_expected(name)
    shapes = shapes_of(raw)
    for shift in (0, 1, 3, 7):
        bufs = {k: guarded(shp, dt) for k, (shp, dt) in shapes.items()}
        with engine.open_evm_tables_from_block(dev_raw(raw, shift), outs={k: v[1] for k, v in bufs.items()}) as s:
            res = s.run()
            torch.cuda.synchronize()
            assert res.ok and res.rows_evaluated == exp["tx"].shape[0]
            got = {k: host(bufs[k][1], shapes[k][1]) for k in bc.OUTPUTS}  # (no cell of the model is all ones: every cell was written)
            assert bc.same(got, exp), shift
            assert all(guards_intact(bufs[k][0]) for k in bc.OUTPUTS), shift
            assert bc.same(s.read(), exp)
            assert not s.read_status().any()
        if raw["calldata"].shape[0] == 0:
            break  # (no calldata: the alignments are one case)


def test_hip_equals_cpu_backend_on_a_skewed_random_block():
    blk, txs, wds = bc.random_block()
    raw = bt.raw_block_data(blk, txs, wds)
    lengths = np.diff(raw["offsets"])
    assert len(txs) == 300 and raw["calldata"].shape[0] == 1 << 16 and lengths.max() >= 8 << 10 and (lengths == 0).sum() >= 50
    cpu = oneshot.evm_tables_from_block(raw, device="cpu")
    hip = oneshot.evm_tables_from_block(raw)
    assert hip[0].ok and hip[0].rows_evaluated == cpu[0].rows_evaluated == 12 * 300 + (1 << 16)
    assert bc.same(hip[1], cpu[1])
    got = bt.tables_from_block(blk, txs, wds, resident=True)  # the mirror's resident form: CUDA tensors
    flat = {"tx": got[0][0], "tx_flags": got[0][1], "block": got[1][0], "block_flags": got[1][1], "withdrawals": got[2]}
    assert all(t.is_cuda for t in flat.values())
    assert bc.same({k: host(flat[k], cpu[1][k].dtype) for k in bc.OUTPUTS}, cpu[1])


def test_two_passes_with_a_byte_and_a_field_changed_in_hbm():
    import torch

    _, blk, txs, wds = bc.case("lengths")
    raw = bc.directed_raw("lengths")
    up = dev_raw(raw, 3)
    with engine.open_evm_tables_from_block(up) as s:
        assert s.run().ok
        assert bc.same(s.read(), bc.directed_expected("lengths"))
        # a zero byte of the 769-byte tx becomes non-zero (its CallData row and the tx's gas cost change), tx 5's nonce becomes p + 6
        off = int(raw["offsets"][11])
        at = off + int(np.flatnonzero(raw["calldata"][off:] == 0)[100])
        up["calldata"][at] = 0x5A
        up["tx_fields"][5, 1] = dev(bc.cells([bc.P + 6]))[0]
        torch.cuda.synchronize()
        txs2 = list(txs)
        data = bytearray(txs[11].call_data)
        data[at - off] = 0x5A
        txs2[11] = _with(txs[11], call_data=bytes(data))
        txs2[5] = _with(txs[5], nonce=bc.P + 6)
        exp2 = bc.ref.model(blk, txs2, wds)
        assert not np.array_equal(exp2["tx"], bc.directed_expected("lengths")["tx"])
        res = s.run()
        assert res.ok and res.launches == 1
        assert bc.same(s.read(), exp2)


def _with(tx, **kw):
    f = dict(id=tx.id, nonce=tx.nonce, gas=tx.gas, gas_price=tx.gas_price, caller_address=tx.caller_address, callee_address=tx.callee_address,
             value=tx.value, call_data=tx.call_data, invalid_tx=tx.invalid_tx, access_list=tx.access_list)
    f.update(kw)
    return bt.Transaction(**f)


@pytest.mark.parametrize("given", list(itertools.product((False, True), repeat=5)))
def test_null_members_of_out_dev(given):
    raw, exp = bc.directed_raw("lengths"), bc.directed_expected("lengths")
    shapes = shapes_of(raw)
    bufs = {k: guarded(*shapes[k]) for k, g in zip(bc.OUTPUTS, given) if g}
    with engine.open_evm_tables_from_block(dev_raw(raw), outs={k: v[1] for k, v in bufs.items()}) as s:
        assert s.run().ok
        got = s.read()  # the session's own buffers, or the caller's: the last pass's outputs either way
    assert bc.same(got, exp)
    for k, (flat, out) in bufs.items():
        assert np.array_equal(host(out, shapes[k][1]), exp[k]) and guards_intact(flat), k


def _golden_case(file, want):
    for name, w, opts, _ in evm_cases.load_cases(os.path.join(GOLDEN, file)):
        if want(w):
            return name, w, opts
    raise AssertionError(f"{file}: no such case")


@pytest.mark.parametrize("file, want", [
    ("evm_begin_tx.npz", lambda w: w["tx"].shape[0] > 0),
    ("evm_calldatacopy.npz", lambda w: w["tx"].shape[0] > 12),           # calldata rows
    ("evm_end_block.npz", lambda w: w["withdrawals"].shape[0] > 0),
    ("evm_blockhash.npz", lambda w: w["block"].shape[0] > 8),            # history hashes
], ids=["begin_tx", "calldatacopy", "end_block", "blockhash"])
def test_chain_into_the_evm_circuit_without_a_host_copy(file, want):
    name, w, opts = _golden_case(file, want)
    w = {k: np.ascontiguousarray(v) for k, v in w.items()}
    with engine.open_evm({k: dev(v) for k, v in w.items()}, bool(opts[0]), bool(opts[1])) as c:  # the golden's own tables
        assert c.run().rows_evaluated == w["steps"].shape[0] - 1
        expected = c.read_status()
    raw, _ = bc.recover_raw(w["tx"], w["block"], w["withdrawals"])
    shapes = shapes_of(raw)
    outs = {k: guarded(*shapes[k])[1] for k in bc.OUTPUTS}
    wire = {k: dev(v) for k, v in w.items() if k not in outs}
    wire.update(outs)
    with engine.open_evm_tables_from_block(dev_raw(raw), outs=outs) as a:
        a.launch()
        with engine.open_evm(wire, bool(opts[0]), bool(opts[1])) as c:  # (same stream: ordered behind the assignment)
            res = c.run()
            status = c.read_status()
        assert a.collect().ok
    assert status.tolist() == expected.tolist(), name
    assert res.fail_count == int((expected != 0).sum())
    for k in bc.OUTPUTS:
        assert np.array_equal(host(outs[k], w[k].dtype), w[k]), k
