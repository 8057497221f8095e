"""Exp circuit witness assignment on the MI355X (k_exp_assign.hip): the golden cases through host buffers and into caller buffers in
HBM, the CPU backend bit for bit at size, and events in HBM -> zk_exp_assign_open -> zk_exp_open on the produced rows without a
host step."""
import numpy as np
import pytest

from tests import exp_assign_cases as C
from zkevm_specs_amd import engine, oneshot

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _single_call_cases():
    for c in C.golden_cases():
        fills = [k for k, x in enumerate(c["calls"]) if x == "fill"]
        if c["exc"][0] or (fills and fills != [len(c["calls"]) - 1]):
            continue
        yield c, C.events_of(c["calls"]), (c["max_exp_steps"] if fills else 0)


def test_golden_cases_hip_host_and_device_buffers():
    import torch

    n = 0
    for c, events, mx in _single_call_cases():
        ev = C.events_wire(events)
        res, rows, table = oneshot.exp_assign(ev, mx)
        assert np.array_equal(rows, c["rows"]), c["name"]
        assert C.sorted_table(table) == C.sorted_table(c["table"]), c["name"]
        if rows.shape[1] == 0 or not events:
            continue
        d_ev = _dev(ev)
        n_rows, n_step, n_table = engine.exp_assign_sizes(d_ev, mx)
        assert (n_rows, n_table) == (rows.shape[1], table.shape[0]), c["name"]
        d_rows = torch.full((21, n_rows, 4), -1, dtype=torch.int64, device="cuda")
        d_table = torch.full((n_table, 11, 4), -1, dtype=torch.int64, device="cuda")
        with engine.open_exp_assign(d_ev, mx, d_rows, d_table) as s:
            assert s.run().fail_count == 0
        assert np.array_equal(d_rows.cpu().numpy().view(np.uint64), c["rows"]), c["name"]
        assert np.array_equal(d_table.cpu().numpy().view(np.uint64), table), c["name"]
        n += 1
    assert n >= 30


@pytest.mark.parametrize("n_events, max_bits, empty_every, max_exp_steps", [(1 << 12, 256, 0, 0), (1 << 16, 16, 0, 0), (3000, 256, 3, 250000)])
def test_hip_equals_cpu_backend_at_size(n_events, max_bits, empty_every, max_exp_steps):
    ev = C.random_events_wire(11 + max_bits, n_events, max_bits)
    if empty_every:  # a mix with empty events: every third exponent is 0 or 1
        ev[::empty_every, 3, 0] &= np.uint64(1)
        ev[::empty_every, 3, 1:] = 0
        ev[::empty_every, 4] = 0
    res_c, rows_c, table_c = oneshot.exp_assign(ev, max_exp_steps, device="cpu")
    res_h, rows_h, table_h = oneshot.exp_assign(ev, max_exp_steps)
    assert rows_c.shape[1] >= (1 << 20) and res_h.fail_count == 0 and res_h.rows_evaluated == rows_c.shape[1]
    assert np.array_equal(rows_h, rows_c) and np.array_equal(table_h, table_c)


def test_resident_chain_events_to_exp_circuit():
    import torch

    rng = __import__("random").Random(5)
    events = C.random_events(rng, 300, max_bits=256, empty_share=0.2)
    ev = C.events_wire(events)
    d_ev = _dev(ev)
    n_rows, n_step, n_table = engine.exp_assign_sizes(d_ev, 12000)
    assert n_rows == 84000 > n_step > 30000
    d_rows = torch.zeros((21, n_rows, 4), dtype=torch.int64, device="cuda")
    with engine.open_exp_assign(d_ev, 12000, d_rows, None) as a:
        assert a.run().fail_count == 0
        with engine.open_exp(d_rows) as x:
            res = x.run()
            assert res.fail_count == 0 and res.rows_evaluated == n_rows
        # one d cell (lo half) of a step row overwritten on the device: the rows the CPU backend names fail, and no other
        row = n_step // 2
        d_rows[16, row, 0] += 1
        with engine.open_exp(d_rows) as x:
            res = x.run()
            status = x.read_status()
        res_c, status_c = oneshot.exp_verify(d_rows.cpu().numpy().view(np.uint64), device="cpu")
        assert res_c.fail_count >= 1 and status_c[row] != 0
        assert np.array_equal(status, status_c) and (res.fail_count, res.first_fail_row, res.first_fail_code) == (
            res_c.fail_count, res_c.first_fail_row, res_c.first_fail_code)


def test_block_one_shot_from_exp_events():
    """zk_block_verify on a synth_block trace with block_ops: the six tallies with exp_events (rows and evm.exp derived on the device,
    the assignment on the EVM chain, the Exp circuit's pass ordered behind it) equal the six with exp_rows + evm.exp, clean and with
    one exponent changed in an event — the EVM circuit's exp lookup of that step, and nothing else, fails.  Both forms at once are an
    error, and so is a rejected event, each with its text."""
    import torch

    from zkevm_specs_amd import _lib
    from zkevm_specs_amd.block import stage_block, verify_block_native
    from zkevm_specs_amd.evm_tables import ExecutionState
    from zkevm_specs_amd.super_circuit import BLOCK_CIRCUITS, SuperCircuit, synth_super_block

    p = synth_super_block(16, seed=7)  # (block_ops on: the default weight of the SHA3 / CODECOPY / EXP kinds at this size)
    dev = lambda x: torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x.view(np.int32) if x.dtype == np.uint32 else x).cuda()  # noqa: E731
    assert p["exp_events"].shape[0] >= 3 and p["rows"]["exp"] >= 10
    tally = lambda res: {k: (res[k].fail_count, res[k].first_fail_row, res[k].first_fail_code, res[k].rows_evaluated) for k in BLOCK_CIRCUITS}  # noqa: E731
    want, total_w, _ = verify_block_native(stage_block(p, dev), 0)
    for _ in range(2):
        got, total_g, ends = verify_block_native(stage_block(p, dev, exp_from_events=True), 0)
        assert total_w == total_g == 0 and tally(got) == tally(want) and all(e > 0 for e in ends)
    # the resident form takes the same opt-in
    with SuperCircuit(p, device=0, to_device=dev, exp_from_events=True) as sc:
        sc.launch()
        results, total, first = sc.collect()
    assert total == 0 and results["exp"].rows_evaluated == p["rows"]["exp"]
    # one exponent changed in an event whose exponent has rows: the assigned rows stay a valid Exp witness (of another power), the
    # EXP step that looks the event's first row up no longer finds its operands' exponentiation
    ev = p["exp_events"]
    k = next(i for i in range(ev.shape[0]) if int(ev[i, 3, 0]) > 3 or ev[i, 3, 1:].any() or ev[i, 4].any())
    ev[k, 3, 0] ^= np.uint64(4)
    got, total, _ = verify_block_native(stage_block(p, dev, exp_from_events=True), 0)
    ev[k, 3, 0] ^= np.uint64(4)
    assert total == 1 == got["evm"].fail_count and all(got[c].fail_count == 0 for c in BLOCK_CIRCUITS if c != "evm")
    assert int(p["evm"]["steps"][got["evm"].first_fail_row, 0, 0]) == int(ExecutionState.EXP)
    # both forms at once, and a rejected event
    b = stage_block(p, dev, exp_from_events=True)
    b["exp_rows"] = dev(p["exp_rows"])
    with pytest.raises(_lib.EngineError, match="exp_events given together"):
        verify_block_native(b, 0)
    old = ev[1, 0].copy()
    ev[1, 0] = ev[0, 0]
    try:
        if ev[0, 3, 0] > 1 and ev[1, 3, 0] > 1:
            with pytest.raises(_lib.EngineError, match="identifier of event 1") as ei:
                verify_block_native(stage_block(p, dev, exp_from_events=True), 0)
            assert ei.value.rc == _lib.ERR_EXP_ORDER
    finally:
        ev[1, 0] = old
    got, total, _ = verify_block_native(stage_block(p, dev, exp_from_events=True), 0)  # every chain ended: the next block verifies again
    assert total == 0 and tally(got) == tally(want)
