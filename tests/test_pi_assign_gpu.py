"""PI circuit witness assignment on the device (csrc/k_pi_assign.hip) against the goldens, the CPU backend at 3.3 x 10^5 rows, and the
resident chain assign -> copy constraints -> gates on device pointers."""
import random

import numpy as np
import pytest

from tests import pi_assign_cases as C
from zkevm_specs_amd import _lib, engine, oneshot, pi_circuit

pytestmark = pytest.mark.gpu
GOLD = C.load()
CASES = C.build_cases()
VALID = [c for c in CASES if c[3] is None]
BIG = (1 << 9, 1 << 17, 1 << 8)


def to_device(pd):
    import torch

    conv = lambda a: torch.from_numpy(a.view({8: np.int64, 4: np.int32, 1: np.uint8}[a.dtype.itemsize])).cuda()  # noqa: E731
    return {k: (conv(v) if k in engine.PI_ASSIGN_INPUTS else v) for k, v in pd.items()}


@pytest.mark.parametrize("case", VALID, ids=[c[0] for c in VALID])
def test_hip_equals_goldens(case):
    name, pd, shape, _ = case
    res, wire = oneshot.pi_assign(pi_circuit.public_data_inputs(pd, *shape))
    assert res.ok and res.rows_evaluated == wire["rows"].shape[1]
    C.check_against_golden(wire, GOLD[name])


def big_public_data(kind):
    rng = random.Random(5 + len(kind))
    if kind == "one_tx_spans_many_tiles":
        lens = [7, 90000, 0, 3] + C._split(rng, 30000, 200)
    elif kind == "many_empty_txs":
        lens = [0 if k % 3 else rng.randrange(600) for k in range(BIG[0])]
    else:
        lens = C._split(rng, BIG[1], 300)  # fills MAX_CALLDATA_BYTES exactly
    return C.rand_public_data(rng, len(lens), lens, BIG[2], random_hashes=True)


@pytest.mark.parametrize("kind", ["full", "one_tx_spans_many_tiles", "many_empty_txs"])
def test_hip_equals_cpu_backend_large(kind):
    pd = pi_circuit.public_data_inputs(big_public_data(kind), *BIG)
    _, cpu = oneshot.pi_assign(pd, device="cpu")
    res, hip = oneshot.pi_assign(pd)
    assert res.ok and hip["rows"].shape[1] == 8454 + 336 * BIG[0] + BIG[1] + 56 * BIG[2]
    for k in engine.PI_ASSIGN_OUTPUTS:
        assert np.array_equal(cpu[k], hip[k]), (kind, k)


def test_resident_chain_and_second_launch():
    import torch

    pd = pi_circuit.public_data_inputs(big_public_data("one_tx_spans_many_tiles"), *BIG)
    _, host = oneshot.pi_assign(pd)
    host_gate, _ = oneshot.pi_verify(host["rows"], host["keccak"], host["gas"], host["rows"].shape[1])
    host_copy, _ = oneshot.pi_copy_verify(host["cc_cells"], host["cc_bytes"], host["cc_lens"])
    copy_res, gate_res = pi_circuit.verify_public_data(to_device(pd))
    assert copy_res.fail_count == 0 and gate_res.fail_count == 0
    assert (copy_res.fail_count, copy_res.rows_evaluated, gate_res.fail_count, gate_res.rows_evaluated) == \
        (host_copy.fail_count, host_copy.rows_evaluated, host_gate.fail_count, host_gate.rows_evaluated)
    # a second zk_launch of one session gives identical outputs
    with engine.open_pi_assign(to_device(pd)) as s:
        assert s.run().ok
        first = s.read()
        assert s.run().ok
        second = s.read()
        assert not s.read_status().any()
    for k in engine.PI_ASSIGN_OUTPUTS:
        assert np.array_equal(first[k], second[k]) and np.array_equal(first[k], host[k]), k
    torch.cuda.synchronize()


def test_rejects_return_their_codes():
    by = {c[0]: c for c in CASES}
    want = {"rej_no_txs": _lib.ERR_PI_TXS, "rej_too_many_txs": _lib.ERR_PI_TXS, "rej_no_withdrawals": _lib.ERR_PI_WITHDRAWALS,
            "rej_too_many_withdrawals": _lib.ERR_PI_WITHDRAWALS, "rej_calldata": _lib.ERR_PI_CALLDATA, "rej_coinbase_wide": _lib.ERR_PI_FIELD,
            "rej_number_wide": _lib.ERR_PI_FIELD, "rej_nonce_wide": _lib.ERR_PI_FIELD, "rej_to_addr_wide": _lib.ERR_PI_FIELD,
            "rej_amount_wide": _lib.ERR_PI_FIELD}
    for name, rc in want.items():
        _, pd, shape, _ = by[name]
        inputs = pi_circuit.public_data_inputs(pd, *shape)
        for form in (inputs, to_device(inputs)):
            with pytest.raises(_lib.EngineError) as e:
                engine.open_pi_assign(form)  # refused at open: no session, no pass
            assert e.value.rc == rc, name


def test_rejects_2p31_rows():
    """circuit_len >= 2^31: ZK_ERR_PI_ROWS from sizes and from open, host and device forms, before anything is allocated"""
    from tests.test_pi_assign_cpu import ROWS_REJECTS

    _, pd, _, _ = VALID[0]
    for label, shape in ROWS_REJECTS.items():
        inputs = pi_circuit.public_data_inputs(pd, *shape)
        for form in (inputs, to_device(inputs)):
            for call in (engine.pi_assign_sizes, engine.open_pi_assign):
                with pytest.raises(_lib.EngineError) as e:
                    call(form)
                assert e.value.rc == _lib.ERR_PI_ROWS, label
