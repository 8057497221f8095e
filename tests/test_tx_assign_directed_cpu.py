"""The directed Tx-assign batches (tests/tx_assign_directed.py) on the CPU backend, cell for cell against the plain-Python model
(tests/tx_assign_ref.py), and the key recovery's plain chains (tx_recover_exact, unreachable from inputs) through hostsim."""
import ctypes

import numpy as np
import pytest

from tests import tx_assign_directed as D
from zkevm_specs_amd import oneshot


def _run(b, device="cpu"):
    res, st, w = oneshot.tx_assign(b.tx, b.randomness, device=device)
    D.check_against_model(b, res, st, w)


@pytest.mark.parametrize("name", D.HASH_NAMES)
def test_hash_matrix_batches(name):
    _run(D.hash_batch(name))


def test_recovery_classes():
    _run(D.recovery_batch())


@pytest.mark.parametrize("kind", ["senders", "zeros"])
def test_keccak_set_batches(kind):
    bs = [b for b in D.keccak_batches() if b.name.startswith(f"keccak_{kind}_")]
    assert len(bs) == 21
    for b in bs:
        _run(b)


def test_plain_chains_recover_the_models_keys(hostsim):
    """tx_recover_prepare -> tx_recover_exact -> tx_recover_finish whatever the GLV split says, on the recovery batch: the valid
    txs' keys are the model's, the failing ones keep their status (site 4 included: the plain chains meet at infinity too)"""
    b = D.recovery_batch()
    t = b.tx
    n = t["fields"].shape[0]
    pk, st = np.zeros((n, 8), dtype=np.uint64), np.zeros(n, dtype=np.uint32)
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    fields, to_none, data, off = (np.ascontiguousarray(t[k]) for k in ("fields", "to_is_none", "calldata", "offsets"))
    hostsim.sim_tx_recover_exact.restype = None
    st[:] = 0xEEEEEEEE  # (the entry writes every status)
    hostsim.sim_tx_recover_exact(vp(fields), vp(to_none), vp(data), vp(off), ctypes.c_uint64(n), ctypes.c_uint64(t["chain_id"]), vp(pk), vp(st))
    assert st.tolist() == D.model(b)[0]
    ok, keys = D.recovery_valid_keys()
    assert len(ok) >= 80
    got = [(int.from_bytes(pk[i, :4].tobytes(), "little"), int.from_bytes(pk[i, 4:].tobytes(), "little")) for i in ok]
    assert got == keys
