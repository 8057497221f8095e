"""The directed Tx-assign batches (tests/tx_assign_directed.py) on the MI355X, bit for bit against the plain-Python model
(tests/tx_assign_ref.py) — never against the CPU backend, which is the same headers compiled for the host: every lane form of the
key recovery, batch sizes that leave a wavefront partly filled, the chunked launch above 2^17 lanes, the keccak-set kernels at
their tile and block edges, and device-pointer inputs at every calldata alignment with a second launch of the same session."""
import numpy as np
import pytest

from tests import tx_assign_directed as D
from zkevm_specs_amd import engine, oneshot

pytestmark = pytest.mark.gpu
LANES = ["1", "2", "4"]


def _run(b):
    res, st, w = oneshot.tx_assign(b.tx, b.randomness)
    D.check_against_model(b, res, st, w)


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("name", D.HASH_NAMES)
def test_hash_matrix_batches_every_lane_form(name, lanes, monkeypatch):
    monkeypatch.setenv("ZK_ECDSA_LANES", lanes)
    _run(D.hash_batch(name))


@pytest.mark.parametrize("lanes", LANES)
def test_recovery_classes_every_lane_form(lanes, monkeypatch):
    monkeypatch.setenv("ZK_ECDSA_LANES", lanes)
    _run(D.recovery_batch())


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 65])
def test_ragged_batch_sizes_every_lane_form(n, lanes, monkeypatch):
    """n txs at 1, 2 or 4 lanes each leave the last wavefront partly without a tx: those lanes carry the point at infinity into the
    cross-lane exchanges, next to failing txs of every site"""
    monkeypatch.setenv("ZK_ECDSA_LANES", lanes)
    _run(D.truncated(D.recovery_batch(), n))


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("kind", ["senders", "zeros"])
def test_keccak_set_batches_every_lane_form(kind, lanes, monkeypatch):
    """tx_keccak_first_kernel / tx_keccak_rank_kernel with m = n + 1 across 256 and 512: duplicates in the lane's own tile, in an
    earlier tile only, across the block edge (255 | 256), all-zero candidates at the edges, and — randomness 1 and 0 — every
    prefix equal, so that the full-row comparison alone decides the order"""
    monkeypatch.setenv("ZK_ECDSA_LANES", lanes)
    for b in D.keccak_batches():
        if b.name.startswith(f"keccak_{kind}_"):
            _run(b)


def test_chunked_launch_of_the_recovery(monkeypatch):
    """n = 2^15 + 67 txs at four lanes each: 2^17 lanes fill the first launch of the recovery, the second starts at tx 2^15 — at
    another phase of the 67-tx pattern (failing txs of sites 1, 3 and 4 among them).  Every status, the units, every tx-table row
    and the keccak table (the valid senders among the 67, each 490 times, and the zero row) against the model.  Host side
    (tiling the inputs, the model's wire): 6.5 s measured on a CPU-only build host; the whole test took 2.6 s beside the MI355X."""
    n = (1 << 15) + 67
    b = D.tiled(D.truncated(D.recovery_batch(), 67), n)
    status, wire = D.model(b)
    senders = {bytes(wire["bytes"][i, :2].tobytes()) for i in range(67) if status[i] == 0}
    assert {x & 0xFF for x in status[:67] if x} == {1, 3, 4} and (1 << 15) % 67 != 0
    assert wire["keccak"].shape[0] == len(senders) + 1  # (the model's set: what the batch aims at)
    monkeypatch.setenv("ZK_ECDSA_LANES", "4")
    res, st, w = oneshot.tx_assign(b.tx, b.randomness)
    D.check_against_model(b, res, st, w)


@pytest.mark.parametrize("lead", [0, 1, 3, 7])
def test_device_pointers_at_every_calldata_alignment_and_relaunch(lead):
    """device-pointer inputs are used in place: the calldata starts `lead` bytes past an aligned address (the reader takes whole
    aligned words, so the buffer keeps 8 spare bytes at both ends); a second launch of the session gives the same wire and the same
    number of keccak rows (the count is cleared and the first-occurrence flags rewritten per launch)"""
    torch = pytest.importorskip("torch")
    b = D.hash_batch("hash_matrix")
    t = b.tx
    dev = torch.device("cuda")
    to_dev = lambda a: torch.from_numpy(a.view({8: np.int64, 4: np.int32, 1: np.uint8}[a.dtype.itemsize])).to(dev)  # noqa: E731
    total = int(t["offsets"][-1])
    buf = torch.full((8 + 8 + total + 8,), 0xA5, dtype=torch.uint8, device=dev)
    view = buf[8 + lead : 8 + lead + total]
    view.copy_(to_dev(t["calldata"]))
    assert view.data_ptr() % 8 == lead
    td = dict(t, fields=to_dev(t["fields"]), to_is_none=to_dev(t["to_is_none"]), offsets=to_dev(t["offsets"]), calldata=view)
    with engine.open_tx_assign(td, b.randomness) as s:
        counts = []
        for _ in range(2):
            res = s.run()
            st = s.read_status()
            w = s.read()
            counts.append(s.n_keccak())
            D.check_against_model(b, res, st, w)
    assert counts[0] == counts[1] == D.model(b)[1]["keccak"].shape[0]
    torch.cuda.synchronize()
    assert bool((buf[: 8 + lead] == 0xA5).all()) and bool((buf[8 + lead + total :] == 0xA5).all())
