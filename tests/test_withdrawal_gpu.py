"""Withdrawal circuit on the MI355X (k_withdrawal.hip): status codes and tallies against the golden cases and the CPU backend, the
device assignment's digests against the host keccak, and row-sharded sessions over the +-1-row halo."""
import random

import numpy as np
import pytest

from tests import withdrawal_ref as W
from tests.withdrawal_cases import big_witness, golden_cases, ints, tamper_cells
from zkevm_specs_amd import engine, oneshot
from zkevm_specs_amd.distributed import shard_rows

pytestmark = pytest.mark.gpu
R = 0x5EED0F0A11D0E5C0FFEE5EED0F0A11D0E5C0FFEE5EED0F0A11D0E5 % W.P
N = 1 << 16


def test_golden_cases_hip():
    n = 0
    for m, w, status, r in golden_cases():
        res, st = oneshot.withdrawal_verify(w, r)
        assert st.tolist() == status.tolist(), m["name"]
        fails = [i for i, c in enumerate(status.tolist()) if c]
        assert res.fail_count == len(fails), m["name"]
        if fails:
            assert (res.first_fail_row, res.first_fail_code) == (fails[0], status[fails[0]]), m["name"]
        n += 1
    assert n >= 60


def test_bench_size_tampered_hip_vs_cpu():
    """2^16 rows with ~1,000 tampered cells: per-row statuses bit-identical to the CPU backend"""
    w, _ = big_witness(N, seed=21, r=R, device="cpu")
    w["rows"] = tamper_cells(w["rows"], np.random.default_rng(5), 1000)
    res_h, st_h = oneshot.withdrawal_verify(w, R)
    res_c, st_c = oneshot.withdrawal_verify(w, R, device="cpu")
    assert np.array_equal(st_h, st_c)
    assert 500 < res_h.fail_count == res_c.fail_count
    assert (res_h.first_fail_row, res_h.first_fail_code) == (res_c.first_fail_row, res_c.first_fail_code)


def test_device_assignment_digests_and_clean_verify():
    """zk_withdrawal_assign of 2^16 withdrawals on the device: rows and keccak rows equal the CPU backend's, a sample of digests and
    RLCs equals the Python keccak / model, and the assigned witness verifies clean on the device"""
    w, inp = big_witness(N, seed=22, r=R, device=None)
    rows_c, k_c = oneshot.withdrawal_assign(inp, N, R, device="cpu")
    assert np.array_equal(w["rows"], rows_c)
    assert np.array_equal(w["keccak"][1:], k_c)
    g = random.Random(3)
    ins = ints(inp)
    for i in [0, N - 1] + [g.randrange(N) for _ in range(254)]:
        fields = ins[i][:4]
        data = W.rlp_list(fields)
        assert ints(w["rows"][i:i + 1])[0][4:6] == W.digest_word(data), i
        assert ints(w["keccak"][i + 1:i + 2])[0] == (1, W.rlc(data, R), len(data)) + W.digest_word(data), i
    res, st = oneshot.withdrawal_verify(w, R)
    assert res.fail_count == 0 and not st.any(), (res.first_fail_row, hex(res.first_fail_code))
    # padding past the withdrawals: the assignment appends (0, 0, 0, 0, Word(0), last root) rows
    rows_p, _ = oneshot.withdrawal_assign(inp[:100], 128, R)
    rows_pc, _ = oneshot.withdrawal_assign(inp[:100], 128, R, device="cpu")
    assert np.array_equal(rows_p, rows_pc) and not rows_p[100:, :6].any()


def test_two_row_sharded_sessions_tally_like_one():
    w, _ = big_witness(N, seed=23, r=R, device="cpu")
    w["rows"] = tamper_cells(w["rows"], np.random.default_rng(6), 300)
    with engine.open_withdrawal(w, R) as s:
        whole = s.run()
        st_whole = s.read_status()
    tot, first, sts = 0, [], []
    for rank in range(2):
        rows, _, lo_l, hi_l, lo = shard_rows(w["rows"], None, rank, 2, "withdrawal", w["max_withdrawals"], w["total_rows"])
        with engine.open_withdrawal(dict(w, rows=rows, row_base=lo - lo_l), R) as s:
            s.set_range(lo_l, hi_l)
            r = s.run()
            sts.append(s.read_status()[lo_l:hi_l])
        tot += r.fail_count
        if r.fail_count:
            first.append((r.first_fail_row - lo_l + lo, r.first_fail_code))
    assert whole.fail_count == tot > 0
    assert (whole.first_fail_row, whole.first_fail_code) == min(first)
    assert np.array_equal(np.concatenate(sts), st_whole)
