"""ECC circuit on the MI355X (k_ecc.hip): status codes, tallies and assigned rows against the oracle (tests/golden/ecc_cases.npz,
tests/bn254_ref.py) and the CPU backend; the EccTableRows of the EVM fixtures; the zk_fr_op Fq / Fq12 known-answer hooks."""
import numpy as np
import pytest

from tests import bn254_ref as b
from tests.ecc_cases import fq12_tower_mul, golden_cases, ops_from_table_rows, random_point_ops, rng, rows_to_ints
from zkevm_specs_amd import oneshot
from zkevm_specs_amd.flatten import flatten_ecc_ops

pytestmark = pytest.mark.gpu
R_KECCAK = 0x0DDBA11CAFE0DDBA11CAFE0DDBA11CAFE0DDBA11CAFE0DDBA11CAFE % b.R


def test_golden_cases_hip():
    n = 0
    for m, w, rows, assigned, status, r in golden_cases():
        assert np.array_equal(oneshot.ecc_assign(w, r), assigned), m["name"]
        res, st = oneshot.ecc_verify(w, rows, r)
        assert st.tolist() == status.tolist(), m["name"]
        fails = [i for i, c in enumerate(status.tolist()) if c]
        assert res.fail_count == len(fails), m["name"]
        if fails:
            assert (res.first_fail_row, res.first_fail_code) == (fails[0], status[fails[0]]), m["name"]
        n += 1
    assert n >= 75


def test_bench_size_tampered_hip_vs_cpu():
    """2^14 adds, 2^12 muls, 2^10 two-pair pairings with a few hundred tampered cells over all three row kinds: HIP == CPU backend"""
    g = rng(11)
    adds, muls = random_point_ops(g, 1 << 8, 1 << 6)
    adds = [adds[i % len(adds)] for i in range(1 << 14)]
    muls = [muls[i % len(muls)] for i in range(1 << 12)]
    a, q1 = b.multiply(b.G1, 12345, b.Fq), (b.G2[0][1], b.G2[0][0], b.G2[1][1], b.G2[1][0])
    qa = b.multiply(b.G2, 12345, b.Fq2)
    qa_w = (qa[0][1], qa[0][0], qa[1][1], qa[1][0])
    pairs = [([a, b.neg(b.G1, b.Fq)], [q1, qa_w], 1), ([a, b.G1], [q1, qa_w], 0)]
    pairs = [pairs[i % 2] for i in range(1 << 10)]
    w = flatten_ecc_ops(adds, muls, pairs)
    rows = oneshot.ecc_assign(w, R_KECCAK)
    assert np.array_equal(rows, oneshot.ecc_assign(w, R_KECCAK, device="cpu"))
    n = rows.shape[0]
    for _ in range(300):
        i = g.randrange(n)
        c = g.choice([0, 1, 3, 5, 7, 9, 10, 11, 12])
        rows[i, c] = [g.choice([0, 1, 2, 3, g.randrange(1 << 64)]), 0, 0, 0]
    res, st = oneshot.ecc_verify(w, rows, R_KECCAK)
    res_c, st_c = oneshot.ecc_verify(w, rows, R_KECCAK, device="cpu")
    assert st.tolist() == st_c.tolist()
    assert (res.fail_count, res.first_fail_row, res.first_fail_code) == (res_c.fail_count, res_c.first_fail_row, res_c.first_fail_code)
    np1 = (1 << 14) + (1 << 12)
    assert st[:1 << 14].any() and st[1 << 14:np1].any() and st[np1:].any()


@pytest.mark.parametrize("name", ["evm_ecAdd", "evm_ecMul"])
def test_evm_fixture_ecc_rows_hip(golden_dir, name):
    import os

    g = np.load(os.path.join(golden_dir, name + ".npz"))
    tab = np.concatenate([g[k] for k in g.files if k.endswith("_ecc")])
    tab = np.unique(tab.reshape(tab.shape[0], -1), axis=0).reshape(-1, 13, 4)
    adds, muls = ops_from_table_rows(tab)
    assert adds or muls
    w = flatten_ecc_ops(adds, muls, [])
    kinds = [1] * len(adds) + [2] * len(muls)
    ordered = [r for k in (1, 2) for r in tab if int(r[0, 0]) == k]
    rows = np.array(ordered, dtype=np.uint64).reshape(-1, 13, 4)
    assert [int(r[0, 0]) for r in rows] == kinds
    _, st = oneshot.ecc_verify(w, rows, R_KECCAK)
    assert st.tolist() == b.verify_status(adds, muls, [], rows_to_ints(rows), R_KECCAK)


def test_fr_op_fq_fq12_hip():
    from zkevm_specs_amd import _lib

    lib = _lib.init()
    g = rng(9)
    n = 48
    a = [g.randrange(b.P) for _ in range(n)]
    c = [g.randrange(b.P) for _ in range(n)]

    def arr(v):
        return np.array([[(x >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for x in v], dtype=np.uint64)

    def ints(o):
        return [sum(int(x[k]) << (64 * k) for k in range(4)) for x in o]

    out = np.zeros((n, 4), dtype=np.uint64)
    xa, xc = arr(a), arr(c)  # kept alive across the calls
    _lib.check(lib.zk_fr_op(18, _lib.ptr(xa), _lib.ptr(xc), _lib.ptr(out), n, 0), "zk_fr_op 18")
    assert ints(out) == [x * y % b.P for x, y in zip(a, c)]
    _lib.check(lib.zk_fr_op(19, _lib.ptr(xa), _lib.ptr(xc), _lib.ptr(out), n, 0), "zk_fr_op 19")
    exp = []
    for k in range(0, n, 12):
        exp += fq12_tower_mul(a[k:k + 12], c[k:k + 12])
    assert ints(out) == exp
