"""ECC circuit (ecAdd / ecMul / ecPairing rows) on the CPU backend behind the C ABI (libzkevm_cpu.so: csrc/ecc_circuit.hpp compiled
for the host) against the plain-Python BN254 model tests/bn254_ref.py, and the model's own self-checks."""
import numpy as np
import pytest

from tests import bn254_ref as b
from tests.ecc_cases import fq12_tower_mul, golden_cases, random_point_ops, rng, rows_to_ints
from zkevm_specs_amd import oneshot
from zkevm_specs_amd.flatten import flatten_ecc_ops

CPU = "cpu"
R_KECCAK = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF % b.R


def test_model_bilinearity():
    a, c = 11, 29
    e_ab = b.pairing(b.multiply(b.G2, c, b.Fq2), b.multiply(b.G1, a, b.Fq))
    assert e_ab == b.pairing(b.G2, b.multiply(b.G1, a * c, b.Fq))
    assert e_ab == b.f12_pow(b.pairing(b.G2, b.G1), a * c)
    assert e_ab != b.ONE12


def test_model_eip197_vectors():
    p1 = (0x2CF44499D5D27BB186308B7AF7AF02AC5BC9EEB6A3D147C186B21FB1B76E18DA,
          0x2C0F001F52110CCFE69108924926E45F0B0C868DF0E7BDE1FE16D3242DC715F6)
    p2 = (1, 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD45)
    q1 = ((0x22606845FF186793914E03E21DF544C34FFE2F2F3504DE8A79D9159ECA2D98D9,
           0x1FB19BB476F6B9E44E2A32234DA8212F61CD63919354BC06AEF31E3CFAFF3EBC),
          (0x2FE02E47887507ADF0FF1743CBAC6BA291E66F59BE6BD763950BB16041A0A85E,
           0x2BD368E28381E8ECCB5FA81FC26CF3F048EEA9ABFDD85D7ED3AB3698D63E4F90))
    q2 = ((0x091058A3141822985733CBDDDFED0FD8D6C104E9E9EFF40BF5ABFEF9AB163BC7,
           0x1971FF0471B09FA93CAAF13CBF443C1AEDE09CC4328F5A62AAD45F40EC133EB4),
          (0x23A8EB0B0996252CB548A4487DA97B02422EBC0E834613F954DE6C7E0AFDC1FC,
           0x2A23AF9A5CE2BA2796C1F4E453A370EB0AF8C212D9DC9ACD8FC02C2E907BAEA2))
    assert b.is_on_curve(q1, b.Fq2, b.B2) and b.is_on_curve(q2, b.Fq2, b.B2)
    assert b.pairing_product_is_one([(p1, q1), (p2, q2)])
    assert not b.pairing_product_is_one([(p1, q1), (p1, q2)])
    # (x, 0) doubles to (-2x, 0) in py_ecc's affine chain
    assert b.double((5, 0), b.Fq) == ((-10) % b.P, 0)


@pytest.mark.parametrize("m, w, rows, assigned, status, r", [pytest.param(*c, id=c[0]["name"]) for c in golden_cases()])
def test_golden_case_cpu(m, w, rows, assigned, status, r):
    got = oneshot.ecc_assign(w, r, device=CPU)
    assert np.array_equal(got, assigned)
    res, st = oneshot.ecc_verify(w, rows, r, device=CPU)
    assert st.tolist() == status.tolist()
    fails = [i for i, c in enumerate(status.tolist()) if c]
    assert res.fail_count == len(fails)
    if fails:
        assert res.first_fail_row == fails[0] and res.first_fail_code == status[fails[0]]
    if m["expect_success"] is not None:
        assert (res.fail_count == 0) == m["expect_success"]
    if m.get("ref_outcome") is not None:  # the unmodified reference (add / mul) raised exactly when a row fails here
        assert (m["ref_outcome"] == "") == (res.fail_count == 0)


def test_random_point_rows_cpu():
    g = rng(7)
    adds, muls = random_point_ops(g, 2000, 300)
    w = flatten_ecc_ops(adds, muls, [])
    rows = oneshot.ecc_assign(w, R_KECCAK, device=CPU)
    exp_rows = b.assign_rows(adds, muls, [], R_KECCAK)
    assert rows_to_ints(rows) == exp_rows
    # tamper a few hundred cells: flipped is_valid, outputs, op types, words
    rows_t = rows.copy()
    ints = [list(r) for r in exp_rows]
    for i in g.sample(range(len(ints)), 300):
        c = g.choice([0, 1, 5, 8, 9, 10, 11, 12])
        v = g.choice([0, 1, 2, 3, g.randrange(1 << 64)])
        ints[i][c] = v
        rows_t[i, c] = [v, 0, 0, 0]
    _, st = oneshot.ecc_verify(w, rows_t, R_KECCAK, device=CPU)
    exp = b.verify_status(adds, muls, [], ints, R_KECCAK)
    assert st.tolist() == exp
    assert sum(1 for c in exp if c) > 300 and sum(1 for c in exp if not c) > 300


def test_pairing_rows_cpu():
    g = rng(3)
    F, F2 = b.Fq, b.Fq2
    ops = []
    for _ in range(4):  # e(aG1, G2) e(-G1, aG2) == 1 and a perturbed copy
        a = g.randrange(1, b.R)
        pa, qa = b.multiply(b.G1, a, F), b.multiply(b.G2, a, F2)
        q1 = (b.G2[0][1], b.G2[0][0], b.G2[1][1], b.G2[1][0])
        qa_w = (qa[0][1], qa[0][0], qa[1][1], qa[1][0])
        ops.append(([pa, b.neg(b.G1, F)], [q1, qa_w], 1))
        ops.append(([pa, b.G1], [q1, qa_w], g.choice([0, 1])))
    w = flatten_ecc_ops([], [], ops)
    rows = oneshot.ecc_assign(w, R_KECCAK, device=CPU)
    exp_rows = b.assign_rows([], [], ops, R_KECCAK)
    assert rows_to_ints(rows) == exp_rows
    _, st = oneshot.ecc_verify(w, rows, R_KECCAK, device=CPU)
    assert st.tolist() == b.verify_status([], [], ops, exp_rows, R_KECCAK)
    assert st[0] == 0 and st[2] == 0


def test_fr_op_fq_and_fq12_cpu():
    from zkevm_specs_amd import _lib

    lib = _lib.init(CPU)
    g = rng(5)
    n = 24
    a = [g.randrange(b.P) for _ in range(n)]
    c = [g.randrange(b.P) for _ in range(n)]

    def arr(v):
        return np.array([[(x >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for x in v], dtype=np.uint64)

    out = np.zeros((n, 4), dtype=np.uint64)
    xa, xc = arr(a), arr(c)  # kept alive across the calls
    assert lib.zk_fr_op(18, _lib.ptr(xa), _lib.ptr(xc), _lib.ptr(out), n, 0) == 0
    assert [sum(int(x[k]) << (64 * k) for k in range(4)) for x in out] == [x * y % b.P for x, y in zip(a, c)]
    assert lib.zk_fr_op(19, _lib.ptr(xa), _lib.ptr(xc), _lib.ptr(out), n, 0) == 0
    got = [sum(int(x[k]) << (64 * k) for k in range(4)) for x in out]
    assert got == fq12_tower_mul(a[:12], c[:12]) + fq12_tower_mul(a[12:], c[12:])

