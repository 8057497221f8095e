"""Directed batches of ecAdd / ecMul / ecPairing calls for the zk_ecc_from_calls tests (CPU and GPU), with assertions on their own
coverage: a batch that stops exercising what it is named for fails here, before any backend is asked.
Calls: adds [(p, q)], muls [(p, s)], pairings [(g1_pts, g2_pts)], G2 tuples in EIP-197 order (x.c1, x.c0, y.c1, y.c0)."""
import functools

from tests import bn254_ref as b
from tests import ecc_calls_ref as ref

P, R = b.P, b.R
W = (1 << 256) - 1
RANDOMNESS = 0x0F1E2D3C4B5A69788796A5B4C3D2E1F00112233445566778899AABBCCDDEEFF % b.FR
O = (0, 0)
G = b.G1
A = b.multiply(G, 5, b.Fq)
B7 = b.multiply(G, 7, b.Fq)
NEG_A = b.neg(A, b.Fq)
OFF = (1, 3)  # y^2 != x^3 + 3
EDGES = (P - 1, P, P + 1, W)
SCALARS = (0, 1, 2, R - 1, R, R + 1, P - 1, P, P + 1, W)


def eip197(q):
    """model point ((x.c0, x.c1), (y.c0, y.c1)) -> the input's word order"""
    return (q[0][1], q[0][0], q[1][1], q[1][0])


Q1 = eip197(b.G2)
Q5 = eip197(b.multiply(b.G2, 5, b.Fq2))
NEG_Q5 = (Q5[0], Q5[1], (-Q5[2]) % P, (-Q5[3]) % P)
O2 = (0, 0, 0, 0)
# EIP-197's published vectors, as the reference's ecPairing tests use them: e(V_P1, V_Q1) e(V_P2, V_Q2) = 1
V_P1 = (0x2CF44499D5D27BB186308B7AF7AF02AC5BC9EEB6A3D147C186B21FB1B76E18DA, 0x2C0F001F52110CCFE69108924926E45F0B0C868DF0E7BDE1FE16D3242DC715F6)
V_P2 = (1, 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD45)
V_Q1 = (0x1FB19BB476F6B9E44E2A32234DA8212F61CD63919354BC06AEF31E3CFAFF3EBC, 0x22606845FF186793914E03E21DF544C34FFE2F2F3504DE8A79D9159ECA2D98D9,
        0x2BD368E28381E8ECCB5FA81FC26CF3F048EEA9ABFDD85D7ED3AB3698D63E4F90, 0x2FE02E47887507ADF0FF1743CBAC6BA291E66F59BE6BD763950BB16041A0A85E)
V_Q2 = (0x1971FF0471B09FA93CAAF13CBF443C1AEDE09CC4328F5A62AAD45F40EC133EB4, 0x091058A3141822985733CBDDDFED0FD8D6C104E9E9EFF40BF5ABFEF9AB163BC7,
        0x2A23AF9A5CE2BA2796C1F4E453A370EB0AF8C212D9DC9ACD8FC02C2E907BAEA2, 0x23A8EB0B0996252CB548A4487DA97B02422EBC0E834613F954DE6C7E0AFDC1FC)
REF_PAIRING_VECTORS = {  # name -> (call, is_valid, out): tests/evm/precompiles/test_ecPairing.py's cases that are whole pairs
    "normal": (([V_P1, V_P2], [V_Q1, V_Q2]), 1, 1),
    "failure_with_valid_input": (([V_P1, V_P1], [V_Q1, V_Q2]), 1, 0),
    "empty_input": (([], []), 1, 1),
    "invalid_input": (([V_P1, (1, 1)], [V_Q1, V_Q2]), 0, 0),
}


@functools.lru_cache(maxsize=None)
def non_subgroup_g2():
    """a point on the twist outside G2 (the twist's cofactor is 2p - r): x = c + u, y from the curve equation"""
    from tests.ecc_cases import fq2_sqrt

    for c in range(1, 100):
        x = (c, 1)
        y = fq2_sqrt(b.Fq2.add(b.Fq2.mul(b.Fq2.mul(x, x), x), b.B2))
        if y is not None and b.multiply((x, y), R, b.Fq2) is not None:
            return eip197((x, y))
    raise AssertionError("no non-subgroup twist point found")


def _with(pt, k, v):
    return tuple(v if j == k else c for j, c in enumerate(pt))


def add_directed():
    d = [("valid", (A, B7)), ("p_inf", (O, A)), ("q_inf", (A, O)), ("both_inf", (O, O)), ("double", (A, A)), ("neg", (A, NEG_A)),
         ("off_p", (OFF, A)), ("off_q", (A, OFF))]
    for k, name in enumerate(("px", "py", "qx", "qy")):
        for e in EDGES:
            words = _with(A + B7, k, e)
            d.append((f"{name}_{'pm1 p pp1 max'.split()[EDGES.index(e)]}", (words[:2], words[2:])))
    return d


def mul_directed():
    d = [(f"s_{k}", (A, s)) for k, s in enumerate(SCALARS)]
    return d + [("p_inf", (O, 12345)), ("off_p", (OFF, 5)), ("px_ge_p", ((1 + P, 2), 5)), ("g_s7", (G, 7))]


def pairing_directed():
    nsg = non_subgroup_g2()
    d = [(name, call) for name, (call, _, _) in REF_PAIRING_VECTORS.items()]
    d += [("one_pair", ([G], [Q1])), ("three_pairs", ([A, NEG_A, O], [Q1, Q1, Q5])), ("bilinear", ([A, G], [Q1, NEG_Q5])),
          ("inf_g1", ([O], [Q1])), ("inf_g2", ([G], [O2])), ("twist_not_g2", ([G], [nsg])), ("off_g1", ([OFF], [Q1])),
          ("bad_first", ([OFF, G, A], [Q1, Q1, Q5])), ("bad_last", ([G, A, G], [Q1, Q5, nsg]))]
    for k in range(6):
        words = _with(G + Q1, k, (G + Q1)[k] + P)
        d.append((f"coord{k}_ge_p", ([words[:2]], [words[2:]])))
    return d


def check_coverage():
    """what the directed lists claim, against the model"""
    adds, muls, prs = dict(add_directed()), dict(mul_directed()), dict(pairing_directed())
    assert len(adds) == 8 + 16 and len(muls) == 10 + 4 and len(prs) == 4 + 9 + 6
    assert ref.add_result(*adds["valid"]) == (True, b.add(A, B7, b.Fq))
    assert ref.add_result(*adds["p_inf"]) == (True, A) and ref.add_result(*adds["q_inf"]) == (True, A)
    assert ref.add_result(*adds["both_inf"]) == (True, O) and ref.add_result(*adds["neg"]) == (True, O)
    assert ref.add_result(*adds["double"]) == (True, b.multiply(G, 10, b.Fq))
    assert ref.add_result(*adds["off_p"]) == (False, O) and ref.add_result(*adds["off_q"]) == (False, O)
    for name, call in adds.items():
        if name[:2] in ("px", "py", "qx", "qy"):
            assert ref.add_result(*call) == (False, O), name  # p - 1 is below the modulus but leaves the curve; the rest fail the range
    for k, s in enumerate(SCALARS):
        ok, out = ref.mul_result(*muls[f"s_{k}"])
        assert ok and out == (b.multiply(A, s, b.Fq) or O)  # the full-width affine chain agrees with s mod r
    assert ref.mul_result(*muls["s_0"])[1] == O and ref.mul_result(*muls["s_4"])[1] == O and ref.mul_result(*muls["s_5"])[1] == A
    assert ref.mul_result(*muls["p_inf"]) == (True, O)
    assert ref.mul_result(*muls["off_p"]) == (False, O) and ref.mul_result(*muls["px_ge_p"]) == (False, O)
    for name, (call, valid, out) in REF_PAIRING_VECTORS.items():
        assert ref.pairing_result(*ref._tup(call)) == (bool(valid), out), name
    assert sorted({len(c[0]) for c in prs.values()}) == [0, 1, 2, 3]
    want = {"one_pair": (True, 0), "three_pairs": (True, 1), "bilinear": (True, 1), "inf_g1": (True, 1), "inf_g2": (True, 1),
            "twist_not_g2": (False, 0), "off_g1": (False, 0), "bad_first": (False, 0), "bad_last": (False, 0)}
    for name, res in want.items():
        assert ref.pairing_result(*ref._tup(prs[name])) == res, name
    nsg = non_subgroup_g2()
    assert b.is_on_curve(b._g2(nsg), b.Fq2, b.B2) and b.multiply(b._g2(nsg), R, b.Fq2) is not None
    for k in range(6):
        assert ref.pairing_result(*ref._tup(prs[f"coord{k}_ge_p"])) == (False, 0)


def _cycle(items, n):
    return [items[k % len(items)][1] for k in range(n)]


SIZES = (1, 63, 64, 65, 257)


@functools.lru_cache(maxsize=None)
def batches():
    """name -> (adds, muls, pairings).  `directed`: every directed call once.  `n<N>`: N calls of each kind, the directed lists
    cycled (so from 63 on every batch holds exact duplicates, and the pairing ops' 0..3 pairs put pair_off across lane 64 inside an
    op).  `adds_only` / `muls_only` / `pairings_only`: a kind alone (null arrays for the others).  `dups`: the same call at the
    front, in the middle and at the end, per kind."""
    check_coverage()
    ad, md, pd = add_directed(), mul_directed(), pairing_directed()
    out = {"directed": ([c for _, c in ad], [c for _, c in md], [c for _, c in pd])}
    for n in SIZES:
        out[f"n{n}"] = (_cycle(ad, n), _cycle(md, n), _cycle(pd, n))
    out["adds_only"] = (_cycle(ad, 3), [], [])
    out["muls_only"] = ([], _cycle(md, 3), [])
    out["pairings_only"] = ([], [], _cycle(pd, 5))
    out["dups"] = ([ad[0][1], ad[4][1], ad[0][1], ad[6][1], ad[0][1]], [md[1][1], md[1][1], md[9][1], md[1][1]],
                   [pd[0][1], pd[4][1], pd[0][1], pd[2][1], pd[2][1]])
    for n in (63, 64, 65, 257):  # an op whose pairs lie on both sides of lane 64 of the per-pair launch
        off = [0]
        for g1s, _ in out[f"n{n}"][2]:
            off.append(off[-1] + len(g1s))
        assert any(lo < 64 < hi for lo, hi in zip(off, off[1:])), n
        assert max(hi - lo for lo, hi in zip(off, off[1:])) <= 3
    m = ref.model(*out["dups"], RANDOMNESS)
    assert m["ecc_table"].shape[0] == 3 + 2 + 3 and m["rows"].shape[0] == 14
    assert ref.model(*out["n65"], RANDOMNESS)["ecc_table"].shape[0] < 3 * 65
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """the model's outputs for a batch, computed once per process and shared (treat as read-only)"""
    return ref.model(*batches()[name], RANDOMNESS)
