"""Cases of the Sig circuit's witness assignment (zk_sig_assign) shared by tests/test_sig_assign_cpu.py and tests/test_sig_assign_gpu.py:
the inputs behind the reference's fixtures (tests/golden/sign_cases.npz `sig:` cases, tests/golden/evm_ecRecover.npz), read back from
the fixtures' own wire, and batches built with the model's ECDSA (tests/sig_assign_ref.py)."""
import functools
import os
import random

import numpy as np

from tests import sig_assign_ref as M
from tests.dropin_cases import sign_cases
from tests.evm_cases import load_cases
from zkevm_specs_amd import engine
from zkevm_specs_amd.wire import cells_to_ints

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N, P, G = M.N, M.P, M.G
BAD = M.BAD
WIRE_KEYS = engine.SIG_ASSIGN_OUTPUTS

# The Sig fixtures a witness builder can reach from signed data.  The reference's other untampered `sig:` cases edit the witness
# after building it and are left out: 5 of 8.
SIG_REACHABLE = ("sig:test_sig_verify", "sig:test_sig_incorrect_signature", "sig:test_sig_incorrect_address")
SIG_EDITED_AFTER_BUILDING = ("sig:test_sig_inconsistent_msg_hash", "sig:test_sig_inconsistent_pub_key_hash", "sig:test_sig_incorrect_keccak",
                             "sig:test_sig_incorrect_msg_hash", "sig:test_sig_incorrect_signature_v")
SIG_REF_KIND = {"sig:test_sig_verify": [0] * 10, "sig:test_sig_incorrect_signature": [1] * 10, "sig:test_sig_incorrect_address": [1]}


def words(vals):
    """ints -> uint64[len, 4] little-endian words"""
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in vals), dtype="<u8").reshape(-1, 4).copy()


def pack(entries, v_offset=0, addr=True, expect_valid=True):
    """entries: (hash bytes, v, r, s, claimed addr, expect_valid) -> the dict of engine._sig_assign_args"""
    n = len(entries)
    f = words([x for e in entries for x in (int.from_bytes(e[0], "little"), e[1], e[2], e[3])]).reshape(n, 4, 4)
    return {"fields": f, "addr": words([e[4] for e in entries]) if addr else None,
            "expect_valid": np.array([e[5] for e in entries], dtype=np.uint32) if expect_valid else None, "v_offset": v_offset}


def model(sig, randomness):
    return M.assign(sig["fields"], sig["addr"], sig["expect_valid"], sig["v_offset"], randomness)


# ---- the reference's fixtures ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sig_fixture_cases():
    """-> [(name, sig inputs read from the fixture's wire, randomness, the fixture)]"""
    out = []
    for name, c in sign_cases():
        if name not in SIG_REACHABLE:
            continue
        n = c["bytes"].shape[0]
        le = lambda row: int.from_bytes(bytes(row.tolist()), "little")  # noqa: E731
        f = words([x for i in range(n) for x in (le(c["bytes"][i, 5]), int(c["meta"][i, 3]), le(c["bytes"][i, 7]), le(c["bytes"][i, 8]))])
        sig = {"fields": f.reshape(n, 4, 4), "addr": np.ascontiguousarray(c["cells"][0]), "expect_valid": None, "v_offset": 0}
        out.append((name, sig, cells_to_ints(c["r"].reshape(1, 4))[0], c))
    return out


ECRECOVER_CASES = (0, 4, 8, 12, 16, 20, 24)  # the un-fuzzed ones (the fuzzed variants' aux cells are not 128-bit words)
ECRECOVER_ZERO_ADDR = 4                      # the reference's `zero_addr` case


@functools.lru_cache(maxsize=None)
def ecrecover_fixture_cases():
    """-> {index: (sig inputs from aux cells 0 - 7 with v_offset 27, randomness = aux cell 11, wire, opts, ref_kind)}"""
    out = {}
    for i, (name, w, opts, ref_kind) in enumerate(load_cases(os.path.join(GOLDEN, "evm_ecRecover.npz"))):
        if i not in ECRECOVER_CASES:
            continue
        assert "#fuzz" not in name and int(w["aux_kind"][0]) == 5
        a = cells_to_ints(w["aux"][0])
        f = words([a[2 * k] | (a[2 * k + 1] << 128) for k in range(4)]).reshape(1, 4, 4)
        out[i] = ({"fields": f, "addr": None, "expect_valid": None, "v_offset": 27}, a[11], w, opts, ref_kind)
    return out


# ---- batches from the model's ECDSA ---------------------------------------------------------------------------------------
def _hash(rng):
    return bytes(rng.getrandbits(8) for _ in range(32))


def signed(rng, sk, hb=None, k=None, v_offset=0):
    """a valid entry: hash, v, r, s, the signer's address as the claimed one, expect_valid 1"""
    hb = hb if hb is not None else _hash(rng)
    while True:
        sg = M.sign(sk, int.from_bytes(hb, "big"), k if k is not None else rng.randrange(1, N))
        if sg is not None:
            break
        k = None
    pub = M._mul(G, sk)
    addr = int.from_bytes(M.keccak256(pub[0].to_bytes(32, "big") + pub[1].to_bytes(32, "big"))[-20:], "big")
    return (hb, sg[0] + v_offset, sg[1], sg[2], addr, 1)


def smallest_r_without_point():
    r = 1
    while pow((r**3 + 7) % P, (P - 1) // 2, P) != P - 1:
        r += 1
    return r


def q_infinity(rng, k, v_offset):
    """R = +-k G and s = +-z / k, so that s R - z G = 0 (the construction of tests/tx_assign_directed.py's recovery batch)"""
    Rk = M._mul(G, k)
    assert Rk[0] < N
    hb = _hash(rng)
    s = int.from_bytes(hb, "big") % N * pow(k, -1, N) % N
    flip = k in (3, 7)
    return (hb, v_offset + ((Rk[1] & 1) ^ flip), Rk[0], (N - s) if flip else s, rng.getrandbits(160), 1)


@functools.lru_cache(maxsize=None)
def directed_entries(v_offset):
    """about 60 signatures: every failure site, both parities, repeated signatures and keys; -> (entries, {label: index})"""
    rng = random.Random(4100 + v_offset)
    e, at = [], {}

    def put(label, entry):
        at[label] = len(e)
        e.append(entry)

    good = lambda: signed(rng, rng.randrange(2, N), v_offset=v_offset)  # noqa: E731
    for label, kw in (("v_2", {1: 2}), ("v_26", {1: 26}), ("r_0", {2: 0}), ("s_0", {3: 0}), ("r_N", {2: N}), ("s_N", {3: N}),
                      ("v_high_limb", {1: v_offset + (1 << 64)}), ("v_top_limb", {1: v_offset + 1 + (1 << 200)})):
        put("ok_before_" + label, good())
        g = list(good())
        for k, x in kw.items():
            g[k] = x
        put(label, tuple(g))
    g = list(good())
    g[2] = smallest_r_without_point()
    put("no_point", tuple(g))
    for k in (2, 3, 5, 7):
        put(f"ok_before_q_infinity_{k}", good())
        put(f"q_infinity_{k}", q_infinity(rng, k, v_offset))
    par = {0: 0, 1: 0}
    while min(par.values()) < 4:  # both parities
        g = good()
        par[g[1] - v_offset] += 1
        put(f"parity_{g[1] - v_offset}_{par[g[1] - v_offset]}", g)
    rep = good()
    for j in range(3):  # the same signature three times: one sig-table row, one keccak row
        put(f"repeat_{j}", rep)
        put(f"ok_after_repeat_{j}", good())
    sk = rng.randrange(2, N)
    for j in range(3):  # one key, three messages: three sig-table rows, one keccak row
        put(f"one_key_{j}", signed(rng, sk, v_offset=v_offset))
    wrong = list(good())  # a claimed address that is not the signer's: cells[0] only
    wrong[4] ^= 1
    put("wrong_claimed_address", tuple(wrong))
    bad_twice = e[at["r_0"]]  # equal failing rows collapse in the sig table too
    put("r_0_again", bad_twice)
    ev0 = list(good())
    ev0[5] = 0
    put("expect_valid_0", tuple(ev0))
    while len(e) < 60:
        put(f"fill_{len(e)}", good())
    return tuple(e), at


def expected_sites(at):
    """{index: site} the directed batch must produce (v = 2 and v = 26 are no parity under either v_offset)"""
    sites = {at[k]: 1 for k in ("v_2", "v_26", "r_0", "s_0", "r_N", "s_N", "v_high_limb", "v_top_limb", "r_0_again")}
    sites[at["no_point"]] = 3
    for k in (2, 3, 5, 7):
        sites[at[f"q_infinity_{k}"]] = 4
    return sites


@functools.lru_cache(maxsize=None)
def lanes_batch():
    """n = 130: two full 64-signature blocks of the 4-lane form and a ragged tail; failing signatures at wavefront and block edges"""
    rng = random.Random(4200)
    e = [signed(rng, rng.randrange(2, N)) for _ in range(130)]
    fails = {0: {1: 2}, 15: {2: 0}, 16: {2: smallest_r_without_point()}, 63: {3: N}, 64: None, 129: {1: 1 << 64}}
    for i, kw in fails.items():
        if kw is None:
            e[i] = q_infinity(rng, 5, 0)
            continue
        g = list(e[i])
        for k, x in kw.items():
            g[k] = x
        e[i] = tuple(g)
    return pack(e), sorted(fails)


@functools.lru_cache(maxsize=None)
def tiles_batch():
    """n = 300 tiled from 40 distinct signatures over 12 keys: the keccak candidates (301 rows) and the sig-table candidates cross the
    256-row tile, with duplicates on both sides of the boundary and at rows 255 / 256 of both candidate arrays"""
    rng = random.Random(4300)
    sks = [rng.randrange(2, N) for _ in range(12)]
    base = [signed(rng, sks[j % 12]) for j in range(40)]
    g = list(base[7])
    g[2] = 0
    base[7] = tuple(g)  # one failing signature among the 40
    seq = [j % 40 for j in range(300)]
    seq[256] = seq[255]  # sig-table candidates 255 / 256
    seq[254] = seq[255]  # keccak candidates 255 / 256 (candidate i + 1 is signature i's)
    return pack([base[j] for j in seq])


def random_curve_point_inputs(n, seed):
    """n signatures as zk_sig_assign inputs: r = the x of R = k0 G + i G (a point exists) with a random s, parity and hash — every one
    recovers some key (the inputs of tests/tx_assign_cases.random_inputs(signed=False))"""
    rng = random.Random(seed)
    R = M._mul(G, rng.getrandbits(200) + 2)
    vals = []
    for _ in range(n):
        vals += [rng.getrandbits(256), rng.getrandbits(1), R[0] % N or 1, rng.randrange(1, N)]
        R = M._add(R, G)
    return {"fields": words(vals).reshape(n, 4, 4), "addr": None, "expect_valid": None, "v_offset": 0}


def compare(got_status, got, want_status, want, label=""):
    assert list(got_status) == list(want_status), (label, "status")
    for k in WIRE_KEYS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (label, k)
