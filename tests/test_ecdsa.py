"""secp256k1 ECDSA verification on the device: the `ecdsa_status` column of the Tx / Sig
units.  CPU: oracle vs the verdicts of the unmodified reference chips (tests/golden/ecdsa_cases.npz,
sign_cases.npz), device function logic (hostsim) vs the oracle.  GPU (marked): the HIP kernel vs the oracle, and
BASELINE config 4 end to end: 2^14 signed synthetic txs -> ECDSA pass fills the units' meta column in HBM -> Tx kernel."""
import ctypes
import os

import numpy as np
import pytest

from oracle import ecdsa_oracle as E
from zkevm_specs_amd.synth import ECDSA_STATUS_PENDING, synth_tx_witness

vp = lambda x: None if x is None else ctypes.c_void_p(x.ctypes.data)  # noqa: E731


def _same(a, b):
    """status equality up to the site of an exception code (the recorded column keeps only the kind)"""
    return [(x if x < 2 else x >> 24) for x in a] == [(y if y < 2 else y >> 24) for y in b]


def _hostsim(lib, sig_bytes, v, layout, v_stride=1):
    """both forms of the kernel: one lane per signature, and the lane-pair form (two partial sums added at the end)"""
    sig_bytes = np.ascontiguousarray(sig_bytes)
    n = sig_bytes.shape[0]
    st, st2 = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    lib.sim_ecdsa_verify(vp(sig_bytes), ctypes.c_uint32(layout), vp(v), ctypes.c_uint32(v_stride), ctypes.c_uint64(n), vp(st))
    assert lib.sim_ecdsa_verify_pairs(vp(sig_bytes), ctypes.c_uint32(layout), vp(v), ctypes.c_uint32(v_stride), ctypes.c_uint64(n), vp(st2)) == 0
    assert st.tolist() == st2.tolist()
    return st.tolist()


def _packed_from_units(bts, is_sig):
    """the five ECDSA inputs of the units' byte rows in the packed layout (msg_hash big-endian)"""
    p = np.ascontiguousarray(bts[:, [2, 3, 5, 7, 8]])
    if not is_sig:
        p[:, 2] = p[:, 2, ::-1]
    return p


def _hostile_cases(seed, n):
    import random

    rng = random.Random(seed)
    valid = E.sign_batch(n, seed)
    cases, vs = [], []
    for (x, y, z, r, s, v) in valid:
        c = rng.randrange(12)
        if c == 0:
            z ^= 1 << rng.randrange(256)
        elif c == 1:
            r = (r + rng.randrange(1, 5)) % E.N
        elif c == 2:
            s = E.N - s
        elif c == 3:
            y = E.P - y
        elif c == 4:
            v = rng.choice([2, 3, 27])
        elif c == 5:
            r = rng.choice([0, E.N, (1 << 256) - 1])
        elif c == 6:
            s = rng.choice([0, E.N, E.N + 7])
        elif c == 7:
            x, y = rng.randrange(E.P), rng.randrange(E.P)
        elif c == 8:
            x = rng.choice([E.P, E.P + 1, (1 << 256) - 1])
        elif c == 9:
            y = rng.choice([E.P, E.P + 1, (1 << 256) - 1, E.P + 7])
        cases.append((x, y, z, r, s))
        vs.append(v)
    return E.pack(cases), np.array(vs, dtype=np.uint32)


def test_field_products_known_answers(hostsim):
    """the folded product mod P = 2^256 - 2^32 - 977 (carry-out and final-subtraction paths included) and the Montgomery
    product mod N against Python integers"""
    import random

    from oracle import wire

    rng = random.Random(1)
    for which, m in ((0, E.P), (1, E.N)):
        edge = [0, 1, 2, m - 1, m - 2, 977, 2**32 + 977, 2**255, 2**128 - 1, 2**128, m >> 1, (1 << 256) - (1 << 224) - 1, 2**32 - 1,
                2**224 - 1, m - 2**32, m - 978]
        edge = [e % m for e in edge]
        pairs = [(a, b) for a in edge for b in edge] + [(rng.randrange(m), rng.randrange(m)) for _ in range(3000)]
        a = wire.ints_to_cells([x for x, _ in pairs])
        b = wire.ints_to_cells([y for _, y in pairs])
        out = np.zeros_like(a)
        hostsim.sim_secp_mul(ctypes.c_int(which), vp(a), vp(b), vp(out), ctypes.c_uint64(len(pairs)))
        rinv = pow(1 << 256, -1, m)
        exp = [x * y % m if which == 0 else x * y * rinv % m for x, y in pairs]
        assert wire.cells_to_ints(out) == exp, which
        if which == 0:  # the dedicated squaring
            hostsim.sim_secp_mul(ctypes.c_int(2), vp(a), vp(a), vp(out), ctypes.c_uint64(len(pairs)))
            assert wire.cells_to_ints(out) == [x * x % m for x, _ in pairs]


def test_scalar_field_inversion_known_answers(hostsim):
    """s^-1 mod N against pow(x, -1, N): sp_inv_n_safegcd (Bernstein-Yang division steps, what the verification uses since round 4) and
    sp_inv_n_binary (the right-shift binary inversion of round 3, kept behind -DZK_SECP_INV_BINARY)"""
    import random

    from oracle import wire

    rng = random.Random(5)
    xs = [1, 2, 3, E.N - 1, E.N - 2, (E.N + 1) // 2, 1 << 255, (1 << 255) - 1, 1 << 128, (1 << 128) - 1, 0xFFFFFFFF, 1 << 32, E.N >> 1]
    xs += [1 << k for k in range(1, 256, 7)] + [(E.N - (1 << k)) for k in range(0, 250, 11)]
    xs += [rng.randrange(1, E.N) for _ in range(4000)]
    xs = [x % E.N or 1 for x in xs]
    a = wire.ints_to_cells(xs)
    out = np.zeros_like(a)
    xs += [rng.randrange(1, 1 << k) for k in range(1, 257, 3) for _ in range(4)]
    xs = [x % E.N or 1 for x in xs]
    a = wire.ints_to_cells(xs)
    out = np.zeros_like(a)
    for which in (3, 4):
        hostsim.sim_secp_mul(ctypes.c_int(which), vp(a), vp(a), vp(out), ctypes.c_uint64(len(xs)))
        assert wire.cells_to_ints(out) == [pow(x, -1, E.N) for x in xs], which


def _group_law_edge_cases():
    """curve keys that drive the joint multiplication through its special cases: Q = +-G, Q = lambda G, u1 or u2 with zero
    windows, R = infinity (u1 G = -u2 Q), acc == table entry (doubling inside an addition)"""
    import random

    rng = random.Random(31)
    lam = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72
    cases = []
    G = E.G
    for d in (1, E.N - 1, 2, lam, E.N - lam, 16, 1 << 128, (1 << 128) - 1, 3, 5):
        Q = E.mul(G, d)
        for _ in range(3):
            k, z = rng.randrange(1, E.N), rng.getrandbits(256)
            r = E.mul(G, k)[0] % E.N
            s = pow(k, -1, E.N) * (z + r * d) % E.N
            if r and s:
                cases.append((Q[0], Q[1], z, r, s))                 # valid
                cases.append((Q[0], Q[1], z, r, (s + 1) % E.N or 1))  # invalid
        # u1 G + u2 Q = infinity: z + r d = 0 (mod N) -> pick r, then z = -r d
        r = rng.randrange(1, E.N)
        cases.append((Q[0], Q[1], (-r * d) % E.N, r, rng.randrange(1, E.N)))
        # sparse scalars: s = 1 -> u1 = z, u2 = r with many zero windows
        cases.append((Q[0], Q[1], 1 << 200, 1 << 64, 1))
        cases.append((Q[0], Q[1], 0, 1, 1))
    return E.pack(cases)


def test_kernel_logic_group_law_edge_cases(hostsim):
    sigs = _group_law_edge_cases()
    exp = E.verify_packed(sigs, None)
    assert _hostsim(hostsim, sigs, None, 0) == exp
    assert sum(1 for e in exp if e == 0) >= 25 and sum(1 for e in exp if e == 1) >= 25


def test_out_of_range_key_coordinates_match_the_eth_keys_standin():
    """Public-key coordinates >= P (the native backend of eth-keys 0.4.0 does not range-check them; oracle/refshim/eth_keys
    restates it): the verdict is that of the coordinates mod P, except for y == P exactly, which stays out of domain
    (csrc/secp256k1.hpp ecdsa_prepare).  Needs the refshim on the path (build container)."""
    import random
    import sys

    shim = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "refshim")
    sys.path.insert(0, shim)
    try:
        from eth_keys import KeyAPI
    finally:
        sys.path.remove(shim)
    rng = random.Random(5)
    n_checked = 0
    for (x, y, z, r, s, v) in E.sign_batch(24, 77):
        for x2, y2 in ((E.P + rng.randrange(1 << 32), y), (x, E.P + 1 + rng.randrange(1 << 32)), ((1 << 256) - 1, (1 << 256) - 1),
                       (x % (1 << 32) + E.P, y), (x, E.P)):
            got = E.verify(x2, y2, z, r, s, v)
            if y2 == E.P:
                assert got == E.KEY_RANGE
                continue
            sig = KeyAPI.Signature(vrs=(v, r, s))
            want = KeyAPI().ecdsa_verify(z.to_bytes(32, "big"), sig, KeyAPI.PublicKey(x2.to_bytes(32, "big") + y2.to_bytes(32, "big")))
            assert got == (0 if want else 1), (hex(x2), hex(y2))
            n_checked += 1
    assert n_checked >= 90


def test_oracle_matches_reference_chips(golden_dir):
    g = np.load(os.path.join(golden_dir, "ecdsa_cases.npz"))
    assert _same(E.verify_packed(g["sigs"], g["v"]), g["util_status"].tolist())   # util/ec.py:109-117, Signature(vrs=[v, r, s])
    assert _same(E.verify_packed(g["sigs"], None), g["tx_status"].tolist())       # tx_circuit.py:147-158, v fixed to 0
    assert (g["util_status"] == 0).sum() >= 40 and (g["util_status"] == 1).sum() >= 15 and (g["util_status"] > 1).sum() >= 5


def _openssl(golden_dir):
    g = np.load(os.path.join(golden_dir, "ecdsa_openssl.npz"))
    return np.ascontiguousarray(g["sigs"]), g["verdict"].tolist()


def _offcurve_cases():
    """Public keys that are NOT on the curve, where eth-keys' case analysis decides: a key with y == 0 counts as the point
    at infinity, so the signature is accepted iff r == (u1 G).x whatever x is; a key on another curve y^2 = x^3 + b' just
    has to go through the same MSB-first chain.  (z, r, s) are built so that u1 G has x == r: z = k s, r = (k G).x."""
    import random

    rng = random.Random(77)
    cases = []
    for i in range(24):
        k, s = rng.randrange(1, E.N), rng.randrange(1, E.N)
        r = E.mul(E.G, k)[0]
        if not 0 < r < E.N:
            continue
        z = k * s % E.N
        x = rng.randrange(E.P)
        cases.append((x, 0, z, r, s))                      # y == 0: ignored -> verified
        cases.append((x, rng.randrange(1, E.P), z, r, s))  # off-curve, y != 0: garbage point added -> not verified
        cases.append((x, 0, z ^ 1, r, s))                  # y == 0, wrong digest -> not verified
    return E.pack(cases)


def test_oracle_matches_openssl(golden_dir):
    """the restated eth-keys algorithm agrees with OpenSSL's own verdict on every OpenSSL-made vector (curve points)"""
    sigs, verdict = _openssl(golden_dir)
    assert len(verdict) >= 256 and 100 <= sum(verdict) <= len(verdict) - 100
    assert E.verify_packed(sigs, None) == verdict
    st = E.verify_packed(_offcurve_cases(), None)
    assert st[0::3] == [0] * (len(st) // 3) and st[1::3] == [1] * (len(st) // 3) and st[2::3] == [1] * (len(st) // 3)


def test_kernel_logic_matches_openssl_and_offcurve_cases(golden_dir, hostsim):
    sigs, verdict = _openssl(golden_dir)
    assert _hostsim(hostsim, sigs, None, 0) == verdict
    off = _offcurve_cases()
    assert _hostsim(hostsim, off, None, 0) == E.verify_packed(off, None)


def test_kernel_logic_matches_oracle(golden_dir, hostsim):
    g = np.load(os.path.join(golden_dir, "ecdsa_cases.npz"))
    v = np.ascontiguousarray(g["v"])
    assert _hostsim(hostsim, g["sigs"], v, 0) == E.verify_packed(g["sigs"], v)
    assert _hostsim(hostsim, g["sigs"], None, 0) == E.verify_packed(g["sigs"], None)
    sigs, v = _hostile_cases(5, 150)
    exp = E.verify_packed(sigs, v)
    assert _hostsim(hostsim, sigs, v, 0) == exp
    assert sum(1 for e in exp if e == 0) > 30 and sum(1 for e in exp if e == 1) > 30 and sum(1 for e in exp if e > 1) > 20


def _sign_units(golden_dir):
    g = np.load(os.path.join(golden_dir, "sign_cases.npz"))
    for i, nm in enumerate(g["names"]):
        k = f"c{i:04d}"
        yield str(nm), g[f"{k}_bytes"], g[f"{k}_cells"], g[f"{k}_meta"], int(g[f"{k}_is_sig"][0])


def test_unit_layout_reproduces_the_recorded_ecdsa_column(golden_dir, hostsim):
    """every Tx / Sig unit of the reference's own tests whose chip attributes are well-formed: the status computed
    from the unit's byte rows equals the column the reference produced by calling the chip"""
    n = 0
    for name, bts, cells, meta, is_sig in _sign_units(golden_dir):
        if "tamper" in name:
            continue  # tampering replaces chip attributes independently of the limbs eth_keys is called with
        ok = (meta[:, 2] & 0x1AC) == 0
        meta = np.ascontiguousarray(meta)
        got = _hostsim(hostsim, bts, meta.reshape(-1)[3:] if is_sig else None, 2 if is_sig else 1, 4)
        assert _same([g for g, o in zip(got, ok) if o], [int(m) for m, o in zip(meta[:, 0], ok) if o]), name
        assert got == E.verify_packed(_packed_from_units(bts, is_sig), meta[:, 3] if is_sig else None), name
        n += int(ok.sum())
    assert n >= 30


# ---- GPU --------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_hip_matches_openssl_vectors(golden_dir):
    """the device verdicts on signatures made and judged by OpenSSL (nothing of this repository in the loop), through
    both C entries (session and one-shot), and the off-curve keys where eth-keys' case analysis decides"""
    from zkevm_specs_amd import engine, oneshot

    sigs, verdict = _openssl(golden_dir)
    assert engine.ecdsa_status(sigs).tolist() == verdict
    res, status = oneshot.ecdsa_verify(sigs)
    assert status.tolist() == verdict and res.fail_count == sum(verdict)
    off = _offcurve_cases()
    assert engine.ecdsa_status(off).tolist() == E.verify_packed(off, None)
    edge = _group_law_edge_cases()
    for lanes in ("1", "2", "4"):  # one lane per signature / lane pairs / lane quads (the library picks by batch size; every form on every vector here)
        os.environ["ZK_ECDSA_LANES"] = lanes
        try:
            assert engine.ecdsa_status(edge).tolist() == E.verify_packed(edge, None)
            assert engine.ecdsa_status(sigs).tolist() == verdict
            assert engine.ecdsa_status(off).tolist() == E.verify_packed(off, None)
        finally:
            del os.environ["ZK_ECDSA_LANES"]


@pytest.mark.gpu
def test_hip_matches_oracle(golden_dir):
    from zkevm_specs_amd import engine

    g = np.load(os.path.join(golden_dir, "ecdsa_cases.npz"))
    assert engine.ecdsa_status(g["sigs"], g["v"]).tolist() == E.verify_packed(g["sigs"], g["v"])
    assert engine.ecdsa_status(g["sigs"]).tolist() == E.verify_packed(g["sigs"], None)
    sigs, v = _hostile_cases(11, 700)
    with engine.open_ecdsa(sigs, v) as s:
        res = s.run()
        got = s.read_status().tolist()
    exp = E.verify_packed(sigs, v)
    assert got == exp and res.fail_count == sum(1 for e in exp if e)


@pytest.mark.gpu
def test_config4_signed_txs_end_to_end_on_device():
    """2^14 signed synthetic txs (BASELINE config 4): the ECDSA pass writes the units' meta column in HBM, then the
    Tx kernel evaluates the same buffers; without the ECDSA pass every unit fails; one forged signature is found."""
    import torch

    from zkevm_specs_amd import engine

    from zkevm_specs_amd.synth import device_keccak_digests

    n, r = 1 << 14, 0x1F2E3D4C5B6A79881726354433221100FFEEDDCCBBAA99887766554433221
    # public-key hashes: keccak-256 through the device table builder, so nothing of the unit is a host-computed stand-in
    w = synth_tx_witness(n, r, seed=4, signed=True, digests_of=device_keccak_digests(r))
    from oracle import keccak as K
    for i in (0, 5000, n - 1):
        pk = bytes(w["bytes"][i, 0][::-1].tolist()) + bytes(w["bytes"][i, 1][::-1].tolist())
        assert bytes(w["bytes"][i, 6].tolist()) == K.keccak256(pk)
    assert (w["meta"][:, 0] == ECDSA_STATUS_PENDING).all()
    w["bytes"][777, 8, 0] ^= 1  # forge s of tx 777
    dev = {k: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v.view(np.int32) if v.dtype == np.uint32 else v).cuda()
           for k, v in w.items()}
    with engine.open_sign(dev, r, False) as s:
        assert s.run().fail_count == n  # PENDING everywhere
    with engine.open_ecdsa(dev["bytes"], layout=engine.ECDSA_LAYOUT_TX_UNITS, out_dev=dev["meta"], out_stride=4) as e:
        res = e.run()
        assert res.fail_count == 1 and res.first_fail_row == 777 and res.rows_evaluated == n
    with engine.open_sign(dev, r, False) as s:
        res = s.run()
    assert res.fail_count == 1 and res.first_fail_row == 777 and res.first_fail_kind == 1
    # a sample of the verdicts against the oracle
    idx = np.arange(0, n, 257)
    st = dev["meta"].cpu().numpy().view(np.uint32)[idx, 0].tolist()
    assert st == E.verify_packed(_packed_from_units(w["bytes"][idx], False))


@pytest.mark.gpu
def test_secp_base_field_product_on_device():
    """csrc/secp256k1.hpp `sp_mul_p` / `sp_sqr_p` as the ECDSA kernel runs them (product scanning + the explicit carry-chain fold of
    round 4) against Python integers: random residues and the operands that exercise every branch of the fold — products whose high
    half is all ones, results in [P, 2^256), the double wrap past 2^256."""
    import random

    from oracle import wire
    from zkevm_specs_amd import engine

    P = 2**256 - 2**32 - 977
    rng = random.Random(41)
    edge = [0, 1, 2, P - 1, P - 2, 2**32 + 977, 2**32 + 976, 2**255, 2**256 - 2**33, P - 2**32, 977, 2**128, 2**128 - 1, (P - 1) // 2,
            (P + 1) // 2, 2**224 - 1, 2**192 + 12345]
    a = edge * len(edge) + [rng.randrange(P) for _ in range(20000)] + [P - 1 - rng.randrange(2**40) for _ in range(2000)]
    b = [y for y in edge for _ in edge] + [rng.randrange(P) for _ in range(20000)] + [P - 1 - rng.randrange(2**40) for _ in range(2000)]
    A, B = wire.ints_to_cells(a), wire.ints_to_cells(b)
    assert wire.cells_to_ints(engine.fr_op(16, A, B)) == [x * y % P for x, y in zip(a, b)]
    assert wire.cells_to_ints(engine.fr_op(17, A, B)) == [x * x % P for x in a]


@pytest.mark.gpu
def test_two_batches_in_one_launch():
    """zk_ecdsa_open_batches: two signature arrays with different layouts (packed big-endian hashes with recovery ids | Tx units with
    little-endian hashes) verified by ONE launch: statuses = batch 0's then batch 1's, each batch's verdict column written where
    that batch asked for it; the same answers as two single-batch sessions and as the oracle."""
    import torch

    from zkevm_specs_amd import engine

    sigs, v = _hostile_cases(5, 300)
    exp0 = E.verify_packed(sigs, v)
    r = 0x1F2E3D4C5B6A79881726354433221100FFEEDDCCBBAA99887766554433221
    w = synth_tx_witness(257, r, seed=8, signed=True)
    w["bytes"][7, 7, 0] ^= 1  # a forged r
    exp1 = engine.ecdsa_status(w["bytes"], layout=engine.ECDSA_LAYOUT_TX_UNITS).tolist()
    assert exp1[7] != 0 and sum(1 for e in exp1 if e) == 1
    # host arrays
    with engine.open_ecdsa_batches([dict(sig_bytes=sigs, v=v), dict(sig_bytes=w["bytes"], layout=engine.ECDSA_LAYOUT_TX_UNITS)]) as s:
        res = s.run()
        got = s.read_status().tolist()
    assert got == exp0 + exp1 and res.fail_count == sum(1 for e in exp0 + exp1 if e)
    # device arrays, verdict columns in place
    d_sigs, d_v = torch.from_numpy(sigs).cuda(), torch.from_numpy(v.view(np.int32)).cuda()
    d_bytes = torch.from_numpy(w["bytes"]).cuda()
    out0 = torch.full((len(exp0),), -1, dtype=torch.int32, device="cuda")
    meta = torch.full((257, 4), -1, dtype=torch.int32, device="cuda")
    with engine.open_ecdsa_batches([dict(sig_bytes=d_sigs, v=d_v, out_dev=out0), dict(sig_bytes=d_bytes, layout=engine.ECDSA_LAYOUT_TX_UNITS,
                                                                                       out_dev=meta, out_stride=4)]) as s:
        s.run()
    assert out0.cpu().numpy().view(np.uint32).tolist() == exp0
    m = meta.cpu().numpy().view(np.uint32)
    assert m[:, 0].tolist() == exp1 and (m[:, 1:] == 0xFFFFFFFF).all()


@pytest.mark.gpu
@pytest.mark.parametrize("lanes,n", [("4", (1 << 15) + 67), ("2", (1 << 16) + 67)])
def test_chunked_launches_match_tiled_openssl_verdicts(golden_dir, lanes, n, monkeypatch):
    """above 2^17 lanes zk_launch_ecdsa runs consecutive launches over one set of key tables: the smallest batch that chunks in the
    four-lane and in the lane-pair form, OpenSSL's vectors tiled (320 does not divide 2^15: the later launch starts inside the
    pattern), every status and the tally against OpenSSL's verdicts"""
    from zkevm_specs_amd import engine

    monkeypatch.setenv("ZK_ECDSA_LANES", lanes)
    sigs, verdict = _openssl(golden_dir)
    idx = np.arange(n) % len(verdict)
    want = np.asarray(verdict, dtype=np.uint32)[idx]
    # (the lane form is the requested one as long as zk_ecdsa_open has the comb of G, which it builds before it chooses: without
    # the comb it would drop four lanes to two, and the first case would fit one launch and still pass)
    assert n * int(lanes) > 1 << 17 and (n - 67) % len(verdict) != 0
    with engine.open_ecdsa(np.ascontiguousarray(sigs[idx])) as s:
        res = s.run()
        got = s.read_status()
    assert np.array_equal(got, want)
    assert res.fail_count == int(np.count_nonzero(want)) and res.first_fail_row == int(np.flatnonzero(want)[0])
