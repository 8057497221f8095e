#!/usr/bin/env python3
"""Golden cases of the Tx circuit's witness assignment: tests/golden/tx_assign_cases.npz.

Runs the unmodified reference's `txs2witness` (src/zkevm_specs/tx_circuit.py:432-481) over the third-party stand-ins of oracle/refshim
(eth_keys, rlp, eth_utils) and records, per case, the raw transactions as the wire of zk_tx_assign takes them, the outcome (0, or the
exception the reference raised: its kind and, for eth_keys' BadSignature, the site of include/zkevm_hip.h) and, for a clean outcome,
the wire of flatten_tx_witness (meta[:, 0] pending).  Verdict cases also record what the reference's `verify_circuit` says about the
witness of a case after one edit (the edits of tests/test_tx_circuit.py).  Needs the reference checkout (--ref-root); the cases are
data, the generator stays out of the test run.
"""
import argparse
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 2**256 - 2**32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-root", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "tx_assign_cases.npz"))
    args = ap.parse_args()
    os.environ["ZK_BACKEND"] = "cpu"
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle", "refshim"), os.path.join(args.ref_root, "src")]
    import eth_keys
    import rlp
    from eth_keys import keys
    from eth_utils import keccak
    from zkevm_specs import tx_circuit as ref
    from zkevm_specs.util import FQ, U64, U160, U256, Word, WordOrValue

    from zkevm_specs_amd.errors import kind_for_exception
    from zkevm_specs_amd.flatten import flatten_tx_witness
    from zkevm_specs_amd.tx_circuit import tx_inputs

    T = ref.Transaction

    def sign_hash(tx, chain_id):
        return keccak(rlp.encode([tx.nonce, tx.gas_price, tx.gas, tx.encode_to(), tx.value, tx.data, chain_id, 0, 0]))

    def sign(sk, tx, chain_id):
        sig = sk.sign_msg_hash(sign_hash(tx, chain_id))
        return T(tx.nonce, tx.gas_price, tx.gas, tx.to, tx.value, tx.data, sig.v + chain_id * 2 + 35, sig.r, sig.s)

    def with_sig(tx, v, r, s):
        return T(tx.nonce, tx.gas_price, tx.gas, tx.to, tx.value, tx.data, v, r, s)

    def sk_of(i):
        return keys.PrivateKey(bytes([(i % 250) + 1]) * 31 + bytes([i // 250 + 1]))

    rng = random.Random(20261016)
    cases = []  # (name, txs, chain_id, MAX_TXS, MAX_CALLDATA_BYTES, randomness, tamper or None)
    r0 = 0x2A3B4C5D6E7F
    # the reference test file's transactions (tests/test_tx_circuit.py: gen_tx, test_verify, gen_valid_witness, test_tx2witness)
    def gen_tx(i, sk, to, chain_id):
        return sign(sk, T(U64(300 + i), U256(1000 + i * 2), U64(20000 + i * 3), U160(to), U256(0x30000 + i * 4), bytes([i] * i), U64(0), U256(0), U256(0)), chain_id)

    sks = [keys.PrivateKey(bytes([b + 1]) * 32) for b in range(16)]
    txs16 = [gen_tx(i, sks[i], int.from_bytes(sks[(i + 1) % 16].public_key.to_canonical_address(), "big"), 1337) for i in range(16)]
    cases.append(("ref_test_verify", txs16, 1337, 20, 300, r0, None))
    txs3 = [gen_tx(i, sks[i], int.from_bytes(sks[(i + 1) % 3].public_key.to_canonical_address(), "big"), 1337) for i in range(3)]
    cases.append(("ref_valid_witness", txs3, 1337, 5, 16, r0, None))
    for tamper in ("bad_keccak", "bad_signature", "bad_address", "bad_msg_hash", "bad_addr_copy", "bad_sign_hash_copy"):
        cases.append((f"ref_{tamper}", txs3, 1337, 5, 16, r0, tamper))
    t0 = sign(keys.PrivateKey(b"\x01" * 32), T(543, 1234, 987654, 0x12345678, 0x1029384756, bytes(range(0, 0xAA, 0x11)), 0, 0, 0), 23)
    cases.append(("ref_tx2witness", [t0], 23, 1, 10, r0, None))
    # random signed txs: calldata lengths around the RLP and keccak-rate boundaries, several chain ids (both parities occur)
    lens = [0, 1, 55, 56, 135, 136, 137, 3000]
    for ci, chain in enumerate([1, 1337, 2**32 + 5, 2**64 - 1]):
        txs = []
        for k, ln in enumerate(lens):
            data = bytes(rng.getrandbits(8) if rng.random() < 0.7 else 0 for _ in range(ln))
            to = None if k % 3 == 2 else rng.getrandbits(160)
            txs.append(sign(sk_of(8 * ci + k), T(rng.getrandbits(64), rng.getrandbits(90), rng.getrandbits(40), to, rng.getrandbits(200), data, 0, 0, 0), chain))
        cases.append((f"random_chain{ci}", txs, chain, 10, sum(lens) + 7, rng.getrandbits(250), None))
    # single-byte RLP edges, to = None / 0, 2^256 - 1 fields, a repeated sender
    edge = []
    for k, (val, data) in enumerate([(0, b"\x00"), (0x7F, b"\x7f"), (0x80, b"\x80"), (2**256 - 1, b""), (1, b"\x00" * 60)]):
        edge.append(sign(sk_of(40), T(val if k != 3 else 2**64 - 1, val, val if val < 2**64 else 0, None if k % 2 else 0, val, data, 0, 0, 0), 5))
    edge.append(sign(sk_of(41), T(2**256 - 1, 2**256 - 1, 2**256 - 1, 2**160 - 1, 2**256 - 1, b"\xff" * 200, 0, 0, 0), 5))
    cases.append(("edges_repeated_sender", edge, 5, 6, 300, r0, None))
    # MAX_TXS / MAX_CALLDATA_BYTES exactly full and one over
    full = [sign(sk_of(50 + k), T(k, k, k, k, k, bytes([k + 1]) * 10, 0, 0, 0), 7) for k in range(4)]
    cases.append(("max_full", full, 7, 4, 40, r0, None))
    cases.append(("max_txs_over", full, 7, 3, 40, r0, None))
    cases.append(("max_calldata_over", full, 7, 4, 39, r0, None))
    cases.append(("empty", [], 7, 3, 5, r0, None))
    # BadSignature causes, each behind a clean tx (the first failing tx raises)
    good = sign(sk_of(60), T(1, 2, 3, 4, 5, b"abc", 0, 0, 0), 9)
    base = sign(sk_of(61), T(6, 7, 8, 9, 10, b"xyz" * 30, 0, 0, 0), 9)
    no_pt = next(x for x in range(3, 10**6) if pow((x**3 + 7) % P, (P - 1) // 2, P) == P - 1)
    bads = {"parity2": with_sig(base, base.sig_v + 2 - (base.sig_v - 35 - 18), base.sig_r, base.sig_s),
            "v_small": with_sig(base, 3, base.sig_r, base.sig_s),
            "r_zero": with_sig(base, base.sig_v, 0, base.sig_s), "r_ge_n": with_sig(base, base.sig_v, N, base.sig_s),
            "s_zero": with_sig(base, base.sig_v, base.sig_r, 0), "s_ge_n": with_sig(base, base.sig_v, base.sig_r, N + 5),
            "r_no_point": with_sig(base, base.sig_v, no_pt, base.sig_s)}
    # Q at infinity: R = k G with s = z / k, so that s R - z G = 0
    z = int.from_bytes(sign_hash(base, 9), "big")
    for k in range(2, 100):
        Rp = eth_keys._mul(eth_keys.G, k)
        if Rp[0] < N:
            bads["q_infinity"] = with_sig(base, 35 + 18 + (Rp[1] & 1), Rp[0], z * pow(k, -1, N) % N)
            break
    for name, bad in bads.items():
        cases.append((f"bad_{name}", [good, bad, good], 9, 4, 200, r0, None))
    cases.append(("neg_nonce_after_bad", [good, bads["r_zero"], T(-1, 0, 0, None, 0, b"", 0, 0, 0)], 9, 4, 200, r0, None))
    cases.append(("neg_value", [good, T(0, 0, 0, None, -5, b"", 0, 0, 0)], 9, 4, 200, r0, None))

    out = {}
    names = []
    for ci, (name, txs, chain, mt, mc, rr, tamper) in enumerate(cases):
        names.append(name)
        tx, host_err = tx_inputs(txs, chain, mt, mc)
        for k in ("fields", "to_is_none", "calldata", "offsets"):
            out[f"c{ci}_{k}"] = tx[k]
        out[f"c{ci}_scalars"] = np.array([chain, mt, mc], dtype=np.uint64)
        out[f"c{ci}_randomness"] = np.frombuffer(rr.to_bytes(32, "little"), dtype="<u8").copy()
        out[f"c{ci}_host_errors"] = np.array(sorted(host_err), dtype=np.int64)
        code, fail_tx = 0, -1
        try:
            w = ref.txs2witness(txs, chain, mt, mc, FQ(rr))
        except Exception as e:  # noqa: BLE001 - the reference's exception is the outcome
            kind = kind_for_exception(e)
            site = 0
            if type(e).__name__ == "BadSignature":
                msg = str(e)
                site = 1 if ("v must" in msg or "out of range" in msg) else 0
                # which tx: the first one the reference would fail on; which site: restated from the shim's checks
                for i, t in enumerate(txs):
                    par = t.sig_v - 35 - chain * 2
                    if i in host_err:
                        break
                    if par not in (0, 1) or not (0 < t.sig_r < N and 0 < t.sig_s < N):
                        fail_tx, site = i, 1
                        break
                    y2 = (t.sig_r**3 + 7) % P
                    y = pow(y2, (P + 1) // 4, P)
                    if y * y % P != y2:
                        fail_tx, site = i, 3
                        break
                    try:
                        ref.txs2witness([t], chain, 1, len(t.data), FQ(rr))
                    except Exception:  # noqa: BLE001
                        fail_tx, site = i, 4
                        break
            code = (kind << 24) | site
            out[f"c{ci}_exc"] = np.array([code, fail_tx], dtype=np.int64)
            print(f"{name}: raises {type(e).__name__} site {site} at tx {fail_tx}")
            continue
        out[f"c{ci}_exc"] = np.array([0, -1], dtype=np.int64)
        f = flatten_tx_witness(w, mt)
        f["meta"][:, 0] = 0xFFFFFFFF
        for k in ("tx_rows", "tx_flags", "bytes", "cells", "meta", "keccak"):
            out[f"c{ci}_{k}"] = np.asarray(f[k])
        if tamper:
            sv = w.sign_verifications
            if tamper == "bad_keccak":
                w = ref.Witness(w.rows, ref.KeccakTable(), sv)
            elif tamper == "bad_signature":
                sv[0].ecdsa_chip.signature = (ref.Secp256k1ScalarField(1), ref.Secp256k1ScalarField(2))
            elif tamper == "bad_address":
                sv[0].address = FQ(1234)
            elif tamper == "bad_msg_hash":
                sv[0].msg_hash = Word(4567)
            elif tamper == "bad_addr_copy":
                w.rows[3].value = WordOrValue(FQ(1213))
            elif tamper == "bad_sign_hash_copy":
                w.rows[11].value = WordOrValue(Word(2324))
        try:
            ref.verify_circuit(w, mt, mc, FQ(rr))
            verdict = 0
        except Exception as e:  # noqa: BLE001
            verdict = kind_for_exception(e)
        out[f"c{ci}_verdict"] = np.array([verdict], dtype=np.int64)
        print(f"{name}: ok, verify_circuit verdict kind {verdict}")
    out["names"] = np.array(names)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out}: {len(names)} cases, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
