"""The golden cases of tools/gen_golden_tx_assign.py (tests/golden/tx_assign_cases.npz) and random signed transactions for the Tx
circuit's witness assignment tests."""
import os
import random
from collections import namedtuple

import numpy as np

from tests.tx_assign_ref import G, N, _add, _mul, rlp
from oracle.keccak import keccak256

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tx_assign_cases.npz")
WIRE_KEYS = ("tx_rows", "tx_flags", "bytes", "cells", "meta", "keccak")
Tx = namedtuple("Tx", "nonce gas_price gas to value data sig_v sig_r sig_s")


def golden_cases():
    """-> list of dicts: name, tx (engine._tx_assign_args input), randomness int, exc (code, failing tx), host_errors, wire or None,
    verdict (kind of the reference's verify_circuit outcome) or None"""
    z = np.load(GOLDEN)
    out = []
    for ci, name in enumerate(z["names"].tolist()):
        chain, mt, mc = (int(x) for x in z[f"c{ci}_scalars"])
        tx = {"fields": z[f"c{ci}_fields"], "to_is_none": z[f"c{ci}_to_is_none"], "calldata": z[f"c{ci}_calldata"],
              "offsets": z[f"c{ci}_offsets"], "chain_id": chain, "max_txs": mt, "max_calldata_bytes": mc}
        c = {"name": name, "tx": tx, "randomness": int.from_bytes(z[f"c{ci}_randomness"].tobytes(), "little"),
             "exc": tuple(int(x) for x in z[f"c{ci}_exc"]), "host_errors": z[f"c{ci}_host_errors"].tolist(), "wire": None, "verdict": None}
        if f"c{ci}_tx_rows" in z:
            c["wire"] = {k: z[f"c{ci}_{k}"] for k in WIRE_KEYS}
            c["verdict"] = int(z[f"c{ci}_verdict"][0])
        out.append(c)
    return out


def txs_of(tx):
    """Transaction-like tuples of zk_tx_assign's inputs"""
    f, off = tx["fields"], tx["offsets"]
    out = []
    for i in range(f.shape[0]):
        v = [int.from_bytes(f[i, k].tobytes(), "little") for k in range(8)]
        data = bytes(tx["calldata"][int(off[i]) : int(off[i + 1])])
        out.append(Tx(v[0], v[1], v[2], None if tx["to_is_none"][i] else v[3], v[4], data, v[5], v[6], v[7]))
    return out


def sign(tx, d, chain_id, k):
    """tx signed with the secret d and nonce k (the model's own ECDSA; low-s not enforced: recovery takes any s)"""
    z = int.from_bytes(keccak256(rlp([tx.nonce, tx.gas_price, tx.gas, b"" if tx.to is None else tx.to.to_bytes(20, "big"), tx.value,
                                      tx.data, chain_id, 0, 0])), "big")
    R = _mul(G, k)
    r = R[0] % N
    s = pow(k, -1, N) * (z + r * d) % N
    return tx._replace(sig_v=35 + 2 * chain_id + ((R[1] & 1) ^ (1 if R[0] >= N else 0)), sig_r=r, sig_s=s)


def random_inputs(n, seed, chain_id=1337, long_every=0, max_len=40, signed=True):
    """n txs as zk_tx_assign inputs.  signed: signatures of secrets d0 + i with nonces k0 + i (the model's ECDSA); else r = the x of
    R = k0 G + i G (a point exists) with a random s and parity — every one recovers some key, and no payload is hashed on the host."""
    rng = random.Random(seed)
    fields = np.zeros((n, 8, 4), dtype=np.uint64)
    to_none = np.zeros(n, dtype=np.uint32)
    datas = []
    d0, k0 = rng.getrandbits(200) + 2, rng.getrandbits(200) + 2
    R = _mul(G, k0)
    for i in range(n):
        ln = rng.randrange(600) if long_every and i % long_every == 0 else rng.randrange(max_len)
        data = bytes(rng.getrandbits(8) if rng.random() < 0.8 else 0 for _ in range(ln))
        to = None if rng.random() < 0.1 else rng.getrandbits(160)
        tx = Tx(rng.getrandbits(64), rng.getrandbits(128), rng.getrandbits(64), to, rng.getrandbits(256), data, 0, 0, 0)
        if signed:
            tx = sign(tx, d0 + i, chain_id, k0 + i)
        else:
            tx = tx._replace(sig_v=35 + 2 * chain_id + rng.getrandbits(1), sig_r=R[0] % N or 1, sig_s=rng.randrange(1, N))
            R = _add(R, G)
        v = [tx.nonce, tx.gas_price, tx.gas, tx.to or 0, tx.value, tx.sig_v, tx.sig_r, tx.sig_s]
        fields[i] = np.frombuffer(b"".join(x.to_bytes(32, "little") for x in v), dtype="<u8").reshape(8, 4)
        to_none[i] = tx.to is None
        datas.append(data)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(d) for d in datas])
    calldata = np.frombuffer(b"".join(datas), dtype=np.uint8).copy()
    return {"fields": fields, "to_is_none": to_none, "calldata": calldata, "offsets": offsets, "chain_id": chain_id, "max_txs": n + 3,
            "max_calldata_bytes": int(offsets[-1]) + 5}
