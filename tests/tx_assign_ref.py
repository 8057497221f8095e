"""Independent plain-Python model of the Tx circuit's witness assignment (txs2witness, tx_circuit.py:432-481) for the tests: its own
RLP, its own secp256k1 key recovery (affine arithmetic with Python's pow) and oracle/keccak.py's keccak-256.  Outputs the wire of
flatten_tx_witness (meta[:, 0] pending) for txs given as zk_tx_assign's inputs.  The key recovery, the two digests and the key's RLC (_rlc, the
loop lifted out of assign unchanged) are memoised on their exact inputs, so a batch tiled from a few distinct txs costs only its row building."""
import functools

import numpy as np

from oracle.keccak import keccak256 as _keccak256
from zkevm_specs_amd.wire import FR_MODULUS, rows_to_colmajor, rows_to_rowmajor

P = 2**256 - 2**32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
G = (0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798, 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8)
PENDING = 0xFFFFFFFF
keccak256 = functools.lru_cache(maxsize=None)(_keccak256)


def rlp(x):
    if isinstance(x, int):
        x = x.to_bytes((x.bit_length() + 7) // 8, "big")
    if isinstance(x, bytes):
        if len(x) == 1 and x[0] < 0x80:
            return x
        return _len(len(x), 0x80) + x
    body = b"".join(rlp(e) for e in x)
    return _len(len(body), 0xC0) + body


def _len(n, base):
    if n < 56:
        return bytes([base + n])
    b = n.to_bytes((n.bit_length() + 7) // 8, "big")
    return bytes([base + 55 + len(b)]) + b


def _add(p, q):
    if p is None:
        return q
    if q is None:
        return p
    if p[0] == q[0]:
        if (p[1] + q[1]) % P == 0:
            return None
        m = 3 * p[0] * p[0] * pow(2 * p[1], -1, P) % P
    else:
        m = (q[1] - p[1]) * pow(q[0] - p[0], -1, P) % P
    x = (m * m - p[0] - q[0]) % P
    return x, (m * (p[0] - x) - p[1]) % P


def _mul(pt, k):
    acc = None
    while k:
        if k & 1:
            acc = _add(acc, pt)
        pt = _add(pt, pt)
        k >>= 1
    return acc


@functools.lru_cache(maxsize=None)
def recover(v, r, s, chain_id, z):
    """-> ((x, y), 0) or (None, site)"""
    parity = v - 35 - 2 * chain_id
    if parity not in (0, 1) or not (0 < r < N and 0 < s < N):
        return None, 1
    y2 = (r**3 + 7) % P
    y = pow(y2, (P + 1) // 4, P)
    if y * y % P != y2:
        return None, 3
    if y & 1 != parity:
        y = P - y
    rinv = pow(r, -1, N)
    q = _add(_mul((r, y), s * rinv % N), _mul(G, -z * rinv % N))
    return (q, 0) if q is not None else (None, 4)


@functools.lru_cache(maxsize=None)
def _rlc(msg, randomness):
    acc = 0
    for b in msg:
        acc = (acc * randomness + b) % FR_MODULUS
    return acc


def assign(fields, to_none, calldata, offsets, chain_id, max_txs, max_calldata, randomness):
    """-> (status list, wire dict)"""
    n = len(to_none)
    status, fixed, cd, units, keccak = [], [], [], [], {(0, 0, 0, 0, 0)}
    for i in range(n):
        f = [int.from_bytes(fields[i, k].tobytes(), "little") for k in range(8)]
        nonce, gas_price, gas, to, value, v, r, s = f
        data = bytes(calldata[int(offsets[i]) : int(offsets[i + 1])])
        to_b = b"" if to_none[i] else to.to_bytes(20, "big")
        h = keccak256(rlp([nonce, gas_price, gas, to_b, value, data, chain_id, 0, 0]))
        z = int.from_bytes(h, "big")
        q, site = recover(v, r, s, chain_id, z)
        status.append(0 if q is None and site == 0 else ((15 << 24) | site if q is None else 0))
        x, y = q if q is not None else (0, 0)
        pk = x.to_bytes(32, "big") + y.to_bytes(32, "big")
        ph = keccak256(pk)
        addr = int.from_bytes(ph[-20:], "big")
        if q is not None:
            keccak.add((1, _rlc(pk, randomness), 64, int.from_bytes(ph[:16], "little"), int.from_bytes(ph[16:], "little")))
        gas_cost = sum(4 if b == 0 else 16 for b in data)
        m128 = (1 << 128) - 1
        vals = [(nonce % FR_MODULUS, 0, 0), (gas % FR_MODULUS, 0, 0), (gas_price & m128, gas_price >> 128, 1), (addr, 0, 0),
                (0 if to_none[i] else to, 0, 0), (1 if to_none[i] else 0, 0, 0), (value & m128, value >> 128, 1), (len(data), 0, 0),
                (gas_cost, 0, 0), (0, 0, 0), (0, 0, 0), (z & m128, z >> 128, 1)]
        fixed += [([i + 1, t + 1, 0, lo, hi], w) for t, (lo, hi, w) in enumerate(vals)]
        cd += [([i + 1, 13, k, b, 0], 0) for k, b in enumerate(data)]
        le = lambda x: list(x.to_bytes(32, "little"))  # noqa: E731
        units.append(([le(x), le(y), le(x), le(y), le(z), le(z), list(ph), le(r), le(s)], [addr, z & m128, z >> 128, 0, 0, 0, 0, 0]))
    for i in range(n, max_txs):
        fixed += [([i + 1, t + 1, 0, 0, 0], 1 if t in (2, 6) else 0) for t in range(12)]
        le = lambda x: list(x.to_bytes(32, "little"))  # noqa: E731
        units.append(([le(G[0]), le(G[1]), le(G[0]), le(G[1]), le(1), le(1), [0] * 32, le(G[0]), le(G[0] + 1)], [0] * 8))
    cd += [([0, 13, 0, 0, 0], 0)] * (max_calldata - len(cd))
    rows = fixed + cd
    wire = {
        "tx_rows": rows_to_rowmajor([r for r, _ in rows], 5), "tx_flags": np.array([w for _, w in rows], dtype=np.uint32),
        "bytes": np.array([u for u, _ in units], dtype=np.uint8).reshape(-1, 9, 32), "cells": rows_to_colmajor([c for _, c in units], 8),
        "meta": np.array([[PENDING, 1, 0, 0]] * len(units), dtype=np.uint32).reshape(-1, 4),
        "keccak": rows_to_rowmajor([list(k) for k in sorted(keccak)], 5),
    }
    return status, wire
