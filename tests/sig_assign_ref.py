"""Independent plain-Python model of the Sig circuit's witness assignment (zk_sig_assign, include/zkevm_hip.h) for the tests: signed data
(msg_hash, v, r, s) -> the Sig units, the keccak set, the EVM circuit's sig table and the ecRecover aux rows.  Built on
tests/tx_assign_ref.py's key recovery, keccak-256 and RLC (all memoised on their exact inputs, so a batch tiled from a few distinct
signatures costs only its row building); the layout below is this file's own statement of it.

Layout, per signature (m = the 32 hash bytes read little-endian, z = the same bytes read big-endian, p = v - v_offset):
  status   (15 << 24) | 1 if p not in {0, 1} or r, s not in (0, N); | 3 if no curve point has x = r; | 4 if Q is at infinity; else 0
  bytes    x LE, y LE, x LE, y LE, hash bytes, hash bytes, keccak256(x BE || y BE), r LE, s LE      (x = y = 0, digest row 0 if status)
  cells    claimed addr (or the recovered one; 0 if status), m lo, m hi, FQ(v.lo) - FQ(v_offset), r lo, r hi, s lo, s hi
  meta     (0xffffffff, expect_valid or 1, 0, p if 0 <= p < 2^32 else 0xffffffff)
  keccak   (1, RLC(x BE || y BE), 64, digest[:16] LE, digest[16:] LE) of every recovered key, with the zero row, as a sorted set
  sig row  (m lo, m hi, FQ(v.lo) - FQ(v_offset), r lo, r hi, s lo, s hi, recovered addr, 1) or (..., 0, 0); first occurrences, input order
  aux      m lo, m hi, v lo, v hi, r lo, r hi, s lo, s hi, recovered addr, RLC(m LE32 || v LE32 || r LE32 || s LE32),
           RLC(recovered addr LE32), randomness
RLC(bytes) is Horner with the first byte at the highest power."""
import numpy as np

from tests.tx_assign_ref import G, N, P, PENDING, _add, _mul, _rlc, keccak256, recover  # noqa: F401 (G, P, _add, _mul: for the cases)
from zkevm_specs_amd.wire import FR_MODULUS, rows_to_colmajor, rows_to_rowmajor

M128 = (1 << 128) - 1
BAD = 15 << 24


def word(x):
    return int.from_bytes(x.tobytes(), "little")


def sign(sk, z, k):
    """ECDSA over secp256k1 with the nonce k -> (parity, r, s), or None where r or s would be 0"""
    R = _mul(G, k % N)
    r = R[0] % N
    s = pow(k, -1, N) * (z + r * sk) % N
    if r == 0 or s == 0 or R[0] >= N:
        return None
    return R[1] & 1, r, s


def assign(fields, addr, expect_valid, v_offset, randomness):
    """-> (status list, wire dict with the keys of engine.SIG_ASSIGN_OUTPUTS)"""
    n = fields.shape[0]
    status, units, aux, sig_rows, seen, keccak = [], [], [], [], set(), {(0, 0, 0, 0, 0)}
    le = lambda x: list(x.to_bytes(32, "little"))  # noqa: E731
    for i in range(n):
        m, v, r, s = (word(fields[i, k]) for k in range(4))
        hb = m.to_bytes(32, "little")
        z = int.from_bytes(hb, "big")
        p = v - v_offset
        # tx_assign_ref.recover takes the Tx form of v: parity = v - 35 - 2 chain_id; chain_id 0 and v = p + 35 gives this parity
        q, site = recover(p + 35, r, s, 0, z) if 0 <= p < (1 << 64) else (None, 1)
        status.append(BAD | site if q is None else 0)
        x, y = q if q is not None else (0, 0)
        ph, rec = bytes(32), 0
        if q is not None:
            pk = x.to_bytes(32, "big") + y.to_bytes(32, "big")
            ph = keccak256(pk)
            rec = int.from_bytes(ph[-20:], "big")
            keccak.add((1, _rlc(pk, randomness), 64, int.from_bytes(ph[:16], "little"), int.from_bytes(ph[16:], "little")))
        vcell = ((v & M128) - v_offset) % FR_MODULUS
        claimed = word(addr[i]) if addr is not None else rec
        units.append(([le(x), le(y), le(x), le(y), list(hb), list(hb), list(ph), le(r), le(s)],
                      [claimed, m & M128, m >> 128, vcell, r & M128, r >> 128, s & M128, s >> 128],
                      [PENDING, int(expect_valid[i]) if expect_valid is not None else 1, 0, p if 0 <= p < (1 << 32) else 0xFFFFFFFF]))
        row = (m & M128, m >> 128, vcell, r & M128, r >> 128, s & M128, s >> 128, rec, 1 if q is not None else 0)
        if row not in seen:
            seen.add(row)
            sig_rows.append(list(row))
        inp = hb + v.to_bytes(32, "little") + r.to_bytes(32, "little") + s.to_bytes(32, "little")
        aux.append([m & M128, m >> 128, v & M128, v >> 128, r & M128, r >> 128, s & M128, s >> 128, rec, _rlc(inp, randomness),
                    _rlc(rec.to_bytes(32, "little"), randomness), randomness])
    wire = {
        "bytes": np.array([u for u, _, _ in units], dtype=np.uint8).reshape(-1, 9, 32),
        "cells": rows_to_colmajor([c for _, c, _ in units], 8) if n else np.zeros((8, 0, 4), dtype=np.uint64),
        "meta": np.array([mt for _, _, mt in units], dtype=np.uint32).reshape(-1, 4),
        "keccak": rows_to_rowmajor([list(k) for k in sorted(keccak)], 5),
        "sig_table": rows_to_rowmajor(sig_rows, 9) if sig_rows else np.zeros((0, 9, 4), dtype=np.uint64),
        "aux": rows_to_rowmajor(aux, 12) if n else np.zeros((0, 12, 4), dtype=np.uint64),
    }
    return status, wire
