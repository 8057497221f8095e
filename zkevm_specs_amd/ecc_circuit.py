"""Host-side mirror of `zkevm_specs.ecc_circuit` (ecc_circuit.py:386-433): circuit2rows assigns every row on the device
(`zk_ecc_assign`), verify_circuit checks the rows against the ops' chips (`zk_ecc_verify`).  Needs no py_ecc: the BN254
arithmetic, the exact affine chains and the pairing are csrc/bn254_fq.hpp.

calls2witness goes one step further back: from the INPUTS of ecAdd / ecMul / ecPairing calls (`zk_ecc_from_calls`) to the ops with
their results filled in, the rows, and the EVM circuit's ecc table and aux rows."""
from typing import List, NamedTuple, Tuple

import numpy as np

from . import oneshot
from .errors import raise_for_code
from .flatten import _word_limbs, flatten_ecc_ops


def _randomness(r):
    return int(r.n if hasattr(r, "n") else r)


def _wire(circuit):
    return flatten_ecc_ops(circuit.add_ops, circuit.mul_ops, circuit.pairing_ops, circuit.max_add_ops, circuit.max_mul_ops,
                           circuit.max_pairing_ops)


def circuit2rows(circuit, randomness_keccak):
    """EccTableRow wire rows uint64[n, 13, 4] of `circuit` (any object with add_ops / mul_ops / pairing_ops / max_*_ops), in
    circuit2rows order; the cells flatten_ecc_table produces."""
    return oneshot.ecc_assign(_wire(circuit), _randomness(randomness_keccak))


def verify_circuit(circuit, randomness_keccak):
    """The reference's verify_circuit: raises the exception of the first failing row (AssertionError / AttributeError)."""
    w = _wire(circuit)
    r = _randomness(randomness_keccak)
    if w["points"].shape[0] + w["pair_out"].shape[0] == 0:
        return None
    rows = oneshot.ecc_assign(w, r)
    res, _ = oneshot.ecc_verify(w, rows, r)
    raise_for_code(res.first_fail_code, f"ECC circuit row {res.first_fail_row}")
    return res


# ---- from the precompiles' inputs (zk_ecc_from_calls) ---------------------------------------------------------------------------
class EcAdd(NamedTuple):
    p: Tuple[int, int]
    q: Tuple[int, int]
    out: Tuple[int, int]


class EcMul(NamedTuple):
    p: Tuple[int, int]
    s: int
    out: Tuple[int, int]


class EcPairing(NamedTuple):
    g1_pts: List[Tuple[int, int]]
    g2_pts: List[Tuple[int, int, int, int]]
    out: int


class EccCallsWitness(NamedTuple):
    add_ops: List[EcAdd]         # the calls as the reference's ops, `out` filled with the precompile's result ((0, 0) / 0 when invalid)
    mul_ops: List[EcMul]
    pairing_ops: List[EcPairing]
    rows: np.ndarray             # uint64[n, 13, 4]: circuit2rows' rows (adds, muls, pairings)
    ecc_table: np.ndarray        # uint64[m, 13, 4]: the EVM circuit's ecc table (a set: first occurrences, input order)
    aux: dict                    # {"aux": uint64[n, 12, 4], "aux_kind": uint32[n]}: flatten_step_aux's arrays, row i for call i
    wire: dict                   # the zk_ecc_ops arrays of the ops (flatten_ecc_ops' keys; max_ok all 1)


def _be_words(data, n_words):
    """the first n_words 32-byte big-endian words of `data`, right-padded with zeros (EIP-196: short input is zero-extended, bytes
    beyond the words are ignored)"""
    data = bytes(data)[: 32 * n_words].ljust(32 * n_words, b"\0")
    return [int.from_bytes(data[32 * k: 32 * k + 32], "big") for k in range(n_words)]


def ecadd_words(data):
    """ecAdd's input bytes -> (p, q)"""
    w = _be_words(data, 4)
    return (w[0], w[1]), (w[2], w[3])


def ecmul_words(data):
    """ecMul's input bytes -> (p, s)"""
    w = _be_words(data, 3)
    return (w[0], w[1]), w[2]


def ecpairing_words(data):
    """ecPairing's input bytes -> (g1_pts, g2_pts), the G2 words in the input's own (EIP-197) order x.c1, x.c0, y.c1, y.c0.  A length
    that is no multiple of 192 cannot be expressed in pairs: the call fails in the EVM and is the caller's to handle."""
    data = bytes(data)
    if len(data) % 192:
        raise ValueError(f"ecPairing input of {len(data)} bytes is not a whole number of pairs")
    w = _be_words(data, len(data) // 32)
    return [(w[k], w[k + 1]) for k in range(0, len(w), 6)], [tuple(w[k + 2: k + 6]) for k in range(0, len(w), 6)]


def ecc_calls_wire(adds, muls, pairings):
    """adds [(p, q)], muls [(p, s)], pairings [(g1_pts, g2_pts)] (tuples, or the ops above: a trailing `out` is ignored) -> the
    zk_ecc_calls arrays: add_in uint64[n, 4, 4], mul_in uint64[n, 3, 4], pair_pts uint64[m, 6, 4], pair_off uint32[n + 1]"""
    add_in = [[_word_limbs(x) for x in (op[0][0], op[0][1], op[1][0], op[1][1])] for op in adds]
    mul_in = [[_word_limbs(x) for x in (op[0][0], op[0][1], op[1])] for op in muls]
    pair_pts, off = [], [0]
    for op in pairings:
        for g1, g2 in zip(op[0], op[1]):
            pair_pts.append([_word_limbs(x) for x in (g1[0], g1[1], g2[0], g2[1], g2[2], g2[3])])
        off.append(len(pair_pts))
    return {"add_in": np.array(add_in, dtype=np.uint64).reshape(len(add_in), 4, 4),
            "mul_in": np.array(mul_in, dtype=np.uint64).reshape(len(mul_in), 3, 4),
            "pair_pts": np.array(pair_pts, dtype=np.uint64).reshape(len(pair_pts), 6, 4),
            "pair_off": np.array(off, dtype=np.uint32)}


def _word_int(cell):
    return sum(int(cell[k]) << (64 * k) for k in range(4))


def calls2witness(adds, muls, pairings, randomness_keccak, device=None):
    """The witness of a block's ecAdd / ecMul / ecPairing calls from their inputs (see ecc_calls_wire), computed on the device
    (`zk_ecc_from_calls`): the reference's ops with `out` filled, the ECC circuit's rows, and the EVM circuit's ecc table and aux rows."""
    adds, muls, pairings = list(adds), list(muls), list(pairings)
    calls = ecc_calls_wire(adds, muls, pairings)
    _, _, out = oneshot.ecc_from_calls(calls, _randomness(randomness_keccak), device=device)
    pts, n_add = out["points"], len(adds)
    res = [(_word_int(w[4]), _word_int(w[5])) for w in pts]
    add_ops = [EcAdd(tuple(op[0]), tuple(op[1]), res[k]) for k, op in enumerate(adds)]
    mul_ops = [EcMul(tuple(op[0]), int(op[1]), res[n_add + k]) for k, op in enumerate(muls)]
    pairing_ops = [EcPairing([tuple(g) for g in op[0]], [tuple(g) for g in op[1]], _word_int(out["pair_out"][k])) for k, op in enumerate(pairings)]
    wire = {"points": pts, "n_add": n_add, "n_mul": len(muls), "pair_pts": calls["pair_pts"], "pair_off": calls["pair_off"],
            "pair_out": out["pair_out"], "max_ok": np.ones(3, dtype=np.uint32)}
    return EccCallsWitness(add_ops, mul_ops, pairing_ops, out["rows"], out["ecc_table"], {"aux": out["aux"], "aux_kind": out["aux_kind"]}, wire)
