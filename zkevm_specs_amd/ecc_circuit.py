"""Host-side mirror of `zkevm_specs.ecc_circuit` (ecc_circuit.py:386-433): circuit2rows assigns every row on the device
(`zk_ecc_assign`), verify_circuit checks the rows against the ops' chips (`zk_ecc_verify`).  Needs no py_ecc: the BN254
arithmetic, the exact affine chains and the pairing are csrc/bn254_fq.hpp."""
from . import oneshot
from .errors import raise_for_code
from .flatten import flatten_ecc_ops


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
