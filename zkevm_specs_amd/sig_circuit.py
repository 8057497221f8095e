"""Host-side mirror of `zkevm_specs.sig_circuit.verify_circuit(witness, keccak_randomness)` (sig_circuit.py:113-122:
`Row.verify` :64-104 per signature row), evaluated on the MI355X (`zk_ecdsa_verify` for the chips' verdicts, then
`zk_sign_verify` with Sig-circuit semantics), and the witness itself from signed data (`zk_sig_assign`): what the reference's
tests build in `signedData2witness` (tests/test_sig_circuit.py:40-67), plus the EVM circuit's sig table and ecRecover aux rows
(tests/evm/precompiles/test_ecRecover.py:78-112) from the same key recovery."""
import sys

import numpy as np

from . import oneshot
from .errors import TX_BAD_SIGNATURE_SITES, UnsupportedOnDevice, bad_signature, raise_for_code
from .flatten import _n, flatten_sig_witness
from .tx_circuit import fill_ecdsa_column
from .wire import FR_MODULUS

_U256 = 1 << 256


def verify_circuit(witness, keccak_randomness):
    if isinstance(witness, SigWitness):  # signed_data2witness's wire-backed witness: straight to the device
        wire = witness.verify_wire()
    else:
        wire = fill_ecdsa_column(flatten_sig_witness(witness, ecdsa_on_device=True))
    if wire["bytes"].shape[0] == 0:
        return None
    res, _ = oneshot.sign_verify(wire, _n(keccak_randomness), is_sig=True)
    raise_for_code(res.first_fail_code, f"Sig circuit row {res.first_fail_row}")
    return res


# ---- signedData2witness on the device: zk_sig_assign ------------------------------------------------------------------------------
class SigWitness:
    """The witness signed_data2witness returns when the reference is not loaded in this process: the wire of flatten_sig_witness
    (`wire`: bytes, cells, meta with meta[:, 0] pending, keccak) as zk_sig_assign wrote it.  verify_circuit takes it as it is."""

    def __init__(self, wire):
        self.wire = wire

    def verify_wire(self, device=None):
        """the wire with the ECDSA verdicts in meta[:, 0] (zk_ecdsa_verify over the units' byte rows, layout 2, v = meta[:, 3])"""
        w = {k: self.wire[k] for k in ("bytes", "cells", "keccak")}
        w["meta"] = self.wire["meta"].copy()
        w["tx_rows"], w["tx_flags"] = np.zeros((0, 5, 4), dtype=np.uint64), np.zeros(0, dtype=np.uint32)
        if w["bytes"].shape[0]:
            _, status = oneshot.ecdsa_verify(w["bytes"], np.ascontiguousarray(w["meta"][:, 3]), layout=2, device=device)
            w["meta"][:, 0] = status
        return w


def sig_inputs(signed_data, v_offset=0):
    """The inputs of zk_sig_assign for the reference tests' `SignedData` tuples (or any objects with msg_hash, sig_v, sig_r, sig_s, addr):
    -> (dict for engine._sig_assign_args, {index: exception for a value outside the device's wire}).  A v / r / s outside [0, 2^256)
    becomes one that fails the same range check."""
    n = len(signed_data)
    vals, addrs, errors = [], [], {}
    for i, d in enumerate(signed_data):
        h = bytes(d.msg_hash)
        if len(h) != 32:
            errors[i] = UnsupportedOnDevice(f"a message hash of {len(h)} bytes: outside the device's wire")
            h = bytes(32)
        row = [int.from_bytes(h, "little")]
        for k, name in enumerate(("sig_v", "sig_r", "sig_s")):
            x = getattr(d, name)
            if not isinstance(x, int) or isinstance(x, bool):
                errors.setdefault(i, UnsupportedOnDevice(f"a {type(x).__name__} signature field: outside the device's wire"))
                x = -1
            row.append(int(x) if 0 <= x < _U256 else (_U256 - 1 if k == 0 else 0))
        vals.append(row)
        addrs.append(int(_n(getattr(d, "addr", 0))) % FR_MODULUS)
    raw = b"".join(x.to_bytes(32, "little") for row in vals for x in row)
    sig = {"fields": np.frombuffer(raw, dtype="<u8").reshape(n, 4, 4).copy(),
           "addr": np.frombuffer(b"".join(x.to_bytes(32, "little") for x in addrs), dtype="<u8").reshape(n, 4).copy(),
           "expect_valid": None, "v_offset": int(v_offset)}
    return sig, errors


def _raise_first(status, errors, n):
    for i in range(n):
        if i in errors:
            raise errors[i]
        if status[i]:
            site = int(status[i]) & 0xFFFFFF
            raise bad_signature(f"signature {i}: {TX_BAD_SIGNATURE_SITES.get(site, 'invalid signature')}")


def _reference_witness(mod, wire):
    """the reference's own Witness / Row / KeccakTable / ECDSAVerifyChip objects over the wire (when the reference is loaded)"""
    from zkevm_specs.util import FQ, Secp256k1BaseField, Secp256k1ScalarField, Word

    from .wire import cells_to_ints

    kt = mod.KeccakTable()
    kints = cells_to_ints(wire["keccak"].reshape(-1, 4))
    for j in range(wire["keccak"].shape[0]):
        e, rlc, ln, lo, hi = kints[5 * j : 5 * j + 5]
        if e == 0 and rlc == 0 and ln == 0 and lo == 0 and hi == 0:
            continue  # (the table's own all-zero row)
        kt.table.add((FQ(e), FQ(rlc), FQ(ln), Word(lo.to_bytes(16, "little") + hi.to_bytes(16, "little"))))
    bts, addr = wire["bytes"], cells_to_ints(wire["cells"][0])
    rows = []
    for i in range(bts.shape[0]):
        b = [bytes(bts[i, k]) for k in range(9)]
        x, y, z = int.from_bytes(b[0], "little"), int.from_bytes(b[1], "little"), int.from_bytes(b[4], "big")
        v, r, s = int(wire["meta"][i, 3]), int.from_bytes(b[7], "little"), int.from_bytes(b[8], "little")
        chip = mod.ECDSAVerifyChip((Secp256k1ScalarField(v), Secp256k1ScalarField(r), Secp256k1ScalarField(s)),
                                   (Secp256k1BaseField(x), Secp256k1BaseField(y)), Secp256k1ScalarField(z))
        rows.append(mod.Row(b[6], FQ(addr[i]), Word(b[5]), chip))
    return mod.Witness(rows, kt)


def signed_data2witness(signed_data, keccak_randomness, device=None):
    """Mirror of the reference tests' `signedData2witness`: the signers' key recovery, the key hashes, the units and the keccak rows
    computed by zk_sig_assign.  Raises eth_keys' BadSignature at the first signature no key can be recovered from.  Returns the
    reference's own Witness objects when the reference is loaded in this process (its tests edit them), else a SigWitness;
    verify_circuit takes either."""
    sig, errors = sig_inputs(signed_data, 0)
    _, status, wire = oneshot.sig_assign(sig, int(_n(keccak_randomness)), device=device)
    _raise_first(status, errors, len(signed_data))
    mod = sys.modules.get("zkevm_specs.sig_circuit")
    if mod is not None and hasattr(mod, "Witness"):
        return _reference_witness(mod, wire)
    return SigWitness(wire)


def sig_table(signed_data, keccak_randomness, v_offset=27, device=None):
    """The EVM circuit's sig table and the ecRecover aux rows of `signed_data` (sig_v: the precompile's input word, parity + v_offset)
    -> (sig rows uint64[m, 9, 4]: the distinct rows in first-occurrence order, aux uint64[n, 12, 4]: row i for signature i), ready for
    zk_evm_tables.sig / .aux (kind 5).  A signature no key can be recovered from gets the row (..., 0, 0), as the precompile returns
    nothing for it."""
    sig, errors = sig_inputs(signed_data, v_offset)
    sig["addr"] = None
    for i in sorted(errors):
        raise errors[i]
    _, _, wire = oneshot.sig_assign(sig, int(_n(keccak_randomness)), device=device)
    return wire["sig_table"], wire["aux"]
