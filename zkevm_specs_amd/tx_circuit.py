"""Host-side mirror of `zkevm_specs.tx_circuit.verify_circuit(witness, MAX_TXS, MAX_CALLDATA_BYTES,
keccak_randomness)` (tx_circuit.py:253-291), evaluated on the MI355X.  The reference verifies every tx's signature
with a third-party secp256k1 call inside `ECDSAVerifyChip.verify` (:147-158); here that verdict is computed on the device
too (`zk_ecdsa_verify` over the chips' limbs) and enters the Tx kernel (`zk_sign_verify`) as the `ecdsa_status` column.
The first failing unit's exception propagates, as in the reference."""
import sys

import numpy as np

from . import oneshot
from .errors import TX_BAD_SIGNATURE_SITES, UnsupportedOnDevice, bad_signature, raise_for_code
from .flatten import _n, flatten_tx_witness


def fill_ecdsa_column(wire, device=None):
    """Verdicts of the deferred chips (flatten_*_witness(..., ecdsa_on_device=True)) -> wire["meta"][:, 0]"""
    idx = np.nonzero(wire["ecdsa_deferred"])[0]
    if idx.size:
        v = None if wire["ecdsa_v"] is None else np.ascontiguousarray(wire["ecdsa_v"][idx])
        _, status = oneshot.ecdsa_verify(np.ascontiguousarray(wire["ecdsa_packed"][idx]), v, layout=0, device=device)
        wire["meta"][idx, 0] = status
    return wire


def verify_circuit(witness, MAX_TXS, MAX_CALLDATA_BYTES, keccak_randomness):
    if isinstance(witness, TxWitness):  # txs2witness's wire-backed witness: straight to the device
        wire = witness.verify_wire(MAX_TXS)
    else:
        wire = fill_ecdsa_column(flatten_tx_witness(witness, MAX_TXS, ecdsa_on_device=True))
    if wire["bytes"].shape[0] == 0:
        return None
    res, _ = oneshot.sign_verify(wire, _n(keccak_randomness), is_sig=False)
    raise_for_code(res.first_fail_code, f"Tx circuit tx_index {res.first_fail_row}")
    return res


verify_tx_circuit = verify_circuit  # round-1 name


def verify_sig_circuit(witness, keccak_randomness):
    from .sig_circuit import verify_circuit as sig_verify_circuit

    return sig_verify_circuit(witness, keccak_randomness)


# ---- txs2witness (tx_circuit.py:432-481) on the device: zk_tx_assign ------------------------------------------------------------
_U256 = 1 << 256
_SECP_N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141


class TxWitness:
    """The witness txs2witness returns when the reference is not loaded in this process: the wire of flatten_tx_witness (`wire`: tx_rows,
    tx_flags, bytes, cells, meta with meta[:, 0] pending, keccak) as zk_tx_assign wrote it.  verify_circuit takes it as it is."""

    def __init__(self, wire, max_txs, max_calldata_bytes):
        self.wire = wire
        self.max_txs = max_txs
        self.max_calldata_bytes = max_calldata_bytes

    def verify_wire(self, max_txs):
        """the wire with the ECDSA verdicts in meta[:, 0] (zk_ecdsa_verify over the units' byte rows, layout 1)"""
        w = dict(self.wire)
        m = min(int(max_txs), self.max_txs)
        w["bytes"], w["meta"] = np.ascontiguousarray(w["bytes"][:m]), w["meta"][:m].copy()
        w["cells"] = np.ascontiguousarray(w["cells"][:, :m])
        if m:
            _, status = oneshot.ecdsa_verify(w["bytes"], None, layout=1)
            w["meta"][:, 0] = status
        return w


def _rlp_error(value):
    """the exception rlp.encode raises for `value` (None if it encodes): rlp's own where it is installed, else the stand-in's classes"""
    try:
        import rlp  # noqa: F401
    except ImportError:
        if isinstance(value, bool):
            return TypeError("cannot RLP-encode bool")
        if isinstance(value, int):
            return ValueError("negative int") if value < 0 else None
        return None if isinstance(value, (bytes, bytearray)) else TypeError(f"cannot RLP-encode {type(value)}")
    try:
        rlp.encode(value)
    except Exception as e:  # noqa: BLE001 - rlp's exception is the outcome
        return e
    return None


def _int_field(value):
    """(wire int, host exception or None) of an int item of the signing payload"""
    if type(value) is int or (isinstance(value, int) and not isinstance(value, bool)):
        if value < 0:
            return 0, _rlp_error(value) or ValueError("negative int")
        if value >= _U256:
            return 0, UnsupportedOnDevice("an int field wider than 256 bits: outside the device's wire")
        return int(value), None
    e = _rlp_error(value)
    if e is not None:
        return 0, e
    if isinstance(value, int):
        return int(value), None
    return 0, UnsupportedOnDevice(f"a {type(value).__name__} field: outside the device's wire")


def _sig_field(value):
    """wire int of sig_r / sig_s: a value outside [0, 2^256) becomes one that fails the range check the same way"""
    if not isinstance(value, int) or isinstance(value, bool):
        return 0, UnsupportedOnDevice(f"a {type(value).__name__} signature field: outside the device's wire")
    return (int(value) if 0 <= value < _U256 else 0), None


def tx_inputs(txs, chain_id, MAX_TXS, MAX_CALLDATA_BYTES):
    """The inputs of zk_tx_assign for the reference's `Transaction` tuples (or any objects with those fields), classified on the host
    where the outcome depends on Python types: -> (dict for engine._tx_assign_args, {tx index: exception its encoding raises})"""
    n = len(txs)
    fields = np.zeros((n, 8, 4), dtype=np.uint64)
    to_none = np.zeros(n, dtype=np.uint32)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    errors = {}
    chain_err = None
    chain = 0
    if isinstance(chain_id, int) and not isinstance(chain_id, bool) and 0 <= chain_id < (1 << 64):
        chain = int(chain_id)
    else:
        _, chain_err = _int_field(chain_id)
        if chain_err is None:
            chain_err = UnsupportedOnDevice("chain_id wider than 64 bits: outside the device's wire")
    vals = np.zeros((n, 8), dtype=object)
    datas = []
    for i, tx in enumerate(txs):
        err = None
        to = tx.to
        if to is None:
            to_none[i] = 1
            to_v = 0
        else:
            try:
                to.to_bytes(20, "big")  # encode_to (tx_circuit.py:311-314), evaluated before rlp.encode
                to_v = int(to)
            except Exception as e:  # noqa: BLE001 - the reference's exception is the outcome
                err, to_v = e, 0
        row = [0] * 8
        for k, name in ((0, "nonce"), (1, "gas_price"), (2, "gas")):
            row[k], e = _int_field(getattr(tx, name))
            err = err or e
        row[3] = to_v
        row[4], e = _int_field(tx.value)
        err = err or e
        data = tx.data
        if not isinstance(data, (bytes, bytearray)):
            e = _rlp_error(data)
            err = err or e or UnsupportedOnDevice(f"a {type(data).__name__} data field: outside the device's wire")
            data = b""
        err = err or chain_err
        if err is None:
            try:
                parity = tx.sig_v - 35 - chain * 2
                row[5] = int(tx.sig_v) if parity in (0, 1) else 0  # any other parity: a wire v that fails the same check
            except Exception as e:  # noqa: BLE001
                err = e
        for k, name in ((6, "sig_r"), (7, "sig_s")):
            row[k], e = _sig_field(getattr(tx, name))
            if err is None and e is not None:
                err = e
        if err is not None:
            errors[i] = err
            row = [0] * 8
            data = b""
        vals[i] = row
        datas.append(bytes(data))
        offsets[i + 1] = offsets[i] + len(data)
    if n:
        raw = b"".join(int(v).to_bytes(32, "little") for v in vals.reshape(-1))
        fields = np.frombuffer(raw, dtype="<u8").reshape(n, 8, 4).copy()
    calldata = np.frombuffer(b"".join(datas), dtype=np.uint8).copy()
    tx = {"fields": fields, "to_is_none": to_none, "calldata": calldata, "offsets": offsets, "chain_id": chain,
          "max_txs": int(MAX_TXS), "max_calldata_bytes": max(int(MAX_CALLDATA_BYTES), int(offsets[-1]))}
    return tx, errors


def _reference_witness(mod, wire, n_real):
    """the reference's own Witness / Row / KeccakTable / SignVerifyChip objects over the wire (when the reference is loaded)"""
    from zkevm_specs.util import FQ, Word

    from .wire import cells_to_ints

    tx_rows = wire["tx_rows"]
    ints = cells_to_ints(tx_rows.reshape(-1, 4))
    rows = []
    for j in range(tx_rows.shape[0]):
        tx_id, tag, index, lo, hi = ints[5 * j : 5 * j + 5]
        val = Word(lo | (hi << 128)) if wire["tx_flags"][j] else FQ(lo)
        rows.append(mod.Row(FQ(tx_id), FQ(tag), FQ(index), val))
    kt = mod.KeccakTable()
    kints = cells_to_ints(wire["keccak"].reshape(-1, 4))
    for j in range(wire["keccak"].shape[0]):
        e, rlc, ln, lo, hi = kints[5 * j : 5 * j + 5]
        if e == 0 and rlc == 0 and ln == 0 and lo == 0 and hi == 0:
            continue  # (the table's own all-zero row)
        kt.table.add((FQ(e), FQ(rlc), FQ(ln), Word(lo.to_bytes(16, "little") + hi.to_bytes(16, "little"))))
    bts = wire["bytes"]
    addr = cells_to_ints(wire["cells"][0])
    svs = []
    for i in range(n_real):
        b = [bytes(bts[i, k]) for k in range(9)]
        x, y, z = int.from_bytes(b[0], "little"), int.from_bytes(b[1], "little"), int.from_bytes(b[4], "little")
        r, s = int.from_bytes(b[7], "little"), int.from_bytes(b[8], "little")
        chip = mod.ECDSAVerifyChip((mod.Secp256k1ScalarField(r), mod.Secp256k1ScalarField(s)),
                                   (mod.Secp256k1BaseField(x), mod.Secp256k1BaseField(y)), mod.Secp256k1ScalarField(z))
        svs.append(mod.SignVerifyChip(b[6], FQ(addr[i]), Word(z), chip))
    pad = bts.shape[0] - n_real
    if pad:
        dummy = mod.ECDSAVerifyChip((mod.Secp256k1ScalarField(mod.DUMMY_SIGNATURE[0]), mod.Secp256k1ScalarField(mod.DUMMY_SIGNATURE[1])),
                                    (mod.Secp256k1BaseField(mod.DUMMY_PUBLIC_KEY[0]), mod.Secp256k1BaseField(mod.DUMMY_PUBLIC_KEY[1])),
                                    mod.Secp256k1ScalarField(mod.DUMMY_MSG_HASH))
        svs += [mod.SignVerifyChip(bytes(32), FQ(0), Word(0), dummy)] * pad
    return mod.Witness(rows, kt, svs)


def txs2witness(txs, chain_id, MAX_TXS, MAX_CALLDATA_BYTES, keccak_randomness, device=None):
    """Mirror of `zkevm_specs.tx_circuit.txs2witness` (tx_circuit.py:432-481): the signing hashes, the senders' key recovery, the
    tx-table rows, the SignVerify units and the keccak rows computed by zk_tx_assign.  Raises as the reference does, at the first
    failing tx: AssertionError for too many txs / calldata bytes, BadSignature (eth_keys') for an unrecoverable signature, rlp's
    exception for a value it refuses (UnsupportedOnDevice for ints wider than the wire).  Returns the reference's own Witness objects
    when the reference is loaded in this process (its tests edit them), else a TxWitness; verify_circuit takes either."""
    assert len(txs) <= MAX_TXS
    tx, errors = tx_inputs(txs, chain_id, MAX_TXS, MAX_CALLDATA_BYTES)
    _, status, wire = oneshot.tx_assign(tx, int(getattr(keccak_randomness, "n", keccak_randomness)), device=device)
    for i in range(len(txs)):
        if i in errors:
            raise errors[i]
        if status[i]:
            site = int(status[i]) & 0xFFFFFF
            raise bad_signature(f"tx {i}: {TX_BAD_SIGNATURE_SITES.get(site, 'invalid signature')}")
    assert int(tx["offsets"][-1]) <= MAX_CALLDATA_BYTES
    mod = sys.modules.get("zkevm_specs.tx_circuit")
    if mod is not None and hasattr(mod, "Witness"):
        return _reference_witness(mod, wire, len(txs))
    return TxWitness(wire, int(MAX_TXS), int(MAX_CALLDATA_BYTES))
