#!/usr/bin/env python3
"""Golden cases of the PI circuit's witness assignment: tests/golden/pi_assign_cases.npz.

Runs the unmodified reference's `public_data2witness` (src/zkevm_specs/pi_circuit.py:839-1073) over the third-party stand-ins of
oracle/refshim on the deterministic public data of tests/pi_assign_cases.build_cases and records, per case, every output of the
assignment: the flattened rows (rpi_bytes_keccakrlc, 32 random bytes per row, as its SHA-256 plus sampled cells; the other 23 columns
in full), the gas-cost and keccak tables, the block / tx / withdrawal tables, the public inputs, copy_constrains and the copy
constraints verify_circuit lists over them; for the rejected inputs the exception's class.  Needs the reference checkout (--ref-root);
the cases are data, the generator stays out of the test run.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-root", required=True, help="checkout of the reference (its src/ is imported unmodified)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "pi_assign_cases.npz"))
    args = ap.parse_args()
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle", "refshim"), os.path.join(args.ref_root, "src")]
    from zkevm_specs import pi_circuit as ref
    from zkevm_specs.util import U64, U160, U256

    from tests.pi_assign_cases import RLC_COLUMN, build_cases, column_digest
    from zkevm_specs_amd.flatten import _n, flatten_keccak_tuples, flatten_pi_gas_table, flatten_pi_rows
    from zkevm_specs_amd.pi_circuit import list_copy_constraints

    def to_ref(pd):
        b = pd.block
        blk = ref.Block(U256(b.hash), U256(b.parent_hash), U256(b.uncle_hash), U160(b.coinbase), U256(b.state_root), U256(b.tx_hash),
                        U256(b.receipt_hash), b.bloom, U256(b.prev_randao), U64(b.number), U64(b.gas_limit), U64(b.gas_used), U64(b.time),
                        b.extra, U256(b.mix_digest), U64(b.nonce), U256(b.base_fee), U256(b.withdrawals_root))
        txs = [ref.Transaction(U64(t.nonce), U256(t.gas_price), U64(t.gas), U160(t.from_addr), None if t.to_addr is None else U160(t.to_addr),
                               U256(t.value), t.data, U256(t.tx_sign_hash)) for t in pd.txs]
        wds = [ref.Withdrawal(U64(w.id), U64(w.validator_id), U160(w.address), U64(w.amount)) for w in pd.withdrawals]
        return ref.PublicData(U64(pd.chain_id), blk, U256(pd.state_root_prev), [U256(h) for h in pd.block_hashes], txs, wds)

    cells = lambda rows: np.frombuffer(b"".join(int(v).to_bytes(32, "little") for r in rows for v in r), dtype="<u8").reshape(len(rows), -1, 4)  # noqa: E731
    out, names = {}, []
    for k, (name, pd, shape, exc) in enumerate(build_cases()):
        key = f"c{k:03d}_"
        names.append(name)
        try:
            w = ref.public_data2witness(to_ref(pd), *shape)
            got = None
        except Exception as e:  # noqa: BLE001 - the class is the recorded outcome
            got = type(e).__name__
        assert got == exc, (name, got, exc)
        if exc is not None:
            out[key + "exception"] = np.array([exc])
            continue
        rows = flatten_pi_rows(w.rows)
        out[key + "rows23"] = rows[[c for c in range(24) if c != RLC_COLUMN]]
        out[key + "rlc_sha"], out[key + "rlc_idx"], out[key + "rlc_val"] = column_digest(rows[RLC_COLUMN])
        out[key + "gas"] = flatten_pi_gas_table(w.calldata_gas_cost_table).reshape(-1, 3, 4)
        out[key + "keccak"] = flatten_keccak_tuples(w.keccak_table.table).reshape(-1, 5, 4)
        out[key + "block_table"] = cells([[_n(x.lo), _n(x.hi)] for x in w.block_table.table])
        out[key + "block_flags"] = np.array([int(x.is_word) for x in w.block_table.table], dtype=np.uint32)
        out[key + "tx_table"] = cells([[_n(t.tx_id), _n(t.tag), _n(t.index), _n(t.value.lo), _n(t.value.hi)] for t in w.tx_table.table])
        out[key + "tx_flags"] = np.array([int(t.value.is_word) for t in w.tx_table.table], dtype=np.uint32)
        out[key + "wd_table"] = cells([[_n(x.id), _n(x.validator_id), _n(x.address.lo), _n(x.address.hi), _n(x.amount)] for x in w.withdrawal_table.table])
        p = w.public_inputs
        out[key + "public_inputs"] = cells([[_n(x.lo), _n(x.hi)] for x in (p.pi_keccak, p.block_hash, p.state_root, p.state_root_prev)])
        cc = [bytes(x) for x in w.copy_constrains]
        out[key + "raw_bytes"] = np.frombuffer(b"".join(cc), dtype=np.uint8)
        out[key + "raw_lens"] = np.array([len(x) for x in cc], dtype=np.uint32)
        w.copy_constrains = list(cc)
        C, pending = list_copy_constraints(w, *shape)
        assert pending is None and not w.copy_constrains
        out[key + "cc_cells"], out[key + "cc_bytes"], out[key + "cc_lens"] = C.wire()
        print(f"{name}: {rows.shape[1]} rows", flush=True)
    out["names"] = np.array(names)
    np.savez_compressed(args.out, **out)
    print(f"{len(names)} cases -> {os.path.getsize(args.out) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
