"""zk_evm_witness_from_trace: a plain-Python model of the expansion, written from the reference's statements.  FQ(x) is x mod p
(util/arithmetic.py), Word(w) is (w mod 2^128, w >> 128) (:99-110), WordOrValue of a Word keeps both halves and of an FQ is (value, 0)
(:171-186); RWTableRow's fields in table.py:447-457's order and StepState's in the order flatten_steps reads them."""
import numpy as np

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
M64, M128 = (1 << 64) - 1, (1 << 128) - 1


def _word(limbs):
    return sum(int(x) << (64 * k) for k, x in enumerate(limbs))


def _cells(rows, nc):
    raw = b"".join(int(v).to_bytes(32, "little") for r in rows for v in r)
    return np.frombuffer(raw, dtype="<u8").reshape(len(rows), nc, 4).astype(np.uint64)


def model(rec):
    """records dict (zkevm_specs_amd.trace) -> dict(rw uint64[n, 14, 4], rw_flags uint32[n], steps uint64[k, 13, 4])"""
    head = [int(h) for h in rec["head"]]
    pool = [_word(w) for w in rec["pool"]]
    at, rows, flags = 0, [], []
    for i, h in enumerate(head):
        def take(bit):
            nonlocal at
            if not (h >> bit) & 1:
                return None
            at += 1
            return pool[at - 1]
        ctr = int(rec["rw_counter"][i]) if rec.get("rw_counter") is not None else int(rec.get("rw_base", 1)) + i
        a, key, v, p, aux = take(20), take(21), take(22), take(23), take(24)
        address = int(rec["addr"][i]) if a is None else a % P       # FQ(address)
        key = 0 if key is None else key                              # Word
        aux = 0 if aux is None else aux
        cells = [ctr, h & 1, (h >> 1) & 15, int(rec["id"][i]), address, (h >> 8) & 255, key & M128, key >> 128]
        for wide, narrow, is_word in ((v, rec["val"], (h >> 16) & 1), (p, rec["prev"], (h >> 17) & 1)):
            if wide is None:
                cells += [int(narrow[i]), 0]                         # a value below 2^64: (v, 0) as a Word or as an FQ
            elif is_word:
                cells += [wide & M128, wide >> 128]                  # WordOrValue(Word(w))
            else:
                cells += [wide % P, 0]                               # WordOrValue(FQ(w))
        cells += [aux & M128, aux >> 128]
        rows.append(cells)
        flags.append((h >> 16) & 3)
    assert at == len(pool)
    steps = []
    for r in rec["steps"]:
        r = [int(x) for x in r]
        steps.append([r[0] & 255, r[1], r[2], (r[0] >> 8) & 1, (r[0] >> 9) & 1, r[9] | (r[10] << 64), r[11] | (r[12] << 64), *r[3:9]])
    return {"rw": _cells(rows, 14), "rw_flags": np.array(flags, dtype=np.uint32), "steps": _cells(steps, 13)}
