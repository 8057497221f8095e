"""Plain-Python model of the gather of zk_copy_assign_from_sources (include/zkevm_hip.h): one loop per byte, no numpy in the logic.

model(events, src_ref, dst_ref, sources) -> (data, offsets, status): the uint16 source data `value | is_code << 8` of every event, its
offsets, and the status per event.  Expected rows are then zk_copy_assign's over (data, offsets)."""
import numpy as np

BYTECODE, MEMORY, TX_CALLDATA, TX_LOG, RLC_ACC = 1, 2, 3, 4, 5
TARGET_MEMORY = 9
H_WRITE, H_TAG_SHIFT, H_ADDR_POOL, H_VALUE_POOL = 1, 1, 1 << 20, 1 << 22
VALUE_ERROR = 9


def code_of(site):
    return (VALUE_ERROR << 24) | site if site else 0


def init_is_code(code):
    """the reference's init_is_code (evm_circuit/typing.py:317-324) over the bytes of one code"""
    out, left = [], 0
    for b in code:
        out.append(1 if left == 0 else 0)
        left = (b - 0x5F if 0x60 <= b <= 0x7F else 0) if left == 0 else left - 1
    return out


def _slices(blob, offsets):
    blob = bytes(np.asarray(blob, dtype=np.uint8).tobytes()) if blob is not None else b""
    offsets = [int(x) for x in offsets] if offsets is not None else [0]
    return [blob[offsets[j]:offsets[j + 1]] for j in range(len(offsets) - 1)]


def _ints(cells):
    """uint64[n, 12, 4] -> list of 12-int rows"""
    cells = np.asarray(cells, dtype=np.uint64)
    return [[int.from_bytes(cells[e, k].tobytes(), "little") for k in range(12)] for e in range(cells.shape[0])]


def model(events, src_ref, dst_ref, sources):
    codes = _slices(sources.get("code"), sources.get("code_offsets"))
    txs = _slices(sources.get("calldata"), sources.get("calldata_offsets"))
    is_code = [init_is_code(c) for c in codes]
    tr = sources.get("trace") or {}
    n_rw = 0 if tr.get("head") is None else len(tr["head"])
    if tr.get("rw_counter") is not None:
        op_at = {int(c): k for k, c in enumerate(tr["rw_counter"])}
    else:
        op_at = {int(tr.get("rw_base", 1)) + k: k for k in range(n_rw)}
    data, offsets, status = [], [0], []
    for e, (s_lo, s_hi, s_tag, _d_lo, _d_hi, d_tag, src_addr, src_end, dst_addr, length, _log, rwc) in enumerate(_ints(events)):
        n_real = min(length, max(src_end - src_addr, 0))
        sref = int(src_ref[e])
        dref = int(dst_ref[e]) if dst_ref is not None else None
        # per-event sites, the lowest wins
        site = 0
        src = codes if s_tag == BYTECODE else txs if s_tag == TX_CALLDATA else None
        if (src is not None and sref >= len(src)) or (d_tag == BYTECODE and dref >= len(codes)):
            site = 1
        elif src is not None and n_real > 0 and src_end > len(src[sref]):
            site = 2
        elif d_tag == BYTECODE and dst_addr + n_real > len(codes[dref]):
            site = 3
        first_bad = 0
        for i in range(n_real):
            if site:
                data.append(0)
                continue
            bad = 0
            if s_tag == MEMORY:
                stride = 2 if d_tag in (MEMORY, TX_LOG) else 1
                k = op_at.get(rwc + i * stride)
                if k is None:
                    bad = 4
                else:
                    h = int(tr["head"][k])
                    is_read = not (h & H_WRITE) and (h >> H_TAG_SHIFT) & 0xF == TARGET_MEMORY and not (h & H_ADDR_POOL)
                    if not (is_read and int(tr["id"][k]) == s_lo and s_hi == 0 and int(tr["addr"][k]) == src_addr + i):
                        bad = 5
                    elif (h & H_VALUE_POOL) or int(tr["val"][k]) >= 256:
                        bad = 6
                    else:
                        value = int(tr["val"][k])
            else:
                value = src[sref][src_addr + i]
            if bad:
                first_bad = first_bad or bad
                data.append(0)
                continue
            c = 0
            if s_tag == BYTECODE:
                c = is_code[sref][src_addr + i]
            elif d_tag == BYTECODE:
                c = is_code[dref][dst_addr + i]
            data.append(value | (c << 8))
        offsets.append(len(data))
        status.append(code_of(site or first_bad))
    return np.array(data, dtype=np.uint16), np.array(offsets, dtype=np.uint64), np.array(status, dtype=np.uint32)
