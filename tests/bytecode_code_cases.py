"""zk_bytecode_from_code: a plain-Python model and the directed case builders (shared by the CPU and GPU tests).

The model is written from the entry's stated semantics (include/zkevm_hip.h), with oracle.keccak.keccak256 for the digest:
  table   per code a Header row (hash lo, hi, 1, 0, 0, len) and per byte a Byte row (hash lo, hi, 2, i, is_code_i, byte_i); the
          push-data counter starts at 0 per code, PUSH1..PUSH32 (0x60..0x7f) set it to 1..32, every other byte sets it to 0
  rows    the Bytecode circuit's 12 cells over those rows (q_first, q_last, hash lo, hi, tag, index, value, is_code, push_data_left,
          value_rlc, length, push_data_size), cut at 2^k rows, padded with Header rows of the empty code
  keccak  per code (2, RLC of the bytes front to back, len, hash lo, hi)
"""
import functools
import random

import numpy as np

from oracle.keccak import keccak256

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
EMPTY_HASH = int.from_bytes(keccak256(b""), "big")
R_DEFAULT = 0x2A3B4C5D6E7F8091A2B3C4D5E6F708192A3B4C5D6E7F8091A2B3C4D5E6F70819 % P
MASK128 = (1 << 128) - 1


def push_size(b):
    return b - 0x5F if 0x60 <= b <= 0x7F else 0


def is_code_of(code):
    out, left = [], 0
    for b in code:
        out.append(left == 0)
        left = push_size(b) if left == 0 else left - 1
    return out


def _wide(vals):
    """python ints -> uint64[len, 4]"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype="<u8").reshape(-1, 4).copy()


def pack(codes):
    """-> (code uint8[n_bytes], offsets uint64[n_codes + 1])"""
    offsets = np.zeros(len(codes) + 1, dtype=np.uint64)
    if codes:
        offsets[1:] = np.cumsum([len(c) for c in codes], dtype=np.uint64)
    return np.frombuffer(b"".join(bytes(c) for c in codes), dtype=np.uint8).copy(), offsets


def model(codes, k, r):
    """-> (table uint64[T, 6, 4], rows uint64[12, 2^k, 4] or None (k == 0), keccak uint64[m, 5, 4]), T = sum(len) + m"""
    T = sum(len(c) for c in codes) + len(codes)
    table = np.zeros((T, 6, 4), dtype=np.uint64)
    extra = np.zeros((T, 3), dtype=np.uint64)  # push_data_left, length, push_data_size
    rlcs = []
    keccak = np.zeros((len(codes), 5, 4), dtype=np.uint64)
    i = 0
    for j, code in enumerate(codes):
        code = bytes(code)
        h = int.from_bytes(keccak256(code), "big")
        n = len(code)
        hc = _wide([h & MASK128, h >> 128])
        table[i : i + n + 1, 0] = hc[0]
        table[i : i + n + 1, 1] = hc[1]
        table[i, 2, 0], table[i, 5, 0] = 1, n
        extra[i : i + n + 1, 1] = n
        rlcs.append(0)
        left, acc = 0, 0
        for q, b in enumerate(code):
            row = table[i + 1 + q]
            row[2, 0], row[3, 0], row[4, 0], row[5, 0] = 2, q, int(left == 0), b
            extra[i + 1 + q, 0], extra[i + 1 + q, 2] = left, push_size(b)
            left = push_size(b) if left == 0 else left - 1
            acc = (acc * r + b) % P
            rlcs.append(acc)
        keccak[j] = _wide([2, acc, n, h & MASK128, h >> 128])
        i += n + 1
    if not k:
        return table, None, keccak
    N = 1 << k
    rows = np.zeros((12, N, 4), dtype=np.uint64)
    rows[0, 0, 0] = 1
    rows[1, N - 1, 0] = 1
    m = min(T, N)
    for dst, src in ((2, 0), (3, 1), (4, 2), (5, 3), (6, 5), (7, 4)):
        rows[dst, :m] = table[:m, src]
    rows[8, :m, 0], rows[10, :m, 0], rows[11, :m, 0] = extra[:m, 0], extra[:m, 1], extra[:m, 2]
    if m:
        rows[9, :m] = _wide(rlcs[:m])
    if m < N:
        pad = _wide([EMPTY_HASH & MASK128, EMPTY_HASH >> 128])
        rows[2, m:], rows[3, m:] = pad[0], pad[1]
        rows[4, m:, 0] = 1
    return table, rows, keccak


def _rand_code(rng, n):
    """n bytes, 30 % of them PUSH1..PUSH32"""
    return bytes(rng.randrange(0x60, 0x80) if rng.random() < 0.3 else rng.randrange(256) for _ in range(n))


def _k_for(codes, slack=3):
    T = sum(len(c) for c in codes) + len(codes) + slack
    return max(1, (T - 1).bit_length())


@functools.lru_cache(maxsize=None)
def directed_cases(seed=20261019):
    """-> tuple of (name, codes, k).  Every case is one call."""
    rng = random.Random(seed)
    cases = []
    edge_lengths = ([0, 1] + list(range(31, 35)) + list(range(62, 67)) + list(range(126, 131))  # chunk edges (L bytes: L + 1 rows)
                    + list(range(135, 138)) + list(range(271, 274))                             # keccak rate blocks
                    + list(range(543, 546)))                                                    # KT_GROUP_MIN_BYTES
    edges = [_rand_code(rng, n) for n in edge_lengths]
    cases.append(("edges", edges, _k_for(edges)))
    cases.append(("edges_k0", edges, 0))
    # push data across the first chunk boundary with every leftover count; the data bytes are PUSH opcodes themselves
    cross = [b"\x00" * j + b"\x7f" + b"\x60" * 200 for j in range(64)]
    cases.append(("push_cross", cross, _k_for(cross)))
    misc = [b"\x7f" * 300, b"\x60" * 300]
    for short in (1, 16, 32):
        misc.append(bytes(rng.randrange(0x60) for _ in range(70)) + b"\x7f" + bytes(rng.randrange(256) for _ in range(32 - short)))
    misc.append(bytes(rng.choice([0x5F] + list(range(0x80, 0x100))) for _ in range(150)))
    cases.append(("push_misc", misc, _k_for(misc)))
    tiny = [_rand_code(rng, rng.randrange(6)) for _ in range(300)]
    tiny[0], tiny[1], tiny[299] = b"", b"\x60", b""
    cases.append(("tiny300", tiny, _k_for(tiny)))
    cases.append(("code_24576", [_rand_code(rng, 24576)], 15))
    cases.append(("code_70000", [_rand_code(rng, 70000)], 17))
    # 2^k - 1, 2^k and 2^k + 1 rows (k = 8), a PUSH32 at byte 240: rows 242..273 would be its data
    for total in (255, 256, 257):
        body = bytearray(_rand_code(rng, total - 1).replace(b"\x7f", b"\x01"))
        body[200:240] = b"\x00" * 40
        body[240:] = (b"\x7f" + b"\x61" * 40)[: len(body) - 240]
        cases.append((f"rows_{total}_k8", [bytes(body)], 8))
    # truncation inside the second code's push-data run: rows 101 + 201 + 51 = 353 > 2^8; row 256 is byte 154 of code 1
    second = bytearray(b"\x00" * 200)
    second[140] = 0x7F
    second[141:173] = b"\x62" * 32
    trunc = [_rand_code(rng, 100), bytes(second), _rand_code(rng, 50)]
    cases.append(("truncated_in_push_data", trunc, 8))
    cases.append(("truncated_k1", trunc, 1))
    cases.append(("no_codes", [], 3))
    cases.append(("no_codes_k0", [], 0))
    return tuple((name, tuple(codes), k) for name, codes, k in cases)


@functools.lru_cache(maxsize=None)
def directed_expected(name, r=R_DEFAULT):
    """the model's outputs for one directed case: computed once, shared (treat as read-only)"""
    _, codes, k = next(c for c in directed_cases() if c[0] == name)
    out = model(list(codes), k, r)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


def golden_codes():
    """the directed codes of at most 600 bytes, in case order, without repeats: what tests/golden/bytecode_code_cases.npz records"""
    seen, out = set(), []
    for _, codes, _ in directed_cases():
        for c in codes:
            if len(c) <= 600 and c not in seen:
                seen.add(c)
                out.append(c)
    return out


def random_set(seed=7, n_codes=200, total=1 << 16):
    """a seeded set of n_codes codes with `total` bytes: many tiny codes, a few of 8..24 KB; 30 % of the bytes are 0x60..0x7f"""
    rng = random.Random(seed)
    while True:
        lengths = [rng.randrange(8 << 10, 24 << 10) for _ in range(3)] + [rng.randrange(0, 40) for _ in range(n_codes - 4)]
        rest = total - sum(lengths)
        if (8 << 10) <= rest <= (24 << 10):
            break
    lengths.append(rest)
    rng.shuffle(lengths)
    return [_rand_code(rng, n) for n in lengths]
