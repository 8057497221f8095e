"""Directed codes for the chunk, batch and round edges of the Bytecode-circuit witness assignment (shared by the CPU and GPU tests).

zk_bytecode_assign and zk_bytecode_from_code cut a bytecode into chunks of 64 (rows, Header row included, or bytes), batches of 64
chunks and rounds of 1,024 chunks; the device forms (csrc/k_assign.hip, csrc/k_bytecode_code.hip) carry the value_rlc and the
push-data counter over those edges in their own way.  The builders here put a chosen push_data_left on a chosen edge:

  ladder codes    non-PUSH filler (random over 0x00..0x5f and 0x80..0xff) and, per (edge chunk c, leftover l in 1..32), a PUSH32 whose
                  last l data bytes lie at and after the edge.  The 32 data bytes are 0x7f, eight 0x60 follow: a wrong counter reads
                  them as code.  The edge of chunk c is row 64 c = byte 64 c - 1 in the rows form (zk_bytecode_assign: the Header row
                  shifts everything by one) and byte 64 c in the code form (zk_bytecode_from_code): one set of ladders per form.
  rows_extras     small codes whose length looks like a PUSH, a PUSH32 as a code's last byte, empty codes; r in EXTRA_R, k in EXTRA_K
  wide values     field elements that are no bytes on either side of the first batch edge and of the round edge (rows form only)

Expected outputs: the plain-Python model of tests/bytecode_code_cases.py (oracle/bytecode_assign_oracle.assign for the wide values,
which the model does not take), computed once per case and shared (read-only).
"""
import functools
import random

import numpy as np

from tests import bytecode_code_cases as bc

P = bc.P
R = bc.R_DEFAULT
FORMS = ("rows", "code")
CHUNK, BATCH_CHUNKS, ROUND_CHUNKS = 64, 64, 1024
LADDER_BYTES = 66000
TWO_ROUNDS_BYTES = 131300
LADDER_NAMES = ("batch_ladder_a", "batch_ladder_b", "round_1", "round_2", "round_31", "round_0")
LADDERS_K = 19     # the six ladders as one call: 6 * 66,001 rows
LADDER_K = 17      # one ladder alone
TWO_ROUNDS_K = 18
EXTRA_R = (0, 1, P - 1, 1 << 128, R)
EXTRA_K = (10, 8, 6, 1)
_FILLER = tuple(range(0x00, 0x60)) + tuple(range(0x80, 0x100))


def edge_byte(c, form):
    """the first byte behind the edge of chunk c: row 64 c of the rows form is byte 64 c - 1"""
    return CHUNK * c - (1 if form == "rows" else 0)


def ladder(rng, n, pairs, form, ff_before=0):
    """n bytes of filler (0xff before byte `ff_before`) with, per (chunk, leftover) of `pairs`, `leftover` bytes of a PUSH32's data at and
    after the chunk's edge"""
    code = bytearray(rng.choice(_FILLER) for _ in range(n))
    code[:ff_before] = b"\xff" * ff_before
    for c, left in pairs:
        assert 1 <= left <= 32
        at = edge_byte(c, form) - 33 + left
        assert at >= 0 and at + 41 <= n
        code[at : at + 41] = b"\x7f" * 33 + b"\x60" * 8
    return bytes(code)


@functools.lru_cache(maxsize=None)
def ladder_codes(form, seed=20261020):
    """-> the six 66,000-byte codes of LADDER_NAMES: leftovers 1..16 and 17..32 on the edges of chunks 64, 128, ..., 1024 (the sixteenth is
    the round edge); leftover 1, 2 and 31 at chunk 1024 with 32, 31 and 2 at chunk 960 (the first of the three also sets 16 at chunk
    896: the two batch ladders have 16 at the round edge only); plain filler, entering every edge with 0"""
    rng = random.Random(seed + FORMS.index(form))
    edges = [BATCH_CHUNKS * i for i in range(1, 17)]
    codes = [ladder(rng, LADDER_BYTES, [(c, i + 1) for i, c in enumerate(edges)], form),
             ladder(rng, LADDER_BYTES, [(c, i + 17) for i, c in enumerate(edges)], form)]
    for left in (1, 2, 31):
        pairs = [(ROUND_CHUNKS, left), (ROUND_CHUNKS - BATCH_CHUNKS, 33 - left)] + ([(ROUND_CHUNKS - 2 * BATCH_CHUNKS, 16)] if left == 1 else [])
        codes.append(ladder(rng, LADDER_BYTES, pairs, form))
    codes.append(ladder(rng, LADDER_BYTES, [], form))
    return tuple(codes)


@functools.lru_cache(maxsize=None)
def two_rounds_code(form, seed=20261021):
    """131,300 bytes, three rounds: leftover 25 at chunk 1024 and 7 at chunk 2048; the filler before chunk 1024 is 0xff, so the value the
    first round hands over is large and feeds the second hand-over"""
    rng = random.Random(seed + FORMS.index(form))
    return ladder(rng, TWO_ROUNDS_BYTES, [(ROUND_CHUNKS, 25), (2 * ROUND_CHUNKS, 7)], form, ff_before=edge_byte(ROUND_CHUNKS, form))


def edge_kind(c):
    return "round" if c % ROUND_CHUNKS == 0 else "batch" if c % BATCH_CHUNKS == 0 else "chunk"


def edge_states(codes, form):
    """kind of edge (round, batch, chunk) -> the set of push_data_left values entering the first row (rows form) or byte (code form) behind
    an edge of that kind, by the plain counter walk"""
    out = {"round": set(), "batch": set(), "chunk": set()}
    for code in codes:
        left, first = 0, edge_byte(1, form)
        for q, b in enumerate(code):
            if q >= first and (q - first) % CHUNK == 0:
                out[edge_kind(1 + (q - first) // CHUNK)].add(left)
            left = bc.push_size(b) if left == 0 else left - 1
    return out


def rows_extras():
    """small codes of the rows form's own edges: lengths 0x60 and 0x7f (the Header row's value looks like a PUSH and must not start push
    data), b"\\xff" * 200, empty and one-byte codes, a PUSH32 as a code's last byte with another code behind it.
    Rows: 0..96 | 97..147 | 148..188 | 189 | 190..191 | 192..319 | 320..520.  Row 256 is byte 63 of the 0x7f-byte code, inside the data of
    its PUSH32 at byte 40 (2^8 rows cut there); row 64 is the first code's first chunk edge (2^6 rows end exactly on it)."""
    rng = random.Random(20261022)
    c60 = bytearray(bc._rand_code(rng, 0x60))
    c60[0] = 0x60
    last_push = bytes(rng.choice(_FILLER) for _ in range(49)) + b"\x7f"
    c7f = bytearray(bc._rand_code(rng, 0x7F).replace(b"\x7f", b"\x01"))
    c7f[8:40] = b"\x00" * 32
    c7f[40:73] = b"\x7f" + b"\x62" * 32
    return (bytes(c60), last_push, bc._rand_code(rng, 40), b"", b"\x7f", bytes(c7f), b"\xff" * 200)


def row_offsets(codes):
    """(offsets uint64[m + 1] into the table's rows, lengths uint64[m]) of zk_bytecode_assign"""
    lengths = np.array([len(c) for c in codes], dtype=np.uint64)
    offsets = np.zeros(len(codes) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lengths + np.uint64(1), dtype=np.uint64)
    return offsets, lengths


def _frozen(out):
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def cases(form):
    """-> tuple of (name, codes, k, r): every call of one form but the wide-value one"""
    out = [("ladders", ladder_codes(form), LADDERS_K, R), ("two_rounds", (two_rounds_code(form),), TWO_ROUNDS_K, R)]
    out += [(f"extras_r{i}_k{k}", rows_extras(), k, r) for i, r in enumerate(EXTRA_R) for k in EXTRA_K]
    if form == "rows":  # the from-code corpus through the row entry (the code form runs it in its own tests)
        out += [(f"corpus_{name}", codes, k, R) for name, codes, k in bc.directed_cases() if k >= 1]
    return tuple(out)


def case_names(form):
    return [c[0] for c in cases(form)]


@functools.lru_cache(maxsize=None)
def expected(form, name):
    """(table, rows, keccak) of the model for one case: computed once, shared (read-only).  The table is the rows form's input."""
    if name.startswith("corpus_"):
        return bc.directed_expected(name[len("corpus_"):])
    if name.startswith("ladder_"):  # one ladder alone, LADDER_K rows
        return _frozen(bc.model([ladder_codes(form)[LADDER_NAMES.index(name[len("ladder_"):])]], LADDER_K, R))
    _, codes, k, r = next(c for c in cases(form) if c[0] == name)
    return _frozen(bc.model(list(codes), k, r))


def case(form, name):
    """-> (codes, k, r, (table, rows, keccak))"""
    if name.startswith("ladder_"):
        return (ladder_codes(form)[LADDER_NAMES.index(name[len("ladder_"):])],), LADDER_K, R, expected(form, name)
    _, codes, k, r = next(c for c in cases(form) if c[0] == name)
    return codes, k, r, expected(form, name)


WIDE_VALUES = ((4095, P - 1), (4096, (1 << 32) + 0x7F), (4097, 1 << 200), (65535, (1 << 64) + 5), (65536, P - 1), (65537, (1 << 32) + 0x60))


@functools.lru_cache(maxsize=None)
def wide_case():
    """batch_ladder_a's table (rows form) with value cells that are no bytes on either side of the first batch edge (row 4096) and of
    the round edge (row 65536) -> (in_rows, offsets, lengths, k, r, rows of oracle.bytecode_assign_oracle.assign)"""
    from oracle import bytecode_assign_oracle, wire

    codes, k, r, exp = case("rows", "ladder_batch_ladder_a")
    in_rows = exp[0].copy()
    for row, val in WIDE_VALUES:
        in_rows[row, 5] = bc._wide([val])[0]
    offsets, lengths = row_offsets(codes)
    rows = wire.rows_to_colmajor(bytecode_assign_oracle.assign(k, wire.rowmajor_to_rows(in_rows), offsets, lengths, r))
    return _frozen((in_rows, offsets, lengths)) + (k, r) + _frozen((rows,))
