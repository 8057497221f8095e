"""Directed failure-site cases of the Withdrawal circuit (csrc/withdrawal_circuit.hpp, k_withdrawal.hip), built at test time from the
plain-Python model tests/withdrawal_ref.py alone: nothing of the package runs while a case or its expectation is made.

A VARIANT is one tampering of an honest witness or of its tables, aimed at one site of one row (the target); a PLACEMENT is the target's
row.  The bases are honest witnesses of N = 577 rows (two 256-lane blocks, one full wavefront and a wavefront of one lane), cut from
chains of consecutive ids that pass a carry: ids crossing 2^128 (the MPT key's high half becomes non-zero part-way through), 2^64, 2^32
and p - 1 -> 0.  A base is named (chain, carry row, rows): the row whose id is the last one before the carry, and how many rows.  The
digest of a withdrawal is computed once per chain element, so a base with the carry on another row costs no hashing.

Every case is (variant, placement, Wit, expected status vector); `cases(site)` materialises a site's cases lazily and asserts, with the
model, that the target row's status is the variant's and (unless the variant says otherwise) the first failure of its witness, and
that a valid companion is clean.  `coverage_required()` is the table of (kind, site) x placement that the cases must hit and the
backends must return; `UNREACHABLE` lists the cells no witness can reach.

The check_* helpers at the end run the cases through a backend (device "cpu" or None for HIP); they import the package lazily."""
import functools
import json
import os
import random
from collections import namedtuple

import numpy as np

from tests import withdrawal_ref as W
from tests.withdrawal_cases import cells, ints, tamper_cells, withdrawal_inputs

P = W.P
R = 0x1D2C3B4A59687786A5B4C3D2E1F00F1E2D3C4B5A69788796A5B4C3D2E1F0  # (< p; tools/gen_golden_withdrawal.py gives the reference the same)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "withdrawal_site_cases.npz")
N = 577                                    # 2 * 256 + 65
PLACEMENTS = (0, 63, 64, 255, 256, 511, 512, 575, 576)
LAST_BASES = (64, 65, 256, 257, 577)      # the last-row sites stand on row n - 1 of these
Form = namedtuple("Form", "n carry far")    # rows of a base, the row of the last id before the carry, a carry row beyond the witness
FULL = Form(N, 289, 300)                   # main base: ids 2^128 - 290 ..., row 290 the first with a non-zero key hi; wrap base: p - 290 ...
SMALL = Form(6, 2, 9)                      # the same variants on 6 rows: what tools/gen_golden_withdrawal_sites.py gives the reference
FORM = FULL                                # (the generator switches it; case() caches the full form only)
CARRIES = {"32": 1 << 32, "64": 1 << 64, "128": 1 << 128, "wrap": P}
UNSUPPORTED = 15
HALO = W.code(UNSUPPORTED, 0xF0)
A1, A2, U3, U4, AMB4 = W.code(W.ASSERT, 1), W.code(W.ASSERT, 2), W.code(W.UNSAT, 3), W.code(W.UNSAT, 4), W.code(W.AMBIGUOUS, 4)
I0, I1, I4 = W.code(W.INDEX, 0), W.code(W.INDEX, 1), W.code(W.INDEX, 4)
# cells that no witness reaches: the MPT query gives all twelve cells (table_probe_inline's mask 0xfff compares every one), so two
# matching rows are identical and count once; MPTTable.lookup with every field fixed cannot see two distinct rows either
UNREACHABLE = {f"{W.AMBIGUOUS}:3": "the MPT lookup fixes all twelve cells: two matching rows are identical and are counted once"}

Wit = namedtuple("Wit", "rows mpt keccak block m")   # rows: list of 8-tuples (all of them: total_rows = len(rows)); tables: lists
Case = namedtuple("Case", "variant placement wit status target code first")


# ---- chains of honest withdrawals: the model's digest once per element ---------------------------------------------------------------
_SPAN = 578  # the longest base (site 1 on row 576 needs a row 577)


@functools.lru_cache(maxsize=None)
def _digest(wd):
    return W.digest_word(W.rlp_list(wd))


@functools.lru_cache(maxsize=None)
def _krow(wd, r):
    data = W.rlp_list(wd)
    return (1, W.rlc(data, r), len(data)) + _digest(wd)


def assign(wds, roots, m, r):
    """W.assign with the digests cached per withdrawal (test_builder_assign_is_the_models pins it to W.assign)"""
    rows = [tuple(wd) + _digest(tuple(wd)) + W.split(root) for wd, root in zip(wds, roots)]
    last = roots[len(wds) - 1] if wds else 0
    rows += [(0, 0, 0, 0, 0, 0) + W.split(last)] * max(0, m - len(rows))
    return rows, [_krow(tuple(wd), r) for wd in wds]


@functools.lru_cache(maxsize=None)
def _chain_fields(kind):
    """validator, address, amount of chain element k (element _SPAN - 2 holds the last id before the carry)"""
    g = random.Random(f"withdrawal-sites-{kind}")
    return [(g.randrange(0, 1 << 64), g.randrange(1, 1 << 160), g.randrange(1, 1 << (8 * g.randrange(1, 9)))) for _ in range(2 * _SPAN)]


def _chain_wd(kind, k):
    v = _chain_fields(kind)[k]
    return ((CARRIES[kind] - 1 - (_SPAN - 2) + k) % P,) + v


@functools.lru_cache(maxsize=None)
def _roots(n):
    g = random.Random(f"withdrawal-roots-{n}")
    return [g.randrange(1 << 129, 1 << 256) for _ in range(n)]


@functools.lru_cache(maxsize=None)
def base(kind, carry_row, n=N):
    """honest witness of n rows whose row `carry_row` holds the chain's last id before its carry (2^k - 1, or p - 1)"""
    assert 0 <= carry_row <= _SPAN - 2 and n <= _SPAN
    k0 = _SPAN - 2 - carry_row
    wds = [_chain_wd(kind, k0 + i) for i in range(n)]
    roots = _roots(n)
    rows, krows = assign(wds, roots, n, R)
    mpt, prev = [], 0
    for wd, root in zip(wds, roots):
        lo, hi = _digest(wd)
        mpt.append(W.mpt_row(wd[2], W.WITHDRAWAL_MOD, wd[0], root, prev, lo | (hi << 128)))
        prev = root
    block = [(W.WITHDRAWAL_ROOT_TAG, 0) + W.split(roots[-1]), (W.WITHDRAWAL_ROOT_TAG - 1, 0) + W.split(roots[-1]), (W.WITHDRAWAL_ROOT_TAG, 3, 1, 2)]
    return Wit(rows, sorted(mpt), sorted(set(krows) | {(0, 0, 0, 0, 0)}), block, n)


def main(n=None):
    return base("128", FORM.carry, FORM.n if n is None else n)


def wrap():
    return base("wrap", FORM.carry, FORM.n)


def status_of(w):
    return W.verify_status(w.rows, w.mpt, w.keccak, w.block, w.m, R)


def wd_query(w, t):
    """the MPT row that row t of w asks for"""
    row = w.rows[t]
    prev = (0, 0) if t == 0 else w.rows[t - 1][6:8]
    proof = W.WITHDRAWAL_MOD if row[3] else W.NON_EXISTING_ACCOUNT
    return (row[2], proof) + W.split(row[0]) + row[6:8] + prev + row[4:6] + (0, 0)


def set_cell(rows, i, c, v):
    out = list(rows)
    r = list(out[i])
    r[c] = v
    out[i] = tuple(r)
    return out


def swap_row(table, old, new):
    assert old in table
    return sorted([x for x in table if x != old] + ([new] if new is not None else []))


def model_krow(fields):
    """the keccak row of a withdrawal (hashed: only for the few rows a companion needs)"""
    return _krow(tuple(fields), R)


# ---- RLP item sizes ------------------------------------------------------------------------------------------------------------------
def item_len(v):
    return len(W.rlp_int(v))


def payload_len(fields):
    return sum(item_len(v) for v in fields)


def value_of_item_len(k, g):
    """a value whose RLP item has k bytes (1: a single byte below 0x80, or 0; k >= 2: k - 1 bytes)"""
    assert 1 <= k <= 33
    if k == 1:
        return g.randrange(0, 0x80)
    lo = 0x80 if k == 2 else 1 << (8 * (k - 2))
    return g.randrange(lo, min(1 << (8 * (k - 1)), P))


def with_payload(fields, target, g):
    """fields with validator and amount resized so that the payload has `target` bytes"""
    f = list(fields)
    rest = target - item_len(f[0]) - item_len(f[2])
    assert 2 <= rest <= 66, (target, rest)
    a = min(33, rest - 1)
    f[3] = max(1, value_of_item_len(a, g))
    f[1] = value_of_item_len(rest - a, g)
    assert payload_len(f) == target and f[3] != 0
    return tuple(f)


# ---- variants --------------------------------------------------------------------------------------------------------------------------
# name -> (site group, expected code at the target (0: a valid companion), fn(t) -> (Wit, target row) or None, first)
# `first` False: the variant is known to fail an earlier row too (the model says how); such a case counts for no coverage cell.
VARIANTS = {}


def variant(name, code, first=True, placements=PLACEMENTS):
    def deco(fn):
        VARIANTS[name] = (name.split("/")[0], code, fn, first, placements)
        return fn
    return deco


def main_for(t):
    """the main base, with a row t + 1 where the target is row 576 and the site needs a successor"""
    return main(FORM.n + (t == FORM.n - 1))


# -- sites 0 / 4 with IndexError: one lane
@variant("0/no_rows_max1", I0, placements=("lane0",))
def _(t):
    return Wit([], main().mpt, main().keccak, main().block, 1), 0


@variant("0/no_rows_max3", I0, placements=("lane0",))
def _(t):
    return Wit([], [], [], [], 3), 0


@variant("4/no_rows_max0", I4, placements=("lane0",))
def _(t):
    return Wit([], main().mpt, main().keccak, main().block, 0), 0


@variant("4/max0_rows_ok", 0, placements=("lane0",))
def _(t):
    return main(min(65, FORM.n))._replace(m=0), 0


@variant("4/max0_rows_block_missing", U4, placements=("lane0",))
def _(t):
    b = main(min(65, FORM.n))
    return b._replace(m=0, block=b.block[1:]), 0


# -- site 1, IndexError: MAX = total_rows + 1, on the last row of every last-row base
@variant("1/index_max_above_rows", I1, placements=tuple(n - 1 for n in LAST_BASES))
def _(t):
    b = main(t + 1)
    return b._replace(m=t + 2), t


# -- site 1, AssertionError: the NEXT row's id is wrong (changing row t's own id would fail row t - 1 first)
for nm, d in (("plus1", 1), ("minus1", -1), ("plus_2_64", 1 << 64), ("plus_2_128", 1 << 128), ("plus_2_192", 1 << 192)):
    def _next_id(t, d=d):
        b = main_for(t)
        return b._replace(rows=set_cell(b.rows, t + 1, 0, (b.rows[t][0] + 1 + d) % P)), t
    variant(f"1/next_{nm}", A1)(_next_id)


@variant("1/p_minus_1_then_1", A1)
def _(t):
    b = base("wrap", t, FORM.n + (t == FORM.n - 1))
    assert b.rows[t][0] == P - 1 and b.rows[t + 1][0] == 0
    return b._replace(rows=set_cell(b.rows, t + 1, 0, 1)), t


for kind in ("32", "64", "128", "wrap"):
    def _carry(t, kind=kind):
        b = base(kind, t, FORM.n + (t == FORM.n - 1))
        assert b.rows[t][0] == CARRIES[kind] - 1 and b.rows[t + 1][0] == CARRIES[kind] % P
        return b, t
    variant(f"1/carry_{kind}_ok", 0)(_carry)


# -- site 2: the row's fields against the keccak table
def _field_to(c, v):
    def fn(t):
        b = main()
        if b.rows[t][c] == v:
            return None
        return b._replace(rows=set_cell(b.rows, t, c, v)), t
    return fn


for c, nm in ((1, "validator"), (2, "address"), (3, "amount")):
    for v in (0, 0x7F, 0x80, 0xFF, 0x100):
        if c == 3 and v == 0:
            continue  # (amount 0 is a padding row: the variants below)
        variant(f"2/{nm}_to_{v:#x}", A2)(_field_to(c, v))
    variant(f"2/{nm}_to_p_minus_1", A2)(_field_to(c, P - 1))
    variant(f"2/{nm}_plus1", A2)(lambda t, c=c: (main()._replace(rows=set_cell(main().rows, t, c, main().rows[t][c] + 1)), t))


def payload_moves(c):
    """(payload length of the honest row, of the tampered one) of a 2/payload_* case"""
    honest = base("32", FORM.far, FORM.n) if "small_ids" in c.variant else main()
    return payload_len(honest.rows[c.target][:4]), payload_len(c.wit.rows[c.target][:4])


def _payload_across(use):
    """validator and amount resized so that the payload lands on the other side of 55 | 56 (56 and more take the two-byte list header)"""
    def fn(t):
        b = base(use, FORM.far if use == "32" else FORM.carry, FORM.n)
        f = with_payload(b.rows[t][:4], 55 if payload_len(b.rows[t][:4]) >= 56 else 56, random.Random(t))
        return b._replace(rows=list(b.rows[:t]) + [f + b.rows[t][4:]] + list(b.rows[t + 1:])), t
    return fn


variant("2/payload_across_55_56", A2)(_payload_across("128"))
variant("2/payload_across_55_56_small_ids", A2)(_payload_across("32"))  # ids of 4 bytes: the honest payload is below 56


for c, nm in ((4, "hash_lo"), (5, "hash_hi")):
    variant(f"2/{nm}_changed", A2)(lambda t, c=c: (main()._replace(rows=set_cell(main().rows, t, c, main().rows[t][c] ^ 1)), t))
    variant(f"2/{nm}_limb1", A2)(lambda t, c=c: (main()._replace(rows=set_cell(main().rows, t, c, main().rows[t][c] ^ (1 << 64))), t))


def _krow_swapped(change):
    def fn(t):
        b = main()
        k = model_krow(b.rows[t][:4])
        return b._replace(keccak=swap_row(b.keccak, k, change(k))), t
    return fn


variant("2/table_other_digest_lo", A2)(_krow_swapped(lambda k: k[:3] + (k[3] ^ 1, k[4])))
variant("2/table_other_digest_hi", A2)(_krow_swapped(lambda k: k[:4] + (k[4] ^ (1 << 127),)))
variant("2/table_len_plus1", A2)(_krow_swapped(lambda k: k[:2] + (k[2] + 1,) + k[3:]))
variant("2/table_len_minus1", A2)(_krow_swapped(lambda k: k[:2] + (k[2] - 1,) + k[3:]))
variant("2/table_disabled", A2)(_krow_swapped(lambda k: (0,) + k[1:]))
variant("2/table_row_missing", A2)(_krow_swapped(lambda k: None))


def _amount0(t, nonexisting=True, zero_row=True, value_is_hash=True):
    """row t made a padding row (amount 0, the other cells kept): the NonExistingAccount row its MPT query wants is added"""
    b = main()
    w = b._replace(rows=set_cell(b.rows, t, 3, 0))
    q = wd_query(w, t)
    if not value_is_hash:
        q = q[:8] + (0, 0, 0, 0)
    return w._replace(mpt=sorted(b.mpt + [q]) if nonexisting else b.mpt, keccak=b.keccak if zero_row else [k for k in b.keccak if k[0]]), t


variant("2/amount0_no_zero_row", A2)(lambda t: _amount0(t, zero_row=False))
variant("2/amount0_ok", 0)(_amount0)


@variant("2/two_rows_share_rlc_len_ok", 0)
def _(t):
    b = main()
    k = model_krow(b.rows[t][:4])
    return b._replace(keccak=sorted(b.keccak + [k[:3] + (k[3] ^ 1, k[4]), k[:3] + (k[3], k[4] ^ 1)])), t


# -- site 3: the twelve cells of the MPT query
MPT_CELLS = ("address", "proof_type", "key_lo", "key_hi", "root_lo", "root_hi", "root_prev_lo", "root_prev_hi", "value_lo", "value_hi",
             "value_prev_lo", "value_prev_hi")


def _mpt_cell(c, use):
    def fn(t):
        b = base(use, FORM.carry, FORM.n)
        q = wd_query(b, t)
        new = W.NON_EXISTING_ACCOUNT if c == 1 else (q[c] ^ 1 if c in (0, 2, 4, 6, 8, 10) else q[c] ^ (1 << 63) ^ (1 if c == 3 else 0))
        return b._replace(mpt=swap_row(b.mpt, q, q[:c] + (new,) + q[c + 1:])), t
    return fn


for c, nm in enumerate(MPT_CELLS):
    variant(f"3/table_{nm}", U3)(_mpt_cell(c, "128"))
variant("3/table_key_hi_wrap_base", U3)(_mpt_cell(3, "wrap"))
variant("3/table_key_lo_wrap_base", U3)(_mpt_cell(2, "wrap"))
variant("3/table_row_missing", U3)(lambda t: (main()._replace(mpt=swap_row(main().mpt, wd_query(main(), t), None)), t))
variant("3/nonexisting_wanted_only_mod", U3)(lambda t: _amount0(t, nonexisting=False))
variant("3/padding_row_value_is_hash", U3)(lambda t: _amount0(t, value_is_hash=False))
for c, nm in ((6, "root_lo"), (7, "root_hi")):
    variant(f"3/row_{nm}", U3)(lambda t, c=c: (main()._replace(rows=set_cell(main().rows, t, c, main().rows[t][c] ^ 1)), t))

    def _prev_root(t, c=c):
        if t == 0:
            return None  # (row 0's previous root is Word(0))
        b = main()
        return b._replace(rows=set_cell(b.rows, t - 1, c, b.rows[t - 1][c] ^ (1 << 100))), t
    variant(f"3/prev_row_{nm}", U3, first=False)(_prev_root)


def _twins(t, present):
    """eight rows that agree with the wanted one on the five hashed cells (one probe chain) and differ in one other cell each"""
    b = main()
    q = wd_query(b, t)
    twins = [q[:c] + (q[c] ^ (1 << (c + 3)),) + q[c + 1:] for c in range(5, 12)] + [q[:5] + (q[5] ^ (1 << 120),) + q[6:]]
    assert len(set(twins)) == 8 and q not in twins
    return b._replace(mpt=sorted([m for m in b.mpt if m != q or present] + twins)), t


variant("3/hash_twins_ok", 0)(lambda t: _twins(t, True))
variant("3/hash_twins_absent", U3)(lambda t: _twins(t, False))


@variant("3/duplicate_rows_ok", 0)
def _(t):
    b = main()
    return b._replace(mpt=b.mpt + [wd_query(b, t)] * 2), t


def _small_mpt(n_mpt, fail):
    """MAX = n_mpt rows over an MPT table of exactly n_mpt rows (capacity steps: 2 n + 2 against 16, 32, 64); `fail`: the last row's
    entry is another withdrawal's"""
    def fn(t):
        n = max(1, n_mpt)
        b = main(64)
        mpt = [wd_query(b, i) for i in range(n_mpt)]
        if fail and n_mpt:
            mpt = mpt[:-1] + [wd_query(b, 40)]
        w = Wit(b.rows[:n], sorted(mpt), b.keccak, [(W.WITHDRAWAL_ROOT_TAG, 0) + b.rows[n - 1][6:8]], n)
        return w, n - 1
    return fn


for n_mpt in (0, 1, 7, 8, 15, 16):
    if n_mpt:
        variant(f"3/mpt_{n_mpt}_rows_ok", 0, placements=("small",))(_small_mpt(n_mpt, False))
    variant(f"3/mpt_{n_mpt}_rows", U3, placements=("small",))(_small_mpt(n_mpt, True))


def _step_mpt(n_mpt, fail):
    """the main base cut to MAX = n_mpt rows and an MPT table of n_mpt rows: 2 * 511 + 2 = 1024 slots, 2 * 512 + 2 -> 2048"""
    def fn(t):
        b = main()
        mpt = [wd_query(b, i) for i in range(n_mpt)]
        if fail:
            mpt[t] = wd_query(b, n_mpt + 3)
        return b._replace(mpt=sorted(mpt), m=n_mpt, block=[(W.WITHDRAWAL_ROOT_TAG, 0) + b.rows[n_mpt - 1][6:8]]), t
    return fn


for n_mpt in (511, 512):
    variant(f"3/mpt_{n_mpt}_rows_ok", 0, placements=(n_mpt - 1,))(_step_mpt(n_mpt, False))
    variant(f"3/mpt_{n_mpt}_rows", U3, placements=(0, 255, 256, n_mpt - 1))(_step_mpt(n_mpt, True))


# -- site 4: the block lookup rides on row MAX - 1
LAST_PLACEMENTS = tuple(sorted(set(PLACEMENTS) | {n - 1 for n in LAST_BASES}))
GARBAGE = (P - 2, 3, 0x80, 0, (1 << 128) - 1, 5, 7, (1 << 128) - 1)


def last_row_base(t, form):
    """row t is the last evaluated row: form "rows" = a base of t + 1 rows, form "max" = the main base with MAX = t + 1 and garbage in the
    rows behind it"""
    if form == "rows":
        if FORM is FULL and t + 1 not in LAST_BASES:
            return None
        return main(t + 1)
    if t == FORM.n - 1:
        return None
    b = main()
    return b._replace(rows=list(b.rows[:t + 1]) + [GARBAGE] * (FORM.n - t - 1), m=t + 1, block=[(W.WITHDRAWAL_ROOT_TAG, 0) + b.rows[t][6:8]] + b.block[1:])


def _block(change, code, also=None):
    def make(form):
        def fn(t):
            b = last_row_base(t, form)
            if b is None:
                return None
            w = b._replace(block=change(list(b.block)))
            return (also(w, t) if also else w), t
        return fn
    return make


def _block_variant(name, code, change, also=None):
    for form in ("rows", "max"):
        variant(f"4/{name}_{form}", code, placements=LAST_PLACEMENTS)(_block(change, code, also)(form))


_block_variant("ok", 0, lambda b: b)
_block_variant("lo_wrong", U4, lambda b: [b[0][:2] + (b[0][2] ^ 1, b[0][3])] + b[1:])
_block_variant("hi_wrong", U4, lambda b: [b[0][:3] + (b[0][3] ^ (1 << 64),)] + b[1:])
_block_variant("tag_wrong", U4, lambda b: [(W.WITHDRAWAL_ROOT_TAG + 1,) + b[0][1:]] + b[1:])
_block_variant("no_rows", U4, lambda b: [])
_block_variant("two_block_numbers", AMB4, lambda b: b + [(b[0][0], 7) + b[0][2:]])
_block_variant("two_block_numbers_high_limb", AMB4, lambda b: b[1:] + [b[0], (b[0][0], 1 << 192) + b[0][2:]])
_block_variant("duplicate_rows_ok", 0, lambda b: [b[0]] + b + [b[0]])
_block_variant("wrong_and_site2", A2, lambda b: b[1:], also=lambda w, t: w._replace(rows=set_cell(w.rows, t, 1, w.rows[t][1] + 1)))
_block_variant("wrong_and_site3", U3, lambda b: b[1:], also=lambda w, t: w._replace(mpt=swap_row(w.mpt, wd_query(w, t), None)))


SITES = ("0", "1", "2", "3", "4")


def variants_of(site):
    return [n for n, v in VARIANTS.items() if v[0] == site]


def case_ids(site):
    return [f"{n}@{p}" for n in variants_of(site) for p in VARIANTS[n][4]]


@functools.lru_cache(maxsize=None)
def case(name, placement):
    """the Case of (variant, placement), checked against the model; None where the variant has no such placement"""
    _, code, fn, first, _ = VARIANTS[name]
    made = fn(placement)
    if made is None:
        return None
    w, target = made
    w = w._replace(rows=list(w.rows), mpt=list(w.mpt), keccak=list(w.keccak), block=list(w.block))
    status = status_of(w)
    assert status[target] == code, (name, placement, hex(status[target]), hex(code))
    if code == 0:
        assert not any(status), (name, placement, W.first_failure(status))
    elif first:
        assert W.first_failure(status) == (target, code), (name, placement, W.first_failure(status))
    else:
        assert W.first_failure(status)[0] < target, (name, placement)
    return Case(name, placement, w, status, target, code, first)


def cases(site):
    return [c for c in (case(n, p) for n in variants_of(site) for p in VARIANTS[n][4]) if c is not None]


def lane_of(c):
    """the coverage column of a case: its target row (the one-lane and small-table cases stand on "lane0" / "small")"""
    return c.placement if isinstance(c.placement, str) else c.target


def coverage_required():
    """(kind:site) -> the placements at which a failing case must stand, as the first failure of its witness"""
    t = {f"{W.INDEX}:0": {"lane0"}, f"{W.INDEX}:4": {"lane0"}, f"{W.INDEX}:1": {n - 1 for n in LAST_BASES},
         f"{W.ASSERT}:1": set(PLACEMENTS), f"{W.ASSERT}:2": set(PLACEMENTS), f"{W.UNSAT}:3": set(PLACEMENTS) | {"small"},
         f"{W.UNSAT}:4": set(LAST_PLACEMENTS) | {"lane0"}, f"{W.AMBIGUOUS}:4": set(LAST_PLACEMENTS)}
    return t


def coverage_of(all_cases, status_of_case):
    """the table from statuses (the model's, or a backend's): the code of each failing first-failure case's target row"""
    t = {}
    for c in all_cases:
        if c.code and c.first:
            code = int(status_of_case(c)[c.target])
            t.setdefault(f"{code >> 24}:{code & 0xFFFFFF}", set()).add(lane_of(c))
    return t


def all_cases():
    return [c for s in SITES for c in cases(s)]


def coverage_table():
    """the builder's own table, asserted complete with the model alone; the cells beyond the required ones are kept as they fall"""
    t = coverage_of(all_cases(), lambda c: c.status)
    need = coverage_required()
    for k, want in need.items():
        assert want <= t.get(k, set()), (k, sorted(map(str, want - t.get(k, set()))))
    assert set(t) == set(need) and not set(t) & set(UNREACHABLE), sorted(t)
    return t


# ---- wire forms --------------------------------------------------------------------------------------------------------------------------
_CELLS = {}


def _cached_cells(table, nc):
    key = (nc, tuple(table))
    if key not in _CELLS:
        if len(_CELLS) > 64:
            _CELLS.clear()
        _CELLS[key] = cells(table, nc)
    return _CELLS[key]


def wire(w):
    """the wire dict of a Wit: every row is sent (total_rows = len(rows)); tables keep their order and their duplicates"""
    return {"rows": _cached_cells(w.rows, 8), "mpt": _cached_cells(w.mpt, 12), "keccak": _cached_cells(w.keccak, 5),
            "block": _cached_cells(w.block, 4), "max_withdrawals": w.m, "total_rows": len(w.rows), "row_base": 0}


def n_eval(w):
    return max(1, min(w.m, len(w.rows)))


# ---- assignment batches ------------------------------------------------------------------------------------------------------------------
Batch = namedtuple("Batch", "name wds roots m r keccak_rows")
ROOTS = (0, (1 << 128) - 1, 1 << 128, P + 5, (1 << 256) - 1, (1 << 256) - P)
R_RANDOM = 0x1A2B3C4D5E6F708192A3B4C5D6E7F8091A2B3C4D5E6F708192A3B4C5D6E7F % P


def length_sweep():
    """each field in turn over byte lengths 0..32 (least and greatest value of the length) and the single bytes, the others fixed"""
    fixed = (0x1234, 0x80, (1 << 160) - 1, 0x7F)
    out = []
    for c in range(4):
        vals = [0, 1, 0x7F, 0x80, 0xFF]
        for ln in range(1, 33):
            vals += [1 << (8 * (ln - 1)), min((1 << (8 * ln)) - 1, P - 1)]
        for v in vals:
            out.append(fixed[:c] + (v,) + fixed[c + 1:])
    return out


def payload_sweep():
    """every payload length 4..132, lengths 55 and 56 from four splits each, and the 134-byte maximum"""
    g = random.Random("withdrawal-payload-sweep")
    out = []
    for total in range(4, 133):
        lens = [1, 1, 1, 1]
        i = total % 4
        for _ in range(total - 4):  # odd totals: round robin over the items; even ones: one item filled to 33 bytes before the next
            while lens[i] == 33:
                i = (i + 1) % 4
            lens[i] += 1
            if total % 2:
                i = (i + 1) % 4
        out.append(tuple(value_of_item_len(k, g) for k in lens))
    for total in (55, 56):
        for lens in ((33, total - 33 - 2, 1, 1), (1, 1, 21, total - 23), (total - 3 * 9, 9, 9, 9), (14, 14, 14, total - 42)):
            out.append(tuple(value_of_item_len(k, g) for k in lens))
    out.append((P - 1,) * 4)
    for wd in out:
        assert all(0 <= v < P for v in wd)
    assert {payload_len(wd) for wd in out} >= set(range(4, 133)) and len(W.rlp_list(out[-1])) == 134
    assert all(len({tuple(item_len(v) for v in wd) for wd in out if payload_len(wd) == t}) >= 3 for t in (55, 56))
    return out


def heavy(wd):
    return payload_len(wd) >= 56 or any(v >= 1 << 248 for v in wd)


def lay_out(wds):
    """heavy cases (a two-byte list header, or a 32-byte field) on lanes 0 and 63 of every 64-lane block and all over the last, partial block"""
    hv, lt = [w for w in wds if heavy(w)], [w for w in wds if not heavy(w)]
    n = len(wds)
    tail = n - (n % 64 or 64)
    want = {i for i in range(n) if i % 64 in (0, 63) or i >= tail}
    assert len(hv) >= len(want)
    front, rest = iter(hv), iter(lt + hv[len(want):])
    out = [next(front) if i in want else next(rest) for i in range(n)]
    assert all(heavy(out[i]) for i in want) and sorted(out) == sorted(wds)
    return out


@functools.lru_cache(maxsize=None)
def batches():
    out = []
    sweep = lay_out(length_sweep() + payload_sweep())
    assert len(sweep) % 64 not in (0, 1)
    roots = [ROOTS[i % len(ROOTS)] for i in range(len(sweep))]
    for nm, r in (("r_random", R_RANDOM), ("r_0", 0), ("r_1", 1), ("r_p_minus_1", P - 1)):
        out.append(Batch(f"sweep_{nm}", sweep, roots, len(sweep) + 70, r, True))
    out.append(Batch("sweep_no_keccak_rows", sweep[:130], roots[:130], 130, R_RANDOM, False))
    hv = [w for w in sweep if heavy(w)]
    pool = [hv[i % len(hv)] for i in range(130)]
    for n_in in (0, 1, 63, 64, 65, 130):
        for m in sorted({0, n_in - 1, n_in, n_in + 1, n_in + 64, n_in + 65}):
            if m >= 0:
                out.append(Batch(f"n{n_in}_max{m}", pool[:n_in], [ROOTS[(i + 3) % len(ROOTS)] for i in range(n_in)], m, R_RANDOM, True))
    return out


def batch_ids():
    return [b.name for b in batches()]


# ---- running the cases through a backend (device "cpu", or None for HIP) -------------------------------------------------------------------
def check_oneshot(c, device):
    """one-shot verification of a case: the whole status vector and the tally against the model; returns the status"""
    from zkevm_specs_amd import oneshot

    res, st = oneshot.withdrawal_verify(wire(c.wit), R, device=device)
    assert st.tolist() == list(c.status), (c.variant, c.placement, _diff(st.tolist(), c.status))
    _check_tally(res, c.status, (c.variant, c.placement))
    return st


def _diff(got, want):
    return [(i, hex(g), hex(w)) for i, (g, w) in enumerate(zip(got, want)) if g != w][:6] + [len(got), len(want)]


def _check_tally(res, status, what):
    fails = [i for i, s in enumerate(status) if s]
    assert res.fail_count == len(fails), what
    if fails:
        assert (res.first_fail_row, res.first_fail_code) == (fails[0], status[fails[0]]), what


def check_session_twice(c, device):
    from zkevm_specs_amd import engine

    with engine.open_withdrawal(wire(c.wit), R, device=device) as s:
        for _ in range(2):
            res = s.run()
            st = s.read_status()
            assert st.tolist() == list(c.status), (c.variant, c.placement, _diff(st.tolist(), c.status))
            _check_tally(res, c.status, (c.variant, c.placement))


def shard(w, lo, hi, left=True, right=True):
    """(wire dict, eval_lo, eval_hi) of global rows [lo, hi) of w held with their +-1 halo (left / right False: without that halo row)"""
    start = max(lo - 1, 0) if left else lo
    end = min(hi + 1, len(w.rows)) if right else hi
    d = wire(w)
    d = dict(d, rows=np.ascontiguousarray(d["rows"][start:end]), row_base=start)
    return d, lo - start, hi - start


def run_shard(d, lo_l, hi_l, device):
    from zkevm_specs_amd import engine

    with engine.open_withdrawal(d, R, device=device) as s:
        s.set_range(lo_l, hi_l)
        res = s.run()
        return res, s.read_status()[lo_l:hi_l].tolist()


def check_cuts(c, cuts, device):
    """ranged sessions over [0, cut_1), [cut_1, cut_2), ...: concatenated statuses, summed tallies and the least first failure equal the
    model's whole run"""
    bounds = [0] + list(cuts) + [n_eval(c.wit)]
    got, tot, first = [], 0, []
    for lo, hi in zip(bounds, bounds[1:]):
        d, lo_l, hi_l = shard(c.wit, lo, hi)
        res, st = run_shard(d, lo_l, hi_l, device)
        got += st
        tot += res.fail_count
        if res.fail_count:
            first.append((res.first_fail_row - lo_l + lo, res.first_fail_code))
    what = (c.variant, c.placement, cuts)
    assert got == list(c.status), what + (_diff(got, c.status),)
    assert tot == sum(1 for s in c.status if s), what
    assert (min(first) if first else (None, 0)) == W.first_failure(c.status), what


def check_shard_rows_world3(c, device):
    """distributed.shard_rows(..., world=3): the package's own cut (unaligned on 577 rows) with its halo and row_base"""
    from zkevm_specs_amd.distributed import shard_rows

    w = wire(c.wit)
    got, tot, first = [], 0, []
    for rank in range(3):
        rows, _, lo_l, hi_l, lo = shard_rows(w["rows"], None, rank, 3, "withdrawal", w["max_withdrawals"], w["total_rows"])
        if lo_l == hi_l:
            continue  # (fewer evaluated rows than ranks: this rank has none)
        res, st = run_shard(dict(w, rows=rows, row_base=lo - lo_l), lo_l, hi_l, device)
        got += st
        tot += res.fail_count
        if res.fail_count:
            first.append((res.first_fail_row - lo_l + lo, res.first_fail_code))
    assert got == list(c.status), (c.variant, c.placement, _diff(got, c.status))
    assert tot == sum(1 for s in c.status if s) and (min(first) if first else (None, 0)) == W.first_failure(c.status)


def halo_expected(c, lo, hi, left, right):
    """the model's statuses of rows [lo, hi) with the refusal on the rows whose neighbour is not held"""
    w, want = c.wit, list(c.status[lo:hi])
    if not left and lo != 0:
        want[0] = HALO
    if not right and hi < len(w.rows) and hi - 1 != w.m - 1:
        want[-1] = HALO
    return want


def check_halo_refusal(c, lo, hi, device):
    """the shard [lo, hi) opened without its left halo row, then without its right one"""
    out = []
    for left, right in ((False, True), (True, False), (False, False)):
        d, lo_l, hi_l = shard(c.wit, lo, hi, left, right)
        res, st = run_shard(d, lo_l, hi_l, device)
        want = halo_expected(c, lo, hi, left, right)
        assert st == want, (c.variant, c.placement, lo, hi, left, right, _diff(st, want))
        _check_tally(res, [0] * lo_l + want, (c.variant, lo, hi, left, right))
        out.append((st, want))
    return out


def boundary_cases(cut):
    """the cases whose target or a neighbour of it is a row at the cut"""
    out = []
    for s in ("1", "2", "3", "4"):
        for n in variants_of(s):
            for p in VARIANTS[n][4]:
                if p in (cut - 1, cut):
                    c = case(n, p)
                    if c is not None and n_eval(c.wit) > cut:
                        out.append(c)
    return out


def check_assignment(b, device):
    """zk_withdrawal_assign of a batch against the model bit for bit"""
    from zkevm_specs_amd import oneshot

    rows, krows = assign(b.wds, b.roots, b.m, b.r)
    inp = withdrawal_inputs(b.wds, b.roots) if b.wds else np.zeros((0, 5, 4), dtype=np.uint64)
    got_rows, got_k = oneshot.withdrawal_assign(inp, b.m, b.r, keccak_rows=b.keccak_rows, device=device)
    assert got_rows.shape[0] == max(len(b.wds), b.m)
    assert ints(got_rows) == rows, (b.name, [i for i, (g, w) in enumerate(zip(ints(got_rows), rows)) if g != w][:8])
    if b.keccak_rows:
        assert ints(got_k) == krows, (b.name, [i for i, (g, w) in enumerate(zip(ints(got_k), krows)) if g != w][:8])
    else:
        assert got_k is None


def check_assign_verify_tamper(device, pad):
    """the backend's own assignment of the main base's withdrawals, under tables built by the model: verifies as the model says (clean
    without padding rows), and so does a copy with 60 tampered cells"""
    from zkevm_specs_amd import oneshot

    b = main()
    wds = [r[:4] for r in b.rows]
    roots = [r[6] | (r[7] << 128) for r in b.rows]
    m = FORM.n + pad
    got_rows, got_k = oneshot.withdrawal_assign(withdrawal_inputs(wds, roots), m, R, device=device)
    model_rows, model_k = assign(wds, roots, m, R)
    assert ints(got_rows) == model_rows and ints(got_k) == model_k
    w = b._replace(rows=model_rows, m=m)
    d = dict(wire(w), rows=got_rows, keccak=np.concatenate([np.zeros((1, 5, 4), dtype=np.uint64), got_k]))
    want = status_of(w._replace(keccak=[(0, 0, 0, 0, 0)] + model_k))
    assert pad or not any(want)
    res, st = oneshot.withdrawal_verify(d, R, device=device)
    assert st.tolist() == want
    _check_tally(res, want, "assigned")
    t = tamper_cells(got_rows, np.random.default_rng(11 + pad), 60)
    want = status_of(w._replace(rows=ints(t), keccak=[(0, 0, 0, 0, 0)] + model_k))
    assert sum(1 for s in want if s) > 40
    res, st = oneshot.withdrawal_verify(dict(d, rows=t), R, device=device)
    assert st.tolist() == want, _diff(st.tolist(), want)
    _check_tally(res, want, "tampered")


# ---- the recorded reference outcomes (tools/gen_golden_withdrawal_sites.py) ------------------------------------------------------------------
def golden_cases():
    """(meta, wire dict, model status, randomness) of every small case the unmodified reference has judged"""
    z = np.load(GOLDEN)
    meta = json.loads(str(z["meta"]))
    r = int(meta["randomness"], 16)
    for i, m in enumerate(meta["cases"]):
        w = {k: z[f"{i}_{k}"] for k in ("rows", "mpt", "keccak", "block")}
        w.update(max_withdrawals=m["max_withdrawals"], total_rows=m["total_rows"], row_base=0)
        yield m, w, z[f"{i}_status"], r


def check_golden(device):
    from zkevm_specs_amd import oneshot

    n = 0
    for m, w, status, r in golden_cases():
        res, st = oneshot.withdrawal_verify(w, r, device=device)
        assert st.tolist() == status.tolist(), m["name"]
        _check_tally(res, status.tolist(), m["name"])
        row, code = W.first_failure(status.tolist())
        assert (code >> 24) == m["first_kind"] and (-1 if row is None else row) == m["first_row"], m["name"]
        n += 1
    return n


# ---- the test bodies shared by tests/test_withdrawal_sites_cpu.py and tests/test_withdrawal_sites_gpu.py -------------------------------------
CUTS = (64, 65, 256, 257)                  # hand-cut shard boundaries 63|64, 64|65, 255|256, 256|257
HALO_VARIANTS = ("1/", "2/amount0", "3/row_root", "3/prev_row_root", "3/table_root_prev", "3/hash_twins", "4/ok_max", "4/lo_wrong_max")


def run_variant_oneshots(name, device, returned):
    n = 0
    for p in VARIANTS[name][4]:
        c = case(name, p)
        if c is not None:
            returned[(name, p)] = check_oneshot(c, device)
            n += 1
    assert n


def rotating_cases(site):
    """one case of every variant of the site, the placement going round with the variant's number"""
    out = []
    for i, n in enumerate(variants_of(site)):
        ps = [p for p in VARIANTS[n][4] if case(n, p) is not None]
        out.append(case(n, ps[i % len(ps)]))
    return out


def halo_cases(cut):
    return [c for c in boundary_cases(cut) if c.variant.startswith(HALO_VARIANTS)]


def check_coverage(returned, device):
    """the coverage table recomputed from what the backend returned (a case whose one-shot test did not run is run here)"""
    def got(c):
        key = (c.variant, c.placement)
        if key not in returned:
            returned[key] = check_oneshot(c, device)
        return returned[key]
    assert coverage_of(all_cases(), got) == coverage_table()
