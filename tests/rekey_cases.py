"""Directed RW tables for the RW -> State re-keying (csrc/state_rekey.hpp, state_rekey_plan.hpp, k_rekey.hip) and a plain-Python model
of its compact-key plan.  Builders and the model only: the tests are in tests/test_state_rekey.py and tests/test_state_fused.py.

Tables are built as uint64[n, 14, 4] with numpy (knob_table: which bits of which key field vary, in which input order, with which
shares of repeated keys, dropped and rejected rows); the integer rows oracle/rw_state_oracle.py wants are derived from the array
(table_ints), and the device's op list is compared with the checker's as arrays.  Every row carries its table index in the value
cells, so rows with equal keys are told apart in the output.

plan_model restates the documented plan rule (state_rekey.hpp "the compact, order-preserving key", state_rekey_plan.hpp
rwk_build_plan) from the integer rows alone; every case in CASES names the (key_bits, fast, ranked fields) it aims at and run_case
asserts them with the model before anything runs, so a case that drifts off its target fails whatever the library does."""
import collections
import functools

import numpy as np

from oracle import rw_state_oracle, wire

FIELDS = ("id", "address", "field_tag", "storage_key", "rw_counter")  # the order of the compact key's runs (RWK_F_*)
ALL_TARGETS = tuple(range(1, 12))
MIX = (8, 9, 6, 3, 7, 10, 5)  # Stack, Memory, AccountStorage, TxAccessListAccountStorage, CallContext, TxLog, Account
SW_TILE, GEN_TILE = 8192, 4096  # keys per tile: rwk_sweep_kernel (fast path) / rwk_hist + rwk_scatter (generic path)
RANK_MAX_ROWS, RANK_MIN_BITS, MAX_JOBS = 16384, 48, 8
CPU_MAX_ROWS = 20000  # cases up to this size also run through the CPU backend
M64 = (1 << 64) - 1


def B(lo, hi):
    return tuple(range(lo, hi))


# ---- arrays <-> integers ----------------------------------------------------------------------------------------------------
def table_ints(rw):
    """uint64[n, ncells, 4] -> list of n lists of Python ints, column by column (only words that are set anywhere are combined)"""
    cols = []
    for c in range(rw.shape[1]):
        acc = rw[:, c, 0].tolist()
        for w in (1, 2, 3):
            if rw[:, c, w].any():
                sh = 64 * w
                acc = [a | (b << sh) for a, b in zip(acc, rw[:, c, w].tolist())]
        cols.append(acc)
    return [list(r) for r in zip(*cols)]


def ops_array(e_ops):
    """the checker's op list -> uint64[12, m, 4], the layout of the device's output"""
    out = np.zeros((12, len(e_ops), 4), dtype=np.uint64)
    for s in range(12):
        col = [o[s] for o in e_ops]
        try:
            out[s, :, 0] = np.array(col, dtype=np.uint64)  # (most slots fit one word)
        except OverflowError:
            out[s] = wire.ints_to_cells(col)
    return out


# ---- the plan model ----------------------------------------------------------------------------------------------------------
def state_keys(rows):
    """per RW row: (state tag, (id, address, field_tag, storage_key, rw_counter)) of the op it becomes, None for a row left out"""
    out = []
    for c in rows:
        try:
            r = rw_state_oracle.rekey_row(c, 0)
        except (ValueError, OverflowError):
            r = None
        if r is None:
            out.append(None)
        else:
            o = r[0]
            out.append((o[2], (o[3], o[4], o[5], o[6], o[0])))
    return out


def _bitlen(x):
    return int(x).bit_length()


def plan_model(rows, allow_ranks=True):
    """The compact-key plan of a table, from its integer rows: per class (state tag) and field word the varying mask is the bits
    that are 1 somewhere and 0 somewhere in the class, its run is lowest to highest set bit; a field is replaced by its rank when its
    width is > 48 bits, the class has <= 16,384 rows, fewer than 8 rank jobs are taken (classes by ascending tag, fields in key order)
    and the rank needs fewer bits than the field.  key_bits = 4 + the widest class; the fast path applies iff the key fits two words
    and eight passes.  -> dict(key_bits, key_words, n_passes, fast, ranked [(tag, field name)], n_ops, classes {tag: dict(count,
    width, runs)}), a run being (field index, word, shift, nbits), or (5 + field index, 0, 0, rank bits) for a rank."""
    keys = state_keys(rows)
    acc = {}
    for k in keys:
        if k is None:
            continue
        a = acc.setdefault(k[0], [0, [0] * 5, [0] * 5])
        a[0] += 1
        for f in range(5):
            a[1][f] |= k[1][f]
            a[2][f] |= ~k[1][f]
    classes, ranked, jobs, widest = {}, [], 0, 0
    for tag in sorted(acc):
        count, ors, nands = acc[tag]
        runs, width = [], 0
        for f in range(5):
            vary = ors[f] & nands[f] & ((1 << 256) - 1)
            f_runs, f_width = [], 0
            for w in range(7, -1, -1):
                m = (vary >> (32 * w)) & 0xFFFFFFFF
                if not m:
                    continue
                lo, hi = (m & -m).bit_length() - 1, _bitlen(m)
                f_runs.append((f, w, lo, hi - lo))
                f_width += hi - lo
            rank_bits = _bitlen(count - 1) or 1
            if allow_ranks and f_width > RANK_MIN_BITS and count <= RANK_MAX_ROWS and jobs < MAX_JOBS and rank_bits < f_width:
                jobs += 1
                ranked.append((tag, FIELDS[f]))
                runs.append((5 + f, 0, 0, rank_bits))
                width += rank_bits
            else:
                runs += f_runs
                width += f_width
        classes[tag] = dict(count=count, width=width, runs=runs)
        widest = max(widest, width)
    key_bits = 4 + widest
    key_words, n_passes = (key_bits + 31) // 32, (key_bits + 7) // 8
    return dict(key_bits=key_bits, key_words=key_words, n_passes=n_passes, fast=key_words <= 2 and n_passes <= 8, ranked=ranked,
                n_ops=1 + sum(c["count"] for c in classes.values()), classes=classes)


def model_keys(rows, plan):
    """the compact key (an int of plan['key_bits'] bits: tag | runs | zero padding) of every row, None for a row left out"""
    keys = state_keys(rows)
    rank_of = {}
    for tag, cp in plan["classes"].items():
        for run in cp["runs"]:
            if run[0] >= 5:
                f = run[0] - 5
                vals = sorted(k[1][f] for k in keys if k is not None and k[0] == tag)
                first = {}
                for i, v in enumerate(vals):
                    first.setdefault(v, i)  # rank = number of members with a smaller value
                rank_of[(tag, f)] = first
    out = []
    for k in keys:
        if k is None:
            out.append(None)
            continue
        tag, f = k
        cp = plan["classes"][tag]
        v = tag
        for fld, word, shift, nbits in cp["runs"]:
            bits = rank_of[(tag, fld - 5)][f[fld - 5]] if fld >= 5 else (f[fld] >> (32 * word + shift)) & ((1 << nbits) - 1)
            v = (v << nbits) | bits
        out.append(v << (plan["key_bits"] - 4 - cp["width"]))
    return out


def straddling_runs(plan):
    """runs of the widest class that cross a boundary between two 32-bit output words of the packed key"""
    cp = max(plan["classes"].values(), key=lambda c: c["width"])
    pos = 32 * plan["key_words"] - plan["key_bits"] + 4  # bits in front of the first run: leading zeros + tag
    out = []
    for run in cp["runs"]:
        if pos // 32 != (pos + run[3] - 1) // 32:
            out.append(run)
        pos += run[3]
    return out


# ---- the knob builder --------------------------------------------------------------------------------------------------------
def _rand_bits(rng, m, bits, by_byte=False):
    """uint64[m, 4]: random bits at the positions `bits` of a 256-bit value, zeros elsewhere; by_byte: the positions that share an
    aligned byte move together (the byte's bits are all 0 or all 1)"""
    out = np.zeros((m, 4), dtype=np.uint64)
    if by_byte:
        for g in sorted({b // 8 for b in bits}):
            mask = sum(1 << (b % 64) for b in bits if b // 8 == g)
            out[:, g // 8] |= rng.integers(0, 2, m, dtype=np.uint64) * np.uint64(mask)
        return out
    for w in range(4):
        mask = sum(1 << (b - 64 * w) for b in bits if b // 64 == w)
        if mask:
            out[:, w] = rng.integers(0, 1 << 64, m, dtype=np.uint64) & np.uint64(mask)
    return out


def _const(v):
    return np.array([(int(v) >> (64 * w)) & M64 for w in range(4)], dtype=np.uint64)


def _shl48(a):
    out = np.zeros_like(a)
    out[:, 0] = a[:, 0] << np.uint64(48)
    for w in (1, 2, 3):
        out[:, w] = (a[:, w] << np.uint64(48)) | (a[:, w - 1] >> np.uint64(16))
    return out


def _cells(target, f, rng):
    """RW rows uint64[m, 14, 4] whose key cells carry the fields f (dict name -> uint64[m, 4]) in the slots of each row's target:
    CallContext's field tag travels in the address cell (kept below 16: the State circuit drops tags above 24), TxLog's address cell
    is log_id << 48 | field_tag << 32 | index"""
    m = len(target)
    rw = np.zeros((m, 14, 4), dtype=np.uint64)
    rw[:, 0] = f["rw_counter"]
    rw[:, 1, 0] = rng.integers(0, 2, m, dtype=np.uint64)
    rw[:, 2, 0] = target
    rw[:, 3] = f["id"]
    rw[:, 4] = f["address"]
    rw[:, 5] = f["field_tag"]
    rw[:, 6, :2] = f["storage_key"][:, :2]
    rw[:, 7, :2] = f["storage_key"][:, 2:]
    cc = target == 7
    rw[cc, 4] = 0
    rw[cc, 4, 0] = f["field_tag"][cc, 0] & np.uint64(15)
    rw[cc, 5] = 0
    tl = target == 10
    packed = _shl48(f["address"][tl])
    packed[:, 0] |= ((f["field_tag"][tl, 0] & np.uint64(0xFFFF)) << np.uint64(32)) | (f["storage_key"][tl, 0] & np.uint64(0xFFFFFFFF))
    rw[tl, 4] = packed
    return rw


def knob_table(n, targets, vary, *, order="random", repeat=1, dup=0.3, dropped=0.004, rejected=0.004, counts=None, base=None,
               by_byte=False, interleave=False, half_equal=None, seed=1):
    """An RW table of n rows -> (rw uint64[n, 14, 4], rw_flags uint32[n]).
      targets     the Target values of the rows that carry keys: drawn at random, cyclically row by row with `interleave`, or with
                  `counts` {target: rows} exactly that many of each (then n = their sum + the dropped and rejected rows)
      vary        {field name: bit positions that vary} (or {target: such a dict}); the other key bits are those of base[field]
                  (default 0).  Of every target's rows one has all its varying bits 0 and one has them all 1, so every varying
                  run's top and bottom bit do vary
      order       of the rows that carry keys: "random", "sorted", "reverse" (descending); repeat: every key (rw_counter included)
                  stands r times, adjacent in the sorted orders
      dup         share of the keys that are another row's full key again
      dropped     share of rows the re-keying drops (CallContext field tag > 24); rejected: share it rejects (half: no such target,
                  half: storage_key hi >= 2^128).  They stand at random positions
      half_equal  (target, field): half of that target's keys carry one and the same value in the field
    Value cells: cell 8 holds the row's table index + 1, cell 12 a second function of it; the rest is random."""
    rng = np.random.default_rng(seed)
    n_drop, n_rej = int(round(n * dropped)), int(round(n * rejected))
    if counts:
        assert n == sum(counts.values()) + n_drop + n_rej
    n_key = n - n_drop - n_rej
    n_groups = -(-n_key // repeat)
    targets = np.array(targets if targets is not None else tuple(counts), dtype=np.uint64)
    if counts:
        assert repeat == 1
        g_target = rng.permutation(np.concatenate([np.full(c, t, dtype=np.uint64) for t, c in counts.items()]))
    elif interleave:
        g_target = targets[np.arange(n_groups) % len(targets)]
    else:
        g_target = targets[rng.integers(0, len(targets), n_groups)]
    per_target = vary and all(isinstance(k, int) for k in vary)
    f = {name: np.zeros((n_groups, 4), dtype=np.uint64) for name in FIELDS}
    for t in np.unique(g_target).tolist():
        idx = np.nonzero(g_target == t)[0]
        v = (vary.get(t, {}) if per_target else vary) or {}
        for name in FIELDS:
            bits = tuple(v.get(name, ()))
            vals = _rand_bits(rng, len(idx), bits, by_byte)
            if len(idx) >= 2:
                vals[0] = 0
                vals[1] = _const(sum(1 << b for b in bits))
            f[name][idx] = vals | _const((base or {}).get(name, 0))
        n_dup = int(dup * (len(idx) - 2))
        if n_dup > 0:  # full keys again: rows 2.. of the target copy rows that are no copies themselves
            pick = rng.permutation(len(idx) - 2) + 2
            dst, src_pool = idx[pick[:n_dup]], np.concatenate([idx[:2], idx[pick[n_dup:]]])
            src = src_pool[rng.integers(0, len(src_pool), n_dup)]
            for name in FIELDS:
                f[name][dst] = f[name][src]
        if half_equal and half_equal[0] == t:  # (after the copies: exactly half of the target's rows)
            same = idx[2 + rng.permutation(len(idx) - 2)[: len(idx) // 2]]
            f[half_equal[1]][same] = _rand_bits(rng, 1, tuple(v.get(half_equal[1], ())))[0] | _const((base or {}).get(half_equal[1], 0))
    rows = np.repeat(np.arange(n_groups), repeat)[:n_key]
    if order == "random" and not interleave:
        rows = rng.permutation(rows)
    key_rw = _cells(g_target[rows], {name: f[name][rows] for name in FIELDS}, rng)
    if order in ("sorted", "reverse") and n_key:
        keys = state_keys(table_ints(key_rw))
        perm = sorted(range(n_key), key=lambda i: (keys[i][0],) + keys[i][1], reverse=order == "reverse")
        key_rw = key_rw[np.array(perm)]
    # dropped and rejected rows, at random positions
    n_sp = n_drop + n_rej
    sp_f = {name: _rand_bits(rng, n_sp, B(0, 20)) for name in FIELDS}
    sp_target = targets[rng.integers(0, len(targets), n_sp)] if n_sp else np.zeros(0, dtype=np.uint64)
    sp = _cells(sp_target, sp_f, rng)
    sp[:n_drop, 2, 0] = 7
    sp[:n_drop, 4] = 0
    sp[:n_drop, 4, 0] = rng.integers(25, 400, n_drop, dtype=np.uint64)
    half = n_drop + n_rej // 2
    sp[n_drop:half, 2, 0] = rng.choice(np.array([0, 12, 13, 255, 1 << 40], dtype=np.uint64), half - n_drop)
    sp[half:, 7, 2] = rng.integers(1, 1 << 40, n_sp - half, dtype=np.uint64)
    rw = np.zeros((n, 14, 4), dtype=np.uint64)
    where = np.zeros(n, dtype=bool)
    where[rng.permutation(n)[:n_sp]] = True
    rw[where] = sp
    rw[~where] = key_rw
    return finish_values(rw, rng)


def finish_values(rw, rng):
    """the value cells of a table whose key cells are set, and its rw_flags: cell 8 = table index + 1 (distinct), cell 12 a second
    function of the index; value hi / committed hi are 128-bit or 0; every cell below 2^128"""
    n = rw.shape[0]
    i = np.arange(n, dtype=np.uint64)
    rw[:, 8, 0] = i + np.uint64(1)
    rw[:, 8, 1] = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    rw[:, 12, 0] = np.uint64(3) * i + np.uint64(1)
    for c in (9, 10, 11, 13):
        some = rng.integers(0, 2, n, dtype=np.uint64) if c in (9, 13) else np.ones(n, dtype=np.uint64)
        rw[:, c, 0] = rng.integers(0, 1 << 64, n, dtype=np.uint64) * some
        rw[:, c, 1] = rng.integers(0, 1 << 64, n, dtype=np.uint64) * some
    return rw, rng.integers(0, 4, n, dtype=np.uint32)


# ---- the cases ---------------------------------------------------------------------------------------------------------------
V52 = {"id": B(0, 12), "address": B(0, 16), "rw_counter": B(0, 20)}                          # 7 passes (odd)
V60 = {"id": B(0, 12), "address": B(0, 16), "storage_key": B(0, 8), "rw_counter": B(0, 20)}  # 8 passes (even)
V65 = {"id": B(0, 20), "address": B(0, 20), "rw_counter": B(0, 21)}                          # 3 words, 9 passes, no field above 48 bits
V105 = {"id": B(0, 20), "address": B(0, 30), "storage_key": B(0, 30), "rw_counter": B(0, 21)}  # 4 words, 14 passes
WIDE = {"id": B(0, 6), "address": B(0, 160), "storage_key": B(0, 256), "rw_counter": B(0, 16)}
NARROW = {"id": B(0, 8), "address": B(0, 10), "rw_counter": B(0, 16)}
N_DIGIT = 5 * SW_TILE  # five fast tiles = ten generic tiles


def _tiled(tile, tile_bits, seed):
    """(d) tile t of the input holds only keys whose top digit is that of t: the id's top `tile_bits` bits are the tile index"""
    rw, fl = knob_table(N_DIGIT, (8,), {"id": B(0, 9), "address": B(0, 16), "rw_counter": B(0, 15)}, dropped=0, rejected=0, seed=seed)
    rw[:, 3, 0] |= (np.arange(N_DIGIT, dtype=np.uint64) // np.uint64(tile)) << np.uint64(9)
    assert int(rw[:, 3, 0].max()) >> 9 == N_DIGIT // tile - 1 < 1 << tile_bits
    return rw, fl


def _one_differs(field_cell, base_value, odd_value, seed):
    """(f) 40,959 rows with one full key and, in the middle of a tile, one row that differs from them in one bit"""
    rw, fl = knob_table(N_DIGIT, (8,), {}, dup=0, dropped=0, rejected=0, base={"id": 5, "address": 1000, "rw_counter": 7}, seed=seed)
    rw[:, field_cell] = _const(base_value)
    rw[2 * SW_TILE + 3617, field_cell] = _const(odd_value)
    return rw, fl


def _case(name, n, build, key_bits, fast=None, ranked=(), env=None, check=None):
    return dict(name=name, n=n, build=build, key_bits=key_bits, fast=(key_bits <= 64) if fast is None else fast, ranked=list(ranked),
                env=env or {}, check=check)


def _knob(n, targets, vary, **kw):
    return functools.partial(knob_table, n, targets, vary, **kw)


NO_FAST = {"ZK_REKEY_NO_FAST": "1"}


def _digit_cases():
    one = (8,)
    forms = [
        ("a-identical", _knob(N_DIGIT, one, {}, dup=0, dropped=0, rejected=0, base={"id": 3, "address": 1023, "rw_counter": 77}, seed=31), 4),
        ("b-sorted", _knob(N_DIGIT, one, V52, order="sorted", dropped=0, rejected=0, seed=32), 52),
        ("c-reverse-x3", _knob(N_DIGIT, one, V52, order="reverse", repeat=3, dup=0, dropped=0, rejected=0, seed=33), 52),
        ("e-digits-00-ff", _knob(N_DIGIT, one, {"id": B(0, 16), "address": B(0, 16), "rw_counter": B(0, 16)}, by_byte=True, dup=0,
                                 dropped=0, rejected=0, seed=35), 52),
        ("f-top-bit", functools.partial(_one_differs, 3, (1 << 40) | 5, 5, 36), 5),
        ("f-bottom-bit", functools.partial(_one_differs, 0, 7, 6, 37), 5),
    ]
    out = []
    for name, build, kb in forms:
        out.append(_case("digits-fast-" + name, N_DIGIT, build, kb))
        out.append(_case("digits-generic-" + name, N_DIGIT, build, kb, env=NO_FAST))
    # (d): the top digit is 0 | tag (4 bits) | tile (3 bits) with 47 key bits, tag (4 bits) | tile (4 bits) with 48
    out.append(_case("digits-fast-d-tile-is-top-digit", N_DIGIT, functools.partial(_tiled, SW_TILE, 3, 34), 47, check=("tiles", SW_TILE)))
    out.append(_case("digits-generic-d-tile-is-top-digit", N_DIGIT, functools.partial(_tiled, GEN_TILE, 4, 34), 48, env=NO_FAST,
                     check=("tiles", GEN_TILE)))
    return out


def _cases():
    c = []
    # tile edges of the fast sweep: 8,192 keys per tile, look-back of eight descriptors per round trip; odd and even pass counts
    for n, v, kb in ((8191, V52, 52), (8192, V60, 60), (8193, V52, 52), (16384, V60, 60), (16385, V52, 52), (73728, V60, 60),
                     (73729, V52, 52), (139269, V60, 60)):
        c.append(_case(f"fast-tiles-{n}", n, _knob(n, MIX, v, seed=n), kb))
    # tile edges of the generic path: 4,096 keys per tile, keys wider than 64 bits by themselves
    for n, v, kb in ((4095, V105, 105), (4096, V65, 65), (4097, V105, 105), (36865, V65, 65)):
        c.append(_case(f"generic-tiles-{n}", n, _knob(n, MIX, v, seed=n), kb))
    both = _knob(36865, MIX, V60, seed=77)
    c.append(_case("both-paths-36865-fast", 36865, both, 60))
    c.append(_case("both-paths-36865-generic", 36865, both, 60, env=NO_FAST))
    c += _digit_cases()
    # plan boundaries: one class (Memory), 9,000 rows, the hostile mix
    for kb, v in ((4, {}), (8, {"rw_counter": B(0, 4)}), (9, {"rw_counter": B(0, 5)}), (32, {"id": B(0, 8), "rw_counter": B(0, 20)}),
                  (33, {"id": B(0, 9), "rw_counter": B(0, 20)}), (64, {"id": B(0, 20), "address": B(0, 20), "rw_counter": B(0, 20)}), (65, V65)):
        c.append(_case(f"plan-key-bits-{kb}", 9000, _knob(9000, (9,), v, seed=100 + kb), kb))
    c.append(_case("plan-mask-80000001", 9000, _knob(9000, (9,), {"id": B(0, 10), "address": (0, 31), "rw_counter": B(0, 16)}, seed=111), 62,
                   check=("run", (1, 0, 0, 32))))
    c.append(_case("plan-run-straddles-words", 9000, _knob(9000, (9,), {"id": B(0, 20), "address": B(0, 20), "rw_counter": B(0, 16)}, seed=112),
                   60, check=("straddle", (1, 0, 0, 20))))
    c.append(_case("plan-storage-key-top-word", 9000, _knob(9000, (6,), {"storage_key": B(224, 256), "rw_counter": B(0, 12)}, seed=113), 48,
                   check=("run", (3, 7, 0, 32))))
    c.append(_case("plan-two-class-widths", 9000, _knob(9000, (8, 9), {8: {"id": B(0, 20), "address": B(0, 10), "rw_counter": B(0, 20)},
                                                                        9: {"rw_counter": B(0, 12)}}, seed=114), 54, check=("widths", {3: 50, 2: 12})))
    c.append(_case("plan-nothing-kept", 9000, _knob(9000, MIX, V52, dropped=0.5, rejected=0.5, seed=115), 4, check=("n_ops", 1)))
    # the rank rule
    for m in (16384, 16385):
        c.append(_case(f"rank-storage-class-{m}", m + 1000 + 16, _knob(m + 1000 + 16, None, {6: WIDE, 8: NARROW}, counts={6: m, 8: 1000},
                                                                       dropped=8 / (m + 1016), rejected=8 / (m + 1016), seed=m),
                       54 if m == 16384 else 442, ranked=[(4, "address"), (4, "storage_key")] if m == 16384 else []))
    c.append(_case("rank-width-48-raw", 9000, _knob(9000, (9,), {"address": B(0, 48), "rw_counter": B(0, 10)}, seed=121), 62))
    c.append(_case("rank-width-49-ranked", 9000, _knob(9000, (9,), {"address": B(0, 49), "rw_counter": B(0, 10)}, seed=122), 28,
                   ranked=[(2, "address")]))
    w3 = {"id": B(0, 50), "address": B(0, 160), "storage_key": B(0, 256), "rw_counter": B(0, 10)}
    c.append(_case("rank-ninth-candidate-raw", 3000, _knob(3000, None, {6: w3, 2: w3, 3: w3}, counts={6: 1000, 2: 1000, 3: 1000}, dropped=0,
                                                            rejected=0, seed=123), 290,
                   ranked=[(t, f) for t in (4, 8) for f in ("id", "address", "storage_key")] + [(9, "id"), (9, "address")]))
    for m, kb in ((257, 4 + 6 + 9 + 9 + 16), (16384, 54)):
        c.append(_case(f"rank-half-equal-{m}", m + 1000, _knob(m + 1000, None, {6: WIDE, 8: NARROW}, counts={6: m, 8: 1000}, dropped=0, rejected=0,
                                                               half_equal=(6, "address"), seed=130 + m), kb,
                       ranked=[(4, "address"), (4, "storage_key")], check=("half_equal", m)))
    # the scan: all eleven targets cyclically row by row; 263,169 = 256 * 1024 + 1025 rows take a second, partial trip through the
    # grid-stride loops of rwk_scan_kernel and rwk_pack64_kernel
    v_scan = {"id": B(0, 12), "address": B(0, 16), "field_tag": B(0, 3), "rw_counter": B(0, 20)}
    for n in (4100, 263169):
        c.append(_case(f"scan-eleven-classes-{n}", n, _knob(n, ALL_TARGETS, v_scan, interleave=True, dropped=0.002, rejected=0.002, seed=n), 55,
                       check=("interleaved", 11)))
    return c


CASES = {c["name"]: c for c in _cases()}
ALL_CASES = list(CASES)
CPU_CASES = [k for k, c in CASES.items() if c["n"] <= CPU_MAX_ROWS and not c["env"]]
SESSION_TABLE = "digits-fast-b-sorted"  # a five-tile fast table; the random-order one below for the consumers


def consumer_table(n):
    """a table the State witness assignment accepts row for row (addresses below 2^160, no Account rows, nothing rejected), for the
    sessions that go on from the sorted order: the hostile mix otherwise, keys of 60 bits (fast path)"""
    return knob_table(n, (8, 9, 6, 3, 2, 7, 10, 4, 11), V60, rejected=0, seed=1000 + n)


def describe(case):
    """n, key_bits, path and tile count of a case, as the documents list them"""
    fast = case["fast"] and not case["env"]
    tile = SW_TILE if fast else GEN_TILE
    return dict(name=case["name"], n=case["n"], key_bits=case["key_bits"], path="fast" if fast else "generic", tiles=-(-case["n"] // tile),
                passes=(case["key_bits"] + 7) // 8, ranked=len(case["ranked"]))


def check_aim(case, rw, rows, plan):
    """what a case claims beyond (key_bits, fast, ranked), from the input and the model alone"""
    kind, arg = case["check"]
    widest = max(plan["classes"].values(), key=lambda cp: cp["width"]) if plan["classes"] else None
    if kind == "run":
        assert arg in widest["runs"], widest["runs"]
    elif kind == "straddle":
        assert arg in straddling_runs(plan), (straddling_runs(plan), widest["runs"])
    elif kind == "widths":
        assert {t: cp["width"] for t, cp in plan["classes"].items()} == arg
    elif kind == "n_ops":
        assert plan["n_ops"] == arg
    elif kind == "tiles":  # every tile has one top digit, and no two tiles the same
        keys = model_keys(rows, plan)
        top = [k >> (8 * (plan["n_passes"] - 1)) for k in keys]
        per_tile = [set(top[t : t + arg]) for t in range(0, len(top), arg)]
        assert all(len(s) == 1 for s in per_tile) and len(set.union(*per_tile)) == len(per_tile), per_tile
    elif kind == "half_equal":
        vals = [k[1][1] for k in state_keys(rows) if k is not None and k[0] == 4]
        assert len(vals) == arg and collections.Counter(vals).most_common(1)[0][1] >= arg // 2
    elif kind == "interleaved":  # no two neighbours of one class, outside the few dropped / rejected rows
        t = rw[:, 2, 0]
        assert np.count_nonzero(t[1:] == t[:-1]) <= 0.01 * len(t) and len(plan["classes"]) == arg
    else:
        raise AssertionError(kind)


def build_case(name):
    """-> (case, rw, rw_flags, integer rows), the plan the case aims at asserted with plan_model"""
    case = CASES[name]
    rw, fl = case["build"]()
    assert rw.shape == (case["n"], 14, 4)
    rows = table_ints(rw)
    plan = plan_model(rows)
    got = (plan["key_bits"], plan["fast"], plan["ranked"])
    assert got == (case["key_bits"], case["fast"], case["ranked"]), (name, got)
    if case["check"]:
        check_aim(case, rw, rows, plan)
    if name.startswith("digits-") and "e-digits" in name:  # every pass's digit but the top one (the tag) is 0x00 or 0xff
        ks = model_keys(rows, plan)
        assert {(k >> (8 * p)) & 0xFF for k in ks for p in range(plan["n_passes"] - 1)} == {0x00, 0xFF}
    return case, rw, fl, rows


def expected(rows, fl):
    """the checker's (ops uint64[12, m, 4], op flags, per-row status) of a table"""
    e_ops, e_flags, e_status = rw_state_oracle.rw_to_state_ops(rows, fl.tolist(), strict=False)
    return ops_array(e_ops), np.array(e_flags, dtype=np.uint32), np.array(e_status, dtype=np.uint32)


def assert_ops_equal(got, exp):
    """(ops, op_flags, status, fail_count) of the library against the checker's, as arrays; the first differing op is named"""
    ops, op_flags, status, fail_count = got
    e_ops, e_flags, e_status = exp
    assert np.array_equal(status, e_status), np.nonzero(status != e_status)[0][:5]
    assert fail_count == np.count_nonzero(e_status)
    assert ops.shape == e_ops.shape, (ops.shape, e_ops.shape)
    if not np.array_equal(ops, e_ops):
        j = int(np.nonzero((ops != e_ops).any(axis=(0, 2)))[0][0])
        raise AssertionError(f"op {j} of {ops.shape[1]}: got RW row {int(ops[7, j, 0]) - 1}, want RW row {int(e_ops[7, j, 0]) - 1}")
    assert np.array_equal(op_flags, e_flags)


def run_case(name, device, monkeypatch):
    """one directed case through zk_state_ops_from_rw on `device`, bit for bit against the checker"""
    from zkevm_specs_amd import oneshot

    case, rw, fl, rows = build_case(name)
    for k in ("ZK_REKEY_NO_FAST", "ZK_REKEY_NO_RANKS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    res, status, ops, op_flags = oneshot.state_ops_from_rw(rw, fl, device=device)
    assert_ops_equal((ops, op_flags, status, res.fail_count), expected(rows, fl))
