"""Seeded cases for the State entries over compact trace records (zk_state_verify_from_trace*, zk_state_ops_from_trace*), built IN RECORD
SPACE: a case is a list of op dicts (tag nibble, is_write, field tag, id, address, storage key, value, prev, aux0 with their forms) that
`records` encodes into the arrays of a zk_trace, so every case is representable by construction.

Two kinds of random table:
  wild   everything the records can hold: the tag nibbles the re-keying rejects, pool addresses wider than 160 bits, Account field tags
         outside 1..4.  The ops form returns per-row codes for these; the verdict form has no witness and raises.
  tame   the same generator without what leaves no witness (tags 1..11, addresses below 2^160 after the reduction, Account field tags
         1..4): the verdict form returns a verdict, row by row.
Consistent tables come from the existing builders of valid RW tables through trace.rw_ops_from_wire; `damage` hurts them in record space.
`assert_coverage` is the builder's own check that the cases hold what they claim."""
import functools
import random

import numpy as np

from zkevm_specs_amd import trace
from zkevm_specs_amd.wire import rows_to_rowmajor

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
M64, M128, M160, M256 = (1 << 64) - 1, (1 << 128) - 1, (1 << 160) - 1, (1 << 256) - 1
SIZES = (1, 2, 62, 63, 64, 65, 127, 251, 252, 253, 1023, 1024, 1025, 4097, 8191, 8192, 8193)
N_BIG = 73729  # ten fast-sort tiles (tests/rekey_cases.py)
ORACLE_MAX = 2000  # cases up to this size are also compared with the plain-Python chain
TARGETS = tuple(range(1, 12))
REJECTED_TAGS = (0, 12, 13, 14, 15)
# Target numbering (evm_circuit/table.py): Account 5, AccountStorage 6, CallContext 7, TxLog 10
T_ACCOUNT, T_STORAGE, T_CALLCTX, T_TXLOG, T_STACK, T_MEMORY = 5, 6, 7, 10, 8, 9
POOL_ADDRESSES = (0, 1, M160, M160 + 1, P - 1, P, P + 1, M256)
KEYS = (None, 0, M128, M128 + 1, M256)
CALLCTX_FIELDS = (0, 24, 25, 1 << 40)


def limbs(x):
    return [(x >> (64 * k)) & M64 for k in range(4)]


def op(tag, *, write=0, ft=0, id=0, addr=0, addr_pool=None, key=None, val=0, val_word=0, val_pool=None, prev=0, prev_word=0, prev_pool=False,
       aux=None, ctr=None):
    """one RW op; addr_pool / val_pool: None = pool exactly when the value needs it (2^64 or more)"""
    return {"tag": tag, "write": write, "ft": ft, "id": id, "addr": addr, "addr_pool": addr > M64 if addr_pool is None else addr_pool,
            "key": key, "val": val, "val_word": val_word, "val_pool": val > M64 if val_pool is None else val_pool, "prev": prev,
            "prev_word": prev_word, "prev_pool": prev_pool or prev > M64, "aux": aux, "ctr": ctr}


def records(ops, counters="base", base=1, seed=0):
    """ops -> the records dict of engine / oneshot (no steps).  counters: 'base' (rw_base + i), 'gaps' (explicit, ascending with gaps),
    'end' (rw_base + i ending at 2^64 - 1), 'explicit_end' (explicit, the last one 2^64 - 1), 'own' (each op's ctr)."""
    n = len(ops)
    head, pool = np.zeros(n, np.uint32), []
    arr = {k: np.zeros(n, np.uint64) for k in ("id", "addr", "val", "prev")}
    for i, o in enumerate(ops):
        h = (o["write"] & 1) | (o["tag"] << 1) | (o["ft"] << 8) | (o["val_word"] << 16) | (o["prev_word"] << 17)
        arr["id"][i] = o["id"]
        for bit, wide, name, value in ((trace.H_ADDR_POOL, o["addr_pool"], "addr", o["addr"]), (trace.H_KEY, o["key"] is not None, None, o["key"]),
                                       (trace.H_VALUE_POOL, o["val_pool"], "val", o["val"]), (trace.H_PREV_POOL, o["prev_pool"], "prev", o["prev"]),
                                       (trace.H_AUX, o["aux"] is not None, None, o["aux"])):
            if wide:
                h |= bit
                pool.append(limbs(value))
            elif name:
                arr[name][i] = value
        head[i] = h
    rec = {"head": head, **arr, "rw_counter": None, "rw_base": base, "pool": np.array(pool, dtype=np.uint64).reshape(len(pool), 4)}
    rng = random.Random(seed)
    if counters == "end":
        rec["rw_base"] = (1 << 64) - n
    elif counters in ("gaps", "explicit_end"):
        c, out = rng.randrange(1, 1 << 40), []
        for _ in range(n):
            out.append(c)
            c += rng.choice((1, 1, 2, 7, 1 << 20))
        if counters == "explicit_end":
            out = [x + (M64 - out[-1]) for x in out]
        rec["rw_counter"] = np.array(out, dtype=np.uint64)
    elif counters == "own":
        rec["rw_counter"] = np.array([o["ctr"] for o in ops], dtype=np.uint64)
    return rec


def ops_of(rec):
    """the inverse of `records` (counters kept as each op's ctr)"""
    pool, at, out = [sum(int(x) << (64 * k) for k, x in enumerate(w)) for w in rec["pool"]], 0, []
    for i, h in enumerate(int(x) for x in rec["head"]):
        def take(bit):
            nonlocal at
            if not h & bit:
                return None
            at += 1
            return pool[at - 1]
        a, key, v, p, aux = take(trace.H_ADDR_POOL), take(trace.H_KEY), take(trace.H_VALUE_POOL), take(trace.H_PREV_POOL), take(trace.H_AUX)
        ctr = int(rec["rw_counter"][i]) if rec.get("rw_counter") is not None else int(rec.get("rw_base", 1)) + i
        out.append(op((h >> 1) & 15, write=h & 1, ft=(h >> 8) & 255, id=int(rec["id"][i]), addr=int(rec["addr"][i]) if a is None else a,
                      addr_pool=a is not None, key=key, val=int(rec["val"][i]) if v is None else v, val_word=(h >> 16) & 1, val_pool=v is not None,
                      prev=int(rec["prev"][i]) if p is None else p, prev_word=(h >> 17) & 1, prev_pool=p is not None, aux=aux, ctr=ctr))
    return out


# ---- random tables --------------------------------------------------------------------------------------------------------------------
def _txlog_addr(rng):
    log_id, ft, index = (rng.choice((0, 1, 0xFFFF)), rng.choice((0, 1, 3, 0xFFFF)), rng.choice((0, 1, M64 >> 32)))
    return (log_id << 48) | (ft << 32) | index


def _value(rng):
    """(val, val_word, val_pool): narrow and wide, with and without the is_word bit, wide values of p or more without it"""
    kind = rng.randrange(8)
    if kind < 3:
        return rng.choice((0, 1, rng.getrandbits(64), M64)), rng.randrange(2), False
    if kind == 3:
        return rng.getrandbits(20), rng.randrange(2), True  # a small value in the pool
    wide = rng.choice((M64 + 1, M128, M128 + 1, P - 1, P, P + 1, M256, rng.getrandbits(256), rng.getrandbits(130)))
    return wide, rng.randrange(2), True


def _key_group(rng, tame):
    """one key (tag, id, address, field tag, storage key) of a new group"""
    tag = rng.choice(TARGETS) if tame or rng.random() > 0.03 else rng.choice(REJECTED_TAGS)
    k = {"tag": tag, "id": rng.choice((0, 1, rng.getrandbits(10), rng.getrandbits(64))), "ft": 0, "key": None, "addr": 0, "addr_pool": False}
    if tag == T_CALLCTX:
        k["addr"] = rng.choice(CALLCTX_FIELDS) if rng.random() < 0.3 else rng.randrange(25)
    elif tag == T_TXLOG:
        k["addr"] = _txlog_addr(rng)
        if rng.random() < 0.1:
            k["addr"], k["addr_pool"] = (M64 + 1 + rng.getrandbits(70)) & M160, True  # a TxLog row with a pool address above 2^64
    elif tag in (T_STACK, T_MEMORY):
        k["addr"] = rng.randrange(1024) if tag == T_STACK else rng.getrandbits(rng.choice((10, 40)))
    else:
        pick = rng.random()
        if pick < 0.35:
            a = rng.choice(POOL_ADDRESSES)
            if tame and P > a > M160 or tame and a == M256:
                a = rng.choice((0, 1, M160, P, P + 1))
            k["addr"], k["addr_pool"] = a, True
        elif pick < 0.7:
            k["addr"], k["addr_pool"] = rng.getrandbits(160), True
        else:
            k["addr"] = rng.getrandbits(rng.choice((8, 64)))
        k["key"] = rng.choice(KEYS) if rng.random() < 0.7 else rng.getrandbits(256)
        k["ft"] = rng.randrange(1, 5) if tag == T_ACCOUNT and (tame or rng.random() > 0.1) else rng.choice((0, 1, 5, 255))
        if tag != T_ACCOUNT and tame:
            k["ft"] = rng.choice((0, 1, 255))
    return k


def random_ops(n, seed, tame):
    """n ops in input (counter) order: key groups of 1..40 accesses, their accesses spread over the table"""
    rng = random.Random(seed * 1000003 + n)
    ops = []
    while len(ops) < n:
        k = _key_group(rng, tame)
        for _ in range(min(rng.choice((1, 1, 2, 3, 5, 8, 17, 40)), n - len(ops))):
            val, word, vpool = _value(rng)
            aux = rng.choice((None, None, 0, rng.getrandbits(64), M256, rng.getrandbits(256)))  # on Storage / Account rows and on tags that ignore it
            prev_pool = rng.random() < 0.15  # a prev pool word, so that the offsets behind it shift
            ops.append(op(k["tag"], write=rng.randrange(2), ft=k["ft"], id=k["id"], addr=k["addr"], addr_pool=k["addr_pool"], key=k["key"], val=val,
                          val_word=word, val_pool=vpool, prev=rng.getrandbits(256) if prev_pool else rng.getrandbits(64), prev_word=rng.randrange(2),
                          prev_pool=prev_pool, aux=aux))
    rng.shuffle(ops)
    return ops


def directed_ops(tame):
    """every directed row of the issue's list once, several accesses of some keys"""
    ops = []
    for t in TARGETS + (() if tame else REJECTED_TAGS):
        ops.append(op(t, id=3, addr=5, ft=1 if t == T_ACCOUNT else 0, val=7))
    for f in CALLCTX_FIELDS:  # CallContext: the field tag travels in addr; 25 and 2^40 are dropped
        ops.append(op(T_CALLCTX, id=9, addr=f, val=f & 0xFF))
    for log_id in (0, 0xFFFF):
        for ft in (0, 0xFFFF):
            for index in (0, 0xFFFFFFFF):
                ops.append(op(T_TXLOG, write=1, id=2, addr=(log_id << 48) | (ft << 32) | index, val=log_id + ft + index))
    ops.append(op(T_TXLOG, write=1, id=2, addr=(1 << 100) | (7 << 48) | (2 << 32) | 5, val=1))  # a pool address above 2^64
    ops.append(op(T_ACCOUNT, id=77, addr=12, ft=2, val=5, aux=5))  # an Account row with a non-zero id
    for a in POOL_ADDRESSES:
        if tame and (P > a > M160 or a == M256):
            continue
        for t in (T_STORAGE, T_ACCOUNT):
            ops.append(op(t, id=1, addr=a, addr_pool=True, ft=1 if t == T_ACCOUNT else 0, key=None if t == T_ACCOUNT else 11, val=3, aux=3))
    for key in KEYS:
        for rep in range(3):
            ops.append(op(T_STORAGE, write=rep & 1, id=1, addr=0xABCDEF, key=key, val=4, val_word=1, aux=4))
    for val in (M64, M64 + 1, M128, M128 + 1, P - 1, P, P + 1, M256):
        for word in (0, 1):
            ops.append(op(T_STACK, write=1, id=4, addr=1000 + len(ops) % 24, val=val, val_word=word))
            ops.append(op(T_STORAGE, write=1, id=1, addr=0x1234, key=val & M128, val=val, val_word=word, aux=val))
    ops.append(op(T_STACK, id=4, addr=1001, val=9, val_pool=True))             # a narrow value in the pool
    ops.append(op(T_MEMORY, id=4, addr=64, val=0xFF, aux=M256))                 # aux0 on a tag that ignores it
    ops.append(op(T_STORAGE, id=1, addr=0x1234, key=5, val=1, val_word=1))       # aux0 absent on a Storage row
    ops.append(op(T_ACCOUNT, addr=0x1234, ft=3, val=1, val_word=1))              # ... and on an Account row
    ops.append(op(T_STORAGE, id=1, addr=0x1234, key=5, val=1, prev=M256, prev_pool=True, aux=8))  # prev in the pool: later offsets shift
    return ops


def _is_tame(o):
    a = o["addr"] % P if o["addr_pool"] else o["addr"]
    return o["tag"] in TARGETS and a <= M160 and (o["tag"] != T_ACCOUNT or 1 <= o["ft"] <= 4)


@functools.lru_cache(maxsize=None)
def case(name):
    """name -> records dict.  'wild_<n>' / 'tame_<n>' random tables, 'directed_wild' / 'directed_tame', 'valid_block' / 'valid_directed'
    (consistent tables), counter forms vary with the size"""
    kind, _, arg = name.partition("_")
    if kind == "directed":
        ops = directed_ops(arg == "tame")
        random.Random(5).shuffle(ops)
        return records(ops, "gaps", seed=5)
    if kind in ("wild", "tame"):
        n = int(arg)
        form = ("base", "gaps", "end", "explicit_end")[SIZES.index(n) % 4] if n in SIZES else "base"
        return records(random_ops(n, 11 if kind == "wild" else 12, kind == "tame"), form, base=1 + n % 5, seed=n)
    if name == "valid_block":
        from tests.test_state_rekey import _valid_block_rw

        rows, flags = _valid_block_rw(300)
    elif name == "valid_directed":
        from tests.test_state_fused import directed_rw_base

        rows, flags = directed_rw_base()
    else:
        raise KeyError(name)
    return trace.rw_ops_from_wire(rows_to_rowmajor(rows, 14), np.array(flags, dtype=np.uint32))


def mutable(name):
    return {k: (v.copy() if hasattr(v, "copy") else v) for k, v in case(name).items()}


WILD = ["directed_wild"] + [f"wild_{n}" for n in SIZES]
TAME = ["directed_tame"] + [f"tame_{n}" for n in SIZES]
VALID = ["valid_block", "valid_directed"]
BIG = f"tame_{N_BIG}"


def damage(name, k, seed):
    """the consistent table `name` with k cells hurt in record space — val, the is_write bit, id, addr, the aux word — counters untouched
    (still strictly ascending), every row still one the assignment takes"""
    rng = random.Random(seed)
    ops = ops_of(case(name))
    for _ in range(k):
        o = ops[rng.randrange(len(ops))]
        what = rng.choice(("val", "val", "write", "id", "addr", "aux"))
        if what == "val":
            o["val"] ^= 1 << rng.randrange(0, 64 if not o["val_pool"] else 100)
        elif what == "write":
            o["write"] ^= 1
        elif what == "id":
            o["id"] = (o["id"] + 1) & 0xFFFFF
        elif what == "addr" and not o["addr_pool"] and o["tag"] in (T_STACK, T_MEMORY):
            o["addr"] = (o["addr"] + 1) & 0x3FF
        elif o["aux"] is not None:
            o["aux"] ^= 1 << rng.randrange(0, 100)
        else:
            o["val"] ^= 1
    return records(ops, "own")


def no_witness(name="valid_block"):
    """(label, records): tables the verdict form has no witness for — a row the re-keying rejects, an address FQ(w) wider than 160 bits,
    an Account field tag outside AccountFieldTag on a key's first access"""
    out = []
    base = ops_of(case(name))
    for tag in REJECTED_TAGS:
        ops = [dict(o) for o in base]
        ops[len(ops) // 2]["tag"] = tag
        out.append((f"tag nibble {tag}", records(ops, "own")))
    storage = [i for i, o in enumerate(base) if o["tag"] == T_STORAGE]
    assert storage
    for a in (M160 + 1, P - 1, M256):
        ops = [dict(o) for o in base]
        ops[storage[0]].update(addr=a, addr_pool=True)
        out.append((f"address {a:#x}", records(ops, "own")))
    base = ops_of(case("valid_directed"))  # (the table with Account rows)
    account = [i for i, o in enumerate(base) if o["tag"] == T_ACCOUNT]
    assert account
    for ft in (0, 5):
        ops = [dict(o) for o in base]
        for i in account:
            ops[i]["ft"] = ft
        out.append((f"Account field tag {ft}", records(ops, "own")))
    return out


# ---- the builder's own coverage -----------------------------------------------------------------------------------------------------------
def features(rec):
    f = set()
    ops = ops_of(rec)
    for o in ops:
        f.add(("tag", o["tag"]))
        if o["tag"] == T_CALLCTX:
            f.add(("callctx", o["addr"]))
        if o["tag"] == T_TXLOG:
            f.add(("txlog", "pool" if o["addr_pool"] else ((o["addr"] >> 48) in (0, 0xFFFF), (o["addr"] >> 32) & 0xFFFF in (0, 0xFFFF), o["addr"] & 0xFFFFFFFF in (0, 0xFFFFFFFF))))
        if o["tag"] == T_ACCOUNT and o["id"]:
            f.add("account with id")
        if o["addr_pool"]:
            f.add(("pool addr", o["addr"]))
        f.add(("key", o["key"] if o["key"] in KEYS else "other"))
        f.add(("value", o["val_pool"], o["val_word"], o["val_pool"] and o["val"] >= P))
        f.add(("aux", o["aux"] is not None, "keyed" if o["tag"] in (T_STORAGE, T_ACCOUNT) else "ignored"))
        if o["prev_pool"]:
            f.add("prev pool")
    c = rec.get("rw_counter")
    f.add(("counters", "base" if c is None else "explicit", (int(c[-1]) if c is not None else rec["rw_base"] + len(ops) - 1) == M64))
    return f


def required_features():
    need = {("tag", t) for t in TARGETS + REJECTED_TAGS} | {("callctx", x) for x in CALLCTX_FIELDS} | {("pool addr", a) for a in POOL_ADDRESSES}
    need |= {("key", k) for k in KEYS} | {("txlog", "pool"), ("txlog", (True, True, True)), "account with id", "prev pool"}
    need |= {("value", False, 0, False), ("value", False, 1, False), ("value", True, 0, False), ("value", True, 1, False), ("value", True, 0, True),
             ("value", True, 1, True)}
    need |= {("aux", a, b) for a in (False, True) for b in ("keyed", "ignored")}
    need |= {("counters", "base", False), ("counters", "explicit", False), ("counters", "base", True), ("counters", "explicit", True)}
    return need


def assert_coverage():
    seen = set()
    for name in WILD + TAME:
        seen |= features(case(name))
    missing = required_features() - seen
    assert not missing, sorted(map(str, missing))
    tame = set()
    for name in TAME:
        ops = ops_of(case(name))
        assert all(_is_tame(o) for o in ops), name
        tame |= features(case(name))
    # the verdict form still sees every target, the dropped CallContext rows, pool addresses at both ends of the 160 bits and either side of p
    assert {("tag", t) for t in TARGETS} <= tame and {("callctx", x) for x in CALLCTX_FIELDS} <= tame
    assert {("pool addr", a) for a in (0, 1, M160, P, P + 1)} <= tame
    sizes = sorted(len(case(n)["head"]) for n in TAME if n != "directed_tame")
    assert sizes == sorted(SIZES)

