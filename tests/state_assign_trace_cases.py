"""Cases for the State witness over compact trace records (zk_state_assign_from_trace*), on top of tests/state_trace_cases.py: AIMED tables,
tame tables in which no row is dropped or rejected, so that n_ops = n_rw + 1 lands on the sizes at which the row writer changes path —
the two lane pairs of a wavefront (32 ops), a wavefront (64), an assignment block (256), several blocks — and tables that steer the root
back-fill: a key group whose first access is the last op of a 256-op block, a table without keyed ops, a table whose last op is keyed.
`assert_built` checks, through the CPU backend's op list, that each of them is what it claims."""
import functools
import random

import numpy as np

from tests import state_trace_cases as sc

AIMED_N_OPS = (2, 63, 64, 65, 255, 256, 257, 1024, 1025, 4098)
TAG, ADDR, FT, KEY = 2, 4, 5, 6  # slots of the op list (include/zkevm_hip.h)
KEYED_TAGS = (4, 6)              # Tag.Storage, Tag.Account


def _kept(ops):
    """the same ops without the rows the re-keying drops: CallContext field tags above 24"""
    for o in ops:
        if o["tag"] == sc.T_CALLCTX and o["addr"] > 24:
            o["addr"] %= 25
    return ops


def _memory(n, id=1):
    return [sc.op(sc.T_MEMORY, write=i & 1, id=id, addr=i, val=i & 0xFF) for i in range(n)]


def _storage(addr, key, times, id=1):
    return [sc.op(sc.T_STORAGE, write=1, id=id, addr=addr, key=key, val=k + 1, val_word=1, aux=7) for k in range(times)]


@functools.lru_cache(maxsize=None)
def case(name):
    """'aimed_<n_ops>', 'block_edge', 'no_keyed', 'last_keyed' -> records dict (never changed: copy before writing)"""
    if name.startswith("aimed_"):
        n_ops = int(name[6:])
        ops = _kept(sc.random_ops(n_ops - 1, 21, True))
        return sc.records(ops, ("base", "gaps")[n_ops % 2], base=1 + n_ops % 3, seed=n_ops)
    if name == "block_edge":
        # State order: StartOp, Memory (254 ops: 1..254), Storage (255..), Account — the Storage group's first access is op 255, the last
        # op of block 0, its later accesses open block 1; more keyed groups behind them, and Memory ops of a second call in front
        ops = _memory(200) + _memory(54, id=2) + _storage(0xABC, 5, 4) + _storage(0xABC, 6, 2) + _storage(0xABD, sc.M256, 3)
        ops += [sc.op(sc.T_ACCOUNT, addr=0x77, ft=1 + k % 4, val=k, aux=k) for k in range(40)]
        random.Random(3).shuffle(ops)
        return sc.records(ops, "gaps", seed=3)
    if name == "no_keyed":
        ops = _memory(300) + [sc.op(sc.T_STACK, write=1, id=4, addr=1000 + k % 24, val=sc.P + k, val_word=k & 1) for k in range(100)]
        ops += [sc.op(sc.T_CALLCTX, id=9, addr=k % 25, val=k) for k in range(30)] + [sc.op(sc.T_TXLOG, write=1, id=2, addr=(k << 48) | 5, val=k) for k in range(20)]
        random.Random(4).shuffle(ops)
        return sc.records(ops, "base", base=7)
    if name == "last_keyed":
        ops = _memory(270) + _storage(0x1234, 11, 3) + [sc.op(sc.T_ACCOUNT, addr=sc.M160, addr_pool=True, ft=4, val=9, val_word=1, aux=sc.M256) for _ in range(2)]
        random.Random(5).shuffle(ops)
        return sc.records(ops, "gaps", seed=5)
    raise KeyError(name)


def mutable(name):
    return {k: (v.copy() if hasattr(v, "copy") else v) for k, v in case(name).items()}


AIMED = [f"aimed_{n}" for n in AIMED_N_OPS]
SHAPED = ["block_edge", "no_keyed", "last_keyed"]
ALL = AIMED + SHAPED


def _op_list(name):
    from zkevm_specs_amd import oneshot

    res, status, ops, _ = oneshot.state_ops_from_trace(case(name), device="cpu")
    assert res.ok and not status.any(), name  # no row rejected
    return ops


def _keyed(ops):
    return np.isin(ops[TAG, :, 0], KEYED_TAGS) & (ops[TAG, :, 1:] == 0).all(axis=1)


def _mpt_key(ops, j):
    return tuple(ops[s, j].tolist() for s in (ADDR, FT, KEY))


def assert_built():
    for n in AIMED_N_OPS:
        name = f"aimed_{n}"
        ops = _op_list(name)
        assert ops.shape[1] == n == len(case(name)["head"]) + 1, name  # no row dropped either
        assert all(sc._is_tame(o) for o in sc.ops_of(case(name))), name
    assert any(_keyed(_op_list(f"aimed_{n}")).any() for n in AIMED_N_OPS[2:])
    ops = _op_list("block_edge")
    keyed = _keyed(ops)
    assert ops.shape[1] > 300 and keyed[255] and not keyed[:255].any()  # op 255 is the first keyed op: its key's first access
    assert _mpt_key(ops, 255) == _mpt_key(ops, 256) == _mpt_key(ops, 258) != _mpt_key(ops, 259)  # ... whose later accesses are in block 1
    ops = _op_list("no_keyed")
    assert ops.shape[1] > 256 and not _keyed(ops).any()
    ops = _op_list("last_keyed")
    keyed = _keyed(ops)
    assert ops.shape[1] > 256 and keyed[-1] and keyed.sum() == 5 and not keyed[:256].any()
