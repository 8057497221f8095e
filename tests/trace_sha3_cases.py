"""Directed record tables for zk_sha3_from_trace*: every step's RW ops are appended with trace.RWDictionary in the order the reference's
gadget reads them (execution/sha3.py: two stack reads, the stack write of the digest, then the copy lookup's Memory reads), the step
records are written beside them.  case(name) -> dict(trace, randomness); expected(name) -> the model's result
(tests/trace_sha3_ref.py), computed once per name.

  lengths / lengths_gaps  a message of every length of LENGTHS (the rate, RLC-chunk and lane-group thresholds of the keccak kernels),
                          dense counters / explicit counters with gaps; two calls interleaved, duplicate messages, non-SHA3 steps of
                          several states between, an offset that is a pool word with size 0, a pushed word below 2^64 (in val: site 7)
  single                  one SHA3 step: its ops are the first and the last of the table
  sites / sites_dense     every site 1-7 in several forms, failing and clean steps mixed (explicit counters: an absent op is a counter
                          nobody holds; dense: the ops past the table's end)
  bytes_edges             message boundaries on both sides of the gather's wavefront and block edges
  ladder_<n>_<p>          n steps, p = all / alt / edges: SHA3 steps on both sides of the step kernel's wavefront and block edges"""
import functools

import numpy as np

from oracle.keccak import keccak256
from tests import trace_sha3_ref as ref
from zkevm_specs_amd.arithmetic import FQ, Word
from zkevm_specs_amd.evm_tables import CallContextFieldTag as CC, ExecutionState as ES
from zkevm_specs_amd.trace import RWDictionary

LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 135, 136, 137, 271, 272, 273, 543, 544, 545, 1087, 1088, 1089, 4200)
LADDER_SIZES = (1, 63, 64, 65, 255, 256, 257, 1025)
LADDER_PATTERNS = ("all", "alt", "edges")
RANDOMNESS = (0x1F2E3D4C5B6A7988 << 180) + (0xCAFE << 64) + 0x1234567
BIG = (1 << 255) + (0xABCDEF << 130) + 12345  # a 256-bit operand: a pool word
SITE_BYTES = (0, 63, 64, 99)                  # byte indices of a 100-byte message the per-byte sites are put on


def message(length, seed):
    return bytes((seed * 131 + i * 7 + (i >> 8) * 3) & 0xFF for i in range(length))


class Builder:
    def __init__(self, gaps=False):
        self.rw, self.steps, self.gaps = RWDictionary(1), [], gaps
        self.want = {}

    def step(self, state, call_id=1, sp=1000):
        if self.gaps:
            self.rw.rw_counter += 1 + len(self.steps) % 3  # counters nobody holds, between the steps
        self.steps.append([int(state), self.rw.rw_counter, call_id, 0, sp, 10**6, 0, 0, 0, 0, 0, 0, 0])
        return len(self.steps) - 1

    def skip(self):
        self.rw.rw_counter += 1  # an absent op: nobody holds this counter

    def sha3(self, data, offset=64, call_id=1, sp=1000, pushed=None, size=None, mut=(), byte_mut=None):
        """A SHA3 step over `data` at memory `offset`.  pushed: the word op 2 writes (default: the digest); size: the size operand
        (default len(data)); mut: what is wrong with ops 0..2; byte_mut: {byte index: what is wrong with its op}"""
        s = self.step(ES.SHA3, call_id, sp=sp)
        digest = int.from_bytes(keccak256(bytes(data)), "big")
        operands = [(0, sp, offset, False), (1, sp + 1, len(data) if size is None else size, False), (2, sp + 1, digest if pushed is None else pushed, True)]
        for k, addr, value, write in operands:
            cid = call_id
            if f"no{k}" in mut:
                self.skip()
                continue
            if f"tag{k}" in mut:
                self.rw.memory_read(call_id, addr, 7)
                continue
            if f"id{k}" in mut:
                cid = call_id + 77
            if f"addr{k}" in mut:
                addr += 5
            if write != (f"flip{k}" in mut):
                self.rw.stack_write(cid, addr, Word(value))
            else:
                self.rw.stack_read(cid, addr, Word(value))
        for i, b in enumerate(data):
            m = (byte_mut or {}).get(i)
            if m == "absent":
                self.skip()
            elif m == "write":
                self.rw.memory_write(call_id, offset + i, b)
            elif m == "id":
                self.rw.memory_read(call_id + 77, offset + i, b)
            elif m == "addr":
                self.rw.memory_read(call_id, offset + i + 1, b)
            elif m == "tag":
                self.rw.stack_read(call_id, offset + i, Word(b))
            elif m == "256":
                self.rw.memory_read(call_id, offset + i, 256)
            elif m == "wide":
                self.rw._append(0, 9, id=call_id, address=offset + i, value=FQ(1 << 70))  # a Memory read whose value is a pool word
            else:
                self.rw.memory_read(call_id, offset + i, b)
        return s

    def plain(self, state=ES.ADD, call_id=1, sp=1000):
        s = self.step(state, call_id, sp=sp)
        self.rw.stack_read(call_id, sp, Word(3))
        self.rw.stack_read(call_id, sp + 1, Word(4))
        self.rw.stack_write(call_id, sp + 1, Word(7))
        return s

    def context(self, call_id=1):
        s = self.step(ES.CALLDATASIZE, call_id)
        self.rw.call_context_read(call_id, CC.CallDataLength, 68)
        self.rw.stack_write(call_id, 999, Word(68))
        return s

    def case(self):
        rec = self.rw.ops()
        rec["steps"] = np.array(self.steps, dtype=np.uint64).reshape(len(self.steps), 13)
        return {"trace": rec, "randomness": RANDOMNESS}


def _lengths(gaps):
    b = Builder(gaps)
    b.plain()
    for j, n in enumerate(LENGTHS):
        b.sha3(message(n, j), offset=32 * j, call_id=1 + j % 2, sp=1000 - j % 3)  # two calls interleaved
        if j % 4 == 1:
            b.plain(ES.MUL, call_id=1 + j % 2)
        if j % 4 == 3:
            b.context(call_id=2)
    b.sha3(message(33, 4), offset=900)            # the bytes of an earlier step again: the duplicate row is kept
    b.sha3(message(33, 4), offset=900, call_id=2)
    b.sha3(b"", offset=BIG)                       # size 0: the offset, a pool word, is not looked at
    b.sha3(message(5, 1), pushed=0x1234)          # a pushed word below 2^64 travels in val: no digest is that small (site 7)
    b.plain(ES.EXP)
    return b.case()


def _single():
    b = Builder()
    b.sha3(message(70, 9))
    return b.case()


def _sites(gaps):
    b = Builder(gaps)
    good = message(100, 3)
    b.sha3(good)
    absent = ("no0", "no1", "no2") if gaps else ()
    for mut in absent + ("tag0", "tag1", "tag2", "id0", "id1", "id2", "addr0", "addr1", "addr2", "flip0", "flip1", "flip2"):
        b.sha3(message(3, 5), mut=(mut,))
        b.plain()
    # site 3: by the size, by the offset, by the sum, by a pool-word size (no byte op follows: the step is no message)
    b.sha3(b"", size=1 << 62)
    b.sha3(b"", size=1, offset=1 << 62)
    b.sha3(b"", size=2, offset=(1 << 62) - 2)
    b.sha3(b"", size=BIG)
    b.sha3(b"", size=0, offset=1 << 62)           # size 0: accepted, whatever the offset
    b.sha3(good, offset=(1 << 62) - 101)          # the largest accepted sum
    # sites 4-6 on byte 0, 63, 64 and the last
    for i in SITE_BYTES:
        for m in (("absent",) if gaps else ()) + ("write", "id", "addr", "tag", "256", "wide"):
            b.sha3(good, byte_mut={i: m})
        b.plain()
    # two sites in one step: the lowest k, the lowest byte index, a byte site in front of site 7
    if gaps:
        b.sha3(message(3, 5), mut=("no0", "tag1"))
    b.sha3(message(3, 5), mut=("tag1", "id0"))
    b.sha3(message(3, 5), mut=("flip2",), size=1 << 62)
    b.sha3(good, byte_mut={70: "256", 9: "write"})
    b.sha3(good, byte_mut={70: "256"}, pushed=5)
    # site 7: one flipped bit in each 64-bit limb of the pushed word
    digest = int.from_bytes(keccak256(good), "big")
    for limb in range(4):
        b.sha3(good, pushed=digest ^ (1 << (64 * limb + 5 + limb)))
    b.sha3(good)
    return b.case()


def _sites_dense_tail():
    """dense counters: the ops past the table's end are absent (site 4 on the last byte, then sites 1 of a step behind the table)"""
    b = Builder()
    b.sha3(message(40, 2))
    b.sha3(message(10, 6))
    b.rw.rows.pop()                               # the last byte's op
    b.steps.append([int(ES.SHA3), b.rw.rw_counter + 5, 1, 0, 1000, 10**6, 0, 0, 0, 0, 0, 0, 0])
    return b.case()


def _bytes_edges():
    b = Builder()
    for j, n in enumerate((63, 1, 1, 0, 190, 1, 1, 254, 0, 0, 1, 1, 300, 64, 64, 128)):
        b.sha3(message(n, 20 + j), offset=7 * j)
    return b.case()


def _ladder(n, pattern):
    b = Builder()
    edges = {0, 63, 64, 255, 256, n - 1}
    for s in range(n):
        if pattern == "all" or (pattern == "alt" and s % 2 == 0) or (pattern == "edges" and s in edges):
            b.sha3(message(s % 3, s), offset=s)
        else:
            b.plain()
    return b.case()


NAMES = ("lengths", "lengths_gaps", "single", "sites", "sites_dense", "sites_dense_tail", "bytes_edges") + tuple(
    f"ladder_{n}_{p}" for n in LADDER_SIZES for p in LADDER_PATTERNS)


@functools.lru_cache(maxsize=None)
def case(name):
    if name.startswith("ladder_"):
        _, n, p = name.split("_")
        return _ladder(int(n), p)
    return {"lengths": lambda: _lengths(False), "lengths_gaps": lambda: _lengths(True), "single": _single, "sites": lambda: _sites(True),
            "sites_dense": lambda: _sites(False), "sites_dense_tail": _sites_dense_tail, "bytes_edges": _bytes_edges}[name]()


@functools.lru_cache(maxsize=None)
def expected(name):
    """the model's result: computed once, shared by the tests, never written to"""
    c = case(name)
    out = ref.derive(c["trace"], c["randomness"])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


OUTPUTS = ("rows", "step", "data", "data_offsets")


def check_against(want, res, status, out, label=""):
    """a pass's Result, statuses and outputs against a model result, bit for bit"""
    assert np.array_equal(status, want["status"]), (label, np.nonzero(status != want["status"])[0][:8])
    for k in OUTPUTS:
        assert out[k].dtype == want[k].dtype and out[k].shape == want[k].shape and np.array_equal(out[k], want[k]), (label, k)
    first = want["first_fail"]
    assert (res.fail_count, res.first_fail_row, res.first_fail_code) == (want["fail_count"], first[0] if first else None, first[1] if first else 0), label
    assert res.rows_evaluated == len(want["status"]), label


def check_outputs(name, res, status, out):
    check_against(expected(name), res, status, out, name)
