"""RW table -> State-circuit verdict without the witness in between (include/zkevm_hip.h zk_state_verify_from_rw*; csrc/state_fused.hpp):
the rows are evaluated in the registers that op2row computes them in.  Checked two ways: against the INDEPENDENT composition of the three
checkers — oracle/rw_state_oracle.py (re-keying + sort), oracle/assign_oracle.py (assign_state_circuit + mock MPT), oracle/state_oracle.py
(check_state_row) — status per row, and against the library's own two-step form (zk_state_assign_from_rw_open, then zk_state_open on what
it wrote) at sizes the Python checkers do not reach.  CPU suite: libzkevm_cpu.so; GPU suite: the HIP path."""
import random

import numpy as np
import pytest

from oracle import assign_oracle, rw_state_oracle, state_oracle, wire
from tests.test_state_rekey import _valid_block_rw, rand_rw_table
from zkevm_specs_amd import engine, oneshot
from zkevm_specs_amd._lib import EngineError
from zkevm_specs_amd.wire import rows_to_rowmajor


def oracle_statuses(rows, flags):
    """check_state_row over assign_state_circuit over the re-keyed, sorted ops — the three checkers back to back"""
    ops, op_flags, _ = rw_state_oracle.rw_to_state_ops(rows, flags, strict=True)
    st_rows, row_flags, mpt, status = assign_oracle.assign(ops, op_flags)
    assert not any(status)
    return state_oracle.verify_rows(st_rows, row_flags, mpt)


def tamper_rw(rows, rng, k):
    """damage k cells of RW rows in ways that keep the table assignable: values, counters, the read / write bit, ids"""
    rows = [list(r) for r in rows]
    for _ in range(k):
        i = rng.randrange(len(rows))
        c = rng.choice([0, 0, 1, 3, 8, 8, 9, 12])
        if c == 1:
            rows[i][1] ^= 1
        elif c == 0:
            rows[i][0] = max(0, rows[i][0] + rng.choice([-1, 1, 7]))
        elif c == 3:
            rows[i][3] = (rows[i][3] + 1) % (1 << 20)
        else:
            rows[i][c] ^= 1 << rng.randrange(0, 100)
    return rows


def fused(rows, flags, device):
    return fused_arrays(rows_to_rowmajor(rows, 14), np.array(flags, dtype=np.uint32), device)


def fused_arrays(rw, fl, device):
    with engine.open_state_verify_from_rw(rw, fl, device=device) as s:
        r = s.run()
        st = s.read_status()
        assert r.rows_evaluated == s.n == len(st)
        for _ in range(2):  # resident passes: the session keeps the sorted order / root ranks, the HIP library launches the evaluation kernel alone
            rb = s.run()
            assert (rb.fail_count, rb.first_fail_row, rb.first_fail_code) == (r.fail_count, r.first_fail_row, r.first_fail_code)
            assert np.array_equal(s.read_status(), st)
    r1, st1 = oneshot.state_verify_from_rw(rw, fl, device=device)
    assert np.array_equal(st, st1) and (r1.fail_count, r1.first_fail_row, r1.first_fail_code) == (r.fail_count, r.first_fail_row, r.first_fail_code)
    return r, st


def two_steps(rows, flags, device):
    return two_steps_arrays(rows_to_rowmajor(rows, 14), np.array(flags, dtype=np.uint32), device)


def two_steps_arrays(rw, fl, device):
    with engine.open_state_assign_from_rw(rw, fl, device=device) as a:
        assert a.run().ok
        full, rf, mpt = a.read()
    with engine.open_state(full, rf, mpt, device=device) as s:
        r = s.run()
        return r, s.read_status()


def check_case(rows, flags, device, with_oracle=True):
    r, st = fused(rows, flags, device)
    r2, st2 = two_steps(rows, flags, device)
    assert np.array_equal(st, st2), [(j, hex(st[j]), hex(st2[j])) for j in np.nonzero(st != st2)[0][:5]]
    assert (r.fail_count, r.first_fail_row, r.first_fail_code) == (r2.fail_count, r2.first_fail_row, r2.first_fail_code)
    if with_oracle:
        want = oracle_statuses(rows, flags)
        assert st.tolist() == want, [(j, hex(st[j]), hex(want[j])) for j in range(len(want)) if st[j] != want[j]][:5]
    return int(r.fail_count)


def run_suite(device, sizes, block_steps):
    rng = random.Random(1234 + len(sizes))
    for n in sizes:  # random tables: no valid State witnesses — equal verdicts row by row, not clean ones
        rows, flags = rand_rw_table(rng, n, 0.0, 0.0)
        assert check_case(rows, flags, device) > 0 or n < 3
    rows, flags = _valid_block_rw(block_steps)  # a consistent trace: the derived witness satisfies the State circuit
    assert check_case(rows, flags, device) == 0
    bad = tamper_rw(rows, rng, max(5, len(rows) // 40))
    assert check_case(bad, flags, device) >= 3
    # no witness: an RW row the re-keying rejects, an address op2row cannot turn into 20 bytes, a first-access value >= 2^256
    for j, c, v in ((len(rows) // 2, 2, 99), (None, 4, 1 << 200), (None, 9, 1 << 130)):
        hurt = [list(r) for r in rows]
        for i in [j] if j is not None else [i for i, r in enumerate(hurt) if r[2] == 6][: 1 if c == 4 else None]:  # (Storage rows)
            hurt[i][c] = v
        with pytest.raises(EngineError, match="State witness assignment|rejects"):
            fused(hurt, flags, device)


def test_cpu_backend_fused_state_verify():
    run_suite("cpu", (1, 2, 63, 64, 65, 700), 300)


@pytest.mark.gpu
def test_gpu_fused_state_verify():
    run_suite(None, (1, 2, 62, 63, 64, 65, 127, 1000, 4097), 1500)


@pytest.mark.gpu
def test_gpu_fused_state_verify_full_block():
    """the 2^18-step block's RW table (694,917 rows): clean, and with 2,000 damaged cells, fused == two steps row by row"""
    from zkevm_specs_amd.synth_block import synth_block_trace

    w = synth_block_trace(1 << 18, seed=7)
    rows, flags = wire.rowmajor_to_rows(w["rw"]), w["rw_flags"].tolist()
    assert check_case(rows, flags, None, with_oracle=False) == 0
    bad = tamper_rw(rows, random.Random(5), 2000)
    assert check_case(bad, flags, None, with_oracle=False) >= 1000


def fused_equals_two_steps_directed(n, device, tamper):
    """the directed consumer table (tests/rekey_cases.py: ten tiles of the fast sort at 73,729 rows, 30 % repeated keys, dropped rows): the
    fused verdict's per-row statuses, over the first pass and two resident ones, against the two-step path; `tamper` value cells damaged"""
    from tests import rekey_cases as rc

    rw, fl = rc.consumer_table(n)
    rng = np.random.default_rng(n + tamper)
    for i in rng.integers(0, n, tamper):
        rw[i, 8, 0] ^= np.uint64(1) << np.uint64(rng.integers(0, 60))
    r, st = fused_arrays(rw, fl, device)
    r2, st2 = two_steps_arrays(rw, fl, device)
    assert np.array_equal(st, st2), [(j, hex(st[j]), hex(st2[j])) for j in np.nonzero(st != st2)[0][:5]]
    assert (r.fail_count, r.first_fail_row, r.first_fail_code) == (r2.fail_count, r2.first_fail_row, r2.first_fail_code)
    assert r.fail_count > 0  # (no valid State witness: equal verdicts row by row, not clean ones)


def test_cpu_backend_fused_directed_table():
    fused_equals_two_steps_directed(20000, "cpu", 60)


@pytest.mark.gpu
@pytest.mark.parametrize("tamper", [0, 200])
def test_gpu_fused_directed_table_73729(tamper):
    fused_equals_two_steps_directed(73729, None, tamper)


@pytest.mark.gpu
def test_gpu_fused_state_verify_fuzz():
    rng = random.Random(77)
    for _ in range(60):
        n = rng.choice([3, 17, 64, 200, 511, 1300])
        rows, flags = rand_rw_table(rng, n, 0.0, 0.0, dup=rng.choice([0.0, 0.3, 0.8]))
        check_case(rows, flags, None, with_oracle=n <= 200)


# ---- Directed RW-level cases: one RW row of a consistent trace damaged at a time (value, previous value, is_write, counter, id, address /
# field tag, committed value, rw_flags), on the first and the last access of a key group of every State tag; for Storage and Account the
# damaged row is also moved — by Stack rows that sort in front of it, or by dropping what sorts behind it — to the first evaluated lane of
# a 63-row wavefront, to its last lane, and to row n - 1 of the sorted State rows.  Each case: fused == two steps == the three checkers.
A_ACC, A_STO = 0x1234567890ABCDEF1234567890ABCDEF12345678, 0xFEDCBA9876543210FEDCBA9876543210FEDCBA98
DIRECTED_TAGS = (2, 3, 4, 5, 6, 7, 8, 9, 10, 11)
PLACED_TAGS = (4, 6)
# State sites the directed RW cases make a failing site of some row, per State tag of the damaged row: measured with the three checkers
# (oracle_statuses), not with the library.  Decomposition checks (4..7, 9) cannot fail on this path — op2row derives limbs and bytes —
# and a damaged row is re-sorted, so many per-tag "unused key is zero" checks are out of reach as well.
FUSED_REACHED = {
    2: [11, 13, 40, 42, 44, 45, 47, 48],
    3: [11, 13, 60, 62, 64],
    4: [10, 11, 12, 13, 70, 71],
    5: [11, 13, 83, 84],
    6: [11, 12, 13, 93, 94, 95],
    7: [13, 100, 101],
    8: [11, 13, 110, 112, 115, 116],
    9: [13, 120, 121, 125],
    10: [13, 130, 132],
    11: [11, 13, 140, 142, 144, 145, 148, 150],
}


def directed_rw_base():
    """the 150-step block's RW table plus accesses the block generator does not make: Storage and Account key groups with several
    accesses (the last access carries the first's value: the mock MPT updates are made from a key's first op), TxAccessListAccount,
    TxLog and TxReceipt rows"""
    rows, flags = _valid_block_rw(150)
    rows, flags = [list(r) for r in rows], list(flags)
    c = max(r[0] for r in rows)

    def add(target, id_, addr, ft, key, is_write, value, committed=0, word=0):
        nonlocal c
        c += 1
        rows.append([c, is_write, target, id_, addr, ft, key & ((1 << 128) - 1), key >> 128, value & ((1 << 128) - 1), value >> 128, 0, 0,
                     committed & ((1 << 128) - 1), committed >> 128])
        flags.append(word)

    add(9, 9000, 64, 0, 0, 0, 0), add(9, 9000, 64, 0, 0, 1, 42), add(9, 9000, 64, 0, 0, 0, 42)  # Memory: read 0, write, read back
    for key in (0x99, (7 << 128) | 5):
        v = (1 << 130) + key % 1000
        add(6, 1, A_STO, 0, key, 1, v, 55, 1), add(6, 1, A_STO, 0, key, 1, 5, 55, 1), add(6, 1, A_STO, 0, key, 1, v, 55, 1), add(6, 1, A_STO, 0, key, 0, v, 55, 1)
    for addr in (A_ACC, 0x77):
        add(5, 0, addr, 1, 0, 1, 1, 0, 0), add(5, 0, addr, 1, 0, 0, 1, 0, 0)
        add(5, 0, addr, 2, 0, 1, (1 << 128) + 3, 1 << 64, 1), add(5, 0, addr, 2, 0, 1, 9, 1 << 64, 1), add(5, 0, addr, 2, 0, 1, (1 << 128) + 3, 1 << 64, 1)
        h = (1 << 250) + addr % 1000  # (an existing code hash: the mock MPT updates have no non-existing proof for a 0 -> 0 leaf)
        add(5, 0, addr, 3, 0, 0, h, h, 1), add(5, 0, addr, 3, 0, 0, h, h, 1)
    for tx in (1, 2):
        add(2, tx, A_ACC, 0, 0, 0, 0), add(2, tx, A_ACC, 0, 0, 1, 1), add(2, tx, A_ACC, 0, 0, 0, 1)
        for log in (1, 2):
            add(10, tx, (log << 48) | (0 << 32), 0, 0, 1, 124), add(10, tx, (log << 48) | (2 << 32) | 1, 0, 0, 1, (1 << 255) + 7, 0, 1), add(10, tx, (log << 48) | (3 << 32), 0, 0, 1, 10)
    gas = 0
    for tx in (1, 2, 3):
        if tx != 2:
            add(11, tx, 0, 1, 0, 0, 1)
        gas += 21000
        add(11, tx, 0, 2, 0, 0, gas)
    return rows, flags


def _state_keys(rows, flags):
    """[(State key tuple with rw_counter, RW row index)] of the rows that become State ops, in the State circuit's order"""
    out = []
    for i, (r, f) in enumerate(zip(rows, flags)):
        op = rw_state_oracle.rekey_row(r, int(f))
        if op is not None:
            o = op[0]
            out.append(((o[2], o[3], o[4], o[5], o[6], o[0]), i))
    return sorted(out)


def _damages(r, f):
    """(name, row, flags, moves) — `moves`: the damage changes a key cell or the counter, so the row sorts elsewhere"""
    def w(j, v):
        x = list(r)
        x[j] = v
        return x
    yield "value+1", w(8, r[8] + 1), f, False
    yield "value=256", w(8, 256), f, False
    yield "value hi", w(9, r[9] ^ (1 << 64)), f, False
    yield "previous value", w(10, r[10] + 1), f, False
    yield "is_write", w(1, r[1] ^ 1), f, False
    yield "committed+1", w(12, r[12] + 1), f, False
    yield "committed hi", w(13, r[13] ^ (1 << 64)), f, False
    yield "value is_word", r, f ^ 1, False
    yield "previous is_word", r, f ^ 2, False
    yield "counter=0", w(0, 0), f, True
    yield "id+1", w(3, r[3] + 1), f, True
    yield "id=0", w(3, 0), f, True
    yield "field tag+1", w(5, r[5] + 1), f, True
    yield "field tag=5", w(5, 5), f, True
    yield "address+1", w(4, r[4] + 1), f, True


def _placed(rows, flags, i, want):
    """the table with RW row i's State row moved: want = 0 / 62: Stack writes of call id 0 (they sort behind the Memory rows and in front of
    everything else) until its State row index is want modulo 63; want = "last": every row that sorts behind its key group dropped"""
    keys = _state_keys(rows, flags)
    pos = 1 + [j for _, j in keys].index(i)  # (the Start row is State row 0)
    if want == "last":
        mine = keys[pos - 1][0][:5]
        keep = {j for k, j in keys if k[:5] <= mine}
        assert keys[pos - 1][0] == max(k for k, j in keys if j in keep)  # the last access of the last group
        out = [(rows[j], flags[j]) for j in range(len(rows)) if j in keep]
        return [r for r, _ in out], [f for _, f in out], len(out)
    assert rows[i][2] not in (9, 8) and not any(r[2] == 8 and r[3] == 0 for r in rows)
    k = (want - pos) % 63
    c = max(r[0] for r in rows)
    pad = [[c + 1 + j, 1, 8, 0, 1023, 0, 0, 0, 7, 0, 0, 0, 0, 0] for j in range(k)]
    return rows + pad, flags + [1] * k, pos + k


def directed_variants(tag):
    """(damaged RW rows, flags) of every directed case of one State tag, placements included"""
    rows, flags = directed_rw_base()
    groups = {}
    for k, i in _state_keys(rows, flags):
        if k[0] == tag:
            groups.setdefault(k[:5], []).append(i)
    multi = [g for g in groups.values() if len(g) > 1]
    single = [g for g in groups.values() if len(g) == 1]
    # the first and the last access of a key group with several, and up to two rows that are their group's only access
    targets = ([multi[0][0], multi[0][-1]] if multi else []) + [g[0] for g in single[:2]]
    assert len(targets) >= 2, tag
    for i in targets:
        for name, r, f, moves in _damages(rows[i], flags[i]):
            hurt, hf = [list(x) for x in rows], list(flags)
            hurt[i], hf[i] = r, f
            yield hurt, hf
            if tag in PLACED_TAGS and not moves and multi and i in (multi[0][0], multi[0][-1]):
                for want in (0, 62):
                    pr, pf, pos = _placed(hurt, hf, i, want)
                    assert pos % 63 == want and [j for _, j in _state_keys(pr, pf)].index(i) + 1 == pos
                    yield pr, pf
                if i == multi[0][-1]:  # the last access: its next row is row 0 through the wrap-around
                    pr, pf, m = _placed(hurt, hf, i, "last")
                    assert len(_state_keys(pr, pf)) == m
                    yield pr, pf


def directed_census(tag, device=None, run=False):
    """State sites the cases of one tag make a failing site, by the three checkers; with `run`, each case also goes through check_case"""
    sites, n, refused = set(), 0, 0
    for vr, vf in directed_variants(tag):
        ops, op_flags, _ = rw_state_oracle.rw_to_state_ops(vr, vf, strict=True)
        if any(assign_oracle.assign(ops, op_flags)[3]):  # no witness (an Account field tag op2row has no proof type for): refused
            if run:
                with pytest.raises(EngineError, match="State witness assignment"):
                    fused(vr, vf, device)
            refused += 1
            continue
        if run:
            check_case(vr, vf, device)
        sites |= {c & 0xFFFFFF for c in oracle_statuses(vr, vf) if c}
        n += 1
    assert n >= 2 * 13 and refused <= 4, (n, refused)
    return sorted(sites)


def run_directed(device, tag):
    assert directed_census(tag, device, run=True) == FUSED_REACHED[tag]


@pytest.mark.parametrize("tag", DIRECTED_TAGS)
def test_cpu_backend_fused_directed_rw_cases(tag):
    run_directed("cpu", tag)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", DIRECTED_TAGS)
def test_gpu_fused_directed_rw_cases(tag):
    run_directed(None, tag)


def test_directed_rw_base_is_a_valid_witness():
    rows, flags = directed_rw_base()
    assert not any(oracle_statuses(rows, flags))
    assert {k[0] for k, _ in _state_keys(rows, flags)} == set(DIRECTED_TAGS)
