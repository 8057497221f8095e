"""Directed checkpoint cases of the EVM circuit on the CPU (tests/golden/checkpoint_cases.npz, tests/checkpoint_cases.py): every case
makes one checkpoint of csrc/evm_circuit.hpp the first one to fail.  The oracle, the kernels' gadget sources in a host loop (hostsim,
both index forms) and the CPU backend behind the C ABI must all return the recorded code, whose kind is the unmodified reference's; the
coverage condition keeps the file honest about which checkpoints of its bases no case reaches."""
import json
import os
import subprocess
import sys

import pytest

from oracle import codes, evm_oracle as eo
from tests import checkpoint_cases as cc
from tests.evm_cases import golden_files, hostsim_status, load_cases, oracle_status

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_UNREACHED_SHARE = 0.20  # of the failable checkpoints of all bases: a cap on what the search may leave, not a target


@pytest.fixture(scope="module")
def loaded(golden_dir):
    return cc.load(golden_dir)


def test_file_is_data_only_and_small(golden_dir, loaded):
    assert os.path.getsize(cc.path(golden_dir)) < 1 << 20
    bases, cases, meta = loaded
    assert len(bases) >= 75 and len(cases) >= 2000
    assert int(meta["seed"]) > 0 and len(json.loads(str(meta["moves"]))) >= 4 and len(json.loads(str(meta["values"]))) >= 14


def test_every_case_fails_at_its_checkpoint_in_oracle_and_kernel_logic(golden_dir, loaded, hostsim):
    """every pair of the patched witness, not only the patched one: oracle == hostsim (both index forms), and the patched pair has the
    recorded code"""
    n = 0
    for k, c, b, name, w, opts in cc.iter_cases(golden_dir, loaded):
        exp = oracle_status(w, opts)
        where = (k, b.file, name, b.pair, c.patches)
        assert exp[b.pair] == c.code and c.code != 0, where
        assert hostsim_status(hostsim, w, opts) == exp, where
        assert hostsim_status(hostsim, w, opts, generic_index=True) == exp, where
        n += 1
    assert n == len(loaded[1])


def test_kind_of_every_case_is_the_references(loaded):
    """codes.kind_of(status) == ref_kind, the exception class of the unmodified reference on that pair, for every case (the recorded
    code is the oracle's, hostsim's and the CPU backend's by the tests around this one)"""
    bases, cases, _ = loaded
    wrong = [(k, bases[c.base].file, bases[c.base].case, bases[c.base].pair, hex(c.code), c.ref_kind, c.patches)
             for k, c in enumerate(cases) if codes.kind_of(c.code) != c.ref_kind]
    assert not wrong, wrong


CHILD = r'''
import json, os, sys
sys.path.insert(0, os.environ["ZK_ROOT"])
from zkevm_specs_amd import _lib, oneshot
assert _lib.BACKEND == "cpu" and _lib.LIB_PATH.endswith("libzkevm_cpu.so")
from tests import checkpoint_cases as cc
from tests.evm_cases import oracle_status
n = 0
for k, c, b, name, w, opts in cc.iter_cases(os.path.join(os.environ["ZK_ROOT"], "tests", "golden")):
    res, st = oneshot.evm_verify(w, bool(opts[0]), bool(opts[1]))
    exp = oracle_status(w, opts)
    assert st.tolist() == exp and exp[b.pair] == c.code, (k, b.file, name, b.pair, c.patches, st.tolist(), exp)
    fails = [j for j, e in enumerate(exp) if e]
    assert res.fail_count == len(fails) and res.first_fail_row == fails[0] and res.first_fail_code == exp[fails[0]], (k, name)
    n += 1
print("RESULT " + json.dumps({"cases": n}))
'''


def test_every_case_through_the_cpu_backend(tmp_path, loaded):
    """libzkevm_cpu.so through zk_evm_verify, the entry tests/test_cpu_backend.py uses (a child process: the backend is chosen at import)"""
    so = os.path.join(ROOT, "zkevm_specs_amd", "libzkevm_cpu.so")
    if not os.path.exists(so):
        import __graft_entry__

        __graft_entry__.build()
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    env = dict(os.environ, ZK_BACKEND="cpu", ZK_ROOT=ROOT, OMP_NUM_THREADS="4")
    p = subprocess.run([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1800)
    assert p.returncode == 0, p.stderr.decode()[-4000:]
    line = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("RESULT ")]
    assert json.loads(line[0][7:])["cases"] == len(loaded[1])


@pytest.fixture(scope="module")
def base_pairs(golden_dir, loaded):
    """per base: (golden case name, is the pair the first / the last of its block, its traced oracle evaluation)"""
    bases = loaded[0]
    out = [None] * len(bases)
    by_file = {}
    for k, b in enumerate(bases):
        by_file.setdefault(b.file, []).append(k)
    for f, ks in by_file.items():
        gold = list(load_cases(os.path.join(golden_dir, f)))
        for k in ks:
            name, w, opts, _ = gold[bases[k].case]
            first, last = cc.pair_flags(opts, w["steps"].shape[0], bases[k].pair)
            out[k] = (name, first, last, int(w["steps"][bases[k].pair, 0, 0]), cc.traced_status(w, opts)[bases[k].pair])
    return out


def test_bases_are_passing_pairs_with_the_recorded_path(loaded, base_pairs):
    """a base is a passing, unfuzzed pair; its passing count and the checkpoints it reaches through require() are what the file says
    (the failable set may only add ordinals that a committed case fails at)"""
    bases, cases, _ = loaded
    census = cc.base_census(bases, cases)
    per_state = {}
    for k, b in enumerate(bases):
        name, _, _, state, (c, count, required) = base_pairs[k]
        assert "#fuzz" not in name
        assert c == 0 and count == b.count and state == b.state, (b.file, name)
        failable, reached, _ = census[k]
        assert set(required) <= failable and failable - set(required) <= reached, (b.file, name)
        assert all(1 <= s <= b.count for s in failable), (b.file, name)
        per_state.setdefault(b.state, []).append(b.count)
    for st, counts in per_state.items():  # distinct passing counts, longest first, at most four
        assert counts == sorted(set(counts), reverse=True) and len(counts) <= 4, cc.state_name(st)


def test_coverage_condition(golden_dir, loaded, base_pairs, capsys):
    """Every failable checkpoint 1..L of every base is the failing site of a committed case or is listed as unreached, with the number
    of candidates that were tried; the unreached share over all bases stays under the cap; every supported state with a passing golden
    pair has a base; a bad state transition (checkpoint 1) is reached for every base whose pair is not the last one."""
    bases, cases, _ = loaded
    census = cc.base_census(bases, cases)
    per_state = {}
    n_failable = n_unreached = 0
    for b, (failable, reached, unreached) in zip(bases, census):
        assert failable == reached | unreached and not (reached & unreached), (b.file, b.case, b.pair)
        assert all(t > 0 for t in b.tried), (b.file, b.case)
        n_failable += len(failable)
        n_unreached += len(unreached)
        row = per_state.setdefault(b.state, [0, 0, 0, 0])
        row[0] += 1
        row[1] += len(failable)
        row[2] += len(reached)
        row[3] += len(unreached)
    with capsys.disabled():
        print("\nstate                                    bases failable reached unreached")
        for st in sorted(per_state):
            print(f"{cc.state_name(st):40s} {per_state[st][0]:5d} {per_state[st][1]:8d} {per_state[st][2]:7d} {per_state[st][3]:9d}")
        print(f"{'all':40s} {len(bases):5d} {n_failable:8d} {n_failable - n_unreached:7d} {n_unreached:9d}  ({100.0 * n_unreached / n_failable:.1f} % unreached)")
    assert n_unreached <= MAX_UNREACHED_SHARE * n_failable
    # every supported state that has a passing pair in the goldens has a base
    passing = set()
    for fn in golden_files(golden_dir):
        for _, w, opts, _ in load_cases(fn):
            for st, c in zip(w["steps"][:-1, 0, 0].tolist(), oracle_status(w, opts)):
                if c == 0:
                    passing.add(int(st))
    assert passing & set(eo.SUPPORTED_STATES) <= {b.state for b in bases}
    # a bad state transition is reached for every base whose pair is not the last one of its block: checkpoint 1, or 3 behind the two
    # checks of a block's first pair (verify_step)
    for k, b in enumerate(bases):
        _, first, last, _, _ = base_pairs[k]
        if not last:
            assert (3 if first else 1) in census[k][1], (b.file, b.case, b.pair)


def test_non_enum_execution_states_have_one_verdict(golden_dir, loaded):
    """An execution_state cell that is no ExecutionState member — 0, one above the last member, 2^64, P - 1 — as curr with next =
    EndTx / BeginTx / EndBlock / an ordinary state, and as next: VALUE_ERROR before every checkpoint (oracle/evm_oracle.py
    verify_step), the class the reference's enum constructor raises.  The cases are in the file (so hostsim, the CPU backend and the
    device see them); this counts them."""
    bases, cases, _ = loaded
    last = max(int(s) for s in eo.ES)
    seen = set()
    for c in cases:
        b = bases[c.base]
        cells = {(row - b.pair, cell): v for t, row, cell, v in c.patches if t == "steps"}
        bad = cells.get((0, 0))
        if bad is not None and bad not in eo._STATE_VALUES:
            assert c.code == codes.code(codes.VALUE_ERROR, 0) and c.ref_kind == codes.VALUE_ERROR
            seen.add((bad, cells.get((1, 0), "kept")))
        if cells.get((1, 0)) is not None and cells[(1, 0)] not in eo._STATE_VALUES:
            assert c.code == codes.code(codes.VALUE_ERROR, 0) and c.ref_kind == codes.VALUE_ERROR
            seen.add(("next", cells[(1, 0)]))
    for bad in (0, last + 1, 1 << 64, eo.P - 1):
        assert ("next", bad) in seen
        nexts = {n for v, n in seen if v == bad}
        assert {int(eo.ES.EndTx), int(eo.ES.BeginTx), int(eo.ES.EndBlock)} <= nexts | {"kept"} and len(nexts) >= 4, (bad, nexts)


def test_state_transition_rule_is_total():
    """_state_transition_ok used to raise ValueError (the enum constructor, through evm_tables.halts) for a curr that is no
    ExecutionState when next is EndTx: it is a total function of two integers now"""
    E = eo.ES
    last = max(int(s) for s in E)
    for bad in (0, last + 1, 1 << 64, eo.P - 1):
        assert eo._state_transition_ok(bad, int(E.EndTx)) is False      # halts nothing, is not BeginTx
        assert eo._state_transition_ok(bad, int(E.BeginTx)) is False    # only EndTx precedes BeginTx
        assert eo._state_transition_ok(bad, int(E.EndBlock)) is False
        assert eo._state_transition_ok(bad, int(E.ADD)) is True         # no rule names the pair
        assert eo._state_transition_ok(int(E.EndTx), bad) is False      # EndTx is followed by BeginTx or EndBlock only
        assert eo._state_transition_ok(int(E.EndBlock), bad) is False
        assert eo._state_transition_ok(int(E.ADD), bad) is True
    assert eo._state_transition_ok(int(E.STOP), int(E.EndTx)) and not eo._state_transition_ok(int(E.ADD), int(E.EndTx))
    # and verify_step gives such a pair its verdict without asking the rule
    from tests.evm_cases import to_witness
    import numpy as np

    steps = np.zeros((2, 13, 4), dtype=np.uint64)
    steps[1, 0, 0] = int(E.EndTx)
    w = {"steps": steps, "rw": np.zeros((0, 14, 4), dtype=np.uint64), "rw_flags": np.zeros(0, dtype=np.uint32),
         "bytecode": np.zeros((0, 6, 4), dtype=np.uint64), "tx": np.zeros((0, 5, 4), dtype=np.uint64), "tx_flags": np.zeros(0, dtype=np.uint32),
         "block": np.zeros((0, 4, 4), dtype=np.uint64), "block_flags": np.zeros(0, dtype=np.uint32)}
    assert eo.verify_steps(to_witness(w)) == [codes.code(codes.VALUE_ERROR, 0)]


def test_census_of_the_corpus_with_and_without_the_checkpoint_cases(golden_dir, capsys):
    """the accounting the file was made for: checkpoints on the accepted paths (per state, the longest passing count) that are the failing
    site of some case — the golden corpus alone, and with the checkpoint cases"""
    cen = cc.census(golden_dir)
    path = sum(v["path"] for v in cen.values())
    before = sum(len(v["corpus"]) for v in cen.values())
    after = sum(len(v["all"]) for v in cen.values())
    with capsys.disabled():
        print("\nstate                                     path corpus  with checkpoint cases")
        for st in sorted(cen):
            print(f"{cc.state_name(st):40s} {cen[st]['path']:5d} {len(cen[st]['corpus']):6d} {len(cen[st]['all']):6d}")
        print(f"{'all':40s} {path:5d} {before:6d} {after:6d}")
    assert len(cen) >= 75 and path >= 4500 and before >= 900  # the corpus as it was counted when the cases were made
    assert all(v["corpus"] <= v["all"] for v in cen.values()) and after > 2 * before


def test_equal_rw_rows_count_once_under_the_last_end_block(golden_dir, hostsim):
    """the reference's rw_table is a set: a wire table with a repeated row has len(rw_table) = rows - 1, and the last EndBlock's
    rw_table_start_lookup(max_rws - total_rws - total_withdrawals) is taken from that.  The two witnesses pass in the reference; the
    oracle and the kernels' logic (host-side duplicate count) must accept them too, and the row must really be repeated"""
    n = 0
    for w, opts, pair in cc.duplicate_rw_row_witnesses(golden_dir):
        rows = [r.tobytes() for r in w["rw"]]
        assert len(set(rows)) == len(rows) - 1
        exp = oracle_status(w, opts)
        assert exp[pair] == 0
        assert hostsim_status(hostsim, w, opts) == exp and hostsim_status(hostsim, w, opts, generic_index=True) == exp
        n += 1
    assert n == 2
