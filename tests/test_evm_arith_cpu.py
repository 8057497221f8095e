"""Directed operands of the EVM arithmetic gadgets on the CPU (tests/evm_arith_cases.py, tests/golden/arith_cases.npz): the long
division behind MOD / SMOD / ADDMOD / MULMOD (csrc/fr.hpp zk_divmod_limbs) takes its rare paths — `cap`, the second reciprocal fix-up,
the second D3 correction, the D6 add-back, every word shift — only on operands that neither the reference's opcode tests nor uniform
random words provide.  The census conditions keep the directed set honest; the oracle, the kernels' gadget sources in a host loop
(hostsim, both index forms) and the CPU backend behind the C ABI must agree on every pair, and the kind of every labelled case is the
unmodified reference's."""
import json
import os
import subprocess
import sys

import pytest

from oracle import codes, wire
from tests import evm_arith_cases as ac
from tests.evm_cases import hostsim_status, load_cases, oracle_status

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def directed():
    return ac.directed_operands()


@pytest.fixture(scope="module")
def trace():
    return ac.directed_trace()


@pytest.fixture(scope="module")
def invalid(trace):
    return ac.invalid_variant(trace)


@pytest.fixture(scope="module")
def loaded(golden_dir):
    return ac.load(golden_dir)


def _table(title, counts_by_form, digits_by_form):
    lines = [title]
    names = ac.BRANCHES + tuple(f"ws{k}" for k in range(8)) + ("bs0", "bsnz")
    for f in sorted(counts_by_form):
        row = "  ".join(f"{nm} {counts_by_form[f].get(nm, 0)}" for nm in names)
        lines.append(f"  {32 * f}/256: {row}  add-back digits {sorted(digits_by_form[f])}")
    return "\n".join(lines)


def test_census_conditions_of_the_directed_set(directed, capsys):
    """caps on what the set may miss: per dividing opcode and per form of its divisions, every path in at least MIN_PER_PATH kept
    tuples; per form, the add-back on the lowest and the highest quotient digit it can fall on"""
    digits_all = {8: set(), 16: set()}
    for op in ac.DIVIDING:
        counts, digits = ac.census(directed[op])
        for w in ac._wanted(op):
            assert counts.get(w, 0) >= ac.MIN_PER_PATH, (op, w, counts.get(w, 0))
        for f in digits:
            digits_all[f] |= digits[f]
        by_form = {f: {nm: c for (ff, nm), c in counts.items() if ff == f} for f in (8, 16) if any(ff == f for ff, _ in counts)}
        with capsys.disabled():
            print("\n" + _table(f"{op}: {len(directed[op])} kept tuples", by_form, digits))
    for f, (lo, hi) in ac.ADDBACK_DIGIT_RANGE.items():
        assert min(digits_all[f]) == lo and max(digits_all[f]) == hi, (f, sorted(digits_all[f]))
    # every valid kept step really is one: the result is the division's, by Python's own operators
    for op in ac.DIVIDING:
        for t, _, _ in directed[op]:
            for n, d, nl in ac.divisions_of(op, t):
                assert n < 1 << (32 * nl) and 0 < d <= ac.M256


def _golden_operands(golden_dir):
    """(opcode, operand tuple) of every unfuzzed, passing golden step of the four dividing opcodes"""
    from zkevm_specs_amd import evm_tables as T

    state_ops = {int(T.ExecutionState[st]): ops for st, ops in T.RESPONSIBLE.items()}
    out = []
    for fn in sorted(set(ac.BASE_FILES.values())):
        for name, w, opts, _ in load_cases(os.path.join(golden_dir, fn)):
            if "#fuzz" in name or oracle_status(w, opts) != [0] * (w["steps"].shape[0] - 1):
                continue
            steps, rw, bc = (wire.rowmajor_to_rows(w[k]) for k in ("steps", "rw", "bytecode"))
            for s in steps[:-1]:
                byte = [r[5] for r in bc if (r[0], r[1], r[2], r[3]) == (s[5], s[6], 2, s[7])]
                names = [o for o in state_ops.get(s[0], ()) if byte and int(T.Opcode[o]) == byte[0]]
                if names and names[0] in ac.DIVIDING:
                    rows = [r for r in rw if s[1] <= r[0] < s[1] + 4 and r[2] == int(T.Target.Stack)]
                    vals = [r[8] + (r[9] << 128) for r in sorted(rows)]
                    out.append((names[0], tuple(vals[:-1])))
    return out


def test_census_of_the_golden_operands(golden_dir, capsys):
    """the "before" figure: what the reference's own opcode tests make the division do (recorded in DESIGN.md §4)"""
    counts, digits, n_div = {8: {}, 16: {}}, {8: set(), 16: set()}, 0
    operands = _golden_operands(golden_dir)
    for op, t in operands:
        names, dg = ac.tuple_paths(op, t)
        n_div += len(ac.divisions_of(op, t))
        for f in names:
            for nm in names[f]:
                counts[f][nm] = counts[f].get(nm, 0) + 1
            digits[f] |= dg[f]
    with capsys.disabled():
        print("\n" + _table(f"golden MOD / SMOD / ADDMOD / MULMOD steps: {len(operands)} steps, {n_div} divisions", counts, digits))
    assert {op for op, _ in operands} == set(ac.DIVIDING) and n_div >= 40


def test_file_is_data_only_small_and_the_search_of_today(golden_dir, loaded):
    """below four times tests/golden/checkpoint_cases.npz; one passing case per (opcode, tuple) of all_cases(), in that order"""
    assert os.path.getsize(ac.path(golden_dir)) < 4 * 64 * 1024
    bases, cases = loaded
    assert bases == ac.find_bases(golden_dir)
    valid = [(c.op, c.operands) for c in cases if c.pushed == ac.evm_result(c.op, c.operands)]
    assert valid == ac.all_cases()
    assert len(cases) - len(valid) >= len(valid) // 6


def test_labelled_cases_in_oracle_and_kernel_logic(golden_dir, loaded, hostsim):
    """status == the recorded code (0 for every valid step but ADDMOD's results >= p), its kind == the reference's; hostsim agrees in
    both index forms"""
    n = n_rejected = 0
    for k, c, w, opts in ac.iter_cases(golden_dir, loaded):
        exp = oracle_status(w, opts)
        where = (k, c)
        assert exp == [c.code] and codes.kind_of(c.code) == c.ref_kind, where
        if c.pushed == ac.evm_result(c.op, c.operands):
            if ac._valid_step(c.op, c.operands):
                assert c.code == 0, where
            else:
                assert c.code != 0 and c.ref_kind == codes.ASSERT, where
                n_rejected += 1
        assert hostsim_status(hostsim, w, opts) == exp, where
        assert hostsim_status(hostsim, w, opts, generic_index=True) == exp, where
        n += 1
    assert n == len(loaded[1]) >= 1000 and n_rejected >= 5


def test_placement_in_the_directed_trace(trace, directed):
    """every whole-wavefront run is one aligned wavefront of one opcode whose steps all take the run's path; every kept tuple that takes
    a rare path sits once between two steps that take none and once in such a run; the listed lanes carry targets"""
    n = len(trace.ops)
    assert n == ac.TRACE_STEPS and len(trace.runs) == len(ac.run_plan()) == 48
    in_run = set()
    for op, f, nm, lo, hi in trace.runs:
        assert lo % ac.WAVE == 0 and hi - lo == ac.WAVE
        for j in range(lo, hi):
            assert trace.ops[j] == op and (f, nm) in ac._rare_of(op, trace.tuples[j]), (op, f, nm, j)
            in_run.add((op, trace.tuples[j]))
    alone = set()
    for j, (op, names) in trace.singles.items():
        assert names and not ac._rare_of(trace.ops[j - 1], trace.tuples[j - 1]) and not ac._rare_of(trace.ops[j + 1], trace.tuples[j + 1]), j
        alone.add((op, trace.tuples[j]))
    for op in ac.DIVIDING:
        for t, names, _ in directed[op]:
            if any(nm in ac.RARE for f in names for nm in names[f]):
                assert (op, t) in alone and (op, t) in in_run, (op, t)
    placed = {(op, t) for op, t in zip(trace.ops, trace.tuples)} | {("ADDMOD", t) for t in trace.rejected.values()}
    assert set(ac.all_cases()) <= placed
    # step 255 of this trace is the STOP that ends the first segment: the last arithmetic lane of that wavefront is 254
    assert trace.ops[255] == "STOP"
    for j in (0, 63, 64, 254, 256, n - 2):
        assert ac._rare_of(trace.ops[j], trace.tuples[j]), j


def test_directed_trace_in_oracle_and_kernel_logic(trace, invalid, hostsim):
    """the valid trace passes everywhere; the invalid variant has the oracle's status on every pair, with both index forms"""
    exp = oracle_status(trace.wire)
    assert exp == [0] * (len(trace.ops) - 1)
    w, changed = invalid
    exp_bad = oracle_status(w)
    assert len(changed) >= len(trace.ops) // 4 and all(exp_bad[j] == 0 for j in range(len(exp_bad)) if j not in changed)
    assert all(exp_bad[j] for j in trace.rejected)
    n_fail = sum(1 for c in exp_bad if c)
    assert n_fail >= len(changed) * 9 // 10  # a few wrong words are accepted (a zero divisor leaves the other result free)
    for wd, e in ((trace.wire, exp), (w, exp_bad)):
        for generic in (False, True):
            got = hostsim_status(hostsim, wd, generic_index=generic)
            bad = [(j, trace.ops[j], trace.tuples[j], hex(got[j]), hex(e[j])) for j in range(len(e)) if got[j] != e[j]]
            assert not bad, (generic, bad[:5])


CHILD = r'''
import json, os, sys
sys.path.insert(0, os.environ["ZK_ROOT"])
from zkevm_specs_amd import _lib, oneshot
assert _lib.BACKEND == "cpu" and _lib.LIB_PATH.endswith("libzkevm_cpu.so")
from tests import evm_arith_cases as ac
from tests.evm_cases import oracle_status
tr = ac.directed_trace()
n = 0
for w in (tr.wire, ac.invalid_variant(tr)[0]):
    res, st = oneshot.evm_verify(w)
    exp = oracle_status(w)
    bad = [(j, tr.ops[j], tr.tuples[j], st[j], exp[j]) for j in range(len(exp)) if st[j] != exp[j]]
    assert not bad, bad[:5]
    fails = [j for j, e in enumerate(exp) if e]
    assert res.fail_count == len(fails) and (not fails or (res.first_fail_row == fails[0] and res.first_fail_code == exp[fails[0]]))
    n += 1
m = 0
for k, c, w, opts in ac.iter_cases(os.path.join(os.environ["ZK_ROOT"], "tests", "golden")):
    res, st = oneshot.evm_verify(w, bool(opts[0]), bool(opts[1]))
    assert st.tolist() == [c.code], (k, c, st.tolist())
    m += 1
print("RESULT " + json.dumps({"traces": n, "cases": m}))
'''


def test_through_the_cpu_backend(tmp_path, loaded):
    """libzkevm_cpu.so through zk_evm_verify (a child process: the backend is chosen at import), as tests/test_evm_checkpoints_cpu.py"""
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
    assert json.loads(line[0][7:]) == {"traces": 2, "cases": len(loaded[1])}
