"""Directed operands of the EVM arithmetic gadgets on the device (tests/evm_arith_cases.py, tests/golden/arith_cases.npz).  The
long division behind MOD / SMOD / ADDMOD / MULMOD runs on the MI355X only inside the EVM kernels; here it runs on operands that take
`cap`, the second reciprocal fix-up, the second D3 correction, the D6 add-back and every word shift, one lane at a time among ordinary
lanes and a whole wavefront at a time, in one 4,096-step trace (64 wavefronts of the hot kernel) and in tiny labelled sessions."""
import pytest

from oracle import codes
from tests import evm_arith_cases as ac
from tests.evm_cases import oracle_status
from zkevm_specs_amd import engine

pytestmark = pytest.mark.gpu

ENTRIES = ("state-sorted", "trace order", "generic index", "one-shot")
N_SLICES = 2


@pytest.fixture(scope="module")
def trace():
    return ac.directed_trace()


@pytest.fixture(scope="module")
def invalid(trace):
    w, changed = ac.invalid_variant(trace)
    return w, changed, oracle_status(w)


@pytest.fixture(scope="module")
def loaded(golden_dir):
    return ac.load(golden_dir)


def _run(w, entry, opts=(0, 0)):
    if entry == "one-shot":
        from zkevm_specs_amd import oneshot

        res, st = oneshot.evm_verify(w, bool(opts[0]), bool(opts[1]))
        return res, st.tolist()
    kw = {"trace order": {"state_sort": False}, "generic index": {"generic_index": True}}.get(entry, {})
    with engine.open_evm(w, bool(opts[0]), bool(opts[1]), **kw) as s:
        res = s.run()
        return res, s.read_status().tolist()


def _check_tally(res, exp):  # as tests/test_evm_gpu.py
    fails = [j for j, c in enumerate(exp) if c]
    assert res.fail_count == len(fails)
    if fails:
        assert res.first_fail_row == fails[0] and res.first_fail_code == exp[fails[0]]
    else:
        assert res.first_fail_row is None


def _wrong(trace, status, exp):
    return [(j, trace.ops[j], [hex(v) for v in trace.tuples[j]], hex(status[j]), hex(exp[j])) for j in range(len(exp)) if status[j] != exp[j]]


@pytest.mark.parametrize("entry", ENTRIES)
def test_valid_directed_trace_passes(trace, entry):
    res, status = _run(trace.wire, entry)
    assert len(status) == ac.TRACE_STEPS - 1
    assert not _wrong(trace, status, [0] * len(status))[:8]
    assert res.ok and res.fail_count == 0


@pytest.mark.parametrize("entry", ENTRIES)
def test_invalid_variant_has_the_oracles_status_on_every_pair(trace, invalid, entry):
    w, changed, exp = invalid
    assert sum(1 for c in exp if c) >= 1000
    res, status = _run(w, entry)
    assert not _wrong(trace, status, exp)[:8]
    _check_tally(res, exp)


@pytest.mark.parametrize("entry", ENTRIES)
def test_whole_wavefront_runs(trace, invalid, entry):
    """every run of run_plan() as its own assertion: 64 lanes of one wavefront all take the path.  Valid: all pass.  Invalid variant:
    the oracle's status lane by lane.  A failure names the run (opcode, form, path) and its steps."""
    _, status = _run(trace.wire, entry)
    w, _, exp = invalid
    _, status_bad = _run(w, entry)
    for op, f, nm, lo, hi in trace.runs:
        bad = [j for j in range(lo, hi) if status[j] != 0]
        assert not bad, (op, f"{32 * f}/256", nm, "valid trace, steps", bad, [hex(status[j]) for j in bad])
        bad = [j for j in range(lo, hi) if status_bad[j] != exp[j]]
        assert not bad, (op, f"{32 * f}/256", nm, "invalid variant, steps", bad, [(hex(status_bad[j]), hex(exp[j])) for j in bad])
    for j, (op, names) in trace.singles.items():  # one lane of its wavefront takes the path
        assert status[j] == 0 and status_bad[j] == exp[j], (op, sorted(names), "single lane, step", j, hex(status[j]), hex(status_bad[j]), hex(exp[j]))


@pytest.mark.parametrize("part", range(N_SLICES))
def test_reference_labelled_cases_on_the_device(golden_dir, loaded, part):
    """tiny state-sorted sessions for every case; every third in trace order, every seventh with the generic index, every fifth through
    the one-shot entry: status == the recorded code, its kind == the reference's"""
    n_cases = len(loaded[1])
    lo, hi = part * n_cases // N_SLICES, (part + 1) * n_cases // N_SLICES
    n = 0
    for k, c, w, opts in ac.iter_cases(golden_dir, loaded):
        if not lo <= k < hi:
            continue
        entries = ["state-sorted"] + [e for e, m in (("trace order", 3), ("generic index", 7), ("one-shot", 5)) if k % m == 0]
        for entry in entries:
            res, status = _run(w, entry, opts)
            assert status == [c.code] and codes.kind_of(status[0]) == c.ref_kind, (k, c.op, [hex(v) for v in c.operands], hex(c.pushed), entry, status)
            _check_tally(res, [c.code])
        n += 1
    assert n == hi - lo >= 500
