"""CPU tests: State-circuit oracle vs the reference's recorded outcomes, and the kernels'
per-row logic (hostsim build of csrc/state_circuit.hpp) vs the oracle."""
import ctypes
import os

import numpy as np
import pytest

from oracle import codes, state_oracle, wire
from zkevm_specs_amd.synth import synth_state_witness


def _cases(golden_dir):
    g = np.load(os.path.join(golden_dir, "state_cases.npz"))
    for i, name in enumerate(g["names"]):
        k = f"c{i:03d}"
        yield str(name), g[k + "_rows"], g[k + "_flags"], g[k + "_mpt"], g[k + "_ref_kind"]


def _hostsim_state(lib, cols, flags, mpt):
    cols, flags, mpt = map(np.ascontiguousarray, (cols, flags, mpt))
    n = cols.shape[1]
    st = np.zeros(n, dtype=np.uint32)
    vp = ctypes.c_void_p
    lib.sim_state_verify(vp(cols.ctypes.data), vp(flags.ctypes.data), ctypes.c_uint64(n), vp(mpt.ctypes.data),
                         ctypes.c_uint64(mpt.shape[0]), vp(st.ctypes.data))
    return st


def test_oracle_matches_reference_outcomes(golden_dir):
    """Every row of every golden case: oracle's exception class == the reference's."""
    n_rows = n_fail = 0
    for name, cols, flags, mpt, ref_kind in _cases(golden_dir):
        got = state_oracle.verify_rows(wire.colmajor_to_rows(cols), flags, wire.rowmajor_to_rows(mpt))
        kinds = [codes.kind_of(c) for c in got]
        assert kinds == ref_kind.tolist(), name
        n_rows += len(kinds)
        n_fail += sum(k != 0 for k in kinds)
    assert n_rows > 4000 and n_fail > 250


def test_kernel_logic_matches_oracle_on_goldens(golden_dir, hostsim):
    for name, cols, flags, mpt, _ in _cases(golden_dir):
        exp = state_oracle.verify_rows(wire.colmajor_to_rows(cols), flags, wire.rowmajor_to_rows(mpt))
        got = _hostsim_state(hostsim, cols, flags, mpt)
        assert got.tolist() == exp, name


@pytest.mark.parametrize("n", [64, 1000, 4096])
def test_synthetic_witness_is_valid(n):
    cols, flags, mpt = synth_state_witness(n, seed=2)
    got = state_oracle.verify_rows(wire.colmajor_to_rows(cols), flags, wire.rowmajor_to_rows(mpt))
    assert not any(got)


def test_kernel_logic_on_tampered_synthetic(hostsim):
    """Flip random cells of a 4096-row synthetic witness; statuses must equal the oracle's."""
    rng = np.random.default_rng(7)
    cols, flags, mpt = synth_state_witness(4096, seed=3)
    for _ in range(200):
        c, i = int(rng.integers(0, 57)), int(rng.integers(0, 4096))
        mode = int(rng.integers(0, 4))
        if mode == 0:
            cols[c, i, 0] ^= np.uint64(1)
        elif mode == 1:
            cols[c, i, int(rng.integers(0, 4))] = np.uint64(rng.integers(0, 2**62))
            cols[c, i, 3] &= np.uint64(0x0FFFFFFFFFFFFFFF)  # keep the cell canonical (< p)
        elif mode == 2:
            cols[c, i] = 0
        else:
            flags[i] ^= np.uint32(1 << int(rng.integers(0, 2)))
    exp = state_oracle.verify_rows(wire.colmajor_to_rows(cols), flags, wire.rowmajor_to_rows(mpt))
    got = _hostsim_state(hostsim, cols, flags, mpt)
    assert got.tolist() == exp
    assert sum(1 for e in exp if e) > 100


def test_oracle_reproduces_the_stored_site_cases(golden_dir):
    """tests/golden/state_site_cases.npz: this copy of the oracle gives every case the failing rows and codes the generator's copy gave
    (full pass over the patched base, no shortcut), and the helper's neighbourhood-only expectation equals the full pass"""
    from tests import state_site_cases as ssc

    data = ssc.load(golden_dir)
    for k, c in enumerate(data.cases):
        _, flags, _, rows, mpt_rows, t, affected = ssc.build(data, c, 0, 0)
        exp = state_oracle.verify_rows(rows, flags, mpt_rows)
        assert exp[t] == c.code and codes.site_of(c.code) == c.site and codes.kind_of(c.code) == c.ref_kind, k
        assert [(j, e) for j, e in enumerate(exp) if e] == c.fails, k
        assert ssc.expected(rows, flags, mpt_rows, affected) == exp, k
        if c.compact_code != ssc.EXCLUDED:
            _, flags, _, rows, mpt_rows, t, _ = ssc.build(data, c, 0, 0, compact=True)
            assert state_oracle.check_row(rows, flags, t, set(tuple(m) for m in mpt_rows)) == c.compact_code, k
    assert len(data.cases) >= 300
