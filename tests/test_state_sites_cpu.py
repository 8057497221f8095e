"""Directed State-circuit failure sites on the host build (libzkevm_cpu.so): tests/golden/state_site_cases.npz through
tests/state_site_cases.py — every case at every position, 57-cell and 15-cell sessions, ranged sessions, the one-shot entry."""
import pytest

from oracle import codes, state_oracle as so
from tests import state_site_cases as ssc

N_SLICES = 4


@pytest.fixture(scope="module")
def data(golden_dir):
    return ssc.load(golden_dir)


def test_file_census_and_line_table(data):
    """at most three sites without a case; one reference line per site, stored shared lines are exactly the sites that share one; every
    case of a site carries that site's line; values at 2^64 and above and at 2^128 and above are among the patches"""
    have, missing = ssc.census(data)
    assert missing == sorted(data.unreached) == [82] and len(data.tried) == len(missing)
    assert sorted(data.site_line) == have
    for c in data.cases:
        assert codes.site_of(c.code) == c.site and data.site_line[c.site] == c.ref_line and c.ref_kind == codes.kind_of(c.code)
        assert c.target <= ssc.MAX_TARGET and (c.target == 0) == c.fixed
    pairs = sorted((a, b) for a in have for b in have if a < b and data.site_line[a] == data.site_line[b])
    assert pairs == sorted(data.shared)
    # sites a value of 2^64 or more / 2^128 or more was patched in for (the kernels' fr_le_u64 / fr_fits64 / fr_fits128 short cuts)
    wide64 = {c.site for c in data.cases for kind, _, _, v in c.patches if kind != ssc.PATCH_FLAGS and v >= 1 << 64}
    wide128 = {c.site for c in data.cases for kind, _, _, v in c.patches if kind != ssc.PATCH_FLAGS and v >= 1 << 128}
    # the range checks and decomposition checks whose cell admits such a value (a wider tag / id / field_tag / limb / byte / is_write cell,
    # an address with limbs to match, a Memory or receipt value), and the compact form's address / key width checks
    assert wide64 >= {1, 2, 3, 4, 5, 6, 7, 8, 46, 48, 63, 145, 149} and wide128 >= {1, 2, 3, 4, 5, 6, 7, 8, 46, 48, 63, 145, 149}, (sorted(wide64), sorted(wide128))
    # position coverage the variants give: row n - 1 (truncated) for tags 4, 6 and 11, and the Start sites at row 0
    last = {data.rows[c.target][so.TAG] for c in data.cases if ssc.truncation(data.rows, c)}
    assert {4, 6, 11} <= last, last
    assert {c.site for c in data.cases if c.fixed} >= set(range(20, 32))
    # every site has a case that shifts: none is exercised on row 0 alone
    assert {c.site for c in data.cases if not c.fixed} == set(have)


def test_padded_bases_pass_the_oracle(data):
    """every (truncation, k) the variants use was checked against the reference by the generator; here the oracle accepts them too"""
    used = set()
    for c in data.cases:
        used |= set(ssc.variants(data.rows, c))
    assert used == data.checked
    for trunc, k in sorted(used):
        _, flags, rows = ssc.padded(data, trunc, k)
        assert not any(so.verify_rows(rows, flags, data.mpt_rows)), (trunc, k)


@pytest.mark.parametrize("form", ssc.FORMS)
@pytest.mark.parametrize("part", range(N_SLICES))
def test_every_case_fails_at_its_site_on_the_host_build(data, part, form):
    ran, n_var, _, _ = ssc.run_slice(data, "cpu", part, N_SLICES, form)
    assert n_var == ssc.expected_variants(data, part, N_SLICES, form) and ran > 0


def test_slices_exercise_the_declared_sites(data):
    """the sites of the cases each form runs, from the file alone (run_slice returns the same sets; the device module sums them)"""
    for form in ssc.FORMS:
        sites = {c.site for c in data.cases if not (form == "compact" and ssc.touches_dropped(c))}
        assert sites == set(ssc.census(data)[0]) - set(ssc.COMPACT_ABSENT if form == "compact" else ())


def test_nothing_is_left_out(data):
    """the slices above are the whole file: the slice bounds tile it, the sites of all cases are the census, and the 15-cell exclusions
    are the cases that patch a dropped column"""
    n = len(data.cases)
    assert [p * n // N_SLICES for p in range(N_SLICES + 1)] == sorted({p * n // N_SLICES for p in range(N_SLICES + 1)}) and n >= 300
    excl = ssc.compact_excluded(data)
    assert excl == [k for k, c in enumerate(data.cases) if c.compact_code == ssc.EXCLUDED] and 0 < len(excl) < n // 2
    runs_compact = {c.site for k, c in enumerate(data.cases) if k not in set(excl)}
    assert {5, 7} <= runs_compact and not {4, 6, 9} & runs_compact  # the decomposition checks left in the 15-cell form / absent from it
    assert runs_compact == set(ssc.census(data)[0]) - set(ssc.COMPACT_ABSENT)
    # cases the 15-cell form reads differently (an address / key cell patched alone): counted; none of them passes there
    reread = [c for c in data.cases if c.compact_code not in (ssc.EXCLUDED, c.code)]
    assert len(reread) == ssc.COMPACT_REREAD and all(c.compact_code != 0 for c in data.cases)
