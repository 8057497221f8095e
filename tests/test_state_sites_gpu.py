"""Directed State-circuit failure sites on the device (tests/golden/state_site_cases.npz, tests/state_site_cases.py): every case makes one
numbered check of csrc/state_circuit.hpp the first failure of its target row, and runs with the target on the first and the last lane of
a 63-row wavefront, the first and the last row of a 252-row block, slots 1 and 15 of the lane-group tiling, and as row n - 1 in front of
the wrap-around — through the LDS-ring kernel, the 15-cell kernel, ranged sessions, the one-shot entry, and (one child process with
ZK_STATE_DMA=0) the lane-group kernel.  A check a kernel lacks, numbers differently or tests more weakly shows as a wrong status."""
import os
import subprocess
import sys

import pytest

from tests import state_site_cases as ssc

pytestmark = pytest.mark.gpu

N_SLICES = 4
_ran = {}  # (form, part) -> (cases, variants, sites, excluded) of the slices that ran in this process


@pytest.fixture(scope="module")
def data(golden_dir):
    return ssc.load(golden_dir)


@pytest.mark.parametrize("form", ssc.FORMS)
@pytest.mark.parametrize("part", range(N_SLICES))
def test_every_case_fails_at_its_site_on_the_device(data, part, form):
    out = ssc.run_slice(data, None, part, N_SLICES, form)
    assert out[1] == ssc.expected_variants(data, part, N_SLICES, form) and out[0] > 0
    _ran[(form, part)] = out


def test_no_case_was_skipped_on_the_device(data):
    """over the slices above: cases run == cases in the file (less the counted 15-cell exclusions), variants run == variants declared,
    sites exercised == the file's census"""
    assert sorted(_ran) == sorted((f, p) for f in ssc.FORMS for p in range(N_SLICES)), "run this module as a whole"
    for form in ssc.FORMS:
        parts = [_ran[(form, p)] for p in range(N_SLICES)]
        excl = sum(p[3] for p in parts)
        assert excl == (len(ssc.compact_excluded(data)) if form == "compact" else 0)
        assert sum(p[0] for p in parts) == len(data.cases) - excl
        assert sum(p[1] for p in parts) == sum(ssc.expected_variants(data, p, N_SLICES, form) for p in range(N_SLICES))
    assert sorted(set().union(*(_ran[("full", p)][2] for p in range(N_SLICES)))) == ssc.census(data)[0]
    assert set().union(*(_ran[("compact", p)][2] for p in range(N_SLICES))) == set(ssc.census(data)[0]) - set(ssc.COMPACT_ABSENT)


def test_lane_group_kernel_fails_every_case_at_its_site(data):
    """ZK_STATE_DMA=0 selects the lane-quad kernel when the library first launches: one child process runs every case and variant"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import sys; sys.path.insert(0, %r); from tests import state_site_cases as s; s.child_main()" % root
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ZK_STATE_DMA="0"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    want = "lane-group ok %d %d %d" % (len(data.cases), ssc.expected_variants(data, 0, 1), len(ssc.census(data)[0]))
    assert p.returncode == 0 and want in p.stdout.decode(), (p.stdout.decode()[-500:], p.stderr.decode()[-2000:])
