"""Directed Copy / Bytecode / Exp failure sites on the device (tests/golden/row_site_cases.npz, tests/row_site_cases.py): every case makes
one numbered check of csrc/copy_circuit.hpp / row_circuits.hpp the first failure of its target row, and runs with the target on the
lanes where the neighbour exchange can go wrong — Copy: lanes 0 / 1, 60 / 61 (successors on the read-only lanes 62 / 63), the first lanes
of the next wavefront, the edges of a 248-row block, the last rows in front of the wrap-around; Bytecode: lanes 0 and 62, the edge of a
252-row block, row n - 1; Exp: a block edge and row n - 1 — through sessions (dense and generic RW index), ranged sessions, the one-shot
entries and, in one child process each, the 256- and 128-thread launch shapes of the Copy kernel."""
import os
import subprocess
import sys

import pytest

from tests import row_site_cases as rsc

pytestmark = pytest.mark.gpu

N_SLICES = {"copy": 8, "bytecode": 3, "exp": 3}
SLICES = [(name, part) for name in rsc.CIRCUITS for part in range(N_SLICES[name])]
_ran = {}


@pytest.fixture(scope="module")
def datas(golden_dir):
    return {name: rsc.load(golden_dir, name) for name in rsc.CIRCUITS}


@pytest.mark.parametrize("name,part", SLICES)
def test_every_case_fails_at_its_site_on_the_device(datas, name, part):
    data = datas[name]
    out = rsc.run_slice(data, None, part, N_SLICES[name])
    assert out[1] == rsc.expected_variants(data, part, N_SLICES[name]) and out[0] > 0
    _ran[(name, part)] = out


@pytest.mark.parametrize("block", (256, 128))
def test_copy_launch_shape_fails_every_case_at_its_site(datas, block):
    """ZK_COPY_BLOCK is read when the library first launches the Copy kernel: one child process per shape runs every Copy case and variant"""
    data = datas["copy"]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import sys; sys.path.insert(0, %r); from tests import row_site_cases as r; r.child_main()" % root
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ZK_COPY_BLOCK=str(block)), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    want = "copy-block %d ok %d %d %d" % (block, len(data.cases), rsc.expected_variants(data, 0, 1), len(rsc.census(data)[0]))
    assert p.returncode == 0 and want in p.stdout.decode(), (p.stdout.decode()[-500:], p.stderr.decode()[-2000:])


def test_no_case_was_skipped_on_the_device(datas):
    """over the slices above: cases run == cases in the file, runs made == runs declared, sites exercised == the file's census"""
    assert sorted(_ran) == sorted(SLICES), "run this module as a whole"
    for name, data in datas.items():
        parts = [_ran[(name, p)] for p in range(N_SLICES[name])]
        assert sum(p[0] for p in parts) == len(data.cases)
        assert sum(p[1] for p in parts) == rsc.expected_variants(data, 0, 1)
        assert sorted(set().union(*(p[2] for p in parts))) == rsc.census(data)[0]
