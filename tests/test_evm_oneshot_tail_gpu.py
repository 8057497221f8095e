"""The one-shot EVM entries with the RW key pack's tail in the open's second launch (ZK_P2_RW_TAIL) and without a status array for
callers who pass no buffer: every row's record written exactly once on either side of the seam, no assumption that the table is
dense (a gap in the tail alone is verified a second time with the generic index), rows too wide for a record in the tail, and the
four status paths — all against oracle/evm_oracle.py.  The knob is read once per process: one child per setting runs every case
(tests/evm_oneshot_tail_cases.py).  Settings: off, one 256-row block in phase 2, half the table, all of it but the first 64 rows."""
import os
import subprocess
import sys

import pytest

from tests import evm_oneshot_tail_cases as otc

pytestmark = pytest.mark.gpu

N_CASES = 5 + 4 + 2 + 5 + 1 + 2  # seam, tail sizes, tiny tables, gaps, wide key cells, status paths


@pytest.fixture(scope="module")
def shared(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("oneshot_tail") / "shared.npz")
    otc.shared_build(path)
    return path


def test_head_ends_on_a_block_boundary_and_keeps_row_0():
    for pm in (0, 1, 80, 500, 999, 5000):
        for n in (1, 2, 63, 64, 65, 129, 320, 3321, 1 << 18):
            h = otc.n_head(n, pm)
            assert 1 <= h <= n and (h == n or h % 64 == 0)
            assert pm != 0 or h == n


@pytest.mark.parametrize("pm,single_block", [(0, False), (80, True), (500, False), (999, False)])
def test_oneshot_matches_the_oracle_at_tail_setting(shared, pm, single_block):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import sys; sys.path.insert(0, %r); from tests import evm_oneshot_tail_cases as c; c.child_main()" % root
    p = subprocess.run([sys.executable, "-c", code, shared, "1" if single_block else "0"], env=dict(os.environ, ZK_P2_RW_TAIL=str(pm)),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0 and "oneshot tail ok %d %d" % (pm, N_CASES) in p.stdout.decode(), (p.stdout.decode()[-500:], p.stderr.decode()[-3000:])
