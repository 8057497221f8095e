"""The reference's tests/test_withdrawal_circuit.py run with its `verify_circuit` rebound to zkevm_specs_amd.withdrawal_circuit.verify_circuit
(tools/run_reference_suite.py), through the CPU backend: the last reference test module that ran on the reference's own Python loop.
Skipped where no reference was staged under oracle/_ref/."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_ROOT = os.path.join(ROOT, "oracle", "_ref")
pytestmark = pytest.mark.skipif(not os.path.isdir(os.path.join(REF_ROOT, "tests")), reason="no reference staged under oracle/_ref/")


def test_reference_withdrawal_tests_pass_through_the_mirror(tmp_path):
    out = tmp_path / "summary.json"
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    env.pop("ZK_BACKEND", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_reference_suite.py"), "--backend", "cpu", "--ref-root", REF_ROOT,
                        "--out", str(out), "--select", "test_withdrawal_circuit.py"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    s = json.loads(out.read_text())
    assert s["not_passed"] == 0, s["not_passed_detail"]
    assert s["tests_run"] == 7
    assert s["calls_through_the_boundary"].get("zkevm_specs_amd.withdrawal_circuit.verify_circuit", 0) >= 6
    assert not s["modules_without_a_rebound_driver"]
