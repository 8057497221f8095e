"""tests/test_wire_marshalling_cpu.py for device tensors through the HIP library: output buffers all given, partly given and absent, a
non-contiguous output buffer (refused), host randomness beside device inputs (what each family's argument builder makes of it), and the
State sessions with and without flat output buffers — against tests/golden/marshalling_calls_hip.json, recorded on an MI355X."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "marshalling_calls_hip.json")
with open(GOLDEN) as _f:
    WANT = json.load(_f)


@pytest.fixture(scope="module")
def got():
    from tests import marshalling_cases

    return json.loads(json.dumps(marshalling_cases.run(None)))


def test_the_list_is_the_recorded_one(got):
    assert sorted(got) == sorted(WANT)
    assert len(WANT) >= 50


@pytest.mark.parametrize("name", sorted(WANT))
def test_marshalling_is_unchanged(name, got):
    g, w = got[name], WANT[name]
    assert g["calls"] == w["calls"]
    assert g.get("raised") == w.get("raised")
    assert g.get("returned") == w.get("returned")
