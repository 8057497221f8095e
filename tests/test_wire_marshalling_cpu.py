"""The Python side of the C ABI marshals the wire-struct assignment families and the State-from-RW / from-trace group exactly as
recorded in tests/golden/marshalling_calls_cpu.json (tools/gen_golden_marshalling.py): the same library calls with the same scalars and
the same null / non-null pointers, the same outputs, the same refusals by class and message.  Host arrays through the CPU backend."""
import json
import os

import pytest

from tests import marshalling_cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "marshalling_calls_cpu.json")
with open(GOLDEN) as _f:
    WANT = json.load(_f)


@pytest.fixture(scope="module")
def got():
    return json.loads(json.dumps(marshalling_cases.run("cpu")))  # (through JSON: tuples become lists, as in the record)


def test_the_list_is_the_recorded_one(got):
    assert sorted(got) == sorted(WANT)
    assert len(WANT) >= 150 and sum("raised" in c for c in WANT.values()) >= 30


@pytest.mark.parametrize("name", sorted(WANT))
def test_marshalling_is_unchanged(name, got):
    g, w = got[name], WANT[name]
    assert g["calls"] == w["calls"]
    assert g.get("raised") == w.get("raised")
    assert g.get("returned") == w.get("returned")
