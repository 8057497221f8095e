"""Sig circuit witness assignment (zk_sig_assign, csrc/sig_assign.hpp) on the CPU backend: the reference's Sig and ecRecover fixtures
rebuilt from their own inputs, a directed batch against the plain-Python model (tests/sig_assign_ref.py), and the Python surface
(sig_circuit.signed_data2witness / verify_circuit / sig_table)."""
import collections
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import sig_assign_cases as C
from zkevm_specs_amd import errors, oneshot
from zkevm_specs_amd import sig_circuit as mirror

R = 0x0BADC0FFEE0DDF00D
SignedData = collections.namedtuple("SignedData", "msg_hash sig_v sig_r sig_s addr")


def sig_fixtures(device):
    """Test 1: the reachable `sig:` cases of sign_cases.npz, bit for bit, then assignment -> ECDSA layout 2 -> the Sig circuit"""
    cases = C.sig_fixture_cases()
    assert [name for name, *_ in cases] == sorted(C.SIG_REACHABLE) and len(C.SIG_EDITED_AFTER_BUILDING) == 5
    for name, sig, r, c in cases:
        res, status, wire = oneshot.sig_assign(sig, r, device=device)
        assert res.fail_count == 0 and not status.any(), name
        for k in ("bytes", "cells", "keccak"):
            assert np.array_equal(wire[k], c[k]), (name, k)
        assert np.array_equal(wire["meta"][:, 1:], c["meta"][:, 1:]), name
        assert (wire["meta"][:, 0] == 0xFFFFFFFF).all(), name
        _, ecd = oneshot.ecdsa_verify(wire["bytes"], np.ascontiguousarray(wire["meta"][:, 3]), layout=2, device=device)
        w = {k: wire[k] for k in ("bytes", "cells", "keccak")}
        w["meta"] = wire["meta"].copy()
        w["meta"][:, 0] = ecd
        w["tx_rows"], w["tx_flags"] = c["tx_rows"], c["tx_flags"]
        _, st = oneshot.sign_verify(w, r, True, device=device)
        assert (st >> 24).tolist() == c["ref_kind"].tolist() == C.SIG_REF_KIND[name], name


def ecrecover_fixtures(device):
    """Test 2: the seven un-fuzzed cases of evm_ecRecover.npz.  Six derive the fixture's own sig-table row and aux cells 8 - 10 and
    verify with them.  The seventh is the reference's `zero_addr` case: its recorded table row denies a signature that does recover
    (the reference's test hands the precompile no address there); the derived row is case 0's, with is_valid 1, and says so."""
    cases = C.ecrecover_fixture_cases()
    assert sorted(cases) == list(C.ECRECOVER_CASES)
    rows, n_site1 = {}, 0
    for i, (sig, r, w, opts, ref_kind) in cases.items():
        res, status, wire = oneshot.sig_assign(sig, r, device=device)
        assert wire["sig_table"].shape == (1, 9, 4) and wire["aux"].shape == (1, 12, 4), i
        rows[i] = wire["sig_table"][0]
        assert np.array_equal(wire["aux"][0, :8], w["aux"][0, :8]) and np.array_equal(wire["aux"][0, 11], w["aux"][0, 11]), i
        if i == C.ECRECOVER_ZERO_ADDR:
            continue
        assert np.array_equal(wire["sig_table"], w["sig"]), i
        assert np.array_equal(wire["aux"][0, 8:11], w["aux"][0, 8:11]), i
        if i:
            assert status.tolist() == [C.BAD | 1] and not wire["sig_table"][0, 7:].any(), i
            n_site1 += 1
        else:
            assert status.tolist() == [0] and wire["sig_table"][0, 8].tolist() == [1, 0, 0, 0]
        derived = dict(w, sig=wire["sig_table"], aux=np.concatenate([wire["aux"], w["aux"][1:]]))
        _, st = oneshot.evm_verify(derived, bool(opts[0]), bool(opts[1]), device=device)
        assert (st >> 24).tolist() == ref_kind.tolist() == [0], i
    assert n_site1 == 5
    z = C.ECRECOVER_ZERO_ADDR
    assert not cases[z][2]["sig"][0, 7:].any()              # the fixture: (..., 0, 0)
    assert np.array_equal(rows[z], rows[0]) and rows[z][8, 0] == 1  # derived: the signature recovers, as in case 0


def directed(device, v_offset):
    """Test 3: the directed batch against the model, with addr / expect_valid given and null"""
    entries, at = C.directed_entries(v_offset)
    assert 55 <= len(entries) <= 70
    for given in (True, False):
        sig = C.pack(entries, v_offset, addr=given, expect_valid=given)
        want_status, want = C.model(sig, R)
        sites = C.expected_sites(at)
        assert {i: s & 0xFFFFFF for i, s in enumerate(want_status) if s} == sites
        assert all(s >> 24 == errors.KIND_UNSUPPORTED for s in want_status if s)
        res, status, wire = oneshot.sig_assign(sig, R, device=device)
        C.compare(status, wire, want_status, want, (v_offset, given))
        assert res.fail_count == len(sites) and res.first_fail_row == min(sites)
        n = len(entries)
        assert wire["sig_table"].shape[0] == n - 2 - 1  # the signature given three times, the failing one given twice
        assert wire["keccak"].shape[0] == 1 + (n - len(sites)) - 2 - 2  # zero row; one row for the three repeats, one for the one key
        assert {int(wire["meta"][i, 3]) for i in range(n) if not want_status[i]} == {0, 1}


def test_reference_sig_fixtures_cpu():
    sig_fixtures("cpu")


def test_reference_ecrecover_fixtures_cpu():
    ecrecover_fixtures("cpu")


@pytest.mark.parametrize("v_offset", [0, 27])
def test_directed_batch_matches_model_cpu(v_offset):
    directed("cpu", v_offset)


@pytest.mark.parametrize("n", [0, 1])
def test_empty_and_single_cpu(n):
    entries, _ = C.directed_entries(0)
    sig = C.pack(entries[:n])
    want_status, want = C.model(sig, R)
    res, status, wire = oneshot.sig_assign(sig, R, device="cpu")
    C.compare(status, wire, want_status, want, n)
    assert wire["keccak"].shape[0] == 1 + n and wire["sig_table"].shape[0] == n and res.fail_count == 0


def _signed_data(entries):
    return [SignedData(e[0], e[1], e[2], e[3], e[4]) for e in entries]


def test_signed_data2witness_raises_bad_signature_at_first_failing_index():
    entries, at = C.directed_entries(0)
    first = min(C.expected_sites(at))
    with pytest.raises(Exception) as ei:
        mirror.signed_data2witness(_signed_data(entries), R, device="cpu")
    assert type(ei.value).__name__ == "BadSignature" and f"signature {first}:" in str(ei.value)
    assert errors.TX_BAD_SIGNATURE_SITES[1] in str(ei.value)
    w = mirror.signed_data2witness(_signed_data(entries[:first]), R, device="cpu")
    assert isinstance(w, mirror.SigWitness) and w.wire["bytes"].shape[0] == first


def test_verify_circuit_takes_a_sig_witness():
    """verify_circuit(SigWitness) passes on signed data and raises AssertionError at a wrong claimed address (a process of its own:
    the backend is chosen when the package is imported)"""
    script = (
        "import collections, sys\n"
        "from tests import sig_assign_cases as C\n"
        "from zkevm_specs_amd import sig_circuit as mirror\n"
        "SD = collections.namedtuple('SD', 'msg_hash sig_v sig_r sig_s addr')\n"
        "entries, at = C.directed_entries(0)\n"
        "good = [SD(*e[:5]) for i, e in enumerate(entries) if i not in C.expected_sites(at) and i != at['wrong_claimed_address']][:12]\n"
        "res = mirror.verify_circuit(mirror.signed_data2witness(good, 77), 77)\n"
        "assert res.fail_count == 0 and res.rows_evaluated == 12\n"
        "bad = good[:5] + [SD(*entries[at['wrong_claimed_address']][:5])] + good[5:]\n"
        "try:\n"
        "    mirror.verify_circuit(mirror.signed_data2witness(bad, 77), 77)\n"
        "except AssertionError as e:\n"
        "    assert 'row 5' in str(e), str(e)\n"
        "    print('raised')\n"
    )
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, ZK_BACKEND="cpu", PYTHONDONTWRITEBYTECODE="1"), capture_output=True, text=True,
                       cwd=root, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("raised"), r.stderr[-2000:]


def test_sig_table_with_duplicates():
    entries, at = C.directed_entries(27)
    pick = [at["repeat_0"], at["one_key_0"], at["repeat_1"], at["r_0"], at["one_key_1"], at["r_0_again"], at["repeat_2"]]
    data = _signed_data([entries[i] for i in pick])
    rows, aux = mirror.sig_table(data, R, device="cpu")
    assert rows.shape == (4, 9, 4) and aux.shape == (7, 12, 4)  # repeat, one_key_0, r_0, one_key_1 in first-occurrence order
    sig = C.pack([entries[i] for i in pick], 27, addr=False, expect_valid=False)
    _, want = C.model(sig, R)
    assert np.array_equal(rows, want["sig_table"]) and np.array_equal(aux, want["aux"])
    assert rows[2, 8].tolist() == [0, 0, 0, 0] and rows[0, 8].tolist() == [1, 0, 0, 0]
    assert np.array_equal(aux[0], aux[2]) and np.array_equal(aux[0], aux[6])
