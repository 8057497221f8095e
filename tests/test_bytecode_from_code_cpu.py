"""zk_bytecode_from_code on the CPU backend (libzkevm_cpu.so: the per-element functions of csrc/bytecode_code.hpp in host loops):
the bytecode table, the Bytecode circuit's rows and the keccak rows from raw contract code, against the reference's recorded outputs,
a plain-Python model, the existing assignment / keccak entries and the Bytecode circuit itself."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import row_oracles, wire
from tests import bytecode_code_cases as bc
from zkevm_specs_amd import _lib, bytecode_circuit, engine, oneshot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
R = bc.R_DEFAULT
CASES = bc.directed_cases()


def run_cpu(codes, k, r=R):
    code, off = bc.pack(list(codes))
    return oneshot.bytecode_from_code(code, off, k, r, device="cpu")


def same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a.shape == b.shape and np.array_equal(a, b))


# ---- (a) the existing goldens of the assignment: every case whose rows are what its own bytes derive
def _recover_codes(in_rows, offsets, lengths):
    """the case's codes from the value cells, or None when the rows cannot have come from bytes"""
    codes = []
    for j in range(len(lengths)):
        lo, hi = int(offsets[j]), int(offsets[j + 1])
        if hi <= lo or hi - lo - 1 != int(lengths[j]):
            return None
        vals = in_rows[lo + 1 : hi, 5]
        if vals[:, 1:].any() or (vals[:, 0] > 255).any():
            return None
        codes.append(bytes(vals[:, 0].astype(np.uint8)))
    if int(offsets[-1]) != in_rows.shape[0]:
        return None
    return codes if same(bc.model(codes, 0, 0)[0], in_rows) else None


def test_existing_assignment_goldens():
    z = np.load(os.path.join(GOLDEN, "bytecode_assign_cases.npz"))
    names = sorted({key.split("_")[0] for key in z.files if key.startswith("c")})
    ran = truncated = 0
    for c in names:
        in_rows, offsets, lengths = z[f"{c}_in_rows"], z[f"{c}_offsets"], z[f"{c}_lengths"]
        codes = _recover_codes(in_rows, offsets, lengths)
        if codes is None:
            continue  # the reference's tampered or inconsistent inputs
        k, r = int(z[f"{c}_k"]), wire.cells_to_ints(z[f"{c}_r"])[0]
        res, table, rows, _ = run_cpu(codes, k, r)
        assert res.ok and res.rows_evaluated == in_rows.shape[0], c
        assert same(table, in_rows), f"{c}: table"
        assert same(rows, z[f"{c}_rows"]), f"{c}: rows"
        ran += 1
        truncated += in_rows.shape[0] > (1 << k)
    assert ran >= 40 and truncated >= 1, (ran, truncated)


# ---- (b) the reference's own is_code and hash of every directed code of at most 600 bytes
def test_reference_is_code_and_hash():
    z = np.load(os.path.join(GOLDEN, "bytecode_code_cases.npz"))
    code, off = z["code"], z["offsets"]
    codes = [bytes(code[int(off[j]) : int(off[j + 1])]) for j in range(len(off) - 1)]
    assert codes == bc.golden_codes()  # the file is what the generator makes of today's directed set
    res, table, _, keccak = run_cpu(codes, 0)
    assert res.ok
    byte_rows = table[:, 2, 0] == 2
    assert np.array_equal(table[byte_rows, 4, 0].astype(np.uint8), z["is_code"]) and not table[:, 4, 1:].any()
    assert np.array_equal(table[byte_rows, 5, 0].astype(np.uint8), code)
    for j, h in enumerate(z["hash"]):
        v = int.from_bytes(bytes(h), "big")
        assert wire.cells_to_ints(keccak[j, 3:5]) == [v & bc.MASK128, v >> 128], j
        assert bc.is_code_of(codes[j]) == [bool(x) for x in z["is_code"][int(off[j]) : int(off[j + 1])]]  # (the model's, too)
    hdr = np.flatnonzero(~byte_rows)
    assert np.array_equal(table[hdr, 0:2], keccak[:, 3:5])


# ---- (c) the directed set against the model, all three outputs
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_directed_against_model(name):
    _, codes, k = next(c for c in CASES if c[0] == name)
    exp = bc.directed_expected(name)
    res, table, rows, keccak = run_cpu(codes, k)
    assert res.ok and res.fail_count == 0 and res.rows_evaluated == exp[0].shape[0]
    assert same(table, exp[0]) and same(rows, exp[1]) and same(keccak, exp[2])


# ---- (d) against the existing entries on the same data
@pytest.mark.parametrize("name", ["edges", "push_cross", "tiny300", "code_24576", "rows_257_k8", "truncated_in_push_data"])
def test_cross_check_existing_entries(name):
    _, codes, k = next(c for c in CASES if c[0] == name)
    code, off = bc.pack(list(codes))
    _, table, rows, keccak = run_cpu(codes, k)
    row_off = off + np.arange(len(codes) + 1, dtype=np.uint64)
    lengths = np.diff(off)
    assert same(rows, oneshot.bytecode_assign(table, row_off, lengths, k, R, device="cpu")[1])
    assert same(keccak, oneshot.keccak_table(code, off, R, 0, device="cpu")[2])


# ---- (e) the Bytecode circuit's verdicts on the assigned rows
@pytest.mark.parametrize("name", ["edges", "push_misc", "tiny300"])
def test_circuit_verdicts(name):
    _, codes, k = next(c for c in CASES if c[0] == name)
    code, off = bc.pack(list(codes))
    _, table, rows, keccak = run_cpu(codes, k)
    res, status = oneshot.bytecode_verify(rows, keccak, R, device="cpu")
    assert res.ok and res.rows_evaluated == 1 << k and not status.any()
    # one table cell damaged, re-assigned through the row path: the first failing row is the one the row oracle names
    row_off = off + np.arange(len(codes) + 1, dtype=np.uint64)
    byte_rows = np.flatnonzero(table[:, 2, 0] == 2)  # (a Header row's is_code and index cells are not constrained)
    n = len(byte_rows)
    for row, cell in ((byte_rows[n // 3], 5), (byte_rows[n // 2], 4), (byte_rows[2 * n // 3], 3), (byte_rows[n - 1], 0)):
        t = table.copy()
        t[row, cell, 0] ^= np.uint64(1)
        bad = oneshot.bytecode_assign(t, row_off, np.diff(off), k, R, device="cpu")[1]
        res, status = oneshot.bytecode_verify(bad, keccak, R, device="cpu")
        exp = row_oracles.bytecode_verify_rows(wire.colmajor_to_rows(bad), wire.rowmajor_to_rows(keccak), R)
        assert status.tolist() == exp and any(exp)
        assert res.first_fail_row == next(i for i, c in enumerate(exp) if c) and res.fail_count == sum(1 for c in exp if c)


# ---- (f) bad arguments: an error, never a result
def _raw_call(code, offsets, n_bytes, n_codes, k, want_rows=True, opts=0):
    lib = _lib.load_cpu()
    rc = np.zeros(4, dtype=np.uint64)
    rc[0] = 5
    table = np.zeros((max(len(code) + len(offsets), 1), 6, 4), dtype=np.uint64)
    rows = np.zeros((12, 1 << min(max(k, 1), 10), 4), dtype=np.uint64)
    keccak = np.zeros((max(len(offsets), 1), 5, 4), dtype=np.uint64)
    t = _lib.ZkCodeSet(_lib.ptr(code), n_bytes, _lib.ptr(offsets), n_codes, k, 0, _lib.ptr(rc))
    w = _lib.ZkCodeWire(_lib.ptr(table), _lib.ptr(rows) if want_rows else None, _lib.ptr(keccak))
    r = _lib.ZkResult()
    ret = lib.zk_bytecode_from_code(ctypes.byref(t), ctypes.byref(w), opts, ctypes.byref(r))
    return ret, lib.zk_last_error().decode()


def test_bad_arguments():
    code = np.arange(10, dtype=np.uint8)
    u = lambda *v: np.array(v, dtype=np.uint64)  # noqa: E731
    assert _raw_call(code, u(0, 4, 10), 10, 2, 5)[0] == 0  # (the well-formed call goes through)
    for what, args in (("decrease", (code, u(0, 6, 4, 10), 10, 3, 5)),
                       ("start", (code, u(1, 4, 10), 10, 2, 5)),
                       ("end", (code, u(0, 4, 9), 10, 2, 5)),
                       ("end", (code, u(0, 4, 11), 10, 2, 5)),
                       ("2^31", (code, u(0, 4, 10), (1 << 31) - 2, 2, 5)),
                       ("2^31", (code, u(0, 4, 10), 10, (1 << 31) - 10, 5)),
                       ("k", (code, u(0, 4, 10), 10, 2, 29)),
                       ("k == 0", (code, u(0, 4, 10), 10, 2, 0))):
        ret, msg = _raw_call(*args)
        assert ret != 0 and "zk_bytecode_from_code" in msg, (what, ret, msg)
    assert _raw_call(code, u(0, 4, 10), 10, 2, 0, want_rows=False)[0] == 0  # k == 0 without rows is the table-only form
    assert _raw_call(code, u(0, 4, 10), 10, 2, 5, opts=_lib.OPT_DEVICE_PTRS)[0] != 0
    for bad in (lambda: oneshot.bytecode_from_code(code, u(0, 6, 4, 10), 5, R, device="cpu"),
                lambda: oneshot.bytecode_from_code(code, u(0, 4, 9), 5, R, device="cpu"),
                lambda: engine.open_bytecode_from_code(code, u(2, 4, 10), 5, R, device="cpu"),
                lambda: engine.open_bytecode_from_code(code, u(0, 4, 10), 29, R, device="cpu")):
        with pytest.raises(_lib.EngineError):
            bad()
    with engine.open_bytecode_from_code(code, u(0, 4, 10), 0, R, device="cpu") as s:  # a read of rows from a session without any
        s.run()
        w = _lib.ZkCodeWire(None, _lib.ptr(np.zeros((12, 2, 4), dtype=np.uint64)), None)
        assert s._lib.zk_bytecode_from_code_read(s._h, ctypes.byref(w)) != 0


# ---- the session form: passes, read()
def test_session_passes():
    _, codes, k = next(c for c in CASES if c[0] == "push_misc")
    exp = bc.directed_expected("push_misc")
    code, off = bc.pack(list(codes))
    with engine.open_bytecode_from_code(code, off, k, R, device="cpu") as s:
        assert s.n == exp[0].shape[0]
        for _ in range(2):
            res = s.run()
            assert res.ok and res.launches == 1 and res.rows_evaluated == s.n
            assert all(same(a, b) for a, b in zip(s.read(), exp))
        assert not s.read_status().any()


# ---- (g) the mirror's forms
def test_mirror_forms():
    _, codes, k = next(c for c in CASES if c[0] == "truncated_in_push_data")
    for kk, name in ((k, "truncated_in_push_data"), (10, None)):
        exp = bc.directed_expected(name) if name else bc.model(list(codes), kk, R)
        rows = bytecode_circuit.assign_bytecode_circuit(kk, [codes[0], bytearray(codes[1]), codes[2]], R, device="cpu")
        assert same(rows, exp[1])
        table, row_off, lengths = bytecode_circuit.bytecode_table([bytearray(c) for c in codes], device="cpu")
        assert same(table, exp[0]) and lengths.tolist() == [len(c) for c in codes]
        assert row_off.tolist() == [0, 101, 302, 353] and row_off.dtype == np.uint64 and lengths.dtype == np.uint64
        assert same(bytecode_circuit.assign_bytecode_circuit(kk, (table, row_off, lengths), R, device="cpu"), exp[1])  # the tuple form, as before
    table, row_off, lengths = bytecode_circuit.bytecode_table([], device="cpu")
    assert table.shape == (0, 6, 4) and row_off.tolist() == [0] and lengths.shape == (0,)


# ---- (h) the header's functions under AddressSanitizer + UBSan: a stand-alone host program, run as a child process
def test_sanitizer_program(tmp_path):
    exe = str(tmp_path / "bytecode_code_asan")
    src = os.path.join(ROOT, "tests", "hostsim", "bytecode_code_asan.cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DZK_HOSTSIM", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",  # (the runtimes inside the program: nothing to preload)
                           "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-o", exe, src])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "bytecode_code_asan: ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
