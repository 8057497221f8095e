"""Refused opens on the HIP backend: the refusal cases the CPU suites hold, run against libzkevm_hip.so with host pointers and with
ZK_OPT_DEVICE_PTRS — the code and the text the CPU-backend test asserts for the case (where the HIP text differs: the literal of
csrc/zkevm_hip.hip) — and, after each family's refusals, one valid open + pass + read of the family's smallest directed case on the same
thread: a refused open leaves the device, the stream and the arena usable."""
import ctypes

import numpy as np
import pytest

from zkevm_specs_amd import _lib, engine, oneshot

pytestmark = pytest.mark.gpu
ptr = _lib.ptr


def dev(x):
    import torch

    if x is None:
        return None
    x = np.ascontiguousarray(x)
    view = {8: np.int64, 4: np.int32, 2: np.int16, 1: np.uint8}[x.dtype.itemsize]
    return torch.from_numpy(x.view(view).copy()).cuda()


FORMS = [("host", lambda x: x, 0), ("resident", dev, _lib.OPT_DEVICE_PTRS)]
FORM_IDS = [f[0] for f in FORMS]


def opened(lib, rc, handle):
    """(rc, text) of an open; a session that was handed out is closed"""
    if rc == 0:
        lib.zk_close(handle)
    return rc, lib.zk_last_error().decode()


# ---- Tx assignment: the golden cases txs2witness refuses, and the four offset refusals of zk_tx_assign_open (n_txs = 2)
def _tx_open(lib, t, to_dev, opts, calldata=True):
    a = {k: to_dev(np.ascontiguousarray(t[k])) for k in ("fields", "to_is_none", "calldata", "offsets")}
    r = to_dev(np.array([7, 0, 0, 0], dtype=np.uint64))
    n = int(t["fields"].shape[0])
    s = _lib.ZkTxInputs(ptr(a["fields"], n), ptr(a["to_is_none"], n), n, ptr(a["calldata"]) if calldata else None, ptr(a["offsets"]),
                        int(t["chain_id"]), int(t["max_txs"]), int(t["max_calldata_bytes"]), ptr(r))
    h = ctypes.c_void_p()
    return opened(lib, lib.zk_tx_assign_open(ctypes.byref(s), None, opts, ctypes.byref(h)), h)


@pytest.mark.parametrize("form,to_dev,opts", FORMS, ids=FORM_IDS)
def test_tx_assign(form, to_dev, opts):
    from tests.tx_assign_cases import WIRE_KEYS, golden_cases, random_inputs

    lib = _lib.init()
    cases = {c["name"]: c for c in golden_cases()}
    assert _tx_open(lib, cases["max_txs_over"]["tx"], to_dev, opts) == (-1, "zk_tx_assign_open: bad arguments")
    assert _tx_open(lib, cases["max_calldata_over"]["tx"], to_dev, opts) == (-1, "zk_tx_assign_open: more calldata bytes than max_calldata_bytes")
    t = random_inputs(2, 1)
    off = [int(x) for x in t["offsets"]]
    assert off[0] == 0 < off[1] < off[2] == t["calldata"].shape[0]
    u = lambda *v: np.array(v, dtype=np.uint64)  # noqa: E731
    assert _tx_open(lib, dict(t, offsets=u(1, off[1], off[2])), to_dev, opts) == (-1, "zk_tx_assign_open: calldata offsets must start at 0")
    assert _tx_open(lib, dict(t, offsets=u(0, off[2], off[1])), to_dev, opts) == (-1, "zk_tx_assign_open: calldata offsets must be non-decreasing")
    assert _tx_open(lib, dict(t, max_calldata_bytes=off[2] - 1), to_dev, opts) == (-1, "zk_tx_assign_open: more calldata bytes than max_calldata_bytes")
    assert _tx_open(lib, t, to_dev, opts, calldata=False) == (-1, "zk_tx_assign_open: calldata is null")
    assert _tx_open(lib, t, to_dev, opts)[0] == 0
    c = cases["ref_tx2witness"]  # the smallest golden case: one tx
    res, status, wire = oneshot.tx_assign(c["tx"], c["randomness"])
    assert res.fail_count == 0 and not status.any()
    for k in WIRE_KEYS:
        assert np.array_equal(wire[k], c["wire"][k]), k


# ---- EVM tables from block data: every domain error of the CPU suite at sizes and at open
def _block_call(lib, raw, fn, to_dev, opts, n_txs=None, n_history=None, n_withdrawals=None):
    n = raw["tx_fields"].shape[0] if n_txs is None else n_txs
    h = raw["history_hashes"].shape[0] if n_history is None else n_history
    m = raw["withdrawals"].shape[0] if n_withdrawals is None else n_withdrawals
    a = {k: to_dev(v) for k, v in raw.items()}
    t = _lib.ZkBlockData(ptr(a["tx_fields"]), ptr(a["to_is_none"]), ptr(a["access_list"]), n, ptr(a["calldata"]), ptr(a["offsets"]), ptr(a["block"]),
                         ptr(a["history_hashes"]), h, ptr(a["withdrawals"]), m)
    if fn == "sizes":
        x, y, z = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        return lib.zk_evm_tables_from_block_sizes(ctypes.byref(t), opts, ctypes.byref(x), ctypes.byref(y), ctypes.byref(z)), lib.zk_last_error().decode()
    hd = ctypes.c_void_p()
    return opened(lib, lib.zk_evm_tables_from_block_open(ctypes.byref(t), None, opts, ctypes.byref(hd)), hd)


@pytest.mark.parametrize("form,to_dev,opts", FORMS, ids=FORM_IDS)
def test_evm_tables_from_block(form, to_dev, opts):
    from tests import block_tables_cases as bc
    from tests.test_block_tables_cpu import _domain_errors

    lib = _lib.init()
    for label, raw, over, code, text in _domain_errors():
        if form == "resident" and over.get("n_withdrawals") and not raw["withdrawals"].shape[0]:
            # an empty array has no device pointer to hand over: a count without its array is refused as a bad argument
            code, text = -1, "bad arguments"
        for fn in ("sizes", "open"):
            rc, msg = _block_call(lib, raw, fn, to_dev, opts, **over)
            assert rc == code and "zk_evm_tables_from_block" in msg and text in msg, (label, fn, rc, msg)
    exp = bc.directed_expected("single_1")
    res, out = oneshot.evm_tables_from_block(bc.directed_raw("single_1"))
    assert res.ok and res.fail_count == 0 and res.rows_evaluated == exp["tx"].shape[0]
    assert bc.same(out, exp)


# ---- Exp assignment: the rejects of test_exp_assign_cpu.test_domain_rejects (its events, restated: the CPU test holds them inline)
def _exp_call(lib, events, max_exp_steps, fn, to_dev, opts):
    ev = to_dev(events)
    t = _lib.ZkExpEvents(ptr(ev, events.shape[0]), events.shape[0], max_exp_steps)
    if fn == "sizes":
        x, y, z = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        return lib.zk_exp_assign_sizes(ctypes.byref(t), opts, ctypes.byref(x), ctypes.byref(y), ctypes.byref(z)), lib.zk_last_error().decode()
    h = ctypes.c_void_p()
    return opened(lib, lib.zk_exp_assign_open(ctypes.byref(t), None, None, opts, ctypes.byref(h)), h)


@pytest.mark.parametrize("form,to_dev,opts", FORMS, ids=FORM_IDS)
def test_exp_assign(form, to_dev, opts):
    from tests import exp_assign_cases as C

    lib = _lib.init()
    ok = [(5, 3, 9), (7, 2, 5)]
    cases = [(C.events_wire([(9, 3, 9), (9, 2, 5)]), 0, _lib.ERR_EXP_ORDER, "event 1"),
             (C.events_wire([(9, 3, 9), (8, 2, 1), (4, 2, 5)]), 0, _lib.ERR_EXP_ORDER, "event 2"),
             (C.events_wire([(C.FR_P, 3, 9)]), 0, _lib.ERR_EXP_CELL, ""),
             (np.zeros((0, 5, 4), dtype=np.uint64), 2**31 // 7 + 1, _lib.ERR_EXP_ROWS, "")]
    for cell, limb in ((0, 3), (1, 2), (2, 3), (3, 2), (4, 2)):
        ev = C.events_wire(ok)
        ev[1, cell, limb] = np.uint64(2**64 - 1)
        cases.append((ev, 0, _lib.ERR_EXP_CELL, "event 1"))
    for ev, mx, code, text in cases:
        for fn in ("sizes", "open"):
            rc, msg = _exp_call(lib, ev, mx, fn, to_dev, opts)
            assert rc == code and text in msg, (fn, rc, msg)
    assert _exp_call(lib, C.events_wire([(9, 3, 9), (2, 2, 1), (10, 2, 5)]), 0, "open", to_dev, opts)[0] == 0  # an empty event's identifier is free
    want_rows, want_table = C.model(ok, 0)
    _, rows, table = oneshot.exp_assign(C.events_wire(ok), 0)
    assert np.array_equal(rows, C.rows_wire(want_rows)) and np.array_equal(table, C.table_wire(want_table))


# ---- Bytecode from code: the bad arguments of test_bytecode_from_code_cpu.test_bad_arguments (restated: the CPU test holds them inline)
def _code_call(lib, code, offsets, n_bytes, n_codes, k, to_dev, opts, want_rows=True):
    r = np.zeros(4, dtype=np.uint64)
    r[0] = 5
    table = np.zeros((max(len(code) + len(offsets), 1), 6, 4), dtype=np.uint64)
    rows = np.zeros((12, 1 << min(max(k, 1), 10), 4), dtype=np.uint64)
    keccak = np.zeros((max(len(offsets), 1), 5, 4), dtype=np.uint64)
    keep = [to_dev(x) for x in (code, offsets, r, table, rows, keccak)]
    t = _lib.ZkCodeSet(ptr(keep[0]), n_bytes, ptr(keep[1]), n_codes, k, 0, ptr(keep[2]))
    w = _lib.ZkCodeWire(ptr(keep[3]), ptr(keep[4]) if want_rows else None, ptr(keep[5]))
    ret = lib.zk_bytecode_from_code(ctypes.byref(t), ctypes.byref(w), opts, ctypes.byref(_lib.ZkResult()))
    return ret, lib.zk_last_error().decode()


@pytest.mark.parametrize("form,to_dev,opts", FORMS, ids=FORM_IDS)
def test_bytecode_from_code(form, to_dev, opts):
    lib = _lib.init()
    code = np.arange(10, dtype=np.uint8)
    u = lambda *v: np.array(v, dtype=np.uint64)  # noqa: E731
    for what, args in (("decrease", (code, u(0, 6, 4, 10), 10, 3, 5)),
                       ("start", (code, u(1, 4, 10), 10, 2, 5)),
                       ("end", (code, u(0, 4, 9), 10, 2, 5)),
                       ("end", (code, u(0, 4, 11), 10, 2, 5)),
                       ("2^31", (code, u(0, 4, 10), (1 << 31) - 2, 2, 5)),
                       ("2^31", (code, u(0, 4, 10), 10, (1 << 31) - 10, 5)),
                       ("k", (code, u(0, 4, 10), 10, 2, 29)),
                       ("k == 0", (code, u(0, 4, 10), 10, 2, 0))):
        ret, msg = _code_call(lib, *args, to_dev, opts)
        assert ret != 0 and "zk_bytecode_from_code" in msg, (what, ret, msg)
    for text, offsets in (("zk_bytecode_from_code_open: offsets must be non-decreasing", u(0, 6, 4, 10)),  # (the literals of this backend)
                          ("zk_bytecode_from_code_open: offsets must start at 0", u(1, 4, 10)),
                          ("zk_bytecode_from_code_open: offsets must end at n_bytes", u(0, 4, 9))):
        assert _code_call(lib, code, offsets, 10, len(offsets) - 1, 5, to_dev, opts) == (-1, text)
    assert _code_call(lib, code, u(0, 4, 10), 10, 2, 0, to_dev, opts, want_rows=False)[0] == 0  # k == 0 without rows is the table-only form
    assert _code_call(lib, code, u(0, 4, 10), 10, 2, 5, to_dev, opts)[0] == 0  # (the well-formed call goes through)
    from tests import bytecode_code_cases as bc
    from tests.test_bytecode_from_code_cpu import R, same

    _, codes, k = next(c for c in bc.directed_cases() if c[0] == "rows_255_k8")  # the smallest directed case with rows
    exp = bc.directed_expected("rows_255_k8")
    packed, off = bc.pack(list(codes))
    res, table, rows, keccak = oneshot.bytecode_from_code(packed, off, k, R)
    assert res.ok and res.fail_count == 0 and res.rows_evaluated == exp[0].shape[0]
    assert same(table, exp[0]) and same(rows, exp[1]) and same(keccak, exp[2])


# ---- Copy assignment from sources: every domain error of the CPU suite at sizes and at open
@pytest.mark.parametrize("form", FORM_IDS)
def test_copy_assign_from_sources(form):
    from tests import copy_sources_cases as cc
    from tests import test_copy_sources_cpu as host
    from tests.test_copy_sources_gpu import resident

    for label, c, rc, text in host.domain_errors():
        args = resident(c) if form == "resident" else (c["events"], c["flags"], c["src_ref"], c["dst_ref"], c["sources"])
        assert host.error_of(engine.copy_assign_from_sources_sizes, *args) == (rc, text), label
        assert host.error_of(engine.open_copy_assign_from_sources, *args, c["r"]) == (rc, text), label
    c = cc.case("lengths")
    cc.check_outputs(c, cc.expected("lengths"), host.run(c, None), None)


# ---- ECC precompile calls: the CPU suite's domain errors (their own checker, on this library)
@pytest.mark.parametrize("form,to_dev,opts", FORMS, ids=FORM_IDS)
def test_ecc_from_calls(form, to_dev, opts):
    from tests import ecc_calls_cases as C
    from tests import ecc_calls_ref as ref
    from tests.test_ecc_calls_cpu import domain_errors
    from zkevm_specs_amd import ecc_circuit as mirror

    domain_errors(_lib.init(), to_dev=to_dev, opts=opts)
    res, status, out = oneshot.ecc_from_calls(mirror.ecc_calls_wire(*C.batches()["n1"]), C.RANDOMNESS)
    want = C.expected("n1")
    assert res.ok and res.rows_evaluated == want["rows"].shape[0] and not status.any()
    ref.assert_equal(out, want, "n1")


# ---- Sig assignment: what signed_data2witness raises from — the first failing signature of the directed batch, by index and code
@pytest.mark.parametrize("form", FORM_IDS)
def test_sig_assign(form):
    from tests import sig_assign_cases as C
    from tests.test_sig_assign_cpu import R

    entries, at = C.directed_entries(0)
    first = min(C.expected_sites(at))
    sig = C.pack(entries[: first + 1])
    want_status, _ = C.model(sig, R)
    assert want_status[first] == C.BAD | 1 and not any(want_status[:first])
    if form == "resident":
        with engine.open_sig_assign({k: dev(v) if hasattr(v, "dtype") else v for k, v in sig.items()}, R) as s:
            res, status = s.run(), s.read_status()
    else:
        res, status, _ = oneshot.sig_assign(sig, R)
    assert status.tolist() == want_status and (res.fail_count, res.first_fail_row, res.first_fail_code) == (1, first, C.BAD | 1)
    sig = C.pack(entries[:first])
    want_status, want = C.model(sig, R)
    res, status, wire = oneshot.sig_assign(sig, R)
    C.compare(status, wire, want_status, want, form)
    assert res.fail_count == 0 and wire["bytes"].shape[0] == first


# ---- the one-shots' shared wire checks (test_session_oneshot_cpu): the one with a check behind it in the library — offsets that do not
#      cover the rows — through raw ctypes, where the Python wrapper would refuse first
@pytest.mark.parametrize("form,to_dev,opts", FORMS, ids=FORM_IDS)
def test_bytecode_assign_offsets(form, to_dev, opts):
    from tests.test_session_oneshot_cpu import golden

    lib = _lib.init()
    g = golden("bytecode_assign_cases.npz")
    in_rows, off, ln, k, r = g["c0003_in_rows"], g["c0003_offsets"], g["c0003_lengths"], int(g["c0003_k"]), g["c0003_r"]
    keep = [to_dev(x) for x in (in_rows, off[:-1], ln[:-1], r)]
    h = ctypes.c_void_p()
    rc = lib.zk_bytecode_assign_open(ptr(keep[0]), in_rows.shape[0], ptr(keep[1]), ptr(keep[2]), len(ln) - 1, k, ptr(keep[3]), None, opts, ctypes.byref(h))
    assert opened(lib, rc, h) == (-1, "zk_bytecode_assign_open: offsets must cover every row")
    with engine.open_bytecode_assign(in_rows, off, ln, k, r) as s:
        res_s, st_s, rows_s = s.run(), s.read_status(), s.rows()
    res_o, rows_o = oneshot.bytecode_assign(in_rows, off, ln, k, r)
    assert res_s.ok and res_o.ok and not st_s.any()
    assert np.array_equal(rows_s, g["c0003_rows"]) and np.array_equal(rows_o, g["c0003_rows"])  # the reference's recorded rows
