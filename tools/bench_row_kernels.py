#!/usr/bin/env python3
"""Throughput of the row-stencil kernels (Bytecode / Exp / Tx-Sig circuits, the ECC circuit) on synthetic witnesses:
rows/s and algorithmic GB/s (SURVEY.md §8d bytes per unit), device-resident inputs, HIP-event kernel
time.  bench.py carries the headline EVM / State workloads; this is the side table in DESIGN.md §3.
`bench_row_kernels.py ecc` runs only the ECC legs (one-shot, then the resident session), `bench_row_kernels.py withdrawal` only the Withdrawal leg, `bench_row_kernels.py
tx_assign` only the Tx witness-assignment leg, `bench_row_kernels.py sig_assign` only the Sig witness-assignment leg, `bench_row_kernels.py exp_assign` only the Exp witness-assignment leg,
`bench_row_kernels.py pi_assign` only the PI witness-assignment leg."""
import json
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from zkevm_specs_amd import _lib, engine
from zkevm_specs_amd.synth import synth_bytecode_witness, synth_exp_witness, synth_state_ops, synth_tx_witness

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
to_dev = lambda x: torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x.view(np.int32) if x.dtype == np.uint32 else x).cuda()
_lib.init(0)
out = {}


def run(name, sess, units, bytes_per_unit):
    with sess as s:
        for _ in range(3):
            s.launch()
        s.collect()
        for _ in range(20):
            s.launch()
        r = s.collect()
        assert r.ok, (name, r)
    out[name] = {"units": units, "kernel_ms": round(r.kernel_ms, 4), "units_per_s": round(units / r.kernel_ms * 1e3),
                 "algorithmic_GBps": round(units * bytes_per_unit / r.kernel_ms / 1e6, 1),
                 "frac_of_8TBps": round(units * bytes_per_unit / r.kernel_ms / 1e6 / 8000, 4)}
    print(name, out[name], flush=True)


def ecc_leg():
    """ECC circuit verification (zk_ecc_verify, one-shot from host buffers; kernel_ms = HIP-event span of the pass): add rows/s at
    2^14 adds, mul rows/s at 2^12 muls, pairings/s at 2^10 two-pair pairing ops, on HIP and on the CPU backend (wall time)."""
    import time

    from tests import bn254_ref as b
    from zkevm_specs_amd import oneshot
    from zkevm_specs_amd.flatten import flatten_ecc_ops

    g = random.Random(4)
    F, F2 = b.Fq, b.Fq2
    pts = [b.multiply(b.G1, g.randrange(1, b.R), F) for _ in range(64)]
    adds = [(pts[i % 64], pts[(7 * i + 3) % 64], b.add(pts[i % 64], pts[(7 * i + 3) % 64], F)) for i in range(64)]
    scal = [g.randrange(1, b.R) for _ in range(64)]
    muls = [(pts[i], scal[i], b.multiply(pts[i], scal[i], F)) for i in range(64)]
    a = g.randrange(1, b.R)
    qa = b.multiply(b.G2, a, F2)
    q1, qa_w = (b.G2[0][1], b.G2[0][0], b.G2[1][1], b.G2[1][0]), (qa[0][1], qa[0][0], qa[1][1], qa[1][0])
    pairing = ([b.multiply(b.G1, a, F), b.neg(b.G1, F)], [q1, qa_w], 1)
    rk = 0x5EED % b.R
    for name, n, ops in (("ecc_add", 1 << 14, ([adds[i % 64] for i in range(1 << 14)], [], [])),
                         ("ecc_mul", 1 << 12, ([], [muls[i % 64] for i in range(1 << 12)], [])),
                         ("ecc_pairing_2pairs", 1 << 10, ([], [], [pairing] * (1 << 10)))):
        w = flatten_ecc_ops(*ops)
        rows = oneshot.ecc_assign(w, rk)
        ms = []
        for _ in range(4):
            res, st = oneshot.ecc_verify(w, rows, rk)
            assert res.fail_count == 0, (name, res.first_fail_code)
            ms.append(res.kernel_ms)
        kms = min(ms[1:])
        t0 = time.perf_counter()
        res_c, _ = oneshot.ecc_verify(w, rows, rk, device="cpu")
        cpu_s = time.perf_counter() - t0
        assert res_c.fail_count == 0
        out[name] = {"rows": n, "hip_kernel_ms": round(kms, 3), "hip_rows_per_s": round(n / kms * 1e3),
                     "cpu_wall_ms": round(cpu_s * 1e3, 1), "cpu_rows_per_s": round(n / cpu_s), "cpu_threads": os.cpu_count()}
        print(name, out[name], flush=True)


def ecc_pairing_ops(n_ops, n_pairs):
    """n_ops pairing ops of n_pairs pairs each whose product is 1 (n_pairs / 2 cancelling couples e(aG1, G2) e(-G1, aG2)) -> ops wire"""
    from tests import bn254_ref as b
    from zkevm_specs_amd.flatten import flatten_ecc_ops

    g = random.Random(4)
    a = g.randrange(1, b.R)
    qa = b.multiply(b.G2, a, b.Fq2)
    q1, qa_w = (b.G2[0][1], b.G2[0][0], b.G2[1][1], b.G2[1][0]), (qa[0][1], qa[0][0], qa[1][1], qa[1][0])
    pairing = ([b.multiply(b.G1, a, b.Fq), b.neg(b.G1, b.Fq)] * (n_pairs // 2), [q1, qa_w] * (n_pairs // 2), 1)
    return flatten_ecc_ops([], [], [pairing] * n_ops)


def ecc_session_leg():
    """ECC circuit in a resident session (zk_ecc_open, ops and rows in HBM; kernel_ms = HIP-event span of a pass: point rows, stage 1
    — one lane per (op, pair) —, stage 2 — one lane per op; mean of 10 passes after 2) beside the one-shot zk_ecc_verify on the same ops:
    2^10 ops of two pairs, and 8 ops of 16 pairs (a rank's handful of ops, the shape the per-pair split exists for)."""
    from zkevm_specs_amd import oneshot

    rk = 0x5EED % P
    for name, n_ops, n_pairs in (("ecc_pairing_2pairs", 1 << 10, 2), ("ecc_pairing_8x16pairs", 8, 16)):
        w = ecc_pairing_ops(n_ops, n_pairs)
        rows = oneshot.ecc_assign(w, rk)
        one = []
        for _ in range(4):
            res, _ = oneshot.ecc_verify(w, rows, rk)
            assert res.fail_count == 0, (name, res.first_fail_code)
            one.append(round(res.kernel_ms, 3))
        wd = {k: (to_dev(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) and k != "max_ok" else v) for k, v in w.items()}
        with engine.open_ecc(wd, to_dev(rows), rk) as s:
            for _ in range(2):
                s.launch()
            s.collect()
            for _ in range(10):
                s.launch()
            r = s.collect()
            assert r.ok, (name, r)
        out[name + "_session"] = {"ops": n_ops, "pairs_per_op": n_pairs, "session_kernel_ms": round(r.kernel_ms, 3),
                                  "oneshot_kernel_ms": one[1:], "session_over_oneshot": round(r.kernel_ms / min(one[1:]), 3),
                                  "ops_per_s": round(n_ops / r.kernel_ms * 1e3)}
        print(name + "_session", out[name + "_session"], flush=True)


def withdrawal_leg():
    """Withdrawal circuit at 2^16 rows: verification in a resident session (zk_withdrawal_open; kernel_ms = HIP-event span of a pass,
    bytes per row = its own row + the MPT row + the keccak row it reads, 8 + 12 + 5 cells), and the assignment (zk_withdrawal_assign,
    one-shot from host buffers: wall time including the staging copies, best of 5 after a warm-up)."""
    import time

    from tests.withdrawal_cases import big_witness
    from zkevm_specs_amd import oneshot

    n, rk = 1 << 16, 0x5EED % P
    w, inp = big_witness(n, seed=1, r=rk, device="cpu")
    run("withdrawal_verify", engine.open_withdrawal(w, rk), n, (8 + 12 + 5) * 32)
    walls = []
    for _ in range(6):
        t0 = time.perf_counter()
        rows, krows = oneshot.withdrawal_assign(inp, n, rk)
        walls.append(time.perf_counter() - t0)
    assert np.array_equal(rows, w["rows"]) and np.array_equal(krows, w["keccak"][1:])
    ms = min(walls[1:]) * 1e3
    out["withdrawal_assign"] = {"units": n, "oneshot_wall_ms": round(ms, 3), "units_per_s": round(n / ms * 1e3)}
    print("withdrawal_assign", out["withdrawal_assign"], flush=True)


def tx_assign_leg():
    """Tx circuit witness assignment (zk_tx_assign_open, inputs in HBM; kernel_ms = HIP-event span of a pass: sign hashes, key
    recovery, rows, units, keccak set) at 2^11 and 2^14 txs, with short calldata (< 40 bytes) and with mixed calldata (every fifth tx
    up to 600 bytes).  Signatures are random (r, s) with a curve point: each recovers some key, as a signed tx's does."""
    from tests.tx_assign_cases import random_inputs

    rk = 0x5EED % P
    for n in (1 << 11, 1 << 14):
        for label, long_every in (("short", 0), ("mixed", 5)):
            t = random_inputs(n, 3, chain_id=1, long_every=long_every, signed=False)
            td = {k: (to_dev(np.ascontiguousarray(v)) if k in engine.TX_ASSIGN_INPUTS else v) for k, v in t.items()}
            name = f"tx_assign_{n}_{label}"
            run(name, engine.open_tx_assign(td, rk), n, 8 * 32 + int(t["offsets"][-1]) / n)
            out[name]["calldata_bytes"] = int(t["offsets"][-1])


def sig_assign_leg():
    """Sig circuit witness assignment (zk_sig_assign_open, inputs in HBM; kernel_ms = HIP-event span of a pass: key recovery, units,
    keccak set, sig table, aux rows) at 2^11, 2^14 and 2^17 signatures — random (r, s) with a curve point, as the Tx leg's.  Then, in
    the same process, five alternating rounds of the 2^14 pass and the Tx assignment's 2^14 short-calldata pass (10 passes each after
    a warm-up): the Sig pass does strictly less work, so its median must not exceed the Tx pass's by more than the Tx pass's own
    spread over the rounds."""
    from tests.sig_assign_cases import random_curve_point_inputs
    from tests.tx_assign_cases import random_inputs

    rk = 0x5EED % P
    dev = lambda d, keys: {k: (to_dev(np.ascontiguousarray(v)) if k in keys and v is not None else v) for k, v in d.items()}  # noqa: E731
    for n in (1 << 11, 1 << 14, 1 << 17):
        sg = random_curve_point_inputs(n, 3)
        run(f"sig_assign_{n}", engine.open_sig_assign(dev(sg, engine.SIG_ASSIGN_INPUTS), rk), n, 4 * 32)
    n = 1 << 14
    sg, tx = random_curve_point_inputs(n, 3), random_inputs(n, 3, chain_id=1, long_every=0, signed=False)
    ms = {"sig_assign": [], "tx_assign": []}
    with engine.open_sig_assign(dev(sg, engine.SIG_ASSIGN_INPUTS), rk) as ss, engine.open_tx_assign(dev(tx, engine.TX_ASSIGN_INPUTS), rk) as ts:
        for rnd in range(6):
            for name, s in (("sig_assign", ss), ("tx_assign", ts)):
                for _ in range(10):
                    s.launch()
                r = s.collect()
                assert r.ok, (name, r)
                if rnd:  # round 0 warms up
                    ms[name].append(round(r.kernel_ms, 4))
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    spread = max(ms["tx_assign"]) - min(ms["tx_assign"])
    out["sig_vs_tx_assign_16384"] = {"sig_assign_kernel_ms": ms["sig_assign"], "tx_assign_kernel_ms": ms["tx_assign"], "sig_median_ms": med["sig_assign"],
                                     "tx_median_ms": med["tx_assign"], "tx_spread_ms": round(spread, 4),
                                     "sig_not_slower": bool(med["sig_assign"] <= med["tx_assign"] + spread)}
    print("sig_vs_tx_assign_16384", out["sig_vs_tx_assign_16384"], flush=True)


def exp_assign_leg():
    """Exp circuit witness assignment (zk_exp_assign_open, events in HBM; kernel_ms = HIP-event span of a pass: power chain + expansion,
    best-of-run mean of 20 passes after 3) at 2^12 events x 256-bit exponents and 2^16 events x 16-bit exponents; bytes per row = the 21
    + 11 cells written.  Beside it, in the same process: the State assignment's rows kernel regime (zk_state_assign_open at 2^20 ops,
    57 cells written per row) and the host path the assignment replaces (synth_block.exp_event_rows + rows_to_colmajor over the
    first 64 events of the 256-bit set, one core, scaled to the set)."""
    import time

    from tests.exp_assign_cases import random_events_wire
    from zkevm_specs_amd.synth_block import exp_event_rows
    from zkevm_specs_amd.wire import cells_to_ints, rows_to_colmajor

    for n, bits in ((1 << 12, 256), (1 << 16, 16)):
        ev = random_events_wire(11 + bits, n, bits)
        s = engine.open_exp_assign(to_dev(ev), 0)
        name = f"exp_assign_{n}x{bits}b"
        rows = s.n
        run(name, s, rows, (21 + 11) * 32)
        out[name]["events"] = n
    ev = random_events_wire(11 + 256, 1 << 12, 256)[:64]
    ints = cells_to_ints(ev)
    t0 = time.perf_counter()
    rows_h = []
    for k in range(64):
        c = ints[5 * k:5 * k + 5]
        rows_h += exp_event_rows(c[1] | c[2] << 128, c[3] | c[4] << 128, c[0])[0]
    rows_to_colmajor(rows_h, 21)
    dt = time.perf_counter() - t0
    out["exp_host_path_64x256b"] = {"rows": len(rows_h), "wall_ms": round(dt * 1e3, 1), "rows_per_s": round(len(rows_h) / dt),
                                    "scaled_to_4096_events_s": round(dt * 64, 2)}
    print("exp_host_path_64x256b", out["exp_host_path_64x256b"], flush=True)
    ops, op_flags, *_ = synth_state_ops(1 << 20, seed=2)
    run("state_assign_2p20", engine.open_state_assign(to_dev(ops), to_dev(op_flags)), 1 << 20, 57 * 32)


def pi_assign_leg():
    """PI circuit witness assignment (zk_pi_assign_open, public data in HBM) at MAX_TXS 2^11 / MAX_CALLDATA_BYTES 2^20 / MAX_WITHDRAWALS
    2^10 and at 2^9 / 2^17 / 2^8: open_ms = wall time of the open (staging-free: the inputs are device tensors; the domain check's
    read-back is its one wait), kernel_ms = HIP-event span of a pass (gas scan, inverses, bytes, digest beside scans + row writer,
    patch; mean of 20 passes after 3); bytes per row = the 24 cells written (768 B: the row writer's share of HBM; tables and
    constraints come on top).  Per-kernel times: one `rocprofv3 --kernel-trace --stats -- python3 tools/bench_row_kernels.py pi_assign`."""
    import time

    g = np.random.default_rng(8)
    words = lambda n, bits: (g.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)  # noqa: E731
                             & np.array([(1 << min(max(bits - 64 * k, 0), 62)) - 1 for k in range(4)], dtype=np.uint64))
    for mt, mc, mw in ((1 << 11, 1 << 20, 1 << 10), (1 << 9, 1 << 17, 1 << 8)):
        cuts = np.sort(g.integers(0, mc + 1, size=mt - 1)).astype(np.uint64)
        offsets = np.concatenate([[0], cuts, [mc]]).astype(np.uint64)
        calldata = g.integers(0, 256, size=mc, dtype=np.uint8) * (g.integers(0, 3, size=mc, dtype=np.uint8) == 0)
        txf = np.stack([words(mt, b) for b in (64, 256, 64, 160, 160, 256, 256)], axis=1)
        wd = np.stack([words(mw, b) for b in (0, 64, 160, 62)], axis=1)
        wd[:, 0, 0] = np.arange(mw, dtype=np.uint64)
        wd[:, 3, 0] |= np.uint64(1)
        block = np.stack([words(1, b)[0] for b in (256, 160, 256, 256, 64, 64, 64, 256, 256)])
        pd = {"chain_id": 1, "block": block, "state_root_prev": words(1, 256)[0], "block_hashes": words(256, 256), "tx_fields": txf,
              "to_is_none": np.zeros(mt, dtype=np.uint32), "calldata": calldata, "offsets": offsets, "withdrawals": wd,
              "max_txs": mt, "max_calldata_bytes": mc, "max_withdrawals": mw}
        pdd = {k: (to_dev(np.ascontiguousarray(v)) if k in engine.PI_ASSIGN_INPUTS else v) for k, v in pd.items()}
        engine.open_pi_assign(pdd).close()  # (warm-up: arena, side stream)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s = engine.open_pi_assign(pdd)
        open_ms = (time.perf_counter() - t0) * 1e3
        name = f"pi_assign_{mt}x{mc}x{mw}"
        run(name, s, s.n, 24 * 32)
        out[name]["open_wall_ms"] = round(open_ms, 3)


if sys.argv[1:] == ["pi_assign"]:
    pi_assign_leg()
    print(json.dumps(out))
    sys.exit(0)
if sys.argv[1:] == ["exp_assign"]:
    exp_assign_leg()
    print(json.dumps(out))
    sys.exit(0)
if sys.argv[1:] == ["sig_assign"]:
    sig_assign_leg()
    print(json.dumps(out))
    sys.exit(0)
if sys.argv[1:] == ["tx_assign"]:
    tx_assign_leg()
    print(json.dumps(out))
    sys.exit(0)
if sys.argv[1:] == ["withdrawal"]:
    withdrawal_leg()
    print(json.dumps(out))
    sys.exit(0)
if sys.argv[1:] == ["ecc"]:
    ecc_leg()
    ecc_session_leg()
    print(json.dumps(out))
    sys.exit(0)

rng = random.Random(1)
r = rng.randrange(P)
k = int(os.environ.get("LOGN", "20"))
codes = [bytes(rng.getrandbits(8) for _ in range(24000)) for _ in range((1 << k) // 24576)]
cols, keccak = synth_bytecode_witness(codes, k, r)
run("bytecode", engine.open_bytecode(cols, keccak, r), 1 << k, 12 * 32)
cols = synth_exp_witness(1 << k, seed=8)
run("exp", engine.open_exp(cols), 1 << k, 21 * 32)
n_tx = 1 << min(k, 17)
w = synth_tx_witness(n_tx, r, seed=4)
run("tx_sign", engine.open_sign(w, r, False), n_tx,
    8 * 32 + 288 + 2 * 5 * 32)
# Copy circuit: events expanded on the device (zk_copy_assign), then evaluated from the same HBM buffers (zk_copy_open)
from zkevm_specs_amd.synth import synth_copy_events
for kk in sorted({15, min(k, 19)}):
    ce = synth_copy_events(1 << kk, seed=6)
    ev, fl, da, of = to_dev(ce["events"]), to_dev(ce["flags"]), torch.from_numpy(ce["data"].view(np.int16)).cuda(), to_dev(ce["offsets"])
    n_rows, n_table, n_rw = engine.copy_assign_sizes(ce["events"], ce["flags"], ce["data"], ce["offsets"])
    c_rows = torch.empty((20, n_rows, 4), dtype=torch.int64, device="cuda")
    c_rf = torch.empty(n_rows, dtype=torch.int32, device="cuda")
    c_rw = torch.empty((n_rw, 14, 4), dtype=torch.int64, device="cuda")
    c_rwf = torch.empty(n_rw, dtype=torch.int32, device="cuda")
    # per output row: 20 circuit cells + the RW row of every second row, written; the events and bytes read are negligible
    run(f"copy_assign_2p{kk}", engine.open_copy_assign(ev, fl, da, of, ce["r"], c_rows, c_rf, None, c_rw, c_rwf), n_rows, 20 * 32 + 4 + 7 * 32)
    run(f"copy_rows_2p{kk}", engine.open_copy(c_rows, c_rf, ce["r"], c_rw, c_rwf, to_dev(ce["bytecode"]), to_dev(ce["tx"]), to_dev(ce["tx_flags"])),
        n_rows, 20 * 32 + 14 * 32)
# keccak table generation (integer-ALU bound: ~3.6 k VALU ops per 136-byte block + ~25 per RLC byte)
n_keys = 1 << k
nrng = np.random.default_rng(6)
keys = torch.from_numpy(nrng.integers(0, 256, size=n_keys * 64, dtype=np.uint8)).cuda()
offs = torch.arange(0, (n_keys + 1) * 64, 64, dtype=torch.int64, device="cuda")
rows_dev = torch.zeros((n_keys, 5, 4), dtype=torch.int64, device="cuda")
run("keccak_table_64B", engine.open_keccak(keys, offs, r, engine.KECCAK_MODE_TABLE, rows_dev=rows_dev), n_keys, 64 + 160)
n_codes = 1 << max(k - 8, 4)
code_bytes = torch.from_numpy(nrng.integers(0, 256, size=n_codes * 24576, dtype=np.uint8)).cuda()
offs = torch.arange(0, (n_codes + 1) * 24576, 24576, dtype=torch.int64, device="cuda")
rows_dev = torch.zeros((n_codes, 5, 4), dtype=torch.int64, device="cuda")
run("keccak_table_24KiB", engine.open_keccak(code_bytes, offs, r, engine.KECCAK_MODE_CIRCUIT, rows_dev=rows_dev), n_codes, 24576 + 160)
# State witness assignment (HBM-bound: 12 slots read + 57 cells written per op; the mock-MPT index, scans and MPT rows ride along)
for kk in sorted({16, k}):
    ops, oflags, *_ = synth_state_ops(1 << kk, seed=2)
    d_ops, d_oflags = to_dev(ops), to_dev(oflags)
    d_rows = torch.empty((57, 1 << kk, 4), dtype=torch.int64, device="cuda")
    d_rflags = torch.empty(1 << kk, dtype=torch.int32, device="cuda")
    d_mpt = torch.empty((1 << kk, 12, 4), dtype=torch.int64, device="cuda")
    run(f"state_assign_2p{kk}", engine.open_state_assign(d_ops, d_oflags, d_rows, d_rflags, d_mpt), 1 << kk, (12 + 57) * 32 + 8)
# Bytecode witness assignment: the unrolled bytecode table of 2^17 / 24,576-byte contracts -> the circuit's 2^17 rows (HBM: 6 cells read, 12 written)
from zkevm_specs_amd.wire import rows_to_rowmajor  # noqa: E402


def unrolled_bytecode_table(codes_):
    """BytecodeTableRows of Bytecode.table_assignments() in wire form (Header row, then a Byte row per byte with is_code)"""
    rows_, offs_, lens_ = [], [0], []
    for ci, code in enumerate(codes_):
        lo, hi = 0x1000 + ci, 0x77
        rows_.append([lo, hi, 1, 0, 0, len(code)])
        left = 0
        for idx, b in enumerate(code):
            is_code = left == 0
            rows_.append([lo, hi, 2, idx, int(is_code), b])
            left = (b - 0x5F if 0x60 <= b <= 0x7F else 0) if is_code else left - 1
        offs_.append(len(rows_))
        lens_.append(len(code))
    return rows_to_rowmajor(rows_, 6), np.array(offs_, dtype=np.uint64), np.array(lens_, dtype=np.uint64)


kb = 17
b_codes = [bytes(rng.getrandbits(8) for _ in range(24000)) for _ in range(((1 << kb) // 24576))]
ub_rows, ub_off, ub_len = unrolled_bytecode_table(b_codes)
d_bc = torch.empty((12, 1 << kb, 4), dtype=torch.int64, device="cuda")
run(f"bytecode_assign_2p{kb}", engine.open_bytecode_assign(to_dev(ub_rows), to_dev(ub_off), to_dev(ub_len), kb, r, rows_dev=d_bc), 1 << kb, (6 + 12) * 32)
# RW table -> State witness in one session (re-keying + radix sort + assignment): the 2^18-step block trace's RW table
from zkevm_specs_amd.synth_block import synth_block_trace  # noqa: E402
wb = synth_block_trace(1 << 18, seed=5)
n_rw = int(wb["rw"].shape[0])
f_rows, f_fl = torch.empty(57 * 4 * (n_rw + 1), dtype=torch.int64, device="cuda"), torch.empty(n_rw + 1, dtype=torch.int32, device="cuda")
f_mpt = torch.empty(48 * (n_rw + 1), dtype=torch.int64, device="cuda")
d_rw, d_rwf = to_dev(wb["rw"]), to_dev(wb["rw_flags"])
run("state_assign_from_rw_2p18", engine.open_state_assign_from_rw(d_rw, d_rwf, f_rows, f_fl, f_mpt), n_rw, (14 + 57) * 32 + 8)
d_ops_b, d_of_b = torch.empty(48 * (n_rw + 1), dtype=torch.int64, device="cuda"), torch.empty(n_rw + 1, dtype=torch.int32, device="cuda")
run("state_ops_from_rw_2p18", engine.open_state_ops_from_rw(d_rw, d_rwf, d_ops_b, d_of_b), n_rw, (14 + 12) * 32 + 8)
# secp256k1 ECDSA verification (integer-ALU bound: ~8.6 k 256-bit Montgomery products per signature)
from zkevm_specs_amd.synth import synth_signatures
n_sig = 1 << 14
sigs = synth_signatures(n_sig, 9)
packed = np.frombuffer(b"".join(x.to_bytes(32, "little") + y.to_bytes(32, "little") + z.to_bytes(32, "big") + rr.to_bytes(32, "little") +
                                ss.to_bytes(32, "little") for x, y, z, rr, ss in sigs), dtype=np.uint8).reshape(n_sig, 5, 32).copy()
for reps in (1, 2, 4, 8):
    d = torch.from_numpy(np.tile(packed, (reps, 1, 1))).cuda()
    run(f"ecdsa_verify_{n_sig * reps}", engine.open_ecdsa(d), n_sig * reps, 160 + 4)
ecc_leg()
ecc_session_leg()
print(json.dumps(out))
