"""The fixed list of calls whose marshalling is recorded (tools/gen_golden_marshalling.py -> tests/golden/marshalling_calls_*.json) and
replayed (tests/test_wire_marshalling_*.py): the seven wire-struct assignment families and the State-from-RW / from-trace group, through
engine's sessions and oneshot's entries.  A case's record is the library calls it made (tests/marshalling_proxy.py) and what it returned
or raised.  The cases are the smallest at which the marshalling can go wrong; none is new to the library (the suites make the same calls)
or it is refused in Python before the library is reached."""
import hashlib
import random
from collections import namedtuple

import numpy as np

from tests import bytecode_code_cases, ecc_calls_cases as EC, pi_assign_cases, sig_assign_cases, state_trace_cases as sc, trace_witness_cases
from tests import trace_witness_ref, tx_assign_cases
from tests.marshalling_proxy import describe, recording
from zkevm_specs_amd import block_tables as bt, ecc_circuit, engine, oneshot, pi_circuit
from zkevm_specs_amd.engine import Result

R = 0x1F2E3D4C5B6A79880796A5B4C3D2E1F00112233445566778899AABBCCDDEEFF
# name: the family; inputs(n) -> its input dict over n items (host arrays); arrays: the dict's array members in ABI order; shapes(x) ->
# output name -> (shape or None, dtype); open(x, outs, device) / oneshot(x, device) / sizes(x, device) or None / args(x, randomness) or
# None: the engine's and oneshot's own functions; counts: the session's count readers; subset: names for read(names=...) or None;
# variants: (label, inputs) with an optional input left out or given; empty: inputs of which one output is empty, or None
Family = namedtuple("Family", "name inputs arrays shapes open oneshot sizes args counts subset variants empty")


# ---- the inputs ------------------------------------------------------------------------------------------------------------------------------
def tx_inputs(n):
    return tx_assign_cases.random_inputs(n, 1, signed=False)


def sig_inputs(n):
    x = sig_assign_cases.random_curve_point_inputs(n, 2)
    rng = random.Random(3)
    return dict(x, addr=sig_assign_cases.words([rng.getrandbits(160) for _ in range(n)]), expect_valid=np.ones(n, dtype=np.uint32))


def ecc_inputs(n):
    """one add, then a mul, then a one-pair pairing"""
    return ecc_circuit.ecc_calls_wire([(EC.A, EC.B7)] * min(n, 1), [(EC.A, 5)] * (n > 1), [([EC.G], [EC.Q1])] * (n > 2))


def pi_inputs(n):
    rng = random.Random(4)
    return pi_circuit.public_data_inputs(pi_assign_cases.rand_public_data(rng, n, [2, 0, 3][:n], 1), 3, 8, 2)


def code_inputs(n, k=6):
    rng = random.Random(5)
    code, offsets = bytecode_code_cases.pack([bytes(rng.randrange(256) for _ in range(3 + i)) for i in range(n)])
    return {"code": code, "offsets": offsets, "k": k}


def block_inputs(n):
    from tests import block_tables_cases as bc

    rng = random.Random(6)
    return bt.raw_block_data(bc._block(rng, 1, number=9), [bc._tx(rng, 1 + i, bc._data(rng, 2 * i)) for i in range(n)], bc._withdrawals(rng, 1))


def trace_inputs(n):
    rec = dict(trace_witness_cases.mutable(f"rw_{n}_a")) if n else {k: np.zeros(0, np.uint32 if k == "head" else np.uint64) for k in engine.TRACE_INPUTS[:5]}
    rec.update(rw_counter=None, rw_base=1, steps=np.array(trace_witness_cases.directed("steps_2")["steps"][:min(n, 2)]))
    if not n:
        rec["pool"] = np.zeros((0, 4), np.uint64)
    return rec


def _without(x, *names, **kw):
    return dict({k: (None if k in names else v) for k, v in x.items()}, **kw)


def _code_shapes(x):
    return {k: (shp, np.uint64) for k, shp in engine.bytecode_from_code_shapes(int(x["code"].shape[0]), int(x["offsets"].shape[0]) - 1, x["k"]).items()}


def _code_open(x, outs, device):
    return engine.open_bytecode_from_code(x["code"], x["offsets"], x["k"], R, table_dev=outs.get("table"), rows_dev=outs.get("rows"),
                                          keccak_dev=outs.get("keccak"), device=device)


def _block_shapes(x):
    return engine.evm_tables_from_block_shapes(engine._rows(x["tx_fields"]), x["calldata"].shape[0], engine._rows(x.get("history_hashes")),
                                               engine._rows(x.get("withdrawals")), x.get("block") is not None)


def families():
    tx3, sig3, tr3, bl3 = tx_inputs(3), sig_inputs(3), trace_inputs(3), block_inputs(3)
    empty_calldata = dict(tx3, calldata=np.zeros(0, np.uint8), offsets=np.zeros(4, np.uint64))
    return [
        Family("tx", tx_inputs, engine.TX_ASSIGN_INPUTS, lambda x: engine.tx_assign_shapes(int(x["fields"].shape[0]), x["max_txs"], x["max_calldata_bytes"]),
               lambda x, outs, device: engine.open_tx_assign(x, R, outs=outs or None, device=device), lambda x, device: oneshot.tx_assign(x, R, device=device),
               None, lambda x, r, outs=None: engine._tx_assign_args(x, r, outs), ("n_keccak",), None, [("empty_calldata", empty_calldata)], None),
        Family("sig", sig_inputs, engine.SIG_ASSIGN_INPUTS, lambda x: engine.sig_assign_shapes(int(x["fields"].shape[0])),
               lambda x, outs, device: engine.open_sig_assign(x, R, outs=outs or None, device=device), lambda x, device: oneshot.sig_assign(x, R, device=device),
               None, lambda x, r, outs=None: engine._sig_assign_args(x, r, outs), ("n_keccak", "n_sig_rows"), None,
               [("without_addr", _without(sig3, "addr")), ("without_expect_valid", _without(sig3, "expect_valid"))], sig_inputs(0)),
        Family("ecc_calls", ecc_inputs, engine.ECC_CALLS_INPUTS,
               lambda x: engine.ecc_calls_shapes(int(x["add_in"].shape[0]), int(x["mul_in"].shape[0]), int(x["pair_off"].shape[0]) - 1),
               lambda x, outs, device: engine.open_ecc_from_calls(x, R % EC.b.FR, outs=outs or None, device=device),
               lambda x, device: oneshot.ecc_from_calls(x, R % EC.b.FR, device=device), None, lambda x, r, outs=None: engine._ecc_calls_args(x, r, outs),
               ("n_table_rows",), None, [], ecc_inputs(1)),
        Family("pi", pi_inputs, engine.PI_ASSIGN_INPUTS,
               lambda x: engine.pi_assign_shapes(x["max_txs"], x["max_calldata_bytes"], x["max_withdrawals"], x["calldata"].shape[0]),
               lambda x, outs, device: engine.open_pi_assign(x, outs=outs or None, device=device), lambda x, device: oneshot.pi_assign(x, device=device),
               engine.pi_assign_sizes, lambda x, r, outs=None: engine._pi_assign_args(x, r, r, outs), (), ("gas", "keccak"), [], None),
        Family("code", code_inputs, ("code", "offsets"), _code_shapes, _code_open,
               lambda x, device: oneshot.bytecode_from_code(x["code"], x["offsets"], x["k"], R, device=device), None,
               lambda x, r, outs=None: engine._bytecode_from_code_args(x["code"], x["offsets"], x["k"], r, outs), (), None, [("k_0", code_inputs(3, 0))],
               code_inputs(0)),
        Family("block_tables", block_inputs, engine.BLOCK_TABLES_INPUTS, _block_shapes,
               lambda x, outs, device: engine.open_evm_tables_from_block(x, outs=outs or None, device=device),
               lambda x, device: oneshot.evm_tables_from_block(x, device=device), engine.evm_tables_from_block_sizes,
               lambda x, r, outs=None: engine._evm_tables_from_block_args(x, outs), (), ("block", "tx_flags"),
               [("without_block", _without(bl3, "block", "history_hashes")), ("without_history_hashes", _without(bl3, "history_hashes")),
                ("without_withdrawals", _without(bl3, "withdrawals")),
                ("empty_calldata", dict(bl3, calldata=np.zeros(0, np.uint8), offsets=np.zeros(4, np.uint64)))], _without(bl3, "withdrawals")),
        Family("trace", trace_inputs, engine.TRACE_INPUTS, lambda x: engine.evm_witness_from_trace_shapes(engine._rows(x.get("head")), engine._rows(x.get("steps"))),
               lambda x, outs, device: engine.open_evm_witness_from_trace(x, outs=outs or None, device=device),
               lambda x, device: oneshot.evm_witness_from_trace(x, device=device), engine.evm_witness_from_trace_sizes,
               lambda x, r, outs=None: engine._evm_witness_from_trace_args(x, outs), (), ("steps",),
               [("rw_base_7", dict(tr3, rw_base=7)), ("with_rw_counter", dict(tr3, rw_counter=np.array([5, 9, 12], dtype=np.uint64))),
                ("without_steps", _without(tr3, "steps")), ("without_prev", _without(tr3, "prev"))], _without(tr3, "steps")),
    ]


# ---- what a case returns, in a comparable form ----------------------------------------------------------------------------------------------
def canon(x):
    if isinstance(x, Result):
        return {"fail_count": x.fail_count, "first_fail_row": x.first_fail_row, "first_fail_code": x.first_fail_code, "rows_evaluated": x.rows_evaluated}
    if hasattr(x, "is_cuda"):
        x = x.cpu().numpy()
    if isinstance(x, np.ndarray):
        return [list(x.shape), str(x.dtype), hashlib.sha1(np.ascontiguousarray(x).tobytes()).hexdigest()]
    if isinstance(x, dict):
        return {str(k): canon(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [canon(v) for v in x]
    if isinstance(x, (np.integer, bool)):
        return int(x)
    if x is None or isinstance(x, (int, str)):
        return x
    return describe(x)


def session(f, x, device, outs=None, names=None):
    """open, one pass, every read the session has"""
    with f.open(x, outs or {}, device) as s:
        got = {"n": s.n, "result": s.run(), "read": s.read(), "status": s.read_status()}
        got.update({c: getattr(s, c)() for c in f.counts})
        if names:
            got["subset"] = s.read(names=names)
    if outs:
        got["outs"] = outs
    return got


def _first(f, x, change):
    """`x` with its first input array replaced by change(array)"""
    k = f.arrays[0]
    return dict(x, **{k: change(x[k])})


def _other_width(a):
    return a.astype(np.uint16 if a.dtype.itemsize != 2 else np.uint8)


def _strided(a):
    return np.repeat(a, 2, axis=0)[::2]


def _host_out(f, x, change=lambda a: a):
    k, (shp, dt) = next((k, v) for k, v in f.shapes(x).items() if v[0] is not None)
    return {k: change(np.zeros(shp, dtype=dt))}


def family_cases_cpu(f):
    cases, x3 = [], f.inputs(3)
    both = lambda label, x: cases.extend([(f"{f.name}:{label}:session", lambda: session(f, x, "cpu")),  # noqa: E731
                                          (f"{f.name}:{label}:oneshot", lambda: f.oneshot(x, "cpu"))])
    for n in (0, 1, 3):
        both(f"{n}_items", f.inputs(n))
    for label, x in f.variants:
        both(label, x)
    both("strided_input", _first(f, x3, _strided))
    both("input_width", _first(f, x3, _other_width))
    both("input_shape", _first(f, x3, lambda a: np.expand_dims(a, -1)))
    cases.append((f"{f.name}:output_width", lambda: session(f, x3, "cpu", _host_out(f, x3, _other_width))))
    cases.append((f"{f.name}:output_shape", lambda: session(f, x3, "cpu", _host_out(f, x3, lambda a: np.expand_dims(a, -1)))))
    cases.append((f"{f.name}:host_outs", lambda: session(f, x3, "cpu", _host_out(f, x3))))
    if f.sizes:
        cases.append((f"{f.name}:sizes", lambda: f.sizes(x3, device="cpu")))
    if f.subset:
        cases.append((f"{f.name}:read_subset", lambda: session(f, x3, "cpu", names=f.subset)))
    return cases


# ---- the State circuit from an RW table / from trace records ---------------------------------------------------------------------------------
def state_records(n):
    return sc.records(sc.random_ops(n, 12, True) if n else [], base=3)


def rw_table(rec):
    w = trace_witness_ref.model({**rec, "steps": np.zeros((0, 13), np.uint64)})
    return w["rw"], w["rw_flags"]


def _run_read(s, read=True):
    with s:
        got = {"n": s.n, "n_ops": getattr(s, "n_ops", None), "result": s.run(), "status": s.read_status()}
        if read:
            got["read"] = s.read()
    return got


def state_cases(device, to_dev=lambda a: a):
    cases = []
    for n in ((0, 1, 65) if device == "cpu" else (1, 65)):  # (no ops at all: host arrays only, where the refusal is the CPU backend's)
        rec = state_records(n)
        rw, fl = rw_table(rec)
        d_rec, d_rw, d_fl = {k: to_dev(v) if hasattr(v, "dtype") else v for k, v in rec.items()}, to_dev(rw), to_dev(fl)

        def add(label, rw_form, trace_form, n=n, d_rw=d_rw, d_fl=d_fl, d_rec=d_rec):  # (bound per size: the thunks run after the loop)
            cases.append((f"state:{n}_ops:{label}_from_rw", lambda: rw_form(d_rw, d_fl)))
            cases.append((f"state:{n}_ops:{label}_from_trace", lambda: trace_form(d_rec)))

        add("open_verify", lambda a, b: _run_read(engine.open_state_verify_from_rw(a, b, device=device), False),
            lambda t: _run_read(engine.open_state_verify_from_trace(t, device=device), False))
        add("open_ops", lambda a, b: _run_read(engine.open_state_ops_from_rw(a, b, device=device)),
            lambda t: _run_read(engine.open_state_ops_from_trace(t, device=device)))
        for compact in (False, True):
            add(f"open_assign_compact_{int(compact)}", lambda a, b, c=compact: _run_read(engine.open_state_assign_from_rw(a, b, device=device, compact=c)),
                lambda t, c=compact: _run_read(engine.open_state_assign_from_trace(t, device=device, compact=c)))
        if device == "cpu":
            add("oneshot_verify", lambda a, b: oneshot.state_verify_from_rw(a, b, device=device), lambda t: oneshot.state_verify_from_trace(t, device=device))
            add("oneshot_ops", lambda a, b: oneshot.state_ops_from_rw(a, b, device=device), lambda t: oneshot.state_ops_from_trace(t, device=device))
            for compact in (False, True):
                cases.append((f"state:{n}_ops:oneshot_assign_compact_{int(compact)}_from_trace",
                              lambda t=rec, c=compact: oneshot.state_assign_from_trace(t, device=device, compact=c)))
        if n == 65:  # flat output buffers: exact, and one entry too short (refused in Python)
            for short in (0, 1):
                def flat(entries, dtype, short=short, n=n):
                    return to_dev(np.zeros(entries * (n + 1) - short, dtype=dtype))

                def outs_back(s, *bufs):
                    return dict(_run_read(s), outs=bufs)

                cases.append((f"state:flat_ops_short_{short}_from_rw", lambda flat=flat, d_rw=d_rw, d_fl=d_fl, d_rec=d_rec: (lambda o, f_: outs_back(
                    engine.open_state_ops_from_rw(d_rw, d_fl, ops_dev=o, op_flags_dev=f_, device=device), o, f_))(flat(48, np.uint64), flat(1, np.uint32))))
                cases.append((f"state:flat_ops_short_{short}_from_trace", lambda flat=flat, d_rw=d_rw, d_fl=d_fl, d_rec=d_rec: (lambda o, f_: outs_back(
                    engine.open_state_ops_from_trace(d_rec, ops_dev=o, op_flags_dev=f_, device=device), o, f_))(flat(48, np.uint64), flat(1, np.uint32))))
                cases.append((f"state:flat_mpt_short_{short}_from_rw", lambda flat=flat, d_rw=d_rw, d_fl=d_fl, d_rec=d_rec: (lambda m: outs_back(
                    engine.open_state_assign_from_rw(d_rw, d_fl, mpt_dev=m, device=device), m))(flat(48, np.uint64))))
                cases.append((f"state:flat_mpt_short_{short}_from_trace", lambda flat=flat, d_rw=d_rw, d_fl=d_fl, d_rec=d_rec: (lambda m: outs_back(
                    engine.open_state_assign_from_trace(d_rec, mpt_dev=m, device=device), m))(flat(48, np.uint64))))
    return cases


# ---- device tensors ---------------------------------------------------------------------------------------------------------------------------
def to_device(a):
    import torch

    if a is None:
        return None
    view = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize]
    return torch.from_numpy(np.array(a).view(view)).cuda()


def family_cases_hip(f):
    x = f.inputs(3)
    d_x = {k: to_device(v) if hasattr(v, "dtype") else v for k, v in x.items()}
    shapes = {k: v for k, v in f.shapes(x).items() if v[0] is not None}

    def buffers(names):
        return {k: to_device(np.zeros(shapes[k][0], dtype=shapes[k][1])) for k in names}

    def strided():
        k, (shp, dt) = next((k, v) for k, v in shapes.items() if int(np.prod(v[0])) > 1)
        return {k: to_device(np.zeros(tuple(shp[:-1]) + (2 * shp[-1],), dtype=dt))[..., ::2]}

    cases = [(f"{f.name}:outs_all", lambda: session(f, d_x, None, buffers(list(shapes)))),
             (f"{f.name}:outs_some", lambda: session(f, d_x, None, buffers(list(shapes)[::2]))),
             (f"{f.name}:outs_none", lambda: session(f, d_x, None)),
             (f"{f.name}:strided_output", lambda: session(f, d_x, None, strided()))]
    # what the argument builder alone makes of two forms (the library is not called with them):
    if f.name not in ("block_tables", "trace"):  # host randomness beside device inputs
        cells = np.frombuffer(int(R % EC.b.FR).to_bytes(32, "little"), dtype="<u8").copy()
        cases.append((f"{f.name}:host_randomness", lambda: [describe(v) for v in f.args(d_x, cells)[:3]]))
    if f.empty is not None:  # an empty output with a buffer given: a zero-row view of an allocation, so its own pointer is not null
        d_e = {k: to_device(v) if hasattr(v, "dtype") else v for k, v in f.empty.items()}
        e_shapes = {k: v for k, v in f.shapes(f.empty).items() if v[0] is not None}
        assert any(v[0][0] == 0 for v in e_shapes.values()), f.name

        def views():
            return {k: to_device(np.zeros((max(shp[0], 1),) + tuple(shp[1:]), dtype=dt))[: shp[0]] for k, (shp, dt) in e_shapes.items()}

        cases.append((f"{f.name}:empty_output", lambda: [describe(v) for v in f.args(d_e, R % EC.b.FR, views())[:3]]))
    return cases


def all_cases(device):
    """[(name, thunk)] for `device` = "cpu" (host arrays through the CPU backend) or None (device tensors through the HIP library)"""
    fams = families()
    if device == "cpu":
        return [c for f in fams for c in family_cases_cpu(f)] + state_cases("cpu")
    return [c for f in fams for c in family_cases_hip(f)] + state_cases(None, to_device)


def run(device):
    """-> {case name: {"calls": [[entry, [argument, ...]], ...], "returned": ... or "raised": [class name, message]}}"""
    cases, out = all_cases(device), {}
    with recording(device) as rec:
        for name, thunk in cases:
            rec.log = []
            try:
                entry = {"returned": canon(thunk())}
            except Exception as e:  # noqa: BLE001 (a refusal is part of the record)
                entry = {"raised": [type(e).__name__, str(e)]}
            assert name not in out, name
            out[name] = dict(calls=rec.log, **entry)
    return out
