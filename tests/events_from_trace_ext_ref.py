"""A plain-Python model of zk_events_from_trace_ext* (include/zkevm_hip.h), written from the entry's description: the copy events of
BeginTx, RETURN / REVERT and DATACOPY steps beside the events zk_events_from_trace derives (those come from the model of that entry,
tests/events_from_trace_ref.py).  Integers are Python ints; nothing here shares code with the library.

derive(rec, codes, hashes) -> dict(copy_events, copy_flags, copy_src_ref, copy_dst_ref, copy_step, exp_events, exp_step, status) of numpy
arrays in the entry's layouts; capacities(rec) -> (copy capacity, EXP capacity)."""
import numpy as np

from tests import events_from_trace_ref as ref
from zkevm_specs_amd.evm_tables import AccountFieldTag, CallContextFieldTag as CC, ExecutionState as ES, Target

LIMIT = ref.LIMIT
BYTECODE, MEMORY, TX_CALLDATA, RLC_ACC = ref.BYTECODE, ref.MEMORY, ref.TX_CALLDATA, ref.RLC_ACC
DST_WORD = 2  # flag bit 1
NEW_STATES = {int(ES[k]) for k in ("BeginTx", "RETURN", "DATACOPY")}
STILL_UNSUPPORTED = {int(ES[k]) for k in ("CREATE", "CREATE2", "CALL_OP")}
PAIR_STATES = {int(ES.BeginTx), int(ES.DATACOPY)}
M128 = (1 << 128) - 1
code_of = ref.code_of


def capacities(rec):
    steps = np.asarray(rec["steps"], dtype=np.uint64).reshape(-1, 13)
    n = len(steps)
    return n + sum(1 for w0 in steps[:, 0].tolist() if w0 & 0xFF in PAIR_STATES), n


def _read(ops, rwc, k, kind, ident, where, write=False):
    """op k of a step: (site, value).  kind "stack": where is the address; "context" / "account": the field tag"""
    op = ops.get(rwc + k) if rwc + k < 1 << 64 else None
    if op is None:
        return 1, None
    ok = bool(op["write"]) == write
    if kind == "stack":
        ok = ok and op["tag"] == Target.Stack and op["id"] == ident and op["addr"] == where
    elif kind == "context":
        ok = ok and op["tag"] == Target.CallContext and op["id"] == ident and op["addr"] == where
    else:
        ok = ok and op["tag"] == Target.Account and op["field"] == where
    return (0, op["value"]) if ok else (2, None)


def _read_all(ops, rwc, wanted):
    """the ops in ascending k -> (site of the first failure, values)"""
    vals = []
    for w in wanted:
        site, v = _read(ops, rwc, *w)
        if site:
            return site, None
        vals.append(v)
    return 0, vals


def _event(src_id, src_tag, dst_id, dst_tag, src_addr, src_end, dst_addr, length, rwc):
    return [src_id & M128, src_id >> 128, src_tag, dst_id & M128, dst_id >> 128, dst_tag, src_addr, src_end, dst_addr, length, 0, rwc]


def new_step_events(step, nxt, ops, first_index):
    """a step of one of the three states -> (status, [(cells[12], flag, src_ref, dst_ref), ...]); nxt: the next record or None"""
    state, root, create = step[0] & 0xFF, (step[0] >> 8) & 1, (step[0] >> 9) & 1
    rwc, call_id, sp = step[1], step[2], step[4]
    if state == int(ES.RETURN):
        if root and not create:
            return 0, []
        if not create and nxt is None:
            return code_of(5), []
        wanted = [(1, "stack", call_id, sp), (2, "stack", call_id, sp + 1)]
        if create:
            wanted.append((4, "account", None, int(AccountFieldTag.CodeHash), True))
        else:
            wanted += [(3, "context", call_id, int(CC.ReturnDataOffset)), (4, "context", call_id, int(CC.ReturnDataLength))]
        site, v = _read_all(ops, rwc, wanted)
        if site:
            return code_of(site), []
        off, length = v[0], v[1]
        if create and length == 0:
            return 0, []
        ints = [rwc, off, length, off + length, rwc + 5] + ([] if create else [v[2], v[3]])
        if any(x >= LIMIT for x in ints):
            return code_of(3), []
        if create:
            h = v[2]
            if h not in first_index:
                return code_of(4), []
            return 0, [(_event(call_id, MEMORY, h, BYTECODE, off, off + length, 0, length, rwc + 5), DST_WORD, 0, first_index[h])]
        return 0, [(_event(call_id, MEMORY, nxt[2], MEMORY, off, off + length, v[2], min(length, v[3]), rwc + 5), 0, 0, 0)]
    if state == int(ES.DATACOPY):
        fields = (CC.CallerId, CC.CallDataOffset, CC.CallDataLength, CC.ReturnDataOffset, CC.ReturnDataLength)
        site, v = _read_all(ops, rwc, [(k + 1, "context", call_id, int(f)) for k, f in enumerate(fields)])
        if site:
            return code_of(site), []
        c, cdo, cdl, rdo, rdl = v
        first_len = rdo + rdl
        inc = first_len + min(first_len, cdl)  # the first event's writes, and its reads below src_addr_end
        if any(x >= LIMIT for x in (rwc, c, cdo, cdl, rdo, rdl, cdo + cdl, first_len, rwc + 6 + inc)):
            return code_of(3), []
        return 0, [(_event(c, MEMORY, c, MEMORY, cdo, cdo + cdl, rdo, first_len, rwc + 6), 0, 0, 0),
                   (_event(c, MEMORY, call_id, MEMORY, cdo, cdo + cdl, 0, rdl, rwc + 6 + inc), 0, 0, 0)]
    # BeginTx
    if nxt is None:
        return code_of(5), []
    if not ((nxt[0] >> 9) & 1 and nxt[1] == rwc + 23):
        return 0, []
    site, v = _read_all(ops, rwc, [(0, "context", rwc, int(CC.TxId)), (14, "context", rwc, int(CC.CallDataLength)), (22, "context", rwc, int(CC.CodeHash))])
    if site:
        return code_of(site), []
    tx, n, h = v
    if n == 0:
        return code_of(5), []
    if any(x >= LIMIT for x in (rwc, tx, n, rwc + 10)) or tx == 0 or tx - 1 >= 1 << 32:
        return code_of(3), []
    if h not in first_index:
        return code_of(4), []
    return 0, [(_event(tx, TX_CALLDATA, rwc, RLC_ACC, 0, n, 0, n, rwc + 10), 0, tx - 1, 0),
               (_event(tx, TX_CALLDATA, h, BYTECODE, 0, n, 0, n, rwc + 10), DST_WORD, tx - 1, first_index[h])]


def derive(rec, codes, hashes):
    ops = ref.ops_by_counter(rec)
    first_index = {}
    for j, h in enumerate(hashes):
        first_index.setdefault(int(h), j)
    codes = [bytes(c) for c in codes]
    steps = np.asarray(rec["steps"], dtype=np.uint64).reshape(-1, 13).tolist()
    cap_copy, _ = capacities(rec)
    copy, flags, srefs, drefs, copy_step, exp, exp_step, status = [], [], [], [], [], [], [], []
    for s, step in enumerate(steps):
        state = step[0] & 0xFF
        if state in NEW_STATES:
            st, events = new_step_events(step, steps[s + 1] if s + 1 < len(steps) else None, ops, first_index)
        else:
            st, ev = ref.step_event(step, ops, codes, first_index)
            events = []
            if ev is not None and ev[0] == "exp":
                exp.append(ev[1]); exp_step.append(s)
            elif ev is not None:
                events = [(ev[1], ev[2], ev[3], 0)]
        if len(copy) + len(events) > cap_copy:  # (cannot happen: the capacity counts the two-event states)
            st, events = code_of(5), []
        status.append(st)
        for cells, flag, sref, dref in events:
            copy.append(cells); flags.append(flag); srefs.append(sref); drefs.append(dref); copy_step.append(s)
    u32 = lambda x: np.array(x, dtype=np.uint32)  # noqa: E731
    return {"copy_events": ref._cells(copy, 12), "copy_flags": u32(flags), "copy_src_ref": u32(srefs), "copy_dst_ref": u32(drefs),
            "copy_step": u32(copy_step), "exp_events": ref._cells(exp, 5), "exp_step": u32(exp_step), "status": u32(status)}


tally_of = ref.tally_of
