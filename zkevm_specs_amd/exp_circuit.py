"""Host-side mirror of `zkevm_specs.exp_circuit.verify_exp_circuit` (exp_circuit.py:88-97), on the MI355X (`zk_exp_verify`), and of
the witness builder `ExpCircuit` (evm_circuit/typing.py:868-994): `add_event` / `fill_dummy_events` collect EXP events on the host and
the rows and the exp table are assigned on the device in one call (`zk_exp_assign`) when they are first needed."""
import numpy as np

from . import _lib, oneshot
from .errors import UnsupportedOnDevice, raise_for_code
from .flatten import flatten_exp_rows

FR_MODULUS = 21888242871839275222246405745257275088548364400416034343698204186575808495617
_U256 = 1 << 256


def exp_events_wire(events):
    """[(identifier, base, exponent)] of ints in the wire's domain -> uint64[n, 5, 4]: identifier, base lo / hi, exponent lo / hi"""
    m = (1 << 128) - 1
    cells = [v for (i, b, e) in events for v in (i, b & m, b >> 128, e & m, e >> 128)]
    raw = b"".join(int(v).to_bytes(32, "little") for v in cells)
    return np.frombuffer(raw, dtype="<u8").reshape(len(events), 5, 4).copy()


class ExpCircuit:
    """`ExpCircuit(max_exp_steps)` of the reference with the witness built on the device.  `add_event` / `fill_dummy_events` chain
    as the reference's do and raise what it raises for arguments Python's own types reject (classified on the host, before any
    launch); `rows` / `table()` give ExpCircuitRow-like objects (objects.exp_rows_from_wire), `wire_rows()` / `wire_table()` the
    arrays themselves (rows uint64[21, n, 4] for zk_exp_open, table uint64[m, 11, 4] for zk_evm_tables.exp).  The events are assigned
    in ONE zk_exp_assign call, whose shape is add_event* [fill_dummy_events]: the shape every caller of the reference has.  What
    that call cannot express raises UnsupportedOnDevice — identifiers of row-producing events that do not strictly increase, and a
    row-producing event added behind the dummy rows; nothing falls back to a host loop."""

    OFFSET_INCREMENT = 7

    def __init__(self, max_exp_steps=100, device=None):
        self.max_exp_steps = max_exp_steps
        self._device = device
        self._events = []   # (identifier mod p, base, exponent) of the row-producing events, in add_event order
        self._pad_steps = 0  # fill_dummy_events was called: dummy rows up to 7 * this many rows
        self._filled = False
        self._cache = None

    # ---- the reference's interface
    def add_event(self, base, exponent, identifier):
        if exponent < 0:  # _exp_by_squaring recurses on exponent // 2, which never leaves -1
            raise RecursionError("maximum recursion depth exceeded")
        # Word(base) is evaluated for every event, before the step loop (typing.py:914)
        if base >= _U256:
            raise AssertionError(f"Word {base} doesn't fit in 256 bits")
        if base < 0:
            raise OverflowError("can't convert negative int to unsigned")
        if exponent > 1 and exponent >= _U256:  # Word(exponent) of the first step
            raise AssertionError(f"Word {exponent} doesn't fit in 256 bits")
        if exponent > 1:
            if self._filled:
                raise UnsupportedOnDevice("ExpCircuit: a row-producing event behind the dummy rows of fill_dummy_events")
            ident = int(getattr(identifier, "n", identifier)) % FR_MODULUS  # FQ(identifier)
            self._events.append((ident, int(base), int(exponent)))
            self._cache = None
        return self

    def fill_dummy_events(self):
        # rows_left = max_exp_rows - len(self.rows): a repeated fill adds rows only up to the largest max_exp_steps seen
        self._pad_steps = max(self._pad_steps, int(self.max_exp_steps))
        self._filled = True
        self._cache = None
        return self

    def table(self):
        return self.rows

    @property
    def rows(self):
        from .objects import exp_rows_from_wire

        return exp_rows_from_wire(self.wire_rows())

    # ---- the wire
    def events_wire(self):
        return exp_events_wire(self._events)

    def wire_rows(self):
        return self._assign()[0]

    def wire_table(self):
        return self._assign()[1]

    def _assign(self):
        if self._cache is None:
            try:
                self._cache = oneshot.exp_assign(self.events_wire(), self._pad_steps, device=self._device)[1:]
            except _lib.EngineError as e:
                if e.rc == _lib.ERR_EXP_ORDER:
                    raise UnsupportedOnDevice(f"ExpCircuit: {e}") from None
                raise
        return self._cache


def verify_exp_circuit(exp_circuit):
    """exp_circuit: object with `.table()` returning ExpCircuitRow-like rows (typing.py:868-880).
    The reference propagates the first failing row's exception (no try/except in the loop)."""
    if isinstance(exp_circuit, ExpCircuit):  # assigned on the device: the wire as it is
        cols = exp_circuit.wire_rows()
        if cols.shape[1] == 0:
            return None
        res, _ = oneshot.exp_verify(cols, device=exp_circuit._device)
    else:
        rows = list(exp_circuit.table())
        if not rows:
            return None
        res, _ = oneshot.exp_verify(flatten_exp_rows(rows))
    raise_for_code(res.first_fail_code, f"Exp circuit row {res.first_fail_row}")
    return res
