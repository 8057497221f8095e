"""A recording stand-in for a loaded engine library (tests only): forwards every call and, for each zk_* entry, logs its name and what
was passed — a scalar's value, null / non-null for a pointer, and the same per field of a struct passed by reference.  The bookkeeping
entries (zk_init, zk_last_error, zk_close) are forwarded unlogged: when they run depends on garbage collection and on which library
formats an error, not on how a call's arguments are marshalled."""
import contextlib
import ctypes

from zkevm_specs_amd import _lib

UNLOGGED = ("zk_init", "zk_last_error", "zk_close")


def describe(x):
    if x is None:
        return "null"
    if isinstance(x, (bool, int)):
        return int(x)
    if isinstance(x, ctypes.c_void_p):
        return "ptr" if x.value else "null"
    if isinstance(x, _lib.ZkResult):
        return "result"
    if isinstance(x, ctypes.Structure):
        return {name: describe(getattr(x, name)) if not issubclass(tp, ctypes.c_void_p) else ("ptr" if getattr(x, name) else "null")
                for name, tp in x._fields_}
    if isinstance(x, ctypes.Array):
        return f"array[{len(x)}]"
    if hasattr(x, "_obj"):  # ctypes.byref(...): a struct is described, anything else is an out-parameter
        return describe(x._obj) if isinstance(x._obj, ctypes.Structure) else "out"
    if isinstance(x, ctypes._SimpleCData):
        return describe(x.value)
    return type(x).__name__


class Recorder:
    def __init__(self, lib):
        self._real, self.log = lib, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("zk_") or name in UNLOGGED:
            return fn

        def call(*args):
            self.log.append([name, [describe(a) for a in args]])
            return fn(*args)

        call.__name__ = name
        return call


@contextlib.contextmanager
def recording(device):
    """the library that `_lib.init(device)` hands out, wrapped for the duration -> its Recorder"""
    slot = "_cpu_lib" if device == "cpu" else "_lib"
    real = _lib.init(device)
    rec = Recorder(real)
    setattr(_lib, slot, rec)
    try:
        yield rec
    finally:
        setattr(_lib, slot, real)
