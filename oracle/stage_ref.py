"""Stage the unmodified reference (zkevm-specs: its src/ and tests/) under the git-ignored oracle/_ref/, called by build().

The differential tests that execute the reference itself (tests/test_reference_suite.py, tests/test_replay.py, and one test each in
tests/test_flatten_ext.py and tests/test_instruction_surface.py) read it from there only, so no test reaches outside the checkout.
Where no reference checkout is available nothing is staged and those tests skip; every other test checks the reference's
recorded behaviour in tests/golden/.  The checkout is taken from $ZKEVM_SPECS_REF, else the build container's one.
"""
import os
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGE = os.path.join(ROOT, "oracle", "_ref")
SRC = os.path.join(STAGE, "src")
TESTS = os.path.join(STAGE, "tests")
DEFAULT_CHECKOUT = "/root/reference"


def _copy_tree(src, dst):
    """plain files only, every copy writable by its owner (the checkout may be read-only; a later stage replaces this one)"""
    for d, dirs, files in os.walk(src):
        dirs[:] = [x for x in dirs if x != "__pycache__"]
        out = os.path.join(dst, os.path.relpath(d, src))
        os.makedirs(out, exist_ok=True)
        for f in files:
            if not f.endswith((".pyc", ".pyo")):
                shutil.copyfile(os.path.join(d, f), os.path.join(out, f))


def stage(checkout=None):
    """copy <checkout>/src and <checkout>/tests to oracle/_ref/; returns oracle/_ref, or None when there is no checkout to stage"""
    checkout = checkout or os.environ.get("ZKEVM_SPECS_REF") or DEFAULT_CHECKOUT
    try:
        ok = all(os.path.isdir(os.path.join(checkout, p)) and os.listdir(os.path.join(checkout, p)) for p in ("src", "tests"))
    except OSError:  # not readable by this user
        ok = False
    if not ok:
        return None
    for p in ("src", "tests"):
        shutil.rmtree(os.path.join(STAGE, p), ignore_errors=True)
        _copy_tree(os.path.join(checkout, p), os.path.join(STAGE, p))
    return STAGE


def staged():
    """True when oracle/_ref/ holds a staged reference"""
    return os.path.isdir(os.path.join(SRC, "zkevm_specs")) and os.path.isdir(TESTS)


if __name__ == "__main__":
    print(stage(sys.argv[1] if len(sys.argv) > 1 else None) or "no reference checkout to stage")
