"""Directed ECC sites on the CPU backend (libzkevm_cpu.so): every sheet of tests/golden/ecc_site_cases.npz through the one-shot
zk_ecc_assign / zk_ecc_verify and the zk_ecc_open / zk_ecc_assign_open sessions, bit for bit against the statuses and rows the
plain-Python model recorded (tests/ecc_site_cases.py)."""
import pytest

from tests import ecc_site_cases as c

CPU = "cpu"


@pytest.fixture(scope="module")
def returned():
    """the statuses the one-shot and session tests got, by sheet name: what the coverage tests below count"""
    return {"oneshot": {}, "session": {}}


@pytest.mark.parametrize("sheet", c.sheets(), ids=c.sheet_ids())
def test_assignment_cpu(sheet):
    c.check_assignment(sheet, CPU)


@pytest.mark.parametrize("sheet", c.sheets(), ids=c.sheet_ids())
def test_oneshot_cpu(sheet, returned):
    returned["oneshot"][sheet.name] = c.oneshot_status(sheet, CPU)


@pytest.mark.parametrize("sheet", c.sheets(), ids=c.sheet_ids())
def test_session_cpu(sheet, returned):
    returned["session"][sheet.name] = c.session_status(sheet, CPU)


@pytest.mark.parametrize("sheet", c.sheets(), ids=c.sheet_ids())
def test_ranges_cpu(sheet):
    c.check_ranges(sheet, CPU)


def test_single_row_ranges_cpu():
    c.check_single_rows(c.sheets()[3], CPU)


def test_range_changes_cpu():
    c.check_range_changes(c.sheets()[6], CPU)


@pytest.mark.parametrize("form", ["oneshot", "session"])
def test_coverage_cpu(form, returned):
    """the coverage table from the statuses the backend returned (run afresh for a sheet whose test above did not run)"""
    got, run = returned[form], c.oneshot_status if form == "oneshot" else c.session_status
    c.check_coverage(lambda s: got[s.name] if s.name in got else got.setdefault(s.name, run(s, CPU)))
