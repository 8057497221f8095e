"""Directed ECC sites on the MI355X: every sheet of tests/golden/ecc_site_cases.npz through the one-shot kernels
(ecc_point_rows_kernel, the one-lane ecc_pairing_rows_kernel), the session pass (ecc_range_point_rows_kernel, ecc_pair_stage1_kernel with
one lane per pair, ecc_pair_stage2_kernel) and zk_ecc_assign / zk_ecc_assign_open, bit for bit against the statuses and rows the
plain-Python model recorded (tests/ecc_site_cases.py).  Reads tests/golden/ only."""
import pytest

from tests import ecc_site_cases as c

pytestmark = pytest.mark.gpu
HIP = None
DEVICE_RESIDENT = (0, 6, 10, 13)  # sheets also run with device-resident arrays (6, 10, 13: a per-pair target on op 64)


@pytest.fixture(scope="module")
def returned():
    """the statuses the one-shot and session tests got, by sheet name: what the coverage tests below count"""
    return {"oneshot": {}, "session": {}}


@pytest.mark.parametrize("sheet", c.sheets(), ids=c.sheet_ids())
def test_assignment_hip(sheet):
    c.check_assignment(sheet, HIP)


@pytest.mark.parametrize("sheet", c.sheets(), ids=c.sheet_ids())
def test_oneshot_hip(sheet, returned):
    returned["oneshot"][sheet.name] = c.oneshot_status(sheet, HIP)


@pytest.mark.parametrize("sheet", c.sheets(), ids=c.sheet_ids())
def test_session_hip(sheet, returned):
    returned["session"][sheet.name] = c.session_status(sheet, HIP)


@pytest.mark.parametrize("k", DEVICE_RESIDENT)
def test_session_device_resident_hip(k):
    c.session_status(c.sheets()[k], HIP, on_device=True)


@pytest.mark.parametrize("sheet", c.sheets(), ids=c.sheet_ids())
def test_ranges_hip(sheet):
    c.check_ranges(sheet, HIP, on_device=c.sheets().index(sheet) in DEVICE_RESIDENT)


def test_single_row_ranges_hip():
    c.check_single_rows(c.sheets()[3], HIP, on_device=True)


def test_range_changes_hip():
    c.check_range_changes(c.sheets()[6], HIP, on_device=True)


@pytest.mark.parametrize("form", ["oneshot", "session"])
def test_coverage_hip(form, returned):
    """the coverage table from the statuses the device returned (run afresh for a sheet whose test above did not run)"""
    got, run = returned[form], c.oneshot_status if form == "oneshot" else c.session_status
    c.check_coverage(lambda s: got[s.name] if s.name in got else got.setdefault(s.name, run(s, HIP)))
