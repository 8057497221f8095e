"""Directed PI / PI-copy / Tx / Sig failure sites on the host: tests/golden/pi_sign_site_cases.npz through tests/pi_sign_site_cases.py —
every case at every position through the host logic harness (the kernels' row functions) and through the host build (libzkevm_cpu.so):
sessions, ranged sessions, the one-shot entries."""
import pytest

from oracle import codes, pi_oracle as PO
from oracle.wire import P
from tests import pi_sign_site_cases as psc

N_SLICES = {"pi": 6, "tx": 4, "sig": 4}
SLICES = [(name, part) for name in ("pi", "tx", "sig") for part in range(N_SLICES[name])]
B64, B128 = 1 << 64, 1 << 128
_ran = {}


@pytest.fixture(scope="module")
def datas(golden_dir):
    return {"pi": psc.load_pi(golden_dir), "copy": psc.load_copy(golden_dir), "tx": psc.load_sign(golden_dir, False), "sig": psc.load_sign(golden_dir, True)}


def _own(case, cell, d=0):
    """value a PI case patches into `cell` of its target row (d = 1: of the successor), or None"""
    return {(row - case.target, c): v for k, _, row, c, v in case.patches if k == psc.P_CELL}.get((d, cell))


def _names(data, prefix, site=None, kind=None):
    return [c for c in data.cases if c.name.split(":")[-1].startswith(prefix) and (site is None or c.site == site) and (kind is None or c.ref_kind == kind)]


def test_file_census_and_line_tables(datas):
    """PI rows: every site of pi_check_row has a case except the stored unreached ones (site 9 alone, with the reason a reader can check);
    one reference line per site, two for site 5; the sites that share a line are the two `for cons in ...: assert` loops.  Copy
    constraints, Tx and Sig units: every site, one line each; 7, 8 and 10 with every kind they carry."""
    pi = datas["pi"]
    have, missing = psc.census(pi.cases, psc.PI_SITES)
    assert missing == sorted(pi.unreached) == [9] and len(pi.tried) == 1 and "site 6" in pi.tried[0]
    assert sorted(pi.site_line) == have
    for s in have:
        assert len(pi.site_line[s]) == psc.PI_N_LINES.get(s, 1), s
    for c in pi.cases:
        assert codes.site_of(c.code) == c.site and c.ref_kind == codes.kind_of(c.code) and (c.site == 0) == (c.code == 0)
        assert c.site == 0 or c.ref_line in pi.site_line[c.site]
        assert c.target < len(pi.rows)
    shared = {(a, b) for a in have for b in have if a < b and set(pi.site_line[a]) & set(pi.site_line[b])}
    assert shared == {p for p in psc.PI_SHARED if 9 not in p}
    assert {s for s in have if any(c.ref_kind == codes.LOOKUP_UNSAT for c in pi.cases if c.site == s)} == {13, 26}
    assert psc.census(datas["copy"], psc.COPY_SITES) == ([1, 2], [])
    for name, sites in (("tx", psc.TX_SITES), ("sig", psc.SIG_SITES)):
        d = datas[name]
        assert psc.census(d.cases, sites) == (list(sites), []) and d.unreached == []
        for c in d.cases:
            assert codes.site_of(c.code) == c.site and c.ref_kind == codes.kind_of(c.code) and (c.site == 0) == (c.code == 0)
            assert c.name.startswith("wire:") == (c.ref_line == 0 and c.site != 0) or c.site == 0
        assert all(len(v) == 1 for v in d.site_line.values()) and sorted(d.site_line) == list(sites)
    kinds = lambda d, s: {c.ref_kind for c in d.cases if c.site == s}  # noqa: E731
    lib = {codes.UNSUPPORTED, codes.OVERFLOW_ERROR, codes.ATTRIBUTE_ERROR, codes.TYPE_ERROR}  # BadSignature, limbs past 2^256, missing parts
    assert kinds(datas["tx"], 7) == lib | {codes.ASSERT} and kinds(datas["sig"], 7) == lib
    assert kinds(datas["tx"], 8) == kinds(datas["tx"], 10) == {codes.ASSERT, codes.INDEX_ERROR}
    # Tx: the caller row's type and its value are one statement; so are none of the others
    assert datas["tx"].site_line[8] == datas["tx"].site_line[9] and len({v for v in datas["tx"].site_line.values()}) == 10


def test_pi_edge_cases_are_in_the_file(datas):
    pi = datas["pi"]
    cs, rows = pi.cases, pi.rows
    at = lambda c: rows[c.target]  # noqa: E731
    # the base holds every gated row kind: gas != gas_next on adjacent rows of one tx, a tx_id step of 2, padding calldata rows, a
    # padding tx, a CallDataLength row of length 0
    cd = [j for j, r in enumerate(rows) if r[PO.Q_TX_CALLDATA]]
    assert any(rows[j][PO.TX_ID] == rows[j + 1][PO.TX_ID] != 0 and bool(rows[j][PO.TX_LO]) != bool(rows[j + 1][PO.TX_LO]) for j in cd)
    assert any(rows[j + 1][PO.TX_ID] - rows[j][PO.TX_ID] == 2 for j in cd) and sum(1 for j in cd if rows[j][PO.TX_ID] == 0) >= 2
    assert any(r[PO.Q_TX_TABLE] and r[PO.TX_TAG] == PO.TAG_CALLDATA_LENGTH and r[PO.TX_LO] == 0 and r[PO.TX_ID] == 2 for r in rows)
    assert sum(1 for r in rows if r[PO.Q_WD]) >= 2 and len(rows) % 64 and len(pi.full.rows) > 9000
    # site 5: the 128-bit bound of both digest halves against a table miss; the table emptied; a row doubled with one cell changed
    l5 = sorted(pi.site_line[5])
    for cell in (PO.DIGEST_LO, PO.DIGEST_HI):
        assert any(c.site == 5 and _own(c, cell) == B128 and c.ref_line == l5[1] for c in cs), cell
        assert any(c.site == 5 and _own(c, cell) == B128 - 1 and c.ref_line == l5[0] for c in cs), cell
    assert any(c.site == 5 and [p[:2] for p in c.patches] == [(psc.P_TEMPTY, psc.T_KECCAK)] and at(c)[PO.Q_KECCAK] == q for c in cs for q in (0, 1))
    assert sum(1 for c in cs if c.site == 0 and [p[:2] for p in c.patches] == [(psc.P_TDUP, psc.T_KECCAK)]) >= 5
    assert {p[3] for c in cs if c.site == 5 for p in c.patches if p[0] == psc.P_TCELL} == {0, 1, 2, 3, 4}
    # site 13: 65535 is in the u16 table, 65536 is not
    v13 = {}
    for c in cs:
        nid = _own(c, PO.TX_ID, 1)
        if nid is not None and len(c.patches) == 3:
            v13[nid - at(c)[PO.TX_ID] - 1] = c.site
    assert v13 == {65535: 0, 65536: 13, 1 << 40: 13}
    # the is-zero inverses at 0 and at a neighbour's inverse
    for site, cell in ((6, PO.TX_ID_INV), (7, PO.TX_LO_INV), (8, PO.TX_DIFF_INV), (23, PO.TX_ID_INV), (24, PO.TX_LO_INV)):
        vals = {_own(c, cell) for c in cs if c.site == site and len(c.patches) == 1}
        assert 0 in vals and any(v not in (None, 0, 1) for v in vals), site
    # site 16 with the row's own byte cost where the successor's differs; 21 / 22 behind 14 / 16
    assert any(c.site == 16 and bool(at(c)[PO.TX_LO]) != bool(rows[c.target + 1][PO.TX_LO]) for c in cs)
    assert any(c.site == 21 and len(c.patches) == 2 for c in cs) and any(c.site == 22 and len(c.patches) == 2 for c in cs)
    # site 26: the table emptied (a CallDataLength row with and without calldata, a plain row), each of a row's three cells, (0, 0, 0)
    e26 = [c for c in cs if c.site == 26 and [p[:2] for p in c.patches] == [(psc.P_TEMPTY, psc.T_GAS)]]
    assert {(at(c)[PO.TX_TAG] == PO.TAG_CALLDATA_LENGTH, at(c)[PO.TX_LO] != 0) for c in e26} == {(True, True), (True, False), (False, True)}
    assert {p[3] for c in cs if c.site == 26 for p in c.patches if p[0] == psc.P_TCELL and p[1] == psc.T_GAS} == {0, 1, 2}
    assert any(c.site == 0 and c.patches == [] and at(c)[PO.TX_TAG] == PO.TAG_CALLDATA_LENGTH and at(c)[PO.TX_LO] == 0 for c in cs)
    # site 27: the last withdrawal row patched — its predecessor fails, the row itself (successor: q_withdrawal_table 0) passes
    wl = max(j for j, r in enumerate(rows) if r[PO.Q_WD])
    assert any(c.site == 27 and c.target == wl - 1 and _own(c, PO.WD_ID, 1) is not None for c in cs)
    assert any(c.site == 0 and c.target == wl and _own(c, PO.WD_ID) is not None for c in cs)
    assert any(c.site == 28 and _own(c, PO.WD_AMOUNT) == 0 for c in cs)
    # cases whose patch lies in the successor row
    assert sum(1 for c in cs if c.wrap) >= 20


def test_copy_edge_cases_are_in_the_file(datas):
    cs = {c.name: c for c in datas["copy"]}
    assert {cs[k].length for k in ("len0", "len1", "len31", "len32")} == {0, 1, 31, 32}
    assert [cs[k].site for k in ("len0", "len1", "len31", "len31/leading-zero", "cell", "len1/bytes-behind-the-length")] == [0] * 6
    assert [cs[k].site for k in ("len32", "len32/zero", "len33")] == [1] * 3
    assert [cs[k].site for k in ("len31/last-byte", "len31/first-byte", "cell/byte31", "wire:len31/cell+p", "wire:cell/data+p")] == [2] * 5
    assert cs["len31/leading-zero"].data[0] == 0 and cs["wire:len31/cell+p"].cell >= P
    assert cs["cell/byte31"].cell ^ cs["cell"].cell == 1 << 248


def test_sign_edge_cases_are_in_the_file(datas):
    tx, sig = datas["tx"], datas["sig"]
    for d in (tx, sig):
        for k in range(3):  # the three byte copies, on either side; the seven malformed bits alone
            for side in ("chip", "ecdsa"):
                assert any(c.site == k + 1 and "/" + side + "/" in c.name for c in _names(d, "copy/")), (k, side)
        for bit in range(7):
            cs = _names(d, "malformed/bit%d/" % bit)
            assert cs and all(int(c.meta[2]) == 1 << bit and c.site == (1 + bit % 2 if bit < 4 else 3 if bit < 6 else 4) for c in cs), bit
        assert _names(d, "keccak/empty", 4) and _names(d, "keccak/len63", 4) and _names(d, "keccak/len65", 4) and _names(d, "keccak/output-swapped", 4)
        own = {c.name.split("own-")[1]: c for c in _names(d, "keccak/two-rows-one-key/", 0)}
        assert sorted(own) == ["first", "second"]
        for which, c in own.items():  # two rows of the unit's (rlc, len) key; the one that holds its hash comes first / second
            h = bytes(c.bytes[6].tolist())
            val = psc.pk_rlc_model(bytes(c.bytes[0].tolist()), bytes(c.bytes[1].tolist()), c.r)[0]
            rows = [k for k in psc.wire.rowmajor_to_rows(c.keccak) if k[:3] == [1, val, 64]]
            assert len(rows) == 2 and rows[0][1:3] == rows[1][1:3] and rows[0][3:] != rows[1][3:]
            assert rows[0 if which == "first" else 1][3:] == [int.from_bytes(h[:16], "little"), int.from_bytes(h[16:], "little")]
        # randomness 0, 1, p - 1 and a full-width one; keys of 0x00 and 0xff bytes; the lazy reduction's 0 .. 5 subtractions; a ninth limb
        assert {0, 1, P - 1} <= {c.r for c in _names(d, "keccak/r", 0)} and any(c.r > 1 << 252 for c in _names(d, "keccak/r-full", 0))
        subs, ninth = set(), 0
        for c in d.cases:
            if c.site == 0 and int(c.meta[2]) == 0 and (d.is_sig or int.from_bytes(c.cells[0].tobytes(), "little")):
                val, n_sub, top = psc.pk_rlc_model(bytes(c.bytes[0].tolist()), bytes(c.bytes[1].tolist()), c.r)
                h = bytes(c.bytes[6].tolist())
                assert [1, val, 64, int.from_bytes(h[:16], "little"), int.from_bytes(h[16:], "little")] in psc.wire.rowmajor_to_rows(c.keccak), c.name
                subs.add(n_sub)
                ninth = max(ninth, top)
        assert subs == {0, 1, 2, 3, 4, 5} and ninth > 0, (subs, ninth)
        ff = [c for c in _names(d, "keccak/pk-ff/r-full/row", 0)]
        assert ff and psc.pk_rlc_model(bytes(ff[0].bytes[0].tolist()), bytes(ff[0].bytes[1].tolist()), ff[0].r)[2] > 0
        assert _names(d, "keccak/pk-00/r/row", 0) and _names(d, "keccak/pk-00/r/no-row", 4) and _names(d, "keccak/pk-ff/r/no-row", 4)
        assert _names(d, "address/byte19", 5) and _names(d, "address/byte0", 5) and _names(d, "address/hash-byte11", 0)
        assert _names(d, "msg_hash/lo", 6) and _names(d, "msg_hash/hi", 6)
        for what in ("zero/r", "zero/s", "N/r", "N/s"):
            assert _names(d, "ecdsa/" + what, 7, codes.UNSUPPORTED), what
    # Tx: the padding slot; a refuted signature; an off-curve key; the tx rows
    assert _names(tx, "padding", 0) and _names(tx, "padding/only-the-disabled-row", 0) and _names(tx, "padding/keccak-empty", 4) and _names(tx, "padding/msg_hash", 6)
    assert _names(tx, "ecdsa/other/", 7, codes.ASSERT) and _names(tx, "ecdsa/off-curve", 7, codes.ASSERT)
    assert _names(tx, "caller/word", 8, codes.ASSERT) and _names(tx, "caller/value", 9) and _names(tx, "sign_hash/lo", 10, codes.ASSERT) and _names(tx, "sign_hash/hi", 11)
    cuts = {c.tx_rows.shape[0]: (c.site, c.ref_kind) for c in _names(tx, "tx-table/")}
    assert cuts == {3: (8, codes.INDEX_ERROR), 4: (10, codes.INDEX_ERROR), 11: (10, codes.INDEX_ERROR), 12: (0, 0)}
    # Sig: r and s as 384-bit sums; v; the 2 x 2 matrix of is_valid
    for k, attr in ((12, "sig_r"), (13, "sig_s")):
        assert _names(sig, attr + "/lo-borrows-from-hi", 0) and _names(sig, attr + "/hi=2^128", k) and _names(sig, attr + "/equal-modulo-2^256", k)
        assert _names(sig, attr + "/p-1", k) and _names(sig, attr + "/carry-out-of-384-bits", k) and _names(sig, attr + "/hi+p", k)
        c = _names(sig, attr + "/carry-out-of-384-bits", k)[0]
        lo, hi = (int.from_bytes(c.cells[2 * k - 20 + j].tobytes(), "little") for j in (0, 1))
        assert lo + (hi << 128) == (1 << 384) + int.from_bytes(bytes(c.bytes[7 + k - 12].tolist()), "little")
    sv = {c.name[6:]: c.site for c in _names(sig, "sig_v/")}
    assert sv == {"0x0": 0, "0x1": 0, "0x2": 14, "0x3": 14, "p-1": 14, hex(B64): 14, hex(B64 + 1): 14, hex(1 << 32): 14, hex(B128 + 1): 14}
    m = {(c.name.split("/")[1], c.name.split("/")[2]): c.site for c in _names(sig, "is_valid/")}
    assert m == {("True", "verified"): 0, ("True", "refuted"): 15, ("False", "verified"): 15, ("False", "refuted"): 0}


def test_rotated_bases_pass_the_oracle(datas):
    """every rotation the variants use was checked against the reference by the generator; here the oracle accepts them too"""
    pi = datas["pi"]
    used = {cut for c in pi.cases for cut in psc.pi_variants(pi, c)}
    assert used == pi.checked
    for c in pi.cases:
        n = len(pi.rows)
        assert {(c.target - cut) % n for cut in psc.pi_variants(pi, c)} >= {0, 63, 64, 255, 256, n - 1}
    for cut in sorted(used):
        assert not any(psc.pi_base_status(pi, cut)), cut


@pytest.mark.parametrize("name,part", SLICES)
def test_every_case_fails_at_its_site_on_the_host(datas, hostsim, name, part):
    data = datas[name]
    if name == "pi":
        out = psc.pi_run_slice(data, "cpu", part, N_SLICES[name], hostsim=hostsim)
        assert out[1] == psc.pi_expected_runs(data, part, N_SLICES[name]) and out[0] > 0
    else:
        out = psc.sign_run_slice(data, "cpu", part, N_SLICES[name], hostsim=hostsim)
        assert out[1] == psc.sign_expected_runs(data, part, N_SLICES[name]) and out[0] > 0
    _ran[(name, part)] = out


def test_copy_constraints_and_the_full_length_witness_on_the_host(datas, hostsim):
    out = psc.copy_run_all(datas["copy"], "cpu", hostsim=hostsim)
    assert out[0] == len(datas["copy"]) and out[1] == 6 * len(datas["copy"]) and out[2] == {1, 2}
    _ran["copy"] = out
    _ran["pifull"] = psc.pi_run_full(datas["pi"], "cpu", hostsim=hostsim)


def test_nothing_is_left_out(datas):
    """the slices above are the whole file: every case ran, in every declared run, and the sites exercised are the census: the share of
    file cases left out is 0"""
    assert sorted(k for k in _ran if isinstance(k, tuple)) == sorted(SLICES) and "copy" in _ran and _ran["pifull"] == 5, "run this module as a whole"
    for name, sites in (("pi", psc.PI_SITES), ("tx", psc.TX_SITES), ("sig", psc.SIG_SITES)):
        data, k = datas[name], N_SLICES[name]
        n = len(data.cases)
        bounds = [p * n // k for p in range(k + 1)]
        assert bounds[0] == 0 and bounds[-1] == n and bounds == sorted(set(bounds))
        parts = [_ran[(name, p)] for p in range(k)]
        assert sum(p[0] for p in parts) == n
        assert sum(p[1] for p in parts) == (psc.pi_expected_runs(data, 0, 1) if name == "pi" else psc.sign_expected_runs(data, 0, 1))
        assert sorted(set().union(*(p[2] for p in parts))) == psc.census(data.cases, sites)[0]
        assert {f for idx in range(n) for f in psc.forms(idx)} == {"session", "ranged", "oneshot"}
