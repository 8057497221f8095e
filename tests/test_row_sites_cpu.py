"""Directed Copy / Bytecode / Exp failure sites on the host: tests/golden/row_site_cases.npz through tests/row_site_cases.py — every case
at every position through the host logic harness (the kernels' row functions with loaded neighbours, both RW-index modes) and through
the host build (libzkevm_cpu.so): sessions, ranged sessions, the one-shot entries."""
import pytest

from oracle import codes, copy_oracle as co, row_oracles as ro
from oracle.wire import P
from tests import row_site_cases as rsc

N_SLICES = {"copy": 6, "bytecode": 3, "exp": 3}
SLICES = [(name, part) for name in rsc.CIRCUITS for part in range(N_SLICES[name])]
B40, B64, B72, B128, B200 = 1 << 40, 1 << 64, 1 << 72, 1 << 128, 1 << 200
_ran = {}


@pytest.fixture(scope="module")
def datas(golden_dir):
    return {name: rsc.load(golden_dir, name) for name in rsc.CIRCUITS}


def _cells(case, kind=rsc.P_CELL, table=0):
    """{(row - target, cell): value} of a case's patches of one kind"""
    return {(row - case.target if kind in (rsc.P_CELL, rsc.P_FLAG) else row, cell): v for k, t, row, cell, v in case.patches if k == kind and t == table}


def _own(case, cell):
    """value a case patches into `cell` of its own target row, or None"""
    return _cells(case).get((0, cell))


def test_file_census_and_line_table(datas):
    """every site has a case except the stored unreached ones (none in Bytecode, at most two over Copy and Exp); one reference line per
    site (two for Copy 22, `lt`'s operand asserts); the sites that share a line are exactly the stored pairs, listed here"""
    missing = {}
    for name, data in datas.items():
        have, missing[name] = rsc.census(data)
        assert missing[name] == sorted(data.unreached) and len(data.tried) == len(missing[name])
        assert sorted(data.site_line) == have
        for s in have:
            assert len(data.site_line[s]) == rsc.SITE_N_LINES.get((name, s), 1), (name, s)
        for c in data.cases:
            assert codes.site_of(c.code) == c.site and c.ref_kind == codes.kind_of(c.code) and (c.site == 0) == (c.code == 0)
            assert c.site == 0 or c.ref_line in data.site_line[c.site]
            assert c.target < len(data.rows)
        pairs = sorted((a, b) for a in have for b in have if a < b and set(data.site_line[a]) & set(data.site_line[b]))
        assert pairs == sorted(data.shared)
    assert len(datas["bytecode"].cases) and missing["bytecode"] == [] and len(rsc.census(datas["bytecode"])[0]) == 23
    assert len(missing["copy"]) + len(missing["exp"]) <= rsc.MAX_UNREACHED["copy+exp"]
    # Copy: the id's type (28 / 35 / 39), the lookup (29 / 36 / 40) and the found row's type (30 / 37 / 41) are one statement each
    assert sorted(datas["copy"].shared) == [(28, 29), (28, 30), (29, 30), (35, 36), (35, 37), (36, 37), (39, 40), (39, 41), (40, 41)]
    # Bytecode: header-to-header is one helper, called for a padding header and for the last row
    assert sorted(datas["bytecode"].shared) == [(9, 22), (10, 23)]
    # Exp: a.to_64s() / b.to_64s() inside one mul_add_words call; Word.from_lo(r) and q.to_64s() inside the other
    assert sorted(datas["exp"].shared) == [(6, 7), (15, 17)]
    # Copy 22: addr raises at the first of lt's asserts, src_addr_end at the second
    l22 = sorted(datas["copy"].site_line[22])
    for c in datas["copy"].cases:
        if c.site == 22 and len(c.patches) == 1:
            assert c.ref_line == (l22[0] if c.patches[0][3] == co.ADDR else l22[1])


def test_copy_edge_cases_are_in_the_file(datas):
    data = datas["copy"]
    cs = data.cases
    rw0, n_rw = data.trows[rsc.T_RW][0][0], len(data.trows[rsc.T_RW])
    # site 22: 2^40 - 1 does not fail there, 2^40 does, for both operands
    for cell in (co.ADDR, co.SRC_END):
        assert any(_own(c, cell) == B40 - 1 and len(c.patches) == 1 and c.site != 22 for c in cs), cell
        assert any(_own(c, cell) == B40 and len(c.patches) == 1 and c.site == 22 for c in cs), cell
    # site 23: src_addr_end == addr fails a non-padding read row, src_addr_end == addr + 1 fails a padding one and passes the other
    at = lambda c: data.rows[c.target]  # noqa: E731
    assert any(c.site == 23 and _own(c, co.SRC_END) == at(c)[co.ADDR] and at(c)[co.IS_PAD] == 0 for c in cs)
    assert any(c.site == 23 and _own(c, co.SRC_END) == at(c)[co.ADDR] + 1 and at(c)[co.IS_PAD] == 1 for c in cs)
    assert any(c.site != 23 and _own(c, co.SRC_END) == at(c)[co.ADDR] + 1 and at(c)[co.IS_PAD] == 0 for c in cs)
    # sites 29 and 40 at the dense index's bounds
    for site in (29, 40):
        dense = [c for c in cs if c.site == site and rsc.is_dense_edge_case(c)]
        vals = {_own(c, co.RWC) for c in dense}
        assert {rw0 - 1, rw0 + n_rw, P - 1} <= vals, (site, vals)
        assert any(v is not None and v >= B64 and rw0 <= v % B64 < rw0 + n_rw and v % B64 == at(c)[co.RWC] for c in dense for v in [_own(c, co.RWC)]), site
        assert all(c.ref_kind == codes.LOOKUP_UNSAT for c in dense)
    # unsatisfied and ambiguous lookups; an identical duplicate passes
    for site in (29, 32, 36, 40):
        assert any(c.site == site and c.ref_kind == codes.LOOKUP_UNSAT and not rsc.is_ambiguity_case(c) for c in cs), site
        assert any(c.site == site and c.ref_kind == codes.LOOKUP_AMBIGUOUS and any(p[0] == rsc.P_TDUP and p[3] != rsc.NO_CELL for p in c.patches) for c in cs), site
    for table in rsc.TABLES["copy"]:
        assert any(c.site == 0 and [p[:2] + p[3:4] for p in c.patches] == [(rsc.P_TDUP, table, rsc.NO_CELL)] for c in cs), table
    # a table type bit, the row's own type bit, a table value
    for site in (30, 37, 41):
        assert any(c.site == site and [p[0] for p in c.patches] == [rsc.P_TFLAG] for c in cs), site
    for site in (28, 35, 39):
        assert any(c.site == site and [p[0] for p in c.patches] == [rsc.P_FLAG] for c in cs), site
    for site, table, cell in ((31, rsc.T_RW, 8), (34, rsc.T_BYTECODE, 5), (38, rsc.T_TX, 3), (42, rsc.T_RW, 8)):
        assert any(c.site == site and [p[:2] + p[3:4] for p in c.patches] == [(rsc.P_TCELL, table, cell)] for c in cs), site
    # tables of zero rows: LookupUnsat, not a read
    for site, table in ((29, rsc.T_RW), (40, rsc.T_RW), (32, rsc.T_BYTECODE), (36, rsc.T_TX)):
        assert any(c.site == site and c.ref_kind == codes.LOOKUP_UNSAT and [p[:2] for p in c.patches] == [(rsc.P_TEMPTY, table)] for c in cs), site


def test_bytecode_edge_cases_are_in_the_file(datas):
    data = datas["bytecode"]
    cs = data.cases
    # site 11: the push table's edges, alone and with the size the low byte asks for; a value that is no byte fails whatever its low byte
    for v in (0x5F, 0x60, 0x7F, 0x80, 255, 256, 256 + 0x60, B64 + 0x60):
        assert any(_own(c, ro.VALUE) == v and len(c.patches) == 1 for c in cs), v
        with_size = [c for c in cs if _own(c, ro.VALUE) == v and _own(c, ro.PUSH_SIZE) == ro._push_size(v & 0xFF) and len(c.patches) == 2]
        assert with_size and all((c.site == 11) == (v > 255) for c in with_size), v
    assert any(c.site == 11 and len(c.patches) == 1 and _own(c, ro.PUSH_SIZE) == data.rows[c.target][ro.PUSH_SIZE] + 1 for c in cs)
    # site 12: push_data_left 2^64
    assert any(c.site == 12 and _own(c, ro.PUSH_LEFT) == B64 for c in cs)
    # site 18: around zero.  push_data_left == 0 on a push-data row fails 12 (is_code must be 1 then, and a row with is_code 1 takes the
    # branch of 17): 18 with left - 1 == p - 1 on the row's own cell cannot be reached; its neighbours are here
    assert any(c.site == 12 and _own(c, ro.PUSH_LEFT) == 0 and len(c.patches) == 1 for c in cs)
    assert any(c.site in (0, 17) and _own(c, ro.PUSH_LEFT) == 0 and _own(c, ro.IS_CODE) == 1 for c in cs)
    assert any(c.site == 18 and _cells(c).get((1, ro.PUSH_LEFT)) == P - 1 for c in cs)
    assert any(c.site == 18 and _own(c, ro.PUSH_LEFT) is not None and _own(c, ro.PUSH_LEFT) >= B64 for c in cs)
    # site 20: the rlc, the length, hash lo, hash hi — on the row and in the table
    for cell in (ro.VALUE_RLC, ro.LENGTH, ro.HASH_LO, ro.HASH_HI):
        assert any(c.site == 20 and _own(c, cell) is not None for c in cs), cell
    for kc in (1, 2, 3, 4):
        assert any(c.site == 20 and [p[:2] + p[3:4] for p in c.patches] == [(rsc.P_TCELL, rsc.T_KECCAK, kc)] for c in cs), kc
    assert any(c.site == 20 and [p[:2] for p in c.patches] == [(rsc.P_TEMPTY, rsc.T_KECCAK)] for c in cs)


def test_exp_edge_cases_are_in_the_file(datas):
    data = datas["exp"]
    cs = data.cases

    def carries(c, first):
        """the carries of the case's patched target row (first: a * b + c = d, else 2 * q + r = exponent)"""
        r = list(data.rows[c.target])
        for (d, cell), v in _cells(c).items():
            if d == 0:
                r[cell] = v
        W = lambda k: (r[k], r[k + 1])  # noqa: E731
        return ro._carries(W(ro.X_A), W(ro.X_B), W(ro.X_C), W(ro.X_D)) if first else ro._carries((2, 0), W(ro.X_Q), (r[ro.X_R], 0), W(ro.X_EXPONENT))

    own_only = [c for c in cs if all(p[0] == rsc.P_CELL and p[2] == c.target for p in c.patches)]
    for site, first, half in ((8, True, 0), (9, True, 1), (18, False, 0), (19, False, 1)):
        before = {8: (), 9: (8,), 18: (8, 9, 12, 13, 15, 17), 19: (8, 9, 12, 13, 15, 17, 18)}[site]
        # the carry exactly 2^72 - 1 passes the check, exactly 2^72 fails it
        assert any(carries(c, first)[half] == B72 - 1 and c.site not in before + (site,) and c.site > 0 for c in own_only), site
        assert any(carries(c, first)[half] == B72 and c.site == site for c in own_only), site
        sub = (ro.X_D if first else ro.X_EXPONENT) + half
        # the subtrahend in [2^128, 2^200), and at 2^200 and above (the field path)
        assert any(c.site == site and B128 <= (_own(c, sub) or 0) < B200 for c in own_only), site
        assert any(c.site == site and (_own(c, sub) or 0) >= B200 for c in own_only), site
        # a borrow: the subtrahend one more than the minuend; a numerator one more than a multiple of 2^128 (modulo p: a zero cell less one is p - 1)
        assert any(c.site == site and len(c.patches) == 1 and _own(c, sub) == (data.rows[c.target][sub] + 1) % P for c in own_only), site
        assert any(c.site == site and len(c.patches) == 1 and _own(c, sub) == (data.rows[c.target][sub] - 1) % P for c in own_only), site
    # ... with the difference made exact again the shifted subtrahend passes 8 / 9
    for half in (0, 1):
        assert any(c.site not in (0, 8, 9) and B128 <= (_own(c, ro.X_D + half) or 0) < B200 and _own(c, ro.X_C + half) is not None for c in own_only), half
        assert any(c.site not in (0, 8, 9) and (_own(c, ro.X_D + half) or 0) >= B200 and _own(c, ro.X_C + half) is not None for c in own_only), half
    # c a large field element
    assert any((_own(c, ro.X_C + 1) or 0) > P - B200 and c.site not in (8, 9) for c in own_only)
    assert any((_own(c, ro.X_C) or 0) > P - B200 and c.site == 8 for c in own_only)
    # sites 6, 7 and 17: 2^128 - 1 passes, 2^128 fails
    for site, cell in ((6, ro.X_A), (6, ro.X_A + 1), (7, ro.X_B), (7, ro.X_B + 1), (17, ro.X_Q), (17, ro.X_Q + 1)):
        assert any(_own(c, cell) == B128 - 1 and len(c.patches) == 1 and c.site != site for c in cs), (site, cell)
        assert any(_own(c, cell) == B128 and len(c.patches) == 1 and c.site == site for c in cs), (site, cell)
    # site 15 on a row that is no step
    assert any(c.site == 15 and data.rows[c.target][ro.X_IS_STEP] == 0 for c in cs)
    assert any(c.site != 15 and _own(c, ro.X_R) == B128 - 1 and data.rows[c.target][ro.X_IS_STEP] == 0 for c in cs)
    # the sites that need several cells patched together
    for site in (24, 27, 29, 31):
        assert any(c.site == site and len(c.patches) > 1 for c in cs), site


def test_wrap_around_pairs(datas):
    """per circuit at least two pairs of cases that differ only in cells of the first row(s) of the rotated / padded witness and give
    different codes on its last row (Copy: also on the last but one)"""
    for name, data in datas.items():
        wraps = [c for c in data.cases if c.wrap]
        pairs = 0
        for i, a in enumerate(wraps):
            for b in wraps[i + 1:]:
                if a.target != b.target or a.patches == b.patches:
                    continue
                vs = [v for v in rsc.variants(data, a) if v in rsc.variants(data, b) and (v[1] or name == "bytecode")]
                for k, cut in vs:
                    ba, ta = rsc.build(data, a, k, cut)
                    bb, tb = rsc.build(data, b, k, cut)
                    n = len(ba.rows)
                    first = (0, 1) if name == "copy" else (0,)
                    differ = [j for j in range(n) if ba.rows[j] != bb.rows[j]]
                    if not differ or not set(differ) <= set(first):
                        continue
                    ea, eb = rsc.expected(data, ba, ta), rsc.expected(data, bb, tb)
                    if name == "copy":
                        assert ba.target == n - 1
                        if ea[n - 1] != eb[n - 1] and ea[n - 2] != eb[n - 2]:
                            pairs += 1
                    else:
                        assert ba.target == n - 1
                        if ea[n - 1] != eb[n - 1]:
                            pairs += 1
        assert pairs >= 2, (name, pairs)


def test_padded_bases_pass_the_oracle(datas):
    """every padded base the variants use was checked against the reference by the generator; here the oracle accepts them too"""
    for name, data in datas.items():
        used = set()
        for c in data.cases:
            used |= set(rsc.variants(data, c))
        assert used == data.checked, name
        for k, cut in sorted(used):
            assert not any(rsc.base_status(data, k, cut)), (name, k, cut)


@pytest.mark.parametrize("name,part", SLICES)
def test_every_case_fails_at_its_site_on_the_host(datas, hostsim, name, part):
    data = datas[name]
    ran, n_run, sites = rsc.run_slice(data, "cpu", part, N_SLICES[name], hostsim=hostsim)
    assert n_run == rsc.expected_variants(data, part, N_SLICES[name]) and ran > 0
    _ran[(name, part)] = (ran, n_run, sites)


def test_nothing_is_left_out(datas):
    """the slices above are the whole file: the slice bounds tile it, every case ran, and the sites exercised are the census"""
    assert sorted(_ran) == sorted(SLICES), "run this module as a whole"
    for name, data in datas.items():
        n, k = len(data.cases), N_SLICES[name]
        bounds = [p * n // k for p in range(k + 1)]
        assert bounds[0] == 0 and bounds[-1] == n and bounds == sorted(set(bounds))
        parts = [_ran[(name, p)] for p in range(k)]
        assert sum(p[0] for p in parts) == n
        assert sum(p[1] for p in parts) == rsc.expected_variants(data, 0, 1)
        assert sorted(set().union(*(p[2] for p in parts))) == rsc.census(data)[0]
        # every form and both index modes occur
        fs = {f for idx, c in enumerate(data.cases) for vi in range(len(rsc.variants(data, c))) for f in rsc.forms(data, idx, c, vi)}
        assert fs == ({"session", "session-generic", "ranged", "oneshot"} if name == "copy" else {"session", "ranged", "oneshot"})
