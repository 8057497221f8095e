"""The host-side rules of the secp256k1 lane forms (csrc/secp_lanes.hpp), through hostsim: which form a batch runs in and how many
lanes of key tables it gets (secp_lane_form), and the launches of a batch over those tables (secp_chunk).  Every other test sets
ZK_ECDSA_LANES, so the rules by batch size are pinned only here."""
import ctypes

import numpy as np
import pytest

K14, K15, K16, K17 = 1 << 14, 1 << 15, 1 << 16, 1 << 17
CAP = K17  # ZK_ECDSA_CHUNK_LANES

# the form by batch size: quads up to 2^14 signatures, pairs up to 2^16, one lane beyond
AUTO = {0: 4, 1: 4, K14: 4, K14 + 1: 2, K16: 2, K16 + 1: 1, K15 + 67: 2, K17 + 1: 1}
# ZK_ECDSA_LANES: "4" and "2" choose that form, anything else one lane
FORCED = {None: None, "1": 1, "2": 2, "4": 4, "3": 1}
# lanes of key tables: n * lanes rounded up to 64, at least 64, at most CAP
QTAB = {
    (0, 1): 64, (0, 2): 64, (0, 4): 64,
    (1, 1): 64, (1, 2): 64, (1, 4): 64,
    (K14, 1): 16384, (K14, 2): 32768, (K14, 4): 65536,
    (K14 + 1, 1): 16448, (K14 + 1, 2): 32832, (K14 + 1, 4): 65600,
    (K16, 1): 65536, (K16, 2): CAP, (K16, 4): CAP,
    (K16 + 1, 1): 65600, (K16 + 1, 2): CAP, (K16 + 1, 4): CAP,
    (K15 + 67, 1): 32896, (K15 + 67, 2): 65728, (K15 + 67, 4): CAP,
    (K17 + 1, 1): CAP, (K17 + 1, 2): CAP, (K17 + 1, 4): CAP,
}  # fmt: skip


def _lane_form(hostsim, n, comb, forced):
    lanes, qtab = ctypes.c_uint32(0), ctypes.c_uint64(0)
    hostsim.sim_secp_lane_form.restype = None
    hostsim.sim_secp_lane_form(ctypes.c_uint64(n), ctypes.c_uint32(1 if comb else 0), ctypes.c_char_p(forced.encode() if forced else None),
                               ctypes.byref(lanes), ctypes.byref(qtab))
    return lanes.value, qtab.value


@pytest.mark.parametrize("comb", [True, False])
@pytest.mark.parametrize("forced", list(FORCED))
@pytest.mark.parametrize("n", list(AUTO))
def test_lane_form(hostsim, n, forced, comb):
    lanes = FORCED[forced] or AUTO[n]
    if lanes == 4 and not comb:  # the four-lane form takes u1 G from the comb table
        lanes = 2
    assert _lane_form(hostsim, n, comb, forced) == (lanes, QTAB[n, lanes])


def test_lane_form_edges(hostsim):
    assert _lane_form(hostsim, 0, True, None) == (4, 64)  # an empty batch still has one wavefront's tables
    assert _lane_form(hostsim, K15 + 67, True, "4") == (4, K17)  # 131,340 lanes: capped
    assert _lane_form(hostsim, K14, False, None) == (2, 2 * K14)  # quads without a comb table: pairs
    assert _lane_form(hostsim, K14, False, "4") == (2, 2 * K14)


CHUNK_CASES = [(n, lanes, 1) for n in (1, 63, 65) for lanes in (1, 2, 4)] + [(K15 + 67, 4, 2), (K16 + 1, 2, 2), (K17 + 1, 1, 2)]


@pytest.mark.parametrize("n,lanes,launches", CHUNK_CASES)
def test_chunk_plan(hostsim, n, lanes, launches):
    got_lanes, qtab = _lane_form(hostsim, n, True, str(lanes))
    assert got_lanes == lanes
    out = np.zeros((8, 4), dtype=np.uint64)
    hostsim.sim_secp_chunks.restype = ctypes.c_uint64
    cnt = hostsim.sim_secp_chunks(ctypes.c_uint64(n), ctypes.c_uint64(qtab), ctypes.c_uint32(lanes), ctypes.c_void_p(out.ctypes.data), ctypes.c_uint64(8))
    assert cnt == launches
    per_chunk = qtab // lanes
    at = 0
    for first, count, grid, block in out[:cnt].tolist():
        assert first == at and 1 <= count <= per_chunk  # [0, n) exactly once, in order
        at += count
        waves = (count * lanes + 63) // 64
        assert (grid, block) == (((waves + 3) // 4, 256) if lanes == 4 else (waves, 64))
    assert at == n
    if launches == 2:
        assert out[0, 1] == per_chunk and out[1, 1] == n - per_chunk
