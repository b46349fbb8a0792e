"""`not gpu`: tests/frame_parity.py -- the tolerance table bites exactly at its bounds, and stats() is what its docstring says.

Synthetic 100 x 100 x 3 uint8 pairs: 10000 pixels and 30000 channel values, so every bound of the table is a whole number of pixels
(1e-3 = 10 pixels) or of channel values off by one (mean 0.02 = 600).  The counts below are the table restated in those units."""
import numpy as np
import pytest

import frame_parity as P

H = W = 100
ROWS = {    # row: (pixels beyond +-1, pixels beyond +-2, channel values off by one) AT the bound; None: not asserted
    "ORACLE_PLANE": (P.ORACLE_PLANE, (10, 5, 600)),
    "ORACLE_MESH": (P.ORACLE_MESH, (20, 10, 900)),
    "ORACLE_MESH_GT1": (P.ORACLE_MESH_GT1, (20, None, 900)),
    "ORACLE_TINY": (P.ORACLE_TINY, (40, None, 1500)),
    "GOURAUD_CROSS": (P.GOURAUD_CROSS, (None, 100, 15000)),
    "REFERENCE_GL": (P.REFERENCE_GL, (100, 40, 10500)),
    "ORACLE_GL": (P.ORACLE_GL, (20, None, 600)),
    "ORACLE_PIXEL_GL": (P.ORACLE_PIXEL_GL, (20, None, 6000)),
    "FACADE_LIGHT": (P.FACADE_LIGHT, (None, 10, 1500)),
    "FACADE_TOP_DOWN": (P.FACADE_TOP_DOWN, (30, None, 1500)),
    "FACADE_OVERLAY": (P.FACADE_OVERLAY, (None, 30, 3000)),
    "FACADE_BBOX": (P.FACADE_BBOX, (None, 100, 9000)),
    "overlay_lines_tol": (P.overlay_lines_tol(100, W, H), (None, 10, 1500)),       # 5e-4 + 0.05 * 100 / 10000 = 1e-3
    "leds_tol": (P.leds_tol(200, W, H), (None, 30, 3000)),                          # 2e-3 + 0.05 * 200 / 10000 = 3e-3
}
CASES = [(name, q) for name, (_tol, at) in ROWS.items() for q in range(3) if at[q] is not None]


def _pair(q, n):
    """A frame pair in which quantity q (0: gt1, 1: gt2, 2: mean) counts n and the other two stay far inside any row."""
    a, b = np.zeros((H, W, 3), np.uint8), np.zeros((H, W, 3), np.uint8)
    if q == 2:
        b.reshape(-1)[:n] = 1                              # n channel values off by one: no pixel beyond +-1
    else:
        b.reshape(-1, 3)[:n, 0] = 2 + q                    # n pixels off by 2 (beyond +-1 only) or by 3 (beyond +-2 too) in one channel
    return a, b


def test_the_table_has_no_row_this_file_leaves_out():
    named = {k for k, v in vars(P).items() if isinstance(v, P.Tol)}
    assert named == set(ROWS) - {"overlay_lines_tol", "leds_tol"}
    assert all(tol.count(None) <= 1 for tol, _at in ROWS.values())                  # every row asserts two quantities at least


@pytest.mark.parametrize("name,q", CASES, ids=[f"{n}-{P.Tol._fields[q]}" for n, q in CASES])
def test_each_bound_passes_at_the_bound_and_fails_one_beyond(name, q):
    tol, at = ROWS[name]
    key = P.Tol._fields[q]
    s = P.stats(*_pair(q, at[q]))
    assert s[key] == at[q] / (H * W * (3 if q == 2 else 1))
    P.assert_within(s, tol, name)
    with pytest.raises(AssertionError, match=f"'{name}', '{key}', "):               # the message: context, the quantity that failed, the bound, all stats
        P.assert_within(P.stats(*_pair(q, at[q] + 1)), tol, name)


@pytest.mark.parametrize("name", [n for n, (tol, _at) in ROWS.items() if None in tol])
def test_a_quantity_a_row_leaves_out_is_not_checked(name):
    tol, _at = ROWS[name]
    s = {key: float("inf") if bound is None else bound for key, bound in zip(P.Tol._fields, tol)}
    P.assert_within(s, tol, name)


def test_stats_on_a_hand_computed_pair():
    a = np.array([[[10, 10, 10], [0, 0, 0]], [[255, 0, 0], [5, 5, 5]]], np.uint8)
    b = np.array([[[10, 12, 10], [3, 0, 0]], [[246, 0, 0], [5, 5, 5]]], np.uint8)
    # per-pixel largest channel error: 2, 3 / 9, 0 (255 - 246 = 9: no uint8 wrap-around); channel errors sum to 2 + 3 + 9 = 14 of 12 values
    assert P.stats(a, b) == dict(mean=14 / 12, gt1=3 / 4, gt2=2 / 4, gt8=1 / 4, max=9)
    mask = np.array([[False, False], [True, False]])                                 # the 9 left out: 3 pixels, 9 values
    assert P.stats(a, b, mask) == dict(mean=5 / 9, gt1=2 / 3, gt2=1 / 3, gt8=0.0, max=3)
    assert P.stats(b, a) == P.stats(a, b) and P.stats(a, a)["max"] == 0
