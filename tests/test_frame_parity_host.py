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


# ---- compare_objects: the per-object and outside-the-objects bounds bite at their bounds ---------------------------------------------

OH = OW = 200           # 40000 pixels: ORACLE_MESH allows 40 beyond +-2 on the frame, more than any count below, so rows (b) and (c) decide


def _object_scene():
    """A grey frame pair and the four per-sample id arrays: object 0 owns a 20 x 20 square (400 interior pixels: 5 % + 2 = 22), object 1 a
    4 x 4 one (16: 2.8, i.e. 2), object 2 a 3 x 5 one (15 interior pixels: not judged on its own); object 3 owns only three of the four samples
    of an 8 x 8 square (no interior pixel)."""
    ref = np.full((OH, OW, 3), 100, np.uint8)
    ids = np.full((4, OH, OW), -1, np.int64)
    ids[:, 10:30, 10:30] = 0
    ids[:, 50:54, 50:54] = 1
    ids[:, 80:83, 80:85] = 2
    ids[:3, 120:128, 120:128] = 3
    return ref, ids


def _spoil(frame, ys, xs, n):
    frame[np.asarray(ys)[:n], np.asarray(xs)[:n], 1] += 3          # beyond +-2 in one channel
    return frame


def test_compare_objects_bounds_the_interior_of_each_object():
    ref, ids = _object_scene()
    assert P.ORACLE_OBJECTS == P.ObjTol(P.ORACLE_MESH, 0.05, 2.0, P.ORACLE_PLANE.gt2) and P.OBJ_MIN_INTERIOR == 16
    yy, xx = np.nonzero(P.interior(ids, 0))
    r = P.compare_objects(_spoil(ref.copy(), yy, xx, 22), ref, ids)
    assert r["judged"] == 2 and r["obj_worst"] == (0, 22, 400) and r["obj_share"] == 22 / 400 and r["outside"] == 0
    with pytest.raises(AssertionError, match="object 0: 23 of its 400 interior pixels"):
        P.compare_objects(_spoil(ref.copy(), yy, xx, 23), ref, ids, ctx="env 5")
    yy, xx = np.nonzero(P.interior(ids, 1))
    assert P.compare_objects(_spoil(ref.copy(), yy, xx, 2), ref, ids)["obj_worst"] == (1, 2, 16)
    with pytest.raises(AssertionError, match="object 1: 3 of its 16 interior pixels"):
        P.compare_objects(_spoil(ref.copy(), yy, xx, 3), ref, ids)
    # an object that is not drawn at all (what shows instead is 5 / 255 away: the frame's mean stays inside its row)
    gone = ref.copy(); gone[50:54, 50:54] = 95
    with pytest.raises(AssertionError, match="object 1: 16 of its 16"):
        P.compare_objects(gone, ref, ids)
    # objects without a countable interior are not judged on their own: rows (a) and (c) still see them
    small = ref.copy(); small[80:83, 80:85] = 95
    assert P.compare_objects(small, ref, ids)["judged"] == 2


def test_compare_objects_bounds_what_leaks_outside_the_objects():
    ref, ids = _object_scene()
    away = P.away_from_objects(ids)
    assert not away[9:31, 9:31].any() and away[8, 8] and away[31, 31] and not away[119, 119] and away[118, 118]      # one pixel around every object sample
    yy, xx = np.nonzero(away)
    assert P.compare_objects(_spoil(ref.copy(), yy, xx, 20), ref, ids)["outside"] == 20          # ORACLE_PLANE.gt2 x 40000 = 20
    with pytest.raises(AssertionError, match="21 pixels beyond \\+-2 away from every object"):
        P.compare_objects(_spoil(ref.copy(), yy, xx, 21), ref, ids)
    ring = ~away & ~(ids >= 0).any(axis=0)                                                        # the ring next to a silhouette belongs to neither row
    yy, xx = np.nonzero(ring)
    r = P.compare_objects(_spoil(ref.copy(), yy, xx, 30), ref, ids)
    assert r["outside"] == 0 and r["obj_share"] == 0.0 and r["frame"]["gt2"] == 30 / (OH * OW)
    with pytest.raises(AssertionError, match="'gt2'"):                                            # ... but to the frame's row, asserted first
        P.compare_objects(_spoil(ref.copy(), yy, xx, 41), ref, ids)


def test_tighter_divides_every_bound():
    t = P.tighter(P.ORACLE_OBJECTS, 4)
    assert t == P.ObjTol(P.Tol(5e-4, 2.5e-4, 0.0075), 0.0125, 0.5, 1.25e-4)
    assert P.tighter(P.ORACLE_MESH_GT1, 2) == P.Tol(1e-3, None, 0.015)


def test_the_raster_pair_row_bites_at_its_bounds():
    """Q_VS_V3 on 10000 pixels: 20 may differ, none by more than 1."""
    assert P.Q_VS_V3 == P.PairTol(2e-3, 1e-5)
    a = np.zeros((H, W, 3), np.uint8)
    b = a.copy(); b.reshape(-1, 3)[:20, 1] = 1
    assert P.assert_pair(a, b, P.Q_VS_V3) == (20 / (H * W), 0.0, 1)
    c = a.copy(); c.reshape(-1, 3)[:21, 1] = 1
    with pytest.raises(AssertionError):
        P.assert_pair(a, c, P.Q_VS_V3, "one too many")
    d = a.copy(); d[0, 0, 2] = 2
    with pytest.raises(AssertionError):
        P.assert_pair(a, d, P.Q_VS_V3, "one pixel beyond 1")
