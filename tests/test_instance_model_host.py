"""`not gpu`: the instance map's model and the box model (tests/instance_model.py) and the host side of dtsim_instances / dtsim_boxes, on the
oracle alone: the nearest-sample rule on hand-made buffers; that the oracle against its nudged self disagrees on at most a quarter of the cap
on every case, and nowhere on the sure mask; that the crowd views keep the occlusions they are there for (distinct ids, adjacent pixels of two
ids: at least half of what the oracle shows, recorded in profiles/instances_parity.txt) and that "inside2" never shows a hidden object; the box
model against a plain loop on random maps; the C-ABI's declarations and constants; and that DuckietownVecEnv refuses bad instance arguments
before a device is touched."""
import os
import re

import numpy as np
import pytest

import crowd_scenes as cs
import instance_model as im
from dtsim import BatchedSimulator, DuckietownVecEnv, _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENVS = [(name, e) for name, c in im.CASES.items() for e in range(c.n_envs)]
INF = np.inf


def test_nearest_sample_owner_ties_sky_and_the_plane():
    # one pixel per column: [4 samples][1][n]
    depths = np.array([[2.0, 2.0, INF, INF, 1.0, 3.0],
                       [2.0, 1.0, INF, 5.0, 1.0, 3.0],
                       [1.0, 1.0, INF, INF, np.nextafter(1.0, 0.0), 3.0],
                       [1.0, 2.0, INF, 4.0, 1.0, np.nextafter(3.0, 0.0)]])[:, None, :]
    srf = np.array([[4] * 6, [-1] * 6, [0] * 6, [63] * 6])[:, None, :]
    srf[:, 0, 2] = -3
    #   tie 2 / 3 -> sample 2: object 0;  tie 1 / 2 -> 1: the tile;  all sky;  sky loses -> 3: object 63;  one ulp nearer -> 2;  -> 3
    assert im.instances_of(depths, srf)[0].tolist() == [1, 0, 0, 64, 1, 64]
    assert im.instances_of(np.full((4, 1, 1), 0.7), np.array([7, -2, 3, 3]).reshape(4, 1, 1)).tolist() == [[8]]      # all equal: the lowest index


def test_compare_holds_the_sure_pixels_exactly_and_caps_the_rest():
    want = np.zeros((10, 100), np.uint8)
    want[2:6, 10:20] = 3
    sure = np.ones(want.shape, bool)
    sure[5, :10] = False
    got = want.copy()
    assert im.compare(got, want, sure, 1e-3)["n_off"] == 0
    got[5, 3] = 3                                             # one unsure pixel of 1000: at the cap
    assert im.compare(got, want, sure, 1e-3)["n_off"] == 1
    got[5, 4] = 4
    with pytest.raises(AssertionError):
        im.compare(got, want, sure, 1e-3)                     # two: beyond it
    got = want.copy()
    got[3, 12] = 4
    with pytest.raises(AssertionError, match="sure pixels differ"):
        im.compare(got, want, sure, 1.0)


@pytest.mark.parametrize("name,e", ENVS)
def test_the_nudged_oracle_stays_within_a_quarter_of_the_cap(name, e):
    """The condition the cap rests on: the oracle's own id flips under a perturbation of the size of float32 rounding leave three quarters of
    it, and none lies on the sure mask."""
    r = im.nudge_share(name, e)
    c = im.CASES[name]
    print(f"{name} env {e}: off {r['off']:.2e} ({r['n_off']} px), unsure {r['unsure']:.3f}, cap / 4 = {c.cap / 4:.2e}")
    assert r["sure_off"] == 0, (name, e, r)
    assert r["off"] <= c.cap / 4, (name, e, r)
    want, sure = im.expected(name, e)
    assert want.shape == (c.H, c.W) and sure.mean() > 0.5
    prof = open(os.path.join(ROOT, "profiles", "instances_parity.txt")).read()
    m = re.search(rf"^{name}\s+env {e}\s.*?off (\S+) \(\s*(\d+) px\)", prof, re.M)
    assert m and int(m.group(2)) == r["n_off"], (name, e, m and m.group(0))


def test_the_cases_reach_what_the_device_test_is_meant_to_see():
    assert not im.expected("planes", 0)[0].any()                                   # no object: all zero
    for name in ("pedestrians", "town", "town_odd"):
        assert all(im.expected(name, e)[0].any() for e in range(im.CASES[name].n_envs)), name
    assert im.CASES["town_odd"].W == 90 and im.CASES["town_odd"].H == 62
    # the two maps' envs each see an id of their own list; map 0's only ids above map 1's object count
    for m, name in enumerate(im.TWO_MAPS):
        n_obj = len(im.fp.scene(name).m.objects)
        for e in range(im.CASES["two_" + name].n_envs):
            want, sure = im.expected("two_" + name, e)
            k = im.TWO_PICKS[m][e]
            assert ((want == k + 1) & sure).sum() > 50 and want.max() <= n_obj, (name, e)     # a countable interior of its own object
    assert min(im.TWO_PICKS[0]) >= 2 and len(im.fp.scene(im.TWO_MAPS[1]).m.objects) == 4


@pytest.mark.parametrize("view", im.CROWD_VIEWS)
def test_the_crowd_views_keep_their_occlusions(view):
    """Distinct ids and 4-adjacent pixel pairs of two different non-zero ids in the expected map: at least half of what the oracle shows
    (im.CROWD_ORACLE, profiles/instances_parity.txt), through the fisheye too."""
    name = "crowd_" + view
    ids, pairs = im.crowding(im.expected(name, 0)[0])
    print(f"crowd {view}: {ids} distinct ids, {pairs} adjacent pairs of two ids")
    ref_ids, ref_pairs = im.CROWD_ORACLE[view]
    assert 2 * ids >= ref_ids and 2 * pairs >= ref_pairs, (view, ids, pairs)
    fi, fpairs = im.crowding(im.expected(name, 0, "fisheye")[0])
    assert 2 * fi >= ref_ids and 2 * fpairs >= ref_pairs, (view, fi, fpairs)
    prof = open(os.path.join(ROOT, "profiles", "instances_parity.txt")).read()
    m = re.search(rf"^{name}\s+env 0\s.*ids\s+(\d+)\s+pairs\s+(\d+)", prof, re.M)
    assert m and (int(m.group(1)), int(m.group(2))) == (ids, pairs), (view, m and m.group(0))
    if view == "far":
        assert ids >= 40                                                               # dozens of objects in one view
    if view == "inside2":
        for kind in (None, "fisheye"):
            want = im.expected(name, 0, kind)[0]
            assert not np.isin(want, np.array(cs.HIDDEN) + 1).any()                    # a hidden object's id never occurs
        assert ids >= 5


def test_the_box_model_against_a_plain_loop():
    rng = np.random.default_rng(5)
    for h, w, hi, p in ((1, 1, 3, 1.0), (1, 5, 70, 0.8), (3, 17, 255, 0.5), (7, 9, 66, 0.2), (12, 16, 255, 1.0), (5, 64, 64, 0.05)):
        for _ in range(3):
            m = (rng.integers(0, hi + 1, (h, w)) * (rng.random((h, w)) < p)).astype(np.uint8)
            got, want = im.box_model(m), im.box_brute(m)
            assert got.dtype == np.int32 and got.shape == (im.MAX_OBJECTS, 5) and np.array_equal(got, want), (h, w, hi)
            n = got[:, 4]
            assert n.sum() == ((m >= 1) & (m <= im.MAX_OBJECTS)).sum() and (got[n == 0] == 0).all()
            assert ((got[:, 2] - got[:, 0]) * (got[:, 3] - got[:, 1]) >= n).all()
    m = np.zeros((4, 6), np.uint8)
    m[1, 2] = m[3, 5] = 64
    m[0, 0] = 65                                                                       # above MAX_OBJECTS: ignored
    b = im.box_model(m[None])
    assert b.shape == (1, 64, 5) and b[0, 63].tolist() == [2, 1, 6, 4, 2] and not b[0, :63].any()


def test_entry_points_are_declared_mirrored_and_exported():
    src = open(os.path.join(ROOT, "include", "dtsim.h")).read()
    assert re.search(r"^int dtsim_instances\(dtsim_t\* h, uint8_t\* inst, uint8_t\* labels, int oh, int ow, uint32_t flags\);", src, re.M)
    assert re.search(r"^int dtsim_instances_masked\(dtsim_t\* h, uint8_t\* inst, uint8_t\* labels, int oh, int ow, uint32_t flags, const uint8_t\* mask\);", src, re.M)
    assert re.search(r"^int dtsim_boxes\(dtsim_t\* h, const uint8_t\* inst, int oh, int ow, int32_t\* out, uint32_t flags, const uint8_t\* mask\);", src, re.M)
    m = re.search(r"DTSIM_INSTANCE_NONE = (\d+)", src)
    assert m and int(m.group(1)) == _ffi.INSTANCE_NONE == 0
    m = re.search(r"#define DTSIM_MAX_OBJECTS (\d+)", src)
    assert m and int(m.group(1)) == _ffi.MAX_OBJECTS == im.MAX_OBJECTS <= 255
    assert re.search(r"#define DTSIM_ABI_VERSION 12\b", src) and _ffi.ABI_VERSION == 12
    lib = _ffi.load()
    for name in ("dtsim_instances", "dtsim_instances_masked", "dtsim_boxes"):
        assert name in _ffi.EXPORTS and getattr(lib, name) is not None
    assert lib.dtsim_abi_version() == 12
    # a null handle is refused before anything touches a device
    assert lib.dtsim_instances(None, None, None, 1, 1, 0) == _ffi.E_INVALID
    assert lib.dtsim_instances_masked(None, None, None, 1, 1, 0, None) == _ffi.E_INVALID
    assert lib.dtsim_boxes(None, None, 1, 1, None, 0, None) == _ffi.E_INVALID
    for name in ("instances", "boxes", "object_classes"):
        assert callable(getattr(BatchedSimulator, name))


@pytest.mark.parametrize("kw,word", [
    (dict(boxes=True), "instance_shape"),
    (dict(instance_shape=(60, 80), motion_blur=True, action_mode="wheels"), "motion_blur"),
    (dict(instance_shape=(60, 80), boxes=True, camera_rand=True, distortion=True), "camera_rand"),
    (dict(instance_shape=(50, 80)), "divide"),                           # 120 % 50
    (dict(instance_shape=(60, 81), boxes=True), "divide"),
    (dict(instance_shape=(0, 80)), "divide"),
    (dict(instance_shape=(240, 320)), "divide"),                         # larger than the camera
    (dict(instance_shape=60), "instance_shape"),
    (dict(instance_shape=(60, 80, 3)), "instance_shape"),
    (dict(instance_shape=("a", "b")), "instance_shape"),
    (dict(instance_shape=(60, 80), label_shape=(50, 80)), "label_shape"),    # the labels' own refusal still comes first
])
def test_vecenv_refuses_bad_instance_arguments_before_a_device_is_touched(kw, word, monkeypatch):
    import torch

    def touched(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(torch.cuda, "set_device", touched)
    monkeypatch.setattr(torch.cuda, "Stream", touched)
    monkeypatch.setattr(_ffi, "load", touched)
    with pytest.raises(ValueError, match=word):
        DuckietownVecEnv("small_loop", 4, camera_width=160, camera_height=120, **kw)
