"""`not gpu`: the model of the maps under per-env distortion tables (tests/camera_rand_maps_model.py), on the host alone.  Its gather through
src_index is dm.remap_nearest of the float maps the index was rounded from, for every table used; the oracle against its nudged self, through
each of the six tables, stays within what tests/test_label_model_host.py and tests/test_instance_model_host.py allow for the built-in fisheye
(a quarter of the case's cap, nothing on the sure pixels); the flag's declaration, its mirror in _ffi, and that DuckietownVecEnv takes the map
options with camera_rand when camera_rand_maps=True opts in, refuses them without it as before, and still refuses them with motion_blur,
before a device is touched."""
import os
import re

import numpy as np
import pytest

import camera_rand_maps_model as cm
import depth_model as dm
import instance_model as im
import label_model as lm
from dtsim import DuckietownVecEnv, _ffi
from dtsim import distortion as pdist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABEL_ENVS = [(n, e) for n in cm.LABEL_CASES for e in range(cm.case_of(n)[2])]
INSTANCE_ENVS = LABEL_ENVS + [("crowd_" + v, 0) for v in im.CROWD_VIEWS] + [(n, e) for n in cm.TWO_MAP_CASES for e in range(cm.case_of(n)[2])]


def test_the_calibrations_and_the_assignment():
    K, D = cm.calibrations()
    assert K.shape == (6, 3, 3) and D.shape == (6, 5)
    assert np.array_equal(K[5], pdist.CAMERA_MATRIX) and np.array_equal(D[5], pdist.DIST_COEFS)
    src = cm.tables()[0]
    assert src.shape == (6, cm.H * cm.W) and src.min() >= -1 and src.max() < cm.H * cm.W
    assert len({src[c].tobytes() for c in range(6)}) == 6                        # six different tables
    cal = cm.env_cal()
    assert cal.shape == (cm.N,) and set(cal.tolist()) == set(range(6))
    assert all(cal[e] != cal[e + 64] for e in range(cm.N - 64))                 # one state, two tables


@pytest.mark.parametrize("c", range(cm.N_CAL))
def test_the_gather_is_the_nearest_source_pixel_of_the_float_maps(c):
    """The two statements of "nearest source pixel": the integer table k_remap_cal reads, and dm.remap_nearest's rounding of the float maps,
    on a depth map, a label map and a sure mask, with each one's fill."""
    src, rx, ry = cm.tables()
    rng = np.random.default_rng(c)
    depth = rng.uniform(0.05, 40.0, (cm.H, cm.W))
    depth[rng.random((cm.H, cm.W)) < 0.1] = np.inf
    lab = rng.integers(1, 256, (cm.H, cm.W)).astype(np.uint8)
    sure = rng.random((cm.H, cm.W)) < 0.7
    for a, fill in ((depth, 0.0), (lab, 0), (sure, True)):
        got, want = cm.gather(a, src[c], fill), dm.remap_nearest(a, (rx[c], ry[c]), fill=fill)
        assert got.dtype == want.dtype and np.array_equal(got, want), (c, a.dtype)
    real = cm.expected("depth", "pedestrians", 1, c)
    assert np.array_equal(real, dm.remap_nearest(cm.rect_depth("pedestrians", 1), (rx[c], ry[c])))
    assert np.array_equal(src[c] < 0, (real == 0).reshape(-1))                   # depth 0 exactly where the table names no source


@pytest.mark.parametrize("name,e", LABEL_ENVS)
def test_the_nudged_label_oracle_stays_within_a_quarter_of_the_cap_through_every_table(name, e):
    cap = cm.case_of(name)[3]
    for c in range(cm.N_CAL):
        r = cm.nudge_share("labels", name, e, c)
        print(f"labels {name} env {e} table {c}: off {r['off']:.2e} ({r['n_off']} px), unsure {r['unsure']:.3f}, cap / 4 = {cap / 4:.2e}")
        assert r["sure_off"] == 0, (name, e, c, r)
        assert r["off"] <= cap / 4, (name, e, c, r)


@pytest.mark.parametrize("name,e", INSTANCE_ENVS)
def test_the_nudged_instance_oracle_stays_within_a_quarter_of_the_cap_through_every_table(name, e):
    cap = cm.case_of(name)[3]
    for c in range(cm.N_CAL):
        r = cm.nudge_share("instances", name, e, c)
        print(f"instances {name} env {e} table {c}: off {r['off']:.2e} ({r['n_off']} px), unsure {r['unsure']:.3f}, cap / 4 = {cap / 4:.2e}")
        assert r["sure_off"] == 0, (name, e, c, r)
        assert r["off"] <= cap / 4, (name, e, c, r)


def test_the_model_restates_the_existing_ones():
    """The rectilinear maps are the existing models' own: depth_model.expected(rmap=None), and instance_model's rule on the label cases it
    does not list."""
    for name in ("pedestrians", "town"):
        for e in range(cm.case_of(name)[2]):
            want = dm.expected(dm.host_camera(dm.CASES[name], e), dm.scene_of(name), dm.host_objects(name)[e])
            assert np.array_equal(cm.rect_depth(name, e), want)
            assert cm.rect_instances(name, e)[0].tobytes() == im.expected(name, e)[0].tobytes()
    assert not cm.rect_instances("planes_dr", 0)[0].any() and not cm.rect_instances("marks_straight", 0)[0].any()      # small_loop: no objects
    assert cm.rect_labels("marks_straight", 0)[0].tobytes() == lm.expected("marks_straight", 0)[0].tobytes()


def test_the_flag_is_declared_mirrored_and_refused_on_a_null_handle():
    src = open(os.path.join(ROOT, "include", "dtsim.h")).read()
    m = re.search(r"^#define DTSIM_MAP_ENV_TABLES (0x[0-9a-fA-F]+)u", src, re.M)
    assert m and int(m.group(1), 16) == _ffi.MAP_ENV_TABLES == 0x100
    assert _ffi.MAP_ENV_TABLES & (_ffi.DEPTH_F16 | 2) == 0                        # clear of the values the existing tests use
    assert re.search(r"#define DTSIM_ABI_VERSION 12\b", src) and _ffi.ABI_VERSION == 12
    lib = _ffi.load()
    f = _ffi.MAP_ENV_TABLES
    assert lib.dtsim_depth(None, None, 1, 1, f) == _ffi.E_INVALID and lib.dtsim_depth_masked(None, None, 1, 1, f, None) == _ffi.E_INVALID
    assert lib.dtsim_labels(None, None, 1, 1, f) == _ffi.E_INVALID and lib.dtsim_labels_masked(None, None, 1, 1, f, None) == _ffi.E_INVALID
    assert lib.dtsim_instances(None, None, None, 1, 1, f) == _ffi.E_INVALID
    assert lib.dtsim_instances_masked(None, None, None, 1, 1, f, None) == _ffi.E_INVALID


CAMERA_RAND = dict(camera_rand=True, distortion=True, camera_width=160, camera_height=120)


def test_vecenv_takes_the_map_options_with_camera_rand_when_opted_in(monkeypatch):
    """With camera_rand_maps=True the argument checks pass (they come before a device is touched): the first thing that fails is the device.
    Without it the combination raises ValueError, naming the option."""
    import torch

    class Touched(Exception):
        pass

    def touched(*a, **k):
        raise Touched
    monkeypatch.setattr(torch.cuda, "set_device", touched)
    monkeypatch.setattr(torch.cuda, "Stream", touched)
    monkeypatch.setattr(_ffi, "load", touched)
    for kw in (dict(depth_shape=(60, 80)), dict(label_shape=(60, 80)), dict(instance_shape=(30, 40), boxes=True),
               dict(depth_shape=(30, 40), label_shape=(30, 40), instance_shape=(30, 40), boxes=True, final_obs=True)):
        with pytest.raises(Touched):
            DuckietownVecEnv("small_loop", 4, camera_rand_maps=True, **kw, **CAMERA_RAND)
        with pytest.raises(ValueError, match="camera_rand_maps=True"):
            DuckietownVecEnv("small_loop", 4, **kw, **CAMERA_RAND)
    with pytest.raises(Touched):                             # the option alone changes no check
        DuckietownVecEnv("small_loop", 4, camera_rand_maps=True, **CAMERA_RAND)


@pytest.mark.parametrize("kw,word", [
    (dict(depth_shape=(60, 80)), "motion_blur"),
    (dict(label_shape=(60, 80)), "motion_blur"),
    (dict(instance_shape=(60, 80), boxes=True), "motion_blur"),
    (dict(depth_shape=(50, 80), motion_blur=False), "divide"),
])
def test_vecenv_still_refuses_motion_blur_and_bad_sizes_with_camera_rand(kw, word, monkeypatch):
    import torch

    def touched(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(torch.cuda, "set_device", touched)
    monkeypatch.setattr(torch.cuda, "Stream", touched)
    monkeypatch.setattr(_ffi, "load", touched)
    kw = dict(dict(motion_blur=True, action_mode="wheels"), **kw)
    if not kw["motion_blur"]:
        kw.pop("action_mode")
    with pytest.raises(ValueError, match=word):
        DuckietownVecEnv("small_loop", 4, camera_rand_maps=True, **kw, **CAMERA_RAND)
