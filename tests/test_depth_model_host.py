"""`not gpu`: the depth map's model (tests/depth_model.py) on the oracle alone.  It DERIVES the tolerance tests/test_gpu_depth.py holds the
device to -- the oracle run twice on every case, as given and from the float32-rounded pose scaled by 1 + 2e-7; 4 x the largest
|delta(1 / d)| over the pixels whose four samples agree on the surface -- and holds the recorded value (depth_model.INV_DEPTH_NUDGE_MAX,
profiles/depth_parity.txt, PARITY.md) to that derivation; it checks that the oracle against its nudged self stays within a quarter of the
cap on every case; that the cases reach what the GPU test is meant to see; the strided map; the C-ABI's declarations; and that
DuckietownVecEnv refuses bad depth arguments before a device is touched."""
import os
import re

import numpy as np
import pytest

import depth_model as dm
import frame_parity as fp
from dtsim import DuckietownVecEnv, _ffi
from oracle import raster

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENVS = [(name, e) for name, c in dm.CASES.items() for e in range(len(c.states))]


def test_the_tolerance_is_the_derived_one():
    worst, at = max((dm.nudge_stats(name, e)["agree_max"], (name, e)) for name, e in ENVS)
    print(f"largest |delta(1/d)| of the nudged oracle on agreeing pixels: {worst:.6e} at {at}; tolerance {4 * worst:.6e}")
    assert worst > 0
    assert abs(worst - dm.INV_DEPTH_NUDGE_MAX) <= 1e-4 * worst, (worst, dm.INV_DEPTH_NUDGE_MAX)      # the recorded value states the derivation
    assert dm.INV_DEPTH_TOL == 4 * dm.INV_DEPTH_NUDGE_MAX
    for name, e in ENVS:                                    # enough pixels agree for the maximum to mean something
        r = dm.nudge_stats(name, e)
        assert r["agree"] >= 0.95 * r["pixels"], (name, e, r)
    # the documents quote it
    prof = open(os.path.join(ROOT, "profiles", "depth_parity.txt")).read()
    assert float(re.search(r"^maximum\s+(\S+)", prof, re.M).group(1)) == dm.INV_DEPTH_NUDGE_MAX
    assert abs(float(re.search(r"^tolerance\s+(\S+)", prof, re.M).group(1)) - dm.INV_DEPTH_TOL) <= 1e-6 * dm.INV_DEPTH_TOL
    parity = open(os.path.join(ROOT, "PARITY.md")).read()
    assert f"{dm.INV_DEPTH_NUDGE_MAX:.3e}" in parity and f"{dm.INV_DEPTH_TOL:.3e}" in parity


@pytest.mark.parametrize("name,e", ENVS)
def test_the_nudged_oracle_stays_within_a_quarter_of_the_cap(name, e):
    """The cap is the device's allowance for samples whose coverage flips at a silhouette or a seam; the oracle's own flips under a
    perturbation of the size of float32 rounding must leave three quarters of it."""
    r = dm.nudge_stats(name, e, dm.INV_DEPTH_TOL)
    assert r["beyond"] <= dm.CASES[name].cap / 4, (name, e, r)
    assert dm.CASES[name].cap == (fp.ORACLE_MESH.gt1 if dm.CASES[name].mesh else fp.ORACLE_PLANE.gt1)
    assert (fp.ORACLE_PLANE.gt1, fp.ORACLE_MESH.gt1) == (1e-3, 2e-3)


def test_the_cases_reach_what_the_device_test_is_meant_to_see():
    # planes: tile, ground and sky in every frame; the poses looking off the map edge are mostly ground under the horizon
    for name in ("planes", "planes_dr"):
        ground_share = []
        for e in range(len(dm.CASES[name].states)):
            d, s = dm.host_buffers(name, e)
            assert {-1, -2, -3} <= set(np.unique(s)), (name, e)
            assert np.isinf(dm.min_depth(d)).sum() > 1000                   # sky: all four samples
            mixed = ~(s == s[0]).all(axis=0)
            assert mixed.sum() >= 20, (name, e)                               # seam / horizon pixels, where the minimum matters
            ground_share.append(float((s == -2).all(axis=0).mean()))
        assert max(ground_share[3:]) > 0.2 and min(ground_share[:3]) < 0.1, ground_share
    cams = [dm.host_camera(dm.CASES["planes_dr"], e) for e in range(len(dm.CASES["planes_dr"].states))]
    assert len({(c.C[1], c.sth, c.ty) for c in cams}) == len(cams)          # every env its own height, pitch and fov
    # meshes: objects in view in every env; the pedestrians have moved since the map's poses
    for name in ("pedestrians", "town", "town_odd"):
        for e in range(len(dm.CASES[name].states)):
            _, s = dm.host_buffers(name, e)
            assert ((s >= 0).any(axis=0)).sum() >= 90, (name, e)
    sc = dm.scene_of("pedestrians")
    moved = [float(np.linalg.norm(st["pos"] - ob.pos)) for st, ob in zip(dm.host_objects("pedestrians")[0], sc.m.objects)]
    assert min(moved) > 0.05, moved
    assert (dm.CASES["town_odd"].W % 4, dm.CASES["town_odd"].H % 8) != (0, 0)


def test_silhouette_pixels_exist_and_the_minimum_differs_from_a_vote():
    """Pixels where the oracle has one to three samples on an object in front of the background: the minimum is the object's depth, far
    (in inverse depth) from the background's -- what a majority vote or a centre ray would report for most of them."""
    n = 0
    for name in ("pedestrians", "town"):
        for e in range(len(dm.CASES[name].states)):
            d, s = dm.host_buffers(name, e)
            sil = dm.silhouette(d, s)
            n += int(sil.sum())
            if sil.any():
                on = np.where(s >= 0, d, np.inf).min(axis=0)
                off = np.where(s < 0, d, np.inf).min(axis=0)
                assert np.array_equal(dm.min_depth(d)[sil], on[sil])
                assert (np.abs(dm.inv(on[sil]) - dm.inv(off[sil])) > 100 * dm.INV_DEPTH_TOL).all()
    assert n >= 300, n


def test_the_strided_map_is_the_slice_of_the_full_one():
    full = np.arange(dm.H * dm.W, dtype=np.float64).reshape(dm.H, dm.W)
    for sy, sx in dm.STRIDES + ((120, 160), (3, 5)):
        oh, ow = dm.H // sy, dm.W // sx
        small = dm.strided(full, sy, sx)
        assert small.shape == (oh, ow)
        want = np.array([[full[i * sy + sy // 2, j * sx + sx // 2] for j in range(ow)] for i in range(oh)])
        assert np.array_equal(small, want)
    batch = np.stack([full, full + 1])
    assert np.array_equal(dm.strided(batch, 4, 8)[1], dm.strided(full + 1, 4, 8))


@pytest.mark.parametrize("kind,border", [("fisheye", False), ("undistort", True)])
def test_the_fisheye_moves_depth_as_it_moves_ids(kind, border):
    """remap_nearest is raster.distort_ids with the fill value 0.  The simulator's own fisheye names a source inside the frame for every pixel
    at the sizes the tests use; the rectify map of undistort=True leaves a border without one."""
    rm = dm.rmap(dm.W, dm.H, kind)
    ids = np.arange(dm.H * dm.W, dtype=np.int64).reshape(dm.H, dm.W) + 1
    moved = raster.distort_ids(ids, *rm)
    got = dm.remap_nearest(ids.astype(np.float64), rm)
    assert np.array_equal(got == 0, moved == -1) and ((moved == -1).sum() > 300) == border
    assert np.array_equal(got[moved >= 0], moved[moved >= 0].astype(np.float64))
    assert (got != ids).mean() > 0.5                          # the map moves most pixels


def test_entry_points_are_declared_mirrored_and_exported():
    src = open(os.path.join(ROOT, "include", "dtsim.h")).read()
    assert re.search(r"^int dtsim_depth\(dtsim_t\* h, void\* out, int oh, int ow, uint32_t flags\);", src, re.M)
    assert re.search(r"^int dtsim_depth_masked\(dtsim_t\* h, void\* out, int oh, int ow, uint32_t flags, const uint8_t\* mask\);", src, re.M)
    m = re.search(r"DTSIM_DEPTH_F16 = (\d+)u?", src)
    assert m and int(m.group(1)) == _ffi.DEPTH_F16
    assert re.search(r"#define DTSIM_ABI_VERSION 12\b", src) and _ffi.ABI_VERSION == 12
    lib = _ffi.load()
    for name in ("dtsim_depth", "dtsim_depth_masked"):
        assert name in _ffi.EXPORTS and getattr(lib, name) is not None
    assert lib.dtsim_abi_version() == 12
    # a null handle is refused before anything touches a device
    assert lib.dtsim_depth(None, None, 1, 1, 0) == _ffi.E_INVALID
    assert lib.dtsim_depth_masked(None, None, 1, 1, 0, None) == _ffi.E_INVALID


@pytest.mark.parametrize("kw,word", [
    (dict(depth_shape=(60, 80), motion_blur=True, action_mode="wheels"), "motion_blur"),
    (dict(depth_shape=(60, 80), camera_rand=True, distortion=True), "camera_rand"),
    (dict(depth_shape=(50, 80)), "divide"),                              # 120 % 50
    (dict(depth_shape=(60, 81)), "divide"),
    (dict(depth_shape=(0, 80)), "divide"),
    (dict(depth_shape=(240, 320)), "divide"),                            # larger than the camera
    (dict(depth_shape=60), "depth_shape"),
    (dict(depth_shape=(60, 80), depth_dtype="float64"), "depth_dtype"),
    (dict(depth_dtype="half"), "depth_dtype"),
])
def test_vecenv_refuses_bad_depth_arguments_before_a_device_is_touched(kw, word, monkeypatch):
    import torch

    def touched(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(torch.cuda, "set_device", touched)
    monkeypatch.setattr(torch.cuda, "Stream", touched)
    monkeypatch.setattr(_ffi, "load", touched)
    with pytest.raises(ValueError, match=word):
        DuckietownVecEnv("small_loop", 4, camera_width=160, camera_height=120, **kw)
