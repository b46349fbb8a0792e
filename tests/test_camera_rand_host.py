"""`not gpu`: camera_rand's host half -- the calibration sampler (the reference's ranges, its own RNG stream), the reset
draws it changes, the fast remap-table builder of libdtsim (bit-identical to the numpy statement of dtsim/distortion.py
for any K and D) and the combinations the facade / BatchedSimulator refuse before any launch."""
import copy

import numpy as np
import pytest

from dtsim import BatchedSimulator, _ffi, assets, maps, reset as R
from dtsim import distortion as pdist
from oracle import distortion as odist


def test_sampler_within_the_reference_ranges_and_deterministic():
    K, D = pdist.sample_calibrations(256, seed=7)
    assert K.shape == (256, 3, 3) and D.shape == (256, 5)
    rg = pdist.camera_rand_ranges()
    vals = {"fx": K[:, 0, 0], "fy": K[:, 1, 1], "cx": K[:, 0, 2], "cy": K[:, 1, 2],
            "k1": D[:, 0], "k2": D[:, 1], "p1": D[:, 2], "p2": D[:, 3], "k3": D[:, 4]}
    for k, v in vals.items():
        lo, hi = min(rg[k]), max(rg[k])
        assert np.all((v >= lo) & (v <= hi)), k
    assert rg["k1"][0] > rg["k1"][1] and rg["p2"][0] > rg["p2"][1]       # the negative coefficients' (high, low) bounds
    assert np.all(D[:, 4] == 0.0)
    assert np.all(K[:, 2] == [0, 0, 1]) and np.all(K[:, 0, 1] == 0) and np.all(K[:, 1, 0] == 0)
    K2, D2 = pdist.sample_calibrations(256, seed=7)
    assert np.array_equal(K, K2) and np.array_equal(D, D2)
    K3, _ = pdist.sample_calibrations(256, seed=8)
    assert not np.array_equal(K, K3)
    assert len({tuple(k.ravel()) for k in K}) == 256                     # every env its own calibration


def test_sampler_leaves_env_generators_alone():
    es = R.EnvResetState(3)
    before = copy.deepcopy(es.np_random.bit_generator.state)
    pdist.sample_calibrations(4, seed=3)
    assert es.np_random.bit_generator.state == before


@pytest.mark.parametrize("dr", [False, True])
def test_draw_prefix_camera_rand_same_draws_only_camera_differs(dr):
    mt = maps.interpret_map(assets.get_map("loop_only_duckies"), "loop_only_duckies")
    out = {}
    for cr in (False, True):
        es = R.EnvResetState(11)
        st, tile, vis = R.draw_prefix(es, mt, domain_rand=dr, camera_rand=cr, dynamics_rand=False, color_sky=list(R.BLUE_SKY),
                                      color_ground=(0.15, 0.15, 0.15), num_tris_distractors=12, n_visible_draw=(), user_tile_start=None)
        out[cr] = (bytes(st), tile, vis, es.np_random.bit_generator.state)
    assert out[False][1:] == out[True][1:]                               # same tile, visibility and RNG position
    a = _ffi.InitState.from_buffer_copy(out[False][0])
    b = _ffi.InitState.from_buffer_copy(out[True][0])
    for name, _ in _ffi.InitState._fields_:
        va, vb = getattr(a, name), getattr(b, name)
        va, vb = (list(va), list(vb)) if hasattr(va, "__len__") else (va, vb)
        if name in ("cam_height", "cam_angle_deg", "cam_fov_y_deg") and not dr:
            assert va != vb, name
        else:
            assert va == vb, name


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def test_fast_builder_nominal_bit_identical():
    src, rx, ry = pdist.build_src_index(pdist.CAMERA_MATRIX[None], pdist.DIST_COEFS[None], 640, 480, return_maps=True)
    px, py = pdist.distortion_maps(640, 480)
    ox, oy = odist.distortion_maps(640, 480)
    assert _same(rx[0], px) and _same(ry[0], py)
    assert _same(rx[0], ox) and _same(ry[0], oy)


@pytest.mark.parametrize("size", [(640, 480), (160, 120)])
def test_fast_builder_sampled_bit_identical(size):
    W, H = size
    K, D = pdist.sample_calibrations(4, seed=21)
    src, rx, ry = pdist.build_src_index(K, D, W, H, return_maps=True)
    for i in range(4):
        ex, ey = pdist.calibration_maps(K[i], D[i], W, H)
        assert _same(rx[i], ex) and _same(ry[i], ey), i
        sx, sy = np.rint(ex), np.rint(ey)
        inside = ~np.isnan(sx) & ~np.isnan(sy) & (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
        want = np.where(inside, np.nan_to_num(sy) * W + np.nan_to_num(sx), -1).astype(np.int64)
        assert np.array_equal(src[i], want), i


def test_fast_builder_fills_holes_in_the_set_order():
    """The hole fill depends on the visiting order; the nominal table has holes, the fill must land on fill_holes'."""
    newK = pdist.optimal_new_camera_matrix()
    mx, my = pdist.rectify_maps(pdist.CAMERA_MATRIX, pdist.DIST_COEFS, newK, (640, 480))
    rx, _ = pdist.invert_map(mx, my)
    assert np.isnan(rx).sum() > 0
    assert len(pdist.hole_order(rx)) == int(np.isnan(rx).sum())


def test_facade_camera_rand_combinations_refused():
    from gym_duckietown.simulator import Simulator
    with pytest.raises(NotImplementedError, match="distortion=True"):
        Simulator(map_name="small_loop", camera_rand=True)
    for kw in ({"enable_leds": True}, {"draw_curve": True}, {"draw_bbox": True}):
        with pytest.raises(ValueError):
            Simulator(map_name="small_loop", camera_rand=True, distortion=True, **kw)
    with pytest.raises(ValueError, match="light_capture"):
        BatchedSimulator("small_loop", 2, camera_rand=True, distortion=True, light_capture=True)
