"""camera_rand on the MI355X: per-env fisheye calibrations (dtsim_set_distortion_luts + k_remap_cal).

Anchor: the nominal calibration installed for every env through the per-env tables gives the bytes of the folded fisheye
(distortion=True) -- the raster renders each output pixel as the ray of its rectilinear source pixel either way.  Per env:
the camera_rand frame of env e is exactly the distortion=False frame of the same state remapped on the host through env
e's tables (the scalar remap at an odd size too), and within the fisheye oracle tolerance of oracle.raster.render_obs.  Masked
renders, the vectorised env, the gym facade, the device reset sampler with undistort=True."""
import math

import numpy as np
import pytest

from dtsim import BatchedSimulator, DuckietownVecEnv, _ffi, assets
from dtsim import distortion as pdist
from frame_parity import ORACLE_MESH, assert_within, stats
from oracle import raster, sim as osim

pytestmark = pytest.mark.gpu


def _acts(T, N, seed=1):
    return np.random.default_rng(seed).uniform(0.2, 0.7, (T, N, 2)).astype(np.float32)


@pytest.mark.parametrize("dr", [False, True])
def test_anchor_nominal_tables_equal_the_folded_fisheye(dr):
    N, W, H = 40, 640, 480
    m = "loop_pedestrians" if dr else "loop_only_duckies"
    sim = BatchedSimulator(m, N, camera_width=W, camera_height=H, domain_rand=dr, distortion=True, seed=5, max_steps=100000)
    sim.step(_acts(4, N), n_steps=4)
    sim.render()
    fold = sim.frames_host()
    if not dr:
        sim.render(segment=True)
        fold_seg = sim.frames_host()
    sim.set_camera_calibrations(pdist.CAMERA_MATRIX[None], pdist.DIST_COEFS[None], np.zeros(N, np.int32))
    sim.render()
    remap = sim.frames_host()
    assert np.array_equal(remap, fold), float((remap != fold).any(axis=-1).mean())
    if not dr:
        sim.render(segment=True)
        remap_seg = sim.frames_host()
        assert np.array_equal(remap_seg, fold_seg), float((remap_seg != fold_seg).any(axis=-1).mean())
    sim.close()


def _pair(W, H, N=64, P=8, seed=3):
    a = BatchedSimulator("loop_only_duckies", N, camera_width=W, camera_height=H, domain_rand=False, distortion=True, camera_rand=True,
                         camera_rand_pool=P, seed=seed, max_steps=100000)
    b = BatchedSimulator("loop_only_duckies", N, camera_width=W, camera_height=H, domain_rand=False, distortion=False, camera_rand=True,
                         per_env_camera=True, seed=seed, max_steps=100000)
    return a, b


@pytest.mark.parametrize("size", [(640, 480), (160, 120)])
def test_per_env_calibrations_equal_host_remap(size):
    W, H = size
    N, P = 64, 8
    a, b = _pair(W, H, N, P)
    K, D, new_K, env_cal = a.camera_calibrations
    assert K.shape == (P, 3, 3) and np.array_equal(env_cal, np.arange(N) % P)
    for e in range(N):
        assert bytes(a.init_states[e]) == bytes(b.init_states[e])
    assert len({a.init_states[e].cam_height for e in range(N)}) > 1           # the camera draws took effect
    assert all(list(a.init_states[e].camera_noise) == [0.0, 0.0, 0.0] for e in range(N))
    acts = _acts(3, N, 2)
    a.step(acts, n_steps=3)
    b.step(acts, n_steps=3)
    a.render()
    b.render()
    fa, fb = a.frames_host(), b.frames_host()
    _, rx, ry = pdist.build_src_index(K, D, W, H, return_maps=True)
    for e in range(N):
        c = int(env_cal[e])
        want = raster.distort(fb[e], rx[c], ry[c])
        assert np.array_equal(fa[e], want), (e, float((fa[e] != want).any(axis=-1).mean()))
    a.close()
    b.close()


@pytest.mark.parametrize("size", [(640, 480), (160, 120)])
def test_per_env_calibrations_against_the_oracle(size):
    W, H = size
    N, P = 64, 8
    a, b = _pair(W, H, N, P)
    b.close()
    K, D, _, env_cal = a.camera_calibrations
    a.step(_acts(3, N, 2), n_steps=3)
    a.render()
    fa = a.frames_host()
    _, rx, ry = pdist.build_src_index(K, D, W, H, return_maps=True)
    om = osim.OracleMap(assets.get_map("loop_only_duckies"), assets.mesh_extents(("duckie",)))
    scene = raster.Scene(om, {t["kind"]: assets.get_texture(t["kind"]) for t in om.grid if t is not None},
                         {"duckie": assets.get_mesh("duckie"), "*": assets.get_mesh("*")})
    pos, ang = a.read(_ffi.FIELD_POS), a.read(_ffi.FIELD_ANGLE)
    vis = a.read(_ffi.FIELD_OBJ_VISIBLE)
    for e in (0, 13):
        st, c = a.init_states[e], int(env_cal[e])
        cam = raster.Camera(pos[e], ang[e], cam_height=st.cam_height, cam_angle_deg=st.cam_angle_deg, cam_fov_y_deg=st.cam_fov_y_deg,
                            horizon_color=list(st.horizon_color), ground_color=list(st.ground_color), width=W, height=H)
        objs = [dict(pos=o.pos, y_rot=o.y_rot, visible=bool(vis[e][k])) for k, o in enumerate(scene.m.objects)]
        # camera_rand renders through the per-env camera path (k_raster_v3dr): the per-channel light of "pixel-dr", as per_env_camera
        ref = raster.render_obs(cam, scene, "pixel-dr", (rx[c], ry[c]), obj_states=objs)
        assert_within(stats(fa[e], ref), ORACLE_MESH, e)
    a.close()


def test_scalar_remap_at_an_odd_size():
    """H * W % 4 != 0: k_remap_cal's one-pixel-per-lane instantiation (the generic per-env raster feeds it)."""
    W, H, N, P = 161, 121, 16, 4
    a, b = _pair(W, H, N, P)
    K, D, _, env_cal = a.camera_calibrations
    acts = _acts(3, N, 6)
    a.step(acts, n_steps=3)
    b.step(acts, n_steps=3)
    a.render()
    b.render()
    fa, fb = a.frames_host(), b.frames_host()
    _, rx, ry = pdist.build_src_index(K, D, W, H, return_maps=True)
    for e in range(N):
        c = int(env_cal[e])
        assert np.array_equal(fa[e], raster.distort(fb[e], rx[c], ry[c])), e
    a.close()
    b.close()


def test_facade_camera_rand():
    from gym_duckietown.simulator import Simulator
    envs = [Simulator(map_name="loop_only_duckies", camera_rand=True, distortion=True, domain_rand=False, seed=12, camera_width=160,
                      camera_height=120) for _ in range(2)]
    K, D, new_K, env_cal = envs[0]._sim.camera_calibrations
    cm = envs[0].camera_model
    assert np.array_equal(cm.camera_matrix, K[0]) and np.array_equal(cm.distortion_coefs.reshape(-1), D[0])
    assert np.array_equal(cm.new_camera_matrix, new_K[0]) and not np.array_equal(K[0], pdist.CAMERA_MATRIX)
    obs = [e.reset() for e in envs]
    assert np.array_equal(obs[0], obs[1]) and 0 < obs[0].mean() < 255
    for _ in range(3):
        obs = [e.step(np.array([0.4, 0.5]))[0] for e in envs]
        assert np.array_equal(obs[0], obs[1])
    assert np.array_equal(obs[0], envs[0]._sim.frames_host()[0])
    for e in envs:
        e.close()


def test_device_resets_with_undistort_scale_the_camera():
    """camera_rand + undistort=True installs no per-env tables; the device reset sampler still scales the camera and draws no noise."""
    N = 32
    sim = BatchedSimulator("loop_only_duckies", N, camera_width=160, camera_height=120, domain_rand=False, distortion=True, camera_rand=True,
                           undistort=True, device_reset=True, seed=2)
    assert sim.camera_calibrations is None
    cam = sim.read(_ffi.FIELD_CAMERA).astype(np.float64)
    assert np.all(cam[:, 3:6] == 0.0) and len(np.unique(cam[:, 0])) > 1
    sim.skip_distort(True)
    sim.reset()
    cam = sim.read(_ffi.FIELD_CAMERA).astype(np.float64)
    assert np.all(cam[:, 3:6] == 0.0) and len(np.unique(cam[:, 0])) > 1
    sim.close()


def test_masked_render_remaps_only_the_masked_envs():
    import torch
    N, W, H = 64, 160, 120
    a = BatchedSimulator("loop_only_duckies", N, camera_width=W, camera_height=H, domain_rand=False, distortion=True, camera_rand=True,
                         camera_rand_pool=8, seed=4, max_steps=100000)
    a.render()
    before = a.frames_host()
    a.step(_acts(8, N, 5), n_steps=8)                       # past the 5-step actuation delay
    sel = np.zeros(N, bool)
    sel[::3] = True
    a.render(mask=torch.as_tensor(sel.astype(np.uint8), device=f"cuda:{a.device_index}"))
    masked = a.frames_host()
    assert np.array_equal(masked[~sel], before[~sel])
    a.render()
    full = a.frames_host()
    assert np.array_equal(masked[sel], full[sel])
    assert not np.array_equal(full[sel], before[sel])
    a.close()


@pytest.mark.parametrize("dr,final_obs", [(False, False), (True, False), (False, True)])
def test_vecenv_camera_rand(dr, final_obs):
    import torch
    N, T = 32, 12
    kw = dict(num_envs=N, obs_shape=(60, 80), camera_width=160, camera_height=120, distortion=True, camera_rand=True,
              domain_rand=dr, final_obs=final_obs, seed=9, max_steps=5)
    envs = [DuckietownVecEnv("loop_only_duckies", **kw) for _ in range(2)]
    cal0 = envs[0].sim.camera_calibrations[3].copy()
    obs = [e.reset() for e in envs]
    assert torch.equal(obs[0], obs[1])
    acts = torch.as_tensor(np.random.default_rng(0).uniform(-0.5, 1.0, (T, N, 2)).astype(np.float32))
    n_done = 0
    for t in range(T):
        outs = [e.step(acts[t]) for e in envs]
        assert torch.equal(outs[0][0], outs[1][0]), t
        n_done += int(outs[0][2].sum())
        if final_obs:
            m = outs[0][3]["final_obs_mask"]
            assert torch.equal(outs[0][3]["final_obs"][m], outs[1][3]["final_obs"][m]), t
    torch.cuda.synchronize()
    assert n_done > 0                                                           # device resets happened (max_steps=5)
    assert np.array_equal(envs[0].sim.camera_calibrations[3], cal0)             # the env -> calibration assignment stays
    cam = envs[0].sim.read(_ffi.FIELD_CAMERA).astype(np.float64)
    if not dr:
        eps = 1e-6
        assert np.all((cam[:, 0] >= 0.108 * 0.92 - eps) & (cam[:, 0] <= 0.108 * 1.08 + eps))
        assert np.all((cam[:, 1] >= math.radians(19.15 * 0.8) - eps) & (cam[:, 1] <= math.radians(19.15 * 1.2) + eps))
        assert np.all((cam[:, 2] >= math.radians(75 * 0.8) - eps) & (cam[:, 2] <= math.radians(75 * 1.2) + eps))
        assert np.all(cam[:, 3:6] == 0.0)
        assert len(np.unique(cam[:, 0])) > 1
    for e in envs:
        e.close()
