"""light_capture=True with domain_rand=False (DTSIM_F_LIGHT_CAPTURE on the shared camera, ABI v12): from the second episode on, the reference
lights each env with the light reset() handed to glLightfv, taken through the camera of the previous episode's last frame (simulator.py:565-584,
1758-1803) -- an eye-space light of its own per env.  The shared-camera render pipeline (the LIGHT instantiations of k_raster_v3 / k_raster_q,
the generic raster through EnvCam) lights every env with its own light in this mode; the default (light_capture=False) is unchanged.

Against the reference itself: the later-episode goldens (last frame before each reset() of the reference on Mesa llvmpipe, first frame after:
`ref_gl_episode2_*` and tests/golden/lightcap_*, made by tests/golden/make_lightcap.py), the first-episode goldens and the reference's
DuckietownEnv driven over several episodes (`lightcap_flow`), at the tolerance of tests/test_gpu_gl_golden.py; at full size against the oracle (oracle/raster.py, "pixel" mode) with
each env's light, at the tolerances of tests/test_gpu_baseline_configs.py.
"""
import ctypes as C

import numpy as np
import pytest

import gl_golden as G
from dtsim import BatchedSimulator, _ffi
from dtsim import distortion as pdist
from frame_parity import (GL_FILTER_DIFFER, ORACLE_MESH, ORACLE_MESH_GT1, ORACLE_PLANE, REFERENCE_GL, assert_within, compare_envs, frames_of, scene,
                          stats, stratified_picks)
from gl_golden import LIGHTCAP_FLOW as FLOW, LIGHTCAP_RESET_CASES as LIGHTCAP_CASES, load_lightcap
from oracle.gl import asset_trees

pytestmark = pytest.mark.gpu
FIRST_LIGHT = np.array([0.0, 3.0, 0.0, 1.0])
# the shared-camera cases of the GL goldens: first-episode frames and the episode-2 golden (the window views go through the facade)
SHARED_CASES = [c for c in G.cases() if "_dr_" not in c and not c.startswith(("view_", "trajectory_", "segment_"))] + LIGHTCAP_CASES


def _load(case):
    return load_lightcap(case) if case.startswith("lightcap_") else G.load(case)


def _set_state(st, d, k, light):
    st.pos[:] = [float(v) for v in d["pos"][k]]
    st.angle = float(d["angle"][k])
    st.cam_height, st.cam_angle_deg, st.cam_fov_y_deg = float(d["cam_height"][k]), float(d["cam_angle"][k]), float(d["cam_fov_y"][k])
    st.camera_noise[:] = [float(v) for v in d["camera_noise"][k]]
    st.horizon_color[:] = [float(v) for v in d["horizon"][k]]
    st.ground_color[:] = [float(v) for v in d["ground"][k]]
    st.light_pos[:] = [float(v) for v in light[k]]
    st.light_ambient[:] = [float(v) for v in d["light_ambient"][k]]
    st.light_diffuse[:] = [float(v) for v in d["light_diffuse"][k]]
    return st


def _render_golden(d, light_capture=True, per_env_camera=False, gl_filter=False):
    """The golden's states uploaded through dtsim_reset(states), each with the eye-space light GL held for it (light_eye)."""
    m = d["meta"]
    n = len(d["frame"])
    sim = BatchedSimulator(m["map_name"], n, asset_root=asset_trees.tree(m["tree"]), camera_width=int(m["W"]), camera_height=int(m["H"]),
                           distortion=False, domain_rand=False, seed=1, max_steps=1000000, light_capture=light_capture,
                           per_env_camera=per_env_camera)
    for k in range(n):
        _set_state(sim.init_states[k], d, k, d["light_eye"])
    sim.reset(states=sim.init_states)
    nobj = d["obj_visible"].shape[1]
    if nobj:
        vis = sim.read(_ffi.FIELD_OBJ_VISIBLE)
        vis[:, :nobj] = d["obj_visible"].astype(np.uint8)
        sim.write(_ffi.FIELD_OBJ_VISIBLE, vis)
    sim.render(gl_filter=gl_filter)
    frames = sim.frames_host().copy()
    pipe = sim.render_pipeline
    sim.close()
    return frames, pipe


def _assert_gl(frames, d, idx, label):
    worst = dict(gt1=0.0, gt2=0.0, mean=0.0)
    for j, k in enumerate(idx):
        s = stats(frames[j], d["frame"][k])
        for key in worst:
            worst[key] = max(worst[key], s[key])
        assert_within(s, REFERENCE_GL, (label, k))
    print(f"\n{label}: worst of {len(idx)} frames vs GL: beyond +-1 {worst['gt1']:.5f}, beyond +-2 {worst['gt2']:.5f}, "
          f"mean abs {worst['mean']:.4f} / 255")


def test_device_capture_on_the_shared_camera_matches_gl():
    """As test_gpu_gl_golden.py::test_device_side_light_capture_matches_gl, on the shared camera: env j stands where the reference's episode
    ended and auto-resets into a spawn-pool entry that carries the RAW light reset() drew; the device must capture GL's eye-space light, and the
    shared-camera pipeline (not the per-env one) must render the reference's first frame of the new episode with it."""
    d = G.load("episode2_t256_160")
    m = d["meta"]
    n = len(d["frame"]) // 2
    before, after = list(range(0, 2 * n, 2)), list(range(1, 2 * n, 2))
    sim = BatchedSimulator(m["map_name"], n, asset_root=asset_trees.tree(m["tree"]), camera_width=int(m["W"]), camera_height=int(m["H"]),
                           distortion=False, domain_rand=False, seed=1, max_steps=1000000, auto_reset=True, light_capture=True)
    for j in range(n):
        _set_state(sim.init_states[j], d, before[j], d["light_eye"])
    sim.reset(states=sim.init_states)
    pool = (_ffi.InitState * n)()
    for j in range(n):
        C.memmove(C.byref(pool[j]), C.byref(sim.init_states[j]), C.sizeof(_ffi.InitState))
        _set_state(pool[j], d, after[j], d["light_raw"])
    _ffi.check(sim._lib, sim._lib.dtsim_set_spawn_pool(sim._h, pool, n))
    sim.write(_ffi.FIELD_DONE, np.ones(n, np.uint8))
    sim.step(np.zeros((1, n, 2), np.float32))                                    # auto-reset: env e -> pool slot (e + n) % n = e; one step at rest
    light = sim.read(_ffi.FIELD_COLORS)[:, 12:16]
    want = d["light_eye"][after]
    assert np.allclose(light, want, rtol=2e-6, atol=2e-4), (light, want)
    assert not np.allclose(want[:, :3], d["light_raw"][after][:, :3], atol=1.0)   # (it did move: not the raw light)
    sim.render()
    assert sim.render_pipeline in ("k_raster_v3+light", "k_raster_q+light"), sim.render_pipeline
    _assert_gl(sim.frames_host(), d, after, "episode2_t256_160, device capture, shared camera")
    sim.close()


@pytest.mark.parametrize("case", SHARED_CASES)
def test_shared_camera_pipelines_match_gl_with_each_env_s_light(case):
    """Every shared-camera quad pipeline with the lights GL held, uploaded through dtsim_reset(states): the LIGHT instantiations
    (lightcap_town_t128_320: k_raster_q<OBJ, S256 = 0, LIGHT> and its exact path with lights that differ between envs)."""
    d = _load(case)
    frames, pipe = _render_golden(d)
    assert pipe.endswith("+light") and pipe.startswith(("k_raster_v3", "k_raster_q")), pipe
    _assert_gl(frames, d, range(len(frames)), f"{case} ({pipe})")


@pytest.mark.parametrize("case", [c for c in SHARED_CASES if "160" in c or "320" in c])
def test_generic_raster_with_each_env_s_light_is_bit_faithful(case):
    """gl_filter=True: the generic raster through the EnvCam records (shared camera, each env's light), at the tolerance of
    test_gpu_gl_golden.py::test_gl_filter_mode_is_bit_faithful."""
    d = _load(case)
    frames, pipe = _render_golden(d, gl_filter=True)
    assert pipe == "k_raster_env+light", pipe
    differ = [float((frames[k] != d["frame"][k]).any(axis=-1).mean()) for k in range(len(frames))]
    st = [stats(frames[k], d["frame"][k]) for k in range(len(frames))]
    print(f"\n{case} (GL filter mode, each env's light): pixels that differ {max(differ):.4f}, beyond +-1 {max(s['gt1'] for s in st):.5f}, "
          f"mean abs {max(s['mean'] for s in st):.4f} / 255")
    assert max(differ) <= GL_FILTER_DIFFER, (case, max(differ))
    for k, s in enumerate(st):
        assert_within(s, ORACLE_MESH_GT1, (case, k))


def test_light_on_with_the_first_light_equals_light_off():
    """Every env lit by (0, 3, 0, 1): the LIGHT kernels' per-(pixel, env) light against the per-pixel table of the light-off kernels -- within
    +-1/255 (the two evaluate N.L in different frames: the last bit of the lit factor may differ)."""
    W, H, N = 640, 480, 72
    for names in ("small_loop", ["loop_only_duckies", "small_loop_only_duckies"]):
        out = {}
        for lc in (False, True):
            sim = BatchedSimulator(names, N, camera_width=W, camera_height=H, distortion=True, domain_rand=False, seed=17, map_cycle=True,
                                   max_steps=100000, light_capture=lc)
            sim.step(np.random.default_rng(4).uniform(0.1, 0.6, (6, N, 2)).astype(np.float32), n_steps=6)
            assert np.array_equal(sim.read(_ffi.FIELD_COLORS)[:, 12:16], np.tile(FIRST_LIGHT, (N, 1)).astype(np.float32))
            sim.render()
            out[lc] = (sim.frames_host().copy(), sim.render_pipeline)
            sim.close()
        diff = np.abs(out[True][0].astype(int) - out[False][0].astype(int))
        print(f"\n{names}: {out[False][1]} vs {out[True][1]}: pixels that differ {float((diff > 0).any(-1).mean()):.5f}, max {int(diff.max())}")
        assert out[True][1] == out[False][1] + "+light"
        assert diff.max() <= 1


def test_shared_camera_light_matches_the_per_env_camera_path():
    """On the episode-2 states, the shared-camera frames with each env's light against per_env_camera=True (the route that was right before)."""
    d = G.load("episode2_t256_160")
    a, pa = _render_golden(d)
    b, pb = _render_golden(d, light_capture=False, per_env_camera=True)
    assert pa.endswith("+light") and not pb.endswith("+light"), (pa, pb)
    for k in range(len(a)):
        within = float((np.abs(a[k].astype(int) - b[k].astype(int)).max(-1) <= 1).mean())
        assert within >= 0.99, (k, within)


def test_vecenv_light_follows_the_episodes():
    """DuckietownVecEnv with light_capture: after 300 steps some envs are past their first episode, and exactly those hold a light other
    than the first episode's (0, 3, 0, 1) -- captured through the camera their previous episode ended with."""
    import torch
    from dtsim.vecenv import DuckietownVecEnv
    N = 256
    env = DuckietownVecEnv("small_loop", N, domain_rand=False, light_capture=True)
    env.reset()
    gen = torch.Generator().manual_seed(0)
    ended = np.zeros(N, bool)
    for _ in range(300):
        a = torch.rand((N, 2), generator=gen) * torch.tensor([1.0, 2.0]) + torch.tensor([0.0, -1.0])
        _, _, done, _ = env.step(a)
        ended |= done.cpu().numpy()
    torch.cuda.synchronize()
    light = env.sim.read(_ffi.FIELD_COLORS)[:, 12:16]
    moved = np.abs(light - FIRST_LIGHT).max(-1) > 1e-6
    print(f"\nvecenv: {int(ended.sum())} of {N} envs past episode 1")
    assert ended.any()
    assert np.array_equal(moved, ended), np.nonzero(moved != ended)[0]
    assert env.sim.render_pipeline.endswith("+light")
    env.close()


def _full_size(names, N, obj, n_min):
    """The bench's set-up (bench.py: spawn pool, auto-reset, vel_steer, 640 x 480 + fisheye) with light_capture, stepped until at least a
    third of the envs are past episode 1; n_min envs or more (stratified over the render order, envs in later episodes among them) against the oracle
    with each env's light as the device holds it."""
    W, H = 640, 480
    sim = BatchedSimulator(names, N, camera_width=W, camera_height=H, distortion=True, domain_rand=False, seed=1000, action_mode="vel_steer",
                           auto_reset=True, do_reset=False, light_capture=True, **({} if isinstance(names, str) else dict(map_cycle=True)))
    sim.make_spawn_pool(N)
    sim.reset(states=sim._pool)
    ep0 = sim.read(_ffi.FIELD_EPISODE)
    rng = np.random.default_rng(1234)
    for _ in range(40):                                    # bounded: 640 steps at most
        sim.step(rng.uniform(-1, 1, (16, N, 2)).astype(np.float32), n_steps=16)
        if (sim.read(_ffi.FIELD_EPISODE) > ep0).mean() >= 1 / 3:
            break
    later = sim.read(_ffi.FIELD_EPISODE) > ep0
    assert later.mean() >= 1 / 3, later.mean()
    sim.render()
    sim.sync()
    assert sim.render_pipeline == "k_raster_v3+light", sim.render_pipeline
    picks = stratified_picks(sim, N, n_min, 3)
    idx = np.nonzero(later)[0]
    picks = sorted(set(picks) | {int(e) for e in idx[:: max(1, len(idx) // 8)]})
    n_later = int(sum(later[e] for e in picks))
    assert n_later >= 8
    cols, mid = sim.read(_ffi.FIELD_COLORS), sim.read(_ffi.FIELD_MAP_ID)
    assert (np.abs(cols[later][:, 12:16] - FIRST_LIGHT).max(-1) > 1e-6).all()
    scenes = [scene(n) for n in ([names] if isinstance(names, str) else names)]
    assert obj == all(bool(sc.m.objects) for sc in scenes)
    # colors=: the light of an env past episode 1 is what the device captured (DTSIM_FIELD_COLORS), not its init state's
    worst, _ = compare_envs(sim, frames_of(sim, picks), picks, lambda e: scenes[int(mid[e])], pdist.distortion_maps(W, H),
                            ORACLE_MESH if obj else ORACLE_PLANE, dr=False, mode="pixel", colors=cols)
    print(f"\n{names}, {N} envs, light_capture: {len(picks)} envs ({n_later} past episode 1) against the oracle: worst", worst)
    sim.close()


def test_c3_full_size_with_light_capture_matches_oracle():
    _full_size("small_loop", 4096, obj=False, n_min=64)


def test_c5_with_light_capture_matches_oracle():
    _full_size(["loop_only_duckies", "small_loop_only_duckies"], 4096, obj=True, n_min=64)


def test_vector_flow_follows_the_reference_over_episodes():
    """The reference's DuckietownEnv over several episodes (lightcap_flow: max_steps 40, recorded (vel, steer) actions, reset() after every done)
    against BatchedSimulator(auto_reset=True, light_capture=True, domain_rand=False) with one env per seed.  Episode 1 starts from
    dtsim_reset(states); episode ep + 1 of env e comes from spawn-pool slot (e + ep * N) % n_pool (physics.hip: k_step's auto-reset), filled with
    the state the reference's reset() drew -- its RAW light: the device captures it through the camera of the pose the episode ended at.
    Per step: pose and speed within 1e-9, reward within 1e-6 (the numpy-2 note of test_gpu_gl_golden.py), done exactly; every kept observation
    (most of them in episodes >= 2) within the GL tolerance."""
    d = load_lightcap(FLOW)
    m = d["meta"]
    S, T = d["traj_done"].shape
    rs = {k[len("reset_"):]: v for k, v in d.items() if k.startswith("reset_")}
    sim = BatchedSimulator(m["map_name"], S, asset_root=asset_trees.tree(m["tree"]), camera_width=int(m["W"]), camera_height=int(m["H"]),
                           distortion=False, domain_rand=False, seed=1, max_steps=int(m["max_steps"]), auto_reset=True, light_capture=True,
                           action_mode="vel_steer", actions_f64=True)             # (the reference's actions are float64)
    first = [int(np.nonzero((rs["seed_index"] == s) & (rs["at_step"] == -1))[0][0]) for s in range(S)]
    for s in range(S):
        _set_state(sim.init_states[s], rs, first[s], rs["light_eye"])
    sim.reset(states=sim.init_states)
    ep0 = sim.read(_ffi.FIELD_EPISODE)
    assert (ep0 == ep0[0]).all()
    n_eps = max(int((rs["seed_index"] == s).sum()) for s in range(S))
    n_pool = S * (int(ep0[0]) + n_eps + 1)
    pool = (_ffi.InitState * n_pool)()
    for slot in range(n_pool):
        C.memmove(C.byref(pool[slot]), C.byref(sim.init_states[slot % S]), C.sizeof(_ffi.InitState))
    for s in range(S):
        later = [int(i) for i in np.nonzero((rs["seed_index"] == s) & (rs["at_step"] >= 0))[0]]
        for j, i in enumerate(later):                                            # the (j + 2)-th episode: counter ep0 + j + 1
            _set_state(pool[(s + (int(ep0[0]) + j + 1) * S) % n_pool], rs, i, rs["light_raw"])
    _ffi.check(sim._lib, sim._lib.dtsim_set_spawn_pool(sim._h, pool, n_pool))
    nobj = rs["obj_visible"].shape[1]
    kept = {(int(s), int(t)): k for k, (s, t) in enumerate(zip(d["kept_seed_index"], d["kept_at_step"]))}
    kept_steps = sorted({t for _s, t in kept})
    worst = dict(gt1=0.0, gt2=0.0, mean=0.0)
    n_later = 0
    for t in range(T):
        sim.step(np.ascontiguousarray(d["traj_actions"][:, t:t + 1, :].transpose(1, 0, 2), np.float64))
        pos, ang, spd = sim.read(_ffi.FIELD_POS), sim.read(_ffi.FIELD_ANGLE), sim.read(_ffi.FIELD_SPEED)
        rew, done = sim.read(_ffi.FIELD_REWARD), sim.read(_ffi.FIELD_DONE)
        for s in range(S):
            assert np.abs(pos[s] - d["traj_pos"][s, t]).max() <= 1e-9 and abs(ang[s] - d["traj_angle"][s, t]) <= 1e-9, (s, t)
            assert abs(spd[s] - d["traj_speed"][s, t]) <= 1e-9, (s, t)
            assert abs(rew[s] - d["traj_reward"][s, t]) <= 1e-6 and bool(done[s]) == bool(d["traj_done"][s, t]), (s, t, rew[s], d["traj_reward"][s, t])
        if t in kept_steps:
            if nobj:
                assert (sim.read(_ffi.FIELD_OBJ_VISIBLE)[:, :nobj] == 1).all()
            sim.render()
            frames = sim.frames_host()
            light = sim.read(_ffi.FIELD_COLORS)[:, 12:16]
            for s in range(S):
                if (s, t) not in kept:
                    continue
                k = kept[(s, t)]
                assert np.allclose(light[s], d["kept_light_eye"][k], rtol=2e-6, atol=2e-4), (s, t, light[s], d["kept_light_eye"][k])
                n_later += int(np.abs(d["kept_light_eye"][k] - FIRST_LIGHT).max() > 0.1)
                st = stats(frames[s], d["kept_frame"][k])
                for key in worst:
                    worst[key] = max(worst[key], st[key])
                assert_within(st, REFERENCE_GL, (s, t))
            assert sim.render_pipeline == "k_raster_v3+light", sim.render_pipeline
    assert n_later >= 20, n_later
    print(f"\nflow: {S} seeds x {T} steps, {len(kept)} kept frames ({n_later} in later episodes) vs GL: beyond +-1 {worst['gt1']:.5f}, "
          f"beyond +-2 {worst['gt2']:.5f}, mean abs {worst['mean']:.4f} / 255")
    sim.close()


def test_multimap_env_forwards_light_capture():
    """MultiMapEnv / DuckietownEnv forward the keyword to the simulator they build (their own resets capture the light on the host)."""
    from gym_duckietown.envs import MultiMapEnv
    env = MultiMapEnv(light_capture=True, seed=3, camera_width=160, camera_height=120, max_steps=20, distortion=False)
    assert all(e._sim.light_capture for e in env.env_list)
    env.reset()
    for _ in range(25):
        _obs, _r, done, _info = env.step(np.array([0.5, 0.2]))
        if done:
            env.reset()
    env.close()
    env = MultiMapEnv(seed=3, camera_width=160, camera_height=120, max_steps=20, distortion=False)
    assert not any(e._sim.light_capture for e in env.env_list)
    env.close()
