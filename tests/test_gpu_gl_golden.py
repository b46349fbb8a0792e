"""GPU parity against the REFERENCE ITSELF: the HIP raster (dtsim_render through the C-ABI) vs frames the unmodified reference
Simulator rendered on Mesa 23.2.1 llvmpipe (tests/golden/ref_gl_*.npz, oracle/make_gl_golden.py).  The state of every golden
frame (pose, camera, colours, the light as GL holds it in eye space, object poses / visibility) is uploaded through
dtsim_reset(states) / dtsim_write; assets are the files the reference read (oracle/gl/asset_trees.py).

Tolerance vs Mesa 23.2.1 llvmpipe (DESIGN.md section 4 derives it; measured values are printed with -s):
  one-ray filter: GL filters RGBA8 textures with 8-bit weights and an 8-bit intermediate (profiles/r06_gl_filter_precision.txt);
  the HIP raster folds the lit factor into 8-bit weights and rounds once -> a +-1/255 difference on a fraction of the textured
  pixels, nothing systematic:  frame_parity.REFERENCE_GL (>= 99 % of pixels within +-1/255, <= 0.4 % beyond +-2/255, mean abs error <= 0.35 / 255).
"""
import ctypes as C

import numpy as np
import pytest

import gl_golden as G
from dtsim import BatchedSimulator, _ffi
from frame_parity import GL_FILTER_DIFFER, ORACLE_MESH_GT1, REFERENCE_GL, assert_within, stats
from oracle.gl import asset_trees

pytestmark = pytest.mark.gpu
CASES = [c for c in G.cases() if not c.startswith(("view_", "trajectory_"))]          # (the window / debugging views go through the facade: last test of the file)


def render_case(d, per_env_camera=None, gl_filter=False):
    m = d["meta"]
    n = len(d["frame"])
    dr = bool(m["dr"])
    if per_env_camera is None:       # the shared-camera pipeline (k_raster_v3) unless a frame's light is not the first episode's (0, 3, 0, 1)
        per_env_camera = (not dr) and bool((np.abs(d["light_eye"] - np.array([0.0, 3.0, 0.0, 1.0])) > 0).any())
    sim = BatchedSimulator(m["map_name"], n, asset_root=asset_trees.tree(m["tree"]), camera_width=int(m["W"]), camera_height=int(m["H"]),
                           distortion=False, domain_rand=dr, seed=1, max_steps=1000000, per_env_camera=per_env_camera)
    for k in range(n):
        st = sim.init_states[k]
        st.pos[:] = [float(v) for v in d["pos"][k]]
        st.angle = float(d["angle"][k])
        st.cam_height, st.cam_angle_deg, st.cam_fov_y_deg = float(d["cam_height"][k]), float(d["cam_angle"][k]), float(d["cam_fov_y"][k])
        st.camera_noise[:] = [float(v) for v in d["camera_noise"][k]]
        st.horizon_color[:] = [float(v) for v in d["horizon"][k]]
        st.ground_color[:] = [float(v) for v in d["ground"][k]]
        st.light_pos[:] = [float(v) for v in d["light_eye"][k]]
        st.light_ambient[:] = [float(v) for v in d["light_ambient"][k]]
        st.light_diffuse[:] = [float(v) for v in d["light_diffuse"][k]]
    sim.reset(states=sim.init_states)
    nobj = d["obj_visible"].shape[1]
    if nobj:
        vis = sim.read(_ffi.FIELD_OBJ_VISIBLE)
        vis[:, :nobj] = d["obj_visible"].astype(np.uint8)
        sim.write(_ffi.FIELD_OBJ_VISIBLE, vis)
    sim.render(segment=bool(m.get("segment")), gl_filter=gl_filter)
    frames = sim.frames_host().copy()
    sim.close()
    return frames


@pytest.mark.parametrize("case", CASES)
def test_frames_match_reference_gl(case):
    d = G.load(case)
    frames = render_case(d)
    all_stats = [stats(frames[k], d["frame"][k]) for k in range(len(frames))]
    worst = {key: max(s[key] for s in all_stats) for key in ("gt1", "gt2", "gt8", "mean")}
    differ = max(float((frames[k] != d["frame"][k]).any(axis=-1).mean()) for k in range(len(frames)))
    print(f"\n{case}: worst of {len(frames)} frames vs GL: pixels that differ {differ:.3f}, beyond +-1 {worst['gt1']:.5f}, beyond +-2 {worst['gt2']:.5f}, "
          f"beyond +-8 {worst['gt8']:.5f}, mean abs {worst['mean']:.4f} / 255")
    for k, s in enumerate(all_stats):
        assert_within(s, REFERENCE_GL, (case, k))


@pytest.mark.parametrize("case,seeds", [("small_loop_t256_160", list(range(10, 26))), ("small_loop_dr_t256_160", list(range(30, 46))),
                                        ("loop_dr_t256_160", list(range(70, 86)))])
def test_drop_in_facade_reproduces_the_reference_s_first_frames(case, seeds):
    """End to end, nothing uploaded by the test: `gym_duckietown.Simulator(map_name, seed=s, ...)` of THIS package (the HIP library behind
    the reference's constructor) against `Simulator(map_name, seed=s, ...)` of the REFERENCE on Mesa llvmpipe -- same seed, same asset files.
    The reset draws must land on the same pose and randomisation (bit-exact: compared with the state the golden recorded from the reference
    instance) and the observation `reset()` returns must be the reference's frame within the tolerance of this file."""
    from gym_duckietown.simulator import Simulator
    d = G.load(case)
    m = d["meta"]
    assert len(seeds) == len(d["frame"])
    worst = dict(gt1=0.0, gt2=0.0, mean=0.0)
    for k, seed in enumerate(seeds):
        env = Simulator(map_name=m["map_name"], domain_rand=bool(m["dr"]), seed=seed, camera_width=int(m["W"]), camera_height=int(m["H"]),
                        max_steps=100000, distortion=False, asset_root=asset_trees.tree(m["tree"]))
        assert np.array_equal(np.asarray(env.cur_pos, dtype=np.float64), d["pos"][k]) and float(env.cur_angle) == float(d["angle"][k]), (case, seed)
        assert np.allclose(np.asarray(env.horizon_color, dtype=np.float64)[:3], d["horizon"][k], rtol=0, atol=0), (case, seed)
        obs = env.render_obs()
        s = stats(obs, d["frame"][k])
        for key in worst:
            worst[key] = max(worst[key], s[key])
        assert_within(s, REFERENCE_GL, (case, seed))
        env.close()
    print(f"\n{case}: facade vs reference, worst of {len(seeds)} seeds: beyond +-1 {worst['gt1']:.5f}, beyond +-2 {worst['gt2']:.5f}, mean abs {worst['mean']:.4f} / 255")


@pytest.mark.parametrize("case,seeds", [("view_top_down_t256_800", [4, 5]), ("view_bbox_t256_320", [4, 5, 6, 7])])
def test_facade_views_match_the_reference_s(case, seeds):
    """render(mode="top_down") and draw_bbox=True of the drop-in Simulator against the reference's frames of the same seeds: the map from above
    with the agent's mesh at its pose; the debugging camera 0.8 m above the robot.  In the bbox view the pixels of the GL_LINE_LOOPs are left
    out (the reference draws them textured and lit by whatever state is current) -- but both must HAVE red lines there."""
    from gym_duckietown.simulator import Simulator
    d = G.load(case)
    m = d["meta"]
    for k, seed in enumerate(seeds):
        bbox = m["view"] == "bbox"
        kw = dict(draw_bbox=True, camera_width=int(m["W"]), camera_height=int(m["H"])) if bbox else {}
        env = Simulator(map_name=m["map_name"], domain_rand=False, seed=seed, max_steps=100000, distortion=False, asset_root=asset_trees.tree(m["tree"]), **kw)
        assert np.array_equal(np.asarray(env.cur_pos, dtype=np.float64), d["pos"][k]) and float(env.cur_angle) == float(d["angle"][k]), (case, seed)
        img = env.render_obs() if bbox else env.render("top_down")
        assert img.shape == d["frame"][k].shape
        if bbox:
            mask = G.line_mask(d, k)
            s = stats(img, d["frame"][k], mask)
            red = lambda f: ((f[..., 0].astype(int) - f[..., 1] > 25) & mask).sum()
            assert red(img) > 20 and red(d["frame"][k]) > 20, (red(img), red(d["frame"][k]))
        else:
            s = stats(img, d["frame"][k])
        print(f"\n{case} seed {seed}: beyond +-1 {s['gt1']:.5f}, beyond +-2 {s['gt2']:.5f}, mean abs {s['mean']:.4f} / 255")
        assert_within(s, REFERENCE_GL, (case, seed))
        env.close()


@pytest.mark.parametrize("case", [c for c in CASES if "160" in c or "320" in c])
def test_gl_filter_mode_is_bit_faithful(case):
    """dtsim_render_ex(DTSIM_RENDER_GL_FILTER): the same states through the generic raster, whose GL_LINEAR is llvmpipe's arithmetic
    (gl_linear_rgb).  What is left against the reference's frames is the per-fragment tile light (< 1 level) and single MSAA samples at
    silhouettes: per frame <= 2.5 % of the pixels differ AT ALL (measured: 0.2 - 1.5 %), <= 0.2 % by more than 1."""
    d = G.load(case)
    frames = render_case(d, gl_filter=True)
    differ = [float((frames[k] != d["frame"][k]).any(axis=-1).mean()) for k in range(len(frames))]
    st = [stats(frames[k], d["frame"][k]) for k in range(len(frames))]
    print(f"\n{case} (GL filter mode): worst of {len(frames)} frames: pixels that differ {max(differ):.4f}, beyond +-1 {max(s['gt1'] for s in st):.5f}, mean abs {max(s['mean'] for s in st):.4f} / 255")
    assert max(differ) <= GL_FILTER_DIFFER, (case, max(differ))
    for k, s in enumerate(st):
        assert_within(s, ORACLE_MESH_GT1, (case, k))


@pytest.mark.parametrize("case", ["trajectory_t256_160", "trajectory_dr_t256_160"])
def test_drop_in_env_follows_the_reference_s_trajectory(case):
    """The whole loop, end to end: `gym_duckietown.envs.DuckietownEnv(map_name, seed=s)` of this package stepped with the actions the golden
    recorded, against what the REFERENCE's DuckietownEnv.step returned for them on Mesa llvmpipe -- pose and speed within 1e-9, reward within 1e-6 (see below), the done flag
    exactly (the episode ends where the reference's ended), and the observations of the kept steps within this file's frame tolerance.
    (Lane pose, collision, reward and done are the reference's own code on that side; the DB18 integrator there is oracle/sim.py's restatement.)"""
    from gym_duckietown.envs import DuckietownEnv
    d = G.load(case)
    m = d["meta"]
    env = DuckietownEnv(map_name=m["map_name"], domain_rand=bool(m["dr"]), seed=int(m["seed"]), camera_width=int(m["W"]), camera_height=int(m["H"]),
                        max_steps=100000, distortion=False, asset_root=asset_trees.tree(m["tree"]))
    acts, T = d["traj_actions"][0], len(d["traj_done"][0])
    kept = {int(s): k for k, s in enumerate(d["step_count"])}
    assert np.array_equal(np.asarray(env.cur_pos, dtype=np.float64), d["pos"][0])
    frames = {0: env.render_obs()}
    for t in range(T):
        obs, reward, done, _info = env.step(acts[t])
        assert np.abs(np.asarray(env.cur_pos, dtype=np.float64) - d["traj_pos"][0][t]).max() <= 1e-9 and abs(float(env.cur_angle) - d["traj_angle"][0][t]) <= 1e-9, (case, t)
        # reward: 1e-6, not 1e-9 -- the golden was recorded under numpy 2, where the reference's `height / mesh.max_coords[1]` (float32 extents) stays float32
        # (NEP 50) and the objects' scale / safety radius carry a 1e-7 relative error; the product follows the float64 arithmetic of the numpy <= 1.20
        # the reference pins (setup.py:28; DESIGN.md section 4, numpy-version note).  Poses are not touched by it.
        assert abs(float(reward) - d["traj_reward"][0][t]) <= 1e-6 and bool(done) == bool(d["traj_done"][0][t]), (case, t, reward, d["traj_reward"][0][t])
        assert abs(float(env.speed) - d["traj_speed"][0][t]) <= 1e-9
        frames[t + 1] = obs
    assert bool(d["traj_done"][0][-1])                   # the recorded episode did end (and so did this one, at the same step)
    for step, k in kept.items():
        s = stats(frames[step], d["frame"][k])
        print(f"\n{case} step {step}: beyond +-1 {s['gt1']:.5f}, beyond +-2 {s['gt2']:.5f}, mean abs {s['mean']:.4f} / 255")
        assert_within(s, REFERENCE_GL, (case, step))
    env.close()


def test_device_side_light_capture_matches_gl():
    """DTSIM_F_LIGHT_CAPTURE: the vector API's device-side resets position the new episode's light as GL does -- through the camera of the pose the
    previous episode ended at.  The `episode2_dr` golden holds, per episode, the last frame before the reference's reset() and the first after it:
    env j is put at the former's state, given a spawn pool whose entry carries the RAW light reset() handed to glLightfv, and auto-reset; the light the
    device then holds must be GL's eye-space light (glGetLightfv) and the frame the reference's first frame of that episode."""
    d = G.load("episode2_dr_t256_160")
    m = d["meta"]
    n = len(d["frame"]) // 2
    before, after = list(range(0, 2 * n, 2)), list(range(1, 2 * n, 2))
    sim = BatchedSimulator(m["map_name"], n, asset_root=asset_trees.tree(m["tree"]), camera_width=int(m["W"]), camera_height=int(m["H"]), distortion=False,
                           domain_rand=True, seed=1, max_steps=1000000, auto_reset=True, light_capture=True)

    def state(st, k, light):
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

    for j in range(n):
        state(sim.init_states[j], before[j], d["light_eye"])                      # (dtsim_reset(states) takes the light as given: eye space)
    sim.reset(states=sim.init_states)
    pool = (_ffi.InitState * n)()
    for j in range(n):
        C.memmove(C.byref(pool[j]), C.byref(sim.init_states[j]), C.sizeof(_ffi.InitState))
        state(pool[j], after[j], d["light_raw"])                                  # the new episode as reset() drew it: the light NOT yet through any model-view
    _ffi.check(sim._lib, sim._lib.dtsim_set_spawn_pool(sim._h, pool, n))
    sim.write(_ffi.FIELD_DONE, np.ones(n, np.uint8))
    sim.step(np.zeros((1, n, 2), np.float32))                                    # auto-reset: env e, episode 1 -> pool slot (e + n) % n = e; then one step at rest
    light = sim.read(_ffi.FIELD_COLORS)[:, 12:16]
    want = d["light_eye"][after]
    assert np.allclose(light, want, rtol=2e-6, atol=2e-4), (light, want)
    assert not np.allclose(want[:, :3], d["light_raw"][after][:, :3], atol=1.0)   # (and it did move: this is not the raw light)
    sim.render()
    frames = sim.frames_host()
    for j in range(n):
        s = stats(frames[j], d["frame"][after[j]])
        assert_within(s, REFERENCE_GL, j)
    sim.close()
