"""GPU: DuckietownVecEnv(flow_shape=..., flow_valid=True) -- info["flow"] / info["flow_valid"] are the optical-flow map and its flags
(dtsim_flow) of the frame `obs` shows against the frame the previous step (or reset) showed, byte for byte what the literal call sequence
(step, render, flow, reset_done, render, flow, flow_mark) gives on a twin BatchedSimulator; an env restarted in the step has all-zero rows;
with final_obs=True info["final_flow"] / info["final_flow_valid"] hold the finished envs' last flow; obs, reward, done and every other info
entry are bit-identical to an env built without the new options.  With final_obs, frame_stack, frame_skip=3, the fisheye, domain_rand and a
depth map beside it.  160 x 120 cameras, N = 66 (one full chunk of 64 and a tail of 2), episodes of 3 or 6 steps: every env finishes."""
import pytest

from dtsim import BatchedSimulator, DuckietownVecEnv, _ffi

pytestmark = pytest.mark.gpu

N, MAX_STEPS = 66, 3
CAM = dict(camera_width=160, camera_height=120)
MAP = "loop_pedestrians"
FLOW = dict(flow_shape=(60, 80), flow_valid=True)
NEW_KEYS = {"flow", "flow_valid", "final_flow", "final_flow_valid"}
CONFIGS = {
    # env arguments (also given to the env without the new options), simulator arguments, env steps per episode, steps of the test
    # (the robot starts every episode at rest and its first sub-update moves nothing: an episode is six sub-updates or more)
    "plain_depth": (dict(obs_shape=(24, 32), depth_shape=(60, 80)), dict(domain_rand=False), 6, 13),
    "final_stack_skip3": (dict(obs_shape=(24, 32), final_obs=True, frame_stack=2), dict(domain_rand=True, frame_skip=3), MAX_STEPS, 7),
    "final_fisheye_skip2": (dict(obs_shape=None, final_obs=True), dict(domain_rand=False, distortion=True, frame_skip=2), MAX_STEPS, 7),
}


def same(x, y):
    import torch
    return x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_the_flow_rides_with_the_observation(cfg):
    import torch
    env_kw, sim_kw, episode, STEPS = CONFIGS[cfg]
    kw = dict(sim_kw, max_steps=episode * sim_kw.get("frame_skip", 1), **CAM)
    A = DuckietownVecEnv(MAP, N, seed=4, **FLOW, **env_kw, **kw)
    B = DuckietownVecEnv(MAP, N, seed=4, **env_kw, **kw)
    ref = BatchedSimulator(MAP, N, action_mode="vel_steer", seed=4, device_reset=True, auto_reset=False, do_reset=False, **kw)
    final = bool(env_kw.get("final_obs"))
    h, w = FLOW["flow_shape"]

    def ref_pass():                                          # the literal sequence: the frames of the current state, then the pass
        ref.render()
        v = torch.empty((N, h, w), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        f = ref.flow(h, w, valid_out=v)
        ref.sync()
        return f.clone(), v.clone()

    oa, ob = A.reset(), B.reset()
    ref.reset()
    torch.cuda.synchronize()
    assert same(oa, ob) and B.flow is None and B.flow_valid is None
    assert A.flow.shape == (N, 2, h, w) and A.flow.dtype == torch.float32 and A.flow_valid.shape == (N, h, w) and A.flow_valid.dtype == torch.uint8
    rf, rv = ref_pass()
    ref.flow_mark()
    assert same(A.flow, rf) and same(A.flow_valid, rv) and not bool(rf.any()) and not bool(rv.any())      # no previous state yet: all zero
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    n_done, n_moving = torch.zeros(N, device="cuda"), 0
    for t in range(STEPS):
        a = torch.rand((N, 2), device="cuda", generator=g) * 2 - 1
        oa, ra, da, ia = A.step(a)
        ob, rb_, db, ib = B.step(a)
        torch.cuda.synchronize()
        ref.step(a)
        before_f, before_v = ref_pass()
        ref_done = torch.as_tensor(ref.field_device(_ffi.FIELD_DONE), device="cuda").to(torch.bool).clone()
        ref.reset_done()
        after_f, after_v = ref_pass()
        ref.flow_mark()
        # everything the env without the new options returns: bit-identical
        assert same(oa, ob) and same(ra, rb_) and same(da, db) and torch.equal(da, ref_done), (cfg, t)
        assert set(ia) - NEW_KEYS == set(ib) and not (set(ib) & NEW_KEYS), (cfg, sorted(ia), sorted(ib))
        for key in ib:
            if key.startswith("final_") and key != "final_obs_mask":
                assert same(ia[key][da], ib[key][db]), (cfg, t, key)
            else:
                assert same(ia[key], ib[key]), (cfg, t, key)
        assert ia["flow"] is A.flow and ia["flow_valid"] is A.flow_valid                # persistent tensors
        assert same(ia["flow"], after_f) and same(ia["flow_valid"], after_v), (cfg, t)
        assert same(after_f[~da], before_f[~da]) and same(after_v[~da], before_v[~da])
        assert not bool(ia["flow"][da].any()) and not bool(ia["flow_valid"][da].any()), (cfg, t)     # restarted: no mark of the new episode
        if final:
            assert same(ia["final_flow"][da], before_f[da]) and same(ia["final_flow_valid"][da], before_v[da]), (cfg, t, int(da.sum()))
            assert ia["final_flow"].shape == A.flow.shape and ia["final_flow_valid"].shape == A.flow_valid.shape
        else:
            assert "final_flow" not in ia and "final_flow_valid" not in ia
        n_moving += int((before_f.abs().flatten(1).amax(dim=1) > 1e-3).sum())   # (three steps from rest: millimetres, fractions of a pixel)
        n_done += da.float()
    assert float(n_done.min()) >= 2, cfg                     # every env finished at least twice
    assert n_moving > N, cfg                                 # the flow is a flow: most steps move the picture
    for e in (A, B):
        e.close()
    ref.close()


def test_default_arguments_make_no_new_call(monkeypatch):
    import torch
    calls = []
    real_f, real_m = BatchedSimulator.flow, BatchedSimulator.flow_mark
    monkeypatch.setattr(BatchedSimulator, "flow", lambda sim, *a, **k: (calls.append("flow"), real_f(sim, *a, **k))[1])
    monkeypatch.setattr(BatchedSimulator, "flow_mark", lambda sim, *a, **k: (calls.append("mark"), real_m(sim, *a, **k))[1])
    env = DuckietownVecEnv("small_loop", 4, obs_shape=(24, 32), seed=4, final_obs=True, max_steps=MAX_STEPS, domain_rand=False, **CAM)
    env.reset()
    for _ in range(4):
        _, _, _, info = env.step(torch.zeros((4, 2), device="cuda"))
        assert not NEW_KEYS & set(info)
    torch.cuda.synchronize()
    assert not calls and env.flow is None and env.flow_valid is None
    env.close()
    env = DuckietownVecEnv("small_loop", 4, obs_shape=(24, 32), seed=4, flow_shape=(60, 80), max_steps=MAX_STEPS, domain_rand=False, **CAM)
    env.reset()
    _, _, _, info = env.step(torch.zeros((4, 2), device="cuda"))
    torch.cuda.synchronize()
    assert calls == ["flow", "mark", "flow", "mark"] and "flow" in info and "flow_valid" not in info and env.flow_valid is None
    env.close()


@pytest.mark.parametrize("kw", [
    dict(flow_valid=True), dict(flow_shape=(0, 8)), dict(flow_shape=(7, 80)), dict(flow_shape=8),
    dict(flow_shape=(60, 80), motion_blur=True, action_mode="wheels"), dict(flow_shape=(60, 80), undistort=True, distortion=True),
    dict(flow_shape=(60, 80), camera_rand=True, distortion=True), dict(flow_shape=(60, 80), camera_rand=True, distortion=True, camera_rand_maps=True),
])
def test_the_constructor_refuses_bad_arguments_before_a_device_is_touched(kw, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the simulator was built")
    monkeypatch.setattr(BatchedSimulator, "__init__", no_device)
    with pytest.raises(ValueError):
        DuckietownVecEnv("small_loop", 4, obs_shape=(24, 32), seed=4, max_steps=MAX_STEPS, **CAM, **kw)
