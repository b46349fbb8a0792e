"""GPU: DuckietownVecEnv(fused_maps=True) -- ONE BatchedSimulator.camera_maps call (dtsim_camera_maps) stands where the depth, label,
instance and flow passes stand.  On small_loop (no mesh objects: the fused pass and the single passes read the same scene) an env with the
option and one without return the same bytes in obs, reward, done and every info tensor, the final_ twins included, across restarts.  On
loop_pedestrians the env is held to a hand-driven twin BatchedSimulator that makes the documented sequence with camera_maps.  A tracer in
the style of tests/test_gpu_vecenv_calls.py holds the calls: with the option a step contains exactly one camera_maps per place the passes
stand and no depth / labels / instances / flow; without it no camera_maps.  160 x 120 and 64 x 48 cameras, 32 and 66 envs."""
import inspect

import pytest

from dtsim import BatchedSimulator, DuckietownVecEnv, _ffi

pytestmark = pytest.mark.gpu
CAM = dict(camera_width=160, camera_height=120)
MAPS = dict(depth_shape=(60, 80), label_shape=(60, 80), instance_shape=(60, 80), boxes=True, flow_shape=(60, 80), flow_valid=True)


def same(x, y):
    import torch
    return x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))


def test_small_loop_the_option_changes_no_byte():
    """32 envs, episodes of 6 steps (the robot starts at rest: shorter ones move the picture by less than a thousandth of a pixel),
    final_obs=True, 13 steps: every env restarts twice, so the masked passes and the final_ twins are exercised; depth in float16, a
    bird's-eye map beside the camera maps."""
    import torch
    N, STEPS = 32, 13
    kw = dict(obs_shape=(24, 32), final_obs=True, depth_dtype="float16", bev_shape=(16, 16), domain_rand=False, max_steps=6, seed=5, **MAPS, **CAM)
    A = DuckietownVecEnv("small_loop", N, fused_maps=True, **kw)
    B = DuckietownVecEnv("small_loop", N, **kw)
    oa, ob = A.reset(), B.reset()
    torch.cuda.synchronize()
    assert same(oa, ob)
    for name in ("depth", "labels", "instances", "boxes", "flow", "flow_valid", "bev"):
        assert same(getattr(A, name), getattr(B, name)), name
    assert not bool(A.flow.any()) and not bool(A.flow_valid.any())                  # after reset(): all 0, as without the option
    g = torch.Generator(device="cuda"); g.manual_seed(2)
    n_done, moved = torch.zeros(N, device="cuda"), 0
    for t in range(STEPS):
        a = torch.rand((N, 2), device="cuda", generator=g) * 2 - 1
        oa, ra, da, ia = A.step(a)
        ob, rb, db, ib = B.step(a)
        torch.cuda.synchronize()
        assert same(oa, ob) and same(ra, rb) and same(da, db), t
        assert set(ia) == set(ib) and {"depth", "labels", "instances", "boxes", "flow", "flow_valid", "final_depth", "final_flow"} <= set(ia)
        for key in ib:
            if key.startswith("final_") and key != "final_obs_mask":
                assert same(ia[key][da], ib[key][db]), (t, key)                     # (the other rows are unspecified)
            else:
                assert same(ia[key], ib[key]), (t, key)
        assert ia["depth"] is A.depth and ia["depth"].dtype == torch.float16 and ia["flow"] is A.flow
        moved += int((ia["final_flow"][da].abs().flatten(1).amax(dim=1) > 1e-3).sum()) + int((ia["flow"].abs().flatten(1).amax(dim=1) > 1e-3).sum())
        n_done += da.float()
    assert float(n_done.min()) >= 2 and moved > 0
    A.close(); B.close()


def test_loop_pedestrians_the_env_is_the_documented_sequence_on_a_twin():
    """66 envs (a full chunk of the env loop and a tail of 2), episodes of 9 steps (the robot starts at rest and the picture first moves at
    its sixth step), 19 steps: reset -> render -> camera_maps -> mark;
    step -> reset_done -> render -> camera_maps -> boxes -> mark, on a twin simulator, byte for byte."""
    import torch
    N, STEPS, MAP = 66, 19, "loop_pedestrians"
    kw = dict(domain_rand=False, max_steps=9, **CAM)
    A = DuckietownVecEnv(MAP, N, seed=4, obs_shape=(24, 32), fused_maps=True, **MAPS, **kw)
    ref = BatchedSimulator(MAP, N, action_mode="vel_steer", seed=4, device_reset=True, auto_reset=False, do_reset=False, **kw)
    h, w = MAPS["depth_shape"]
    none = torch.zeros(N, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def ref_pass():
        ref.render()
        out = ref.camera_maps(h, w, depth=True, labels=True, instances=True, flow=True, flow_valid=True)
        out["boxes"] = ref.boxes(out["instances"])
        ref.sync()
        return {k: v.clone() for k, v in out.items()}

    A.reset()
    ref.reset()
    ref.flow_mark(mask=none)                                 # (marks of no env: camera_maps refuses a handle without any)
    want = ref_pass()
    ref.flow_mark()
    torch.cuda.synchronize()
    for k, v in want.items():
        assert same(getattr(A, k), v), k
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    n_done, seen, moved = torch.zeros(N, device="cuda"), 0, 0
    for t in range(STEPS):
        a = torch.rand((N, 2), device="cuda", generator=g) * 2 - 1
        _, _, da, ia = A.step(a)
        torch.cuda.synchronize()
        ref.step(a)
        ref.sync()                                           # (the twin's stream is its own: the read below runs on torch's)
        ref_done = torch.as_tensor(ref.field_device(_ffi.FIELD_DONE), device="cuda").to(torch.bool).clone()
        ref.reset_done()
        want = ref_pass()
        ref.flow_mark()
        assert torch.equal(da, ref_done), t
        for k, v in want.items():
            assert same(ia[k], v), (t, k)
        assert not bool(ia["flow"][da].any()) and not bool(ia["flow_valid"][da].any()), t       # restarted: no mark of the new episode
        seen += int((ia["instances"] > 0).sum())
        moved += int((ia["flow"].abs().flatten(1).amax(dim=1) > 1e-3).sum())
        n_done += da.float()
    assert float(n_done.min()) >= 2 and seen > 100 and moved > 0                   # duckies in view, a flow that is one
    A.close()
    ref.close()


# ---- the calls: a copy of tests/test_gpu_vecenv_calls.py's tracer, with camera_maps and flow traced ----------------------------------------------

TRACED = ("reset", "step", "render", "observe", "push_observation", "depth", "labels", "instances", "boxes", "flow", "flow_mark", "camera_maps",
          "bev", "copy_rows", "reset_done")


class Tracer:
    """Wraps the TRACED methods of env.sim on the instance; every call goes through to the real method and leaves (name, mask) in `calls`,
    the mask as a data pointer until names() knows the step's `done`."""

    def __init__(self, env):
        self.env, self.calls = env, []
        for name in TRACED:
            setattr(env.sim, name, self._wrap(name, getattr(env.sim, name)))

    def _wrap(self, name, real):
        sig = inspect.signature(real)

        def call(*a, **kw):
            m = sig.bind(*a, **kw).arguments.get("mask")
            self.calls.append((name, None if m is None else m.data_ptr()))
            return real(*a, **kw)
        return call

    def names(self, done=None):
        known = {None: None}
        if done is not None:
            known[done.data_ptr()] = "done"
        out = tuple((n, known.get(m, "other")) for n, m in self.calls)
        self.calls = []
        return out


def c(name, mask=None):
    return (name, mask)


# configuration -> (env arguments, the calls of one step() with fused_maps=True, the same with fused_maps=False)
EXPECTED = {
    "plain_all": (dict(depth_shape=(24, 32), label_shape=(24, 32), instance_shape=(24, 32), boxes=True, flow_shape=(24, 32), flow_valid=True),
                  (c("step"), c("reset_done"), c("render"), c("observe"), c("camera_maps"), c("boxes"), c("flow_mark")),
                  (c("step"), c("reset_done"), c("render"), c("observe"), c("depth"), c("instances"), c("boxes"), c("flow"), c("flow_mark"))),
    "final_depth_labels_bev": (dict(depth_shape=(24, 32), label_shape=(24, 32), bev_shape=(8, 8), final_obs=True),
                               (c("step"), c("render"), c("observe"), c("camera_maps"), c("bev"), c("copy_rows", "done"), c("copy_rows", "done"),
                                c("copy_rows", "done"), c("copy_rows", "done"), c("reset_done"), c("render", "done"), c("observe", "done"),
                                c("camera_maps", "done"), c("bev", "done")),
                               (c("step"), c("render"), c("observe"), c("depth"), c("labels"), c("bev"), c("copy_rows", "done"), c("copy_rows", "done"),
                                c("copy_rows", "done"), c("copy_rows", "done"), c("reset_done"), c("render", "done"), c("observe", "done"),
                                c("depth", "done"), c("labels", "done"), c("bev", "done"))),
    "plain_flow_alone": (dict(flow_shape=(24, 32)),
                         (c("step"), c("reset_done"), c("render"), c("observe"), c("camera_maps"), c("flow_mark")),
                         (c("step"), c("reset_done"), c("render"), c("observe"), c("flow"), c("flow_mark"))),
}


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("cfg", list(EXPECTED))
def test_a_step_makes_one_camera_maps_call_in_place_of_the_single_passes(cfg, fused):
    import torch
    N, STEPS = 4, 4
    env_kw, want_fused, want_single = EXPECTED[cfg]
    env = DuckietownVecEnv("small_loop", N, seed=3, max_steps=3, domain_rand=False, obs_shape=(24, 32), fused_maps=fused, camera_width=64,
                           camera_height=48, **env_kw)
    tr = Tracer(env)
    env.reset()
    reset = tr.names()
    single = {"depth", "labels", "instances", "flow"}
    assert [n for n, _ in reset].count("camera_maps") == (1 if fused else 0) and (not fused or not single & {n for n, _ in reset})
    a = torch.full((N, 2), 0.5, device="cuda")
    n_done = torch.zeros(N, device="cuda")
    for t in range(STEPS):
        _, _, done, _ = env.step(a)
        got = tr.names(done)
        assert got == (want_fused if fused else want_single), (cfg, fused, t)
        n_done += done.float()
    torch.cuda.synchronize()
    env.close()
    assert float(n_done.min()) >= 1                          # every env finished, so every masked call had rows to work on
