"""GPU: DuckietownVecEnv(depth_shape=...) -- info["depth"] is the depth map (dtsim_depth) of the state whose observation `obs` shows, byte
for byte what the literal call sequence gives on a twin BatchedSimulator; with final_obs=True info["final_depth"] holds, for the envs that
finished a step, the depth before the reset, and their rows of info["depth"] their new episode's first state; without depth_shape there is
no such key and obs / reward / done are bit-identical."""
import pytest

from dtsim import BatchedSimulator, DuckietownVecEnv, _ffi

pytestmark = pytest.mark.gpu

N, STEPS, MAX_STEPS = 6, 30, 9
CAM = dict(camera_width=64, camera_height=48)
CONFIGS = {
    # map, obs_shape, depth_shape, depth_dtype, env arguments, simulator arguments
    "plain": ("small_loop", (24, 32), (24, 32), "float32", dict(), dict(domain_rand=False)),
    "final": ("small_loop", (24, 32), (48, 64), "float32", dict(final_obs=True), dict(domain_rand=True)),
    "final_objects_fisheye": ("small_loop_only_duckies", (24, 32), (12, 16), "float16", dict(final_obs=True), dict(domain_rand=False, distortion=True)),
    "stack_final": ("small_loop", (24, 32), (24, 32), "float32", dict(final_obs=True, frame_stack=3, grayscale=True), dict(domain_rand=False)),
    "stack": ("small_loop", (24, 32), (24, 32), "float32", dict(frame_stack=2), dict(domain_rand=False)),
    "raw_frames_final": ("small_loop", None, (24, 32), "float32", dict(final_obs=True), dict(domain_rand=False)),
}


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_depth_rides_with_the_observation(cfg):
    import torch
    map_name, obs_shape, ds, dtype, env_kw, sim_kw = CONFIGS[cfg]
    kw = dict(sim_kw, max_steps=MAX_STEPS, **CAM)
    A = DuckietownVecEnv(map_name, N, obs_shape=obs_shape, seed=4, depth_shape=ds, depth_dtype=dtype, **env_kw, **kw)
    B = DuckietownVecEnv(map_name, N, obs_shape=obs_shape, seed=4, **env_kw, **kw)
    ref = BatchedSimulator(map_name, N, action_mode="vel_steer", seed=4, device_reset=True, auto_reset=False, do_reset=False, **kw)
    final = bool(env_kw.get("final_obs"))

    def ref_depth():
        ref.render()
        d = ref.depth(ds[0], ds[1], dtype=dtype)
        ref.sync()
        return d.clone()

    oa, ob = A.reset(), B.reset()
    ref.reset()
    assert torch.equal(oa, ob) and B.depth is None
    assert A.depth.shape == (N, *ds) and A.depth.dtype == getattr(torch, dtype)
    torch.cuda.synchronize()
    assert torch.equal(A.depth, ref_depth())                 # the first frames' map: env.depth
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    n_done, n_new = torch.zeros(N, device="cuda"), 0
    for t in range(STEPS):
        a = torch.rand((N, 2), device="cuda", generator=g) * 2 - 1
        oa, ra, da, ia = A.step(a)
        ob, rb, db, ib = B.step(a)
        torch.cuda.synchronize()
        ref.step(a)                                          # by hand: step -> render -> depth -> reset_done -> render -> depth
        before = ref_depth()
        ref_done = torch.as_tensor(ref.field_device(_ffi.FIELD_DONE), device="cuda").to(torch.bool).clone()
        ref.reset_done()
        after = ref_depth()
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db) and torch.equal(da, ref_done), (cfg, t)
        assert "depth" not in ib and "final_depth" not in ib
        assert ia["depth"] is A.depth                        # one persistent tensor
        assert torch.equal(ia["depth"].view(torch.uint8), after.view(torch.uint8)), (cfg, t)       # byte for byte, the restarted envs' new state included
        assert torch.equal(after[~da], before[~da])          # (an env that did not finish is in the state the step left)
        if final:
            assert ia["final_depth"].shape == A.depth.shape and ia["final_depth"].dtype == A.depth.dtype
            assert torch.equal(ia["final_depth"][da], before[da]), (cfg, t, int(da.sum()))
        else:
            assert "final_depth" not in ia
        n_new += int((after[da] != before[da]).flatten(1).any(dim=1).sum())
        n_done += da.float()
    assert float(n_done.min()) >= 2, cfg                     # every env finished at least twice
    if sim_kw["domain_rand"]:
        assert n_new > 0                                     # a new episode draws another camera: another depth map (with the shared camera the
        #                                                      planes' depth does not depend on the pose, so small maps of two states can agree)
    for e in (A, B):
        e.close()
    ref.close()
