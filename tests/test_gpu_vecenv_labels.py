"""GPU: DuckietownVecEnv(label_shape=...) -- info["labels"] is the label map (dtsim_labels) of the state whose observation `obs` shows, byte
for byte what the literal call sequence gives on a twin BatchedSimulator; with final_obs=True info["final_labels"] holds, for the envs that
finished a step, the labels before the reset, and their rows of info["labels"] their new episode's first state; with depth_shape as well the
depth is bit-identical to an env built without label_shape; without label_shape there is no such key and obs / reward / done are
bit-identical.  64 x 48 cameras, N = 4, max_steps = 3: every env finishes."""
import pytest

from dtsim import BatchedSimulator, DuckietownVecEnv, _ffi

pytestmark = pytest.mark.gpu

N, STEPS, MAX_STEPS = 4, 8, 3
CAM = dict(camera_width=64, camera_height=48)
CONFIGS = {
    # map, obs_shape, label_shape, depth_shape, env arguments, simulator arguments
    "plain": ("small_loop", (24, 32), (24, 32), None, dict(), dict(domain_rand=False)),
    "final_dr": ("small_loop", (24, 32), (48, 64), None, dict(final_obs=True), dict(domain_rand=True)),
    "final_objects_fisheye_depth": ("small_loop_only_duckies", (24, 32), (12, 16), (24, 32), dict(final_obs=True), dict(domain_rand=False, distortion=True)),
    "stack_final_depth": ("small_loop", (24, 32), (24, 32), (12, 16), dict(final_obs=True, frame_stack=3, grayscale=True), dict(domain_rand=False)),
    "stack": ("small_loop", (24, 32), (24, 32), None, dict(frame_stack=2), dict(domain_rand=False)),
    "raw_frames_final": ("small_loop", None, (24, 32), None, dict(final_obs=True), dict(domain_rand=False)),
}


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_labels_ride_with_the_observation(cfg):
    import torch
    map_name, obs_shape, ls, ds, env_kw, sim_kw = CONFIGS[cfg]
    kw = dict(sim_kw, max_steps=MAX_STEPS, **CAM)
    A = DuckietownVecEnv(map_name, N, obs_shape=obs_shape, seed=4, label_shape=ls, depth_shape=ds, **env_kw, **kw)
    B = DuckietownVecEnv(map_name, N, obs_shape=obs_shape, seed=4, depth_shape=ds, **env_kw, **kw)
    ref = BatchedSimulator(map_name, N, action_mode="vel_steer", seed=4, device_reset=True, auto_reset=False, do_reset=False, **kw)
    final = bool(env_kw.get("final_obs"))

    def ref_labels():
        ref.render()
        d = ref.labels(ls[0], ls[1])
        ref.sync()
        return d.clone()

    oa, ob = A.reset(), B.reset()
    ref.reset()
    assert torch.equal(oa, ob) and B.labels is None
    assert A.labels.shape == (N, *ls) and A.labels.dtype == torch.uint8
    torch.cuda.synchronize()
    assert torch.equal(A.labels, ref_labels())               # the first frames' map: env.labels
    assert int(A.labels.min()) >= (0 if sim_kw.get("distortion") else 1) and len(torch.unique(A.labels)) >= 3
    if ds is not None:
        assert torch.equal(A.depth.view(torch.uint8), B.depth.view(torch.uint8))
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    n_done, n_new = torch.zeros(N, device="cuda"), 0
    for t in range(STEPS):
        a = torch.rand((N, 2), device="cuda", generator=g) * 2 - 1
        oa, ra, da, ia = A.step(a)
        ob, rb, db, ib = B.step(a)
        torch.cuda.synchronize()
        ref.step(a)                                          # by hand: step -> render -> labels -> reset_done -> render -> labels
        before = ref_labels()
        ref_done = torch.as_tensor(ref.field_device(_ffi.FIELD_DONE), device="cuda").to(torch.bool).clone()
        ref.reset_done()
        after = ref_labels()
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db) and torch.equal(da, ref_done), (cfg, t)
        assert "labels" not in ib and "final_labels" not in ib
        assert ia["labels"] is A.labels                      # one persistent tensor
        assert torch.equal(ia["labels"], after), (cfg, t)    # byte for byte, the restarted envs' first frames included
        assert torch.equal(after[~da], before[~da])          # (an env that did not finish is in the state the step left)
        if final:
            assert ia["final_labels"].shape == A.labels.shape and ia["final_labels"].dtype == torch.uint8
            assert torch.equal(ia["final_labels"][da], before[da]), (cfg, t, int(da.sum()))
            assert torch.equal(ia["final_obs"], ib["final_obs"]) and torch.equal(ia["final_obs_mask"], ib["final_obs_mask"])
        else:
            assert "final_labels" not in ia
        if ds is not None:                                   # depth beside it: bit-identical to the env without label_shape
            assert torch.equal(ia["depth"].view(torch.uint8), ib["depth"].view(torch.uint8)), (cfg, t)
            if final:
                assert torch.equal(ia["final_depth"][da].view(torch.uint8), ib["final_depth"][db].view(torch.uint8)), (cfg, t)
        else:
            assert "depth" not in ia
        n_new += int((after[da] != before[da]).flatten(1).any(dim=1).sum())
        n_done += da.float()
    assert float(n_done.min()) >= 2, cfg                     # every env finished at least twice
    assert n_new > 0                                         # a restarted env stands elsewhere: other markings in view
    for e in (A, B):
        e.close()
    ref.close()
