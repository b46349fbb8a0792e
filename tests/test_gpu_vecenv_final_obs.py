"""GPU: DuckietownVecEnv(final_obs=True) -- info["final_obs"] holds, for the envs that finished a step, the observation the reference's
step() returns (rendered before the reset), while obs / reward / done / done_code stay bit-identical to the default env; and the
truncated / terminated split of done_code."""
import numpy as np
import pytest

from dtsim import BatchedSimulator, DuckietownVecEnv, _ffi

pytestmark = pytest.mark.gpu

N, STEPS, MAX_STEPS = 96, 70, 30
CAM = dict(camera_width=160, camera_height=120)
CONFIGS = {
    "plain": ("small_loop", (60, 80), dict(domain_rand=False)),
    "light_capture": ("small_loop", (60, 80), dict(domain_rand=False, light_capture=True)),
    "domain_rand": ("small_loop", (60, 80), dict(domain_rand=True)),
    "objects": ("small_loop_only_duckies", (60, 80), dict(domain_rand=False)),
    "raw_frames": ("small_loop", None, dict(domain_rand=False)),
}


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_final_obs_matches_pre_reset_render(cfg):
    import torch
    map_name, obs_shape, kw = CONFIGS[cfg]
    kw = dict(kw, max_steps=MAX_STEPS, **CAM)
    A = DuckietownVecEnv(map_name, N, obs_shape=obs_shape, seed=4, final_obs=True, **kw)
    B = DuckietownVecEnv(map_name, N, obs_shape=obs_shape, seed=4, **kw)
    ref = BatchedSimulator(map_name, N, action_mode="vel_steer", seed=4, device_reset=True, auto_reset=False, do_reset=False, **kw)
    oa, ob = A.reset(), B.reset()
    ref.reset()
    assert torch.equal(oa, ob)
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    n_done, n_differ = torch.zeros(N, device="cuda"), 0
    for t in range(STEPS):
        a = torch.rand((N, 2), device="cuda", generator=g) * 2 - 1
        oa, ra, da, ia = A.step(a)
        ob, rb, db, ib = B.step(a)
        torch.cuda.synchronize()
        ref.step(a)                                        # by hand: step -> full render -> observe -> reset_done
        ref.render()
        if obs_shape is None:
            ro = ref.frames_device()
        else:
            ro = ref.observe(obs_shape[0], obs_shape[1], chw=True, normalize=True)
        ref.sync()
        want = torch.as_tensor(ro, device="cuda").clone()
        ref_done = torch.as_tensor(ref.field_device(_ffi.FIELD_DONE), device="cuda").to(torch.bool).clone()
        ref.reset_done()
        ref.sync()
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db), (cfg, t)
        assert torch.equal(ia["done_code"], ib["done_code"]) and torch.equal(ia["episode_steps"], ib["episode_steps"]), (cfg, t)
        assert torch.equal(da, ref_done), (cfg, t)
        assert torch.equal(ia["final_obs_mask"], da) and ia["final_obs"].shape == oa.shape and ia["final_obs"].dtype == oa.dtype
        fo = ia["final_obs"][da]
        assert torch.equal(fo, want[da]), (cfg, t, int(da.sum()))
        n_differ += int((fo != oa[da]).flatten(1).any(dim=1).sum())   # the first frame of the next episode is another picture
        # the truncated / terminated split, on both envs
        for info, done in ((ia, da), (ib, db)):
            code, steps = info["done_code"], info["episode_steps"]
            assert torch.equal(info["truncated"], done & (code == _ffi.DONE_MAX_STEPS))
            assert torch.equal(info["terminated"], done & ~info["truncated"])
            assert bool((steps[info["truncated"]] == MAX_STEPS).all())
            assert bool(info["terminated"][done & (steps < MAX_STEPS)].all())
        n_done += da.float()
    assert float(n_done.min()) >= 2, cfg                  # every env finished at least twice
    assert n_differ > 0
    for e in (A, B):
        e.close()
    ref.close()
