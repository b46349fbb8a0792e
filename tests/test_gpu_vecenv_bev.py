"""GPU: DuckietownVecEnv(bev_shape=..., bev_instances=True) -- info["bev"] / info["bev_instances"] are the bird's-eye class and id maps
(dtsim_bev) of the state whose observation `obs` shows, byte for byte what the literal call sequence gives on a twin BatchedSimulator that
never renders; with final_obs=True info["final_bev"] / info["final_bev_instances"] hold, for the envs that finished a step, the rows before
the reset, and their rows of info["bev"] their new episode's first state; obs, reward, done and every other info entry (depth and labels
among them) are bit-identical to an env built without the new options.  The pass reads the state, not the camera: camera_rand (a fisheye per
env) and motion_blur (the map of the state after the last sub-update) construct, step and match the same sequence.
64 x 48 cameras, N = 66 (one full chunk of 64 and a tail of 2), max_steps = 3: every env finishes."""
import pytest

from dtsim import BatchedSimulator, DuckietownVecEnv, _ffi

pytestmark = pytest.mark.gpu

N, STEPS, MAX_STEPS = 66, 8, 3
CAM = dict(camera_width=64, camera_height=48)
MAP = "loop_pedestrians"
BEV = dict(bev_shape=(40, 56), bev_cell=0.03, bev_rows_behind=8, bev_instances=True)
NEW_KEYS = {"bev", "bev_instances", "final_bev", "final_bev_instances"}
CONFIGS = {
    # env arguments (also given to the env without the new options), simulator arguments
    "plain": (dict(depth_shape=(12, 16), label_shape=(24, 32)), dict(domain_rand=False)),
    "final": (dict(final_obs=True, depth_shape=(12, 16), label_shape=(24, 32)), dict(domain_rand=True)),
    "camera_rand": (dict(final_obs=True), dict(domain_rand=False, camera_rand=True, distortion=True)),
    "blur": (dict(motion_blur=True, action_mode="wheels"), dict(domain_rand=False)),
}


def same(x, y):
    import torch
    return x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_the_bev_maps_ride_with_the_observation(cfg):
    import torch
    env_kw, sim_kw = CONFIGS[cfg]
    kw = dict(sim_kw, max_steps=MAX_STEPS, **CAM)
    A = DuckietownVecEnv(MAP, N, obs_shape=(24, 32), seed=4, **BEV, **env_kw, **kw)
    B = DuckietownVecEnv(MAP, N, obs_shape=(24, 32), seed=4, **env_kw, **kw)
    blur = A._blur
    ref_kw = dict(kw, frame_rate=30 * (len(blur) - 1)) if blur else kw
    ref = BatchedSimulator(MAP, N, action_mode=env_kw.get("action_mode", "vel_steer"), seed=4, device_reset=True, auto_reset=False, do_reset=False, **ref_kw)
    final = bool(env_kw.get("final_obs"))
    (h, w), cell, rb = BEV["bev_shape"], BEV["bev_cell"], BEV["bev_rows_behind"]

    def ref_pass():                                          # no render: the pass reads the state
        i = torch.empty((N, h, w), dtype=torch.uint8, device="cuda")
        c = ref.bev(h, w, cell=cell, rows_behind=rb, instances_out=i)
        ref.sync()
        return c.clone(), i.clone()

    oa, ob = A.reset(), B.reset()
    ref.reset()
    torch.cuda.synchronize()
    assert same(oa, ob) and B.bev is None and B.bev_instances is None
    assert A.bev.shape == A.bev_instances.shape == (N, h, w) and A.bev.dtype == A.bev_instances.dtype == torch.uint8
    rc, ri = ref_pass()
    assert torch.equal(A.bev, rc) and torch.equal(A.bev_instances, ri)         # the first states' maps: env.bev / env.bev_instances
    assert int(rc.min()) >= 2
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    n_done, n_new, n_obj = torch.zeros(N, device="cuda"), 0, int(ri.any())
    for t in range(STEPS):
        a = torch.rand((N, 2), device="cuda", generator=g) * 2 - 1
        ac = a.clamp(-1.0, 1.0)                              # (made before the synchronize below: the twin's stream does not wait for torch's)
        oa, ra, da, ia = A.step(a)
        ob, rb_, db, ib = B.step(a)
        torch.cuda.synchronize()
        if blur:                                             # by hand: the window's sub-updates, then the map of the state they leave
            for _ in range(len(blur) - 1):
                ref.step(ac, flags=_ffi.STEP_ONE_UPDATE)
        else:
            ref.step(a)
        before_c, before_i = ref_pass()
        ref_done = torch.as_tensor(ref.field_device(_ffi.FIELD_DONE), device="cuda").to(torch.bool).clone()
        ref.reset_done()
        after_c, after_i = ref_pass()
        # everything the env without the new options returns: bit-identical
        assert same(oa, ob) and same(ra, rb_) and same(da, db) and torch.equal(da, ref_done), (cfg, t)
        assert set(ia) - NEW_KEYS == set(ib) and not (set(ib) & NEW_KEYS), (cfg, sorted(ia), sorted(ib))
        for key in ib:
            if key in ("final_obs", "final_depth", "final_labels"):
                assert same(ia[key][da], ib[key][db]), (cfg, t, key)
            else:
                assert same(ia[key], ib[key]), (cfg, t, key)
        assert ia["bev"] is A.bev and ia["bev_instances"] is A.bev_instances      # persistent tensors
        assert torch.equal(ia["bev"], after_c) and torch.equal(ia["bev_instances"], after_i), (cfg, t)    # the restarted envs' first states included
        assert torch.equal(after_c[~da], before_c[~da]) and torch.equal(after_i[~da], before_i[~da])
        if final:
            assert same(ia["final_bev"][da], before_c[da]) and same(ia["final_bev_instances"][da], before_i[da]), (cfg, t, int(da.sum()))
            assert ia["final_bev"].shape == ia["final_bev_instances"].shape == A.bev.shape
        else:
            assert "final_bev" not in ia and "final_bev_instances" not in ia
        n_new += int((after_c[da] != before_c[da]).flatten(1).any(dim=1).sum())
        n_obj += int(after_i.any())
        n_done += da.float()
    assert float(n_done.min()) >= 2, cfg                     # every env finished at least twice
    assert n_new > 0 and n_obj > 0, cfg                      # restarts moved the window, and a duckie lay in one
    for e in (A, B):
        e.close()
    ref.close()


def test_default_arguments_make_no_new_call(monkeypatch):
    import torch
    calls = []
    real = BatchedSimulator.bev
    monkeypatch.setattr(BatchedSimulator, "bev", lambda sim, *a, **k: (calls.append(1), real(sim, *a, **k))[1])
    env = DuckietownVecEnv(MAP, 4, obs_shape=(24, 32), seed=4, final_obs=True, label_shape=(24, 32), max_steps=MAX_STEPS, domain_rand=False, **CAM)
    env.reset()
    for _ in range(4):
        _, _, _, info = env.step(torch.zeros((4, 2), device="cuda"))
        assert not NEW_KEYS & set(info)
    torch.cuda.synchronize()
    assert not calls and env.bev is None and env.bev_instances is None
    env.close()
    env = DuckietownVecEnv(MAP, 4, obs_shape=(24, 32), seed=4, bev_shape=(8, 8), max_steps=MAX_STEPS, domain_rand=False, **CAM)
    env.reset()
    _, _, _, info = env.step(torch.zeros((4, 2), device="cuda"))
    torch.cuda.synchronize()
    assert len(calls) == 2 and "bev" in info and "bev_instances" not in info and env.bev_instances is None     # one pass per shown state, no id map
    env.close()


@pytest.mark.parametrize("kw", [
    dict(bev_instances=True), dict(bev_shape=(0, 8)), dict(bev_shape=(8, 2000)), dict(bev_shape=8), dict(bev_shape=(8, 8), bev_cell=0.0),
    dict(bev_shape=(8, 8), bev_cell=float("inf")), dict(bev_shape=(8, 8), bev_rows_behind=9), dict(bev_shape=(8, 8), bev_rows_behind=-1),
])
def test_the_constructor_refuses_bad_arguments(kw):
    with pytest.raises(ValueError):
        DuckietownVecEnv(MAP, 4, obs_shape=(24, 32), seed=4, max_steps=MAX_STEPS, **CAM, **kw)
