"""GPU: DuckietownVecEnv(ipm_shape=..., ipm_valid=True) -- info["ipm"] / info["ipm_valid"] are the ground-projected camera image and its
flags (dtsim_ipm) of the frame whose observation `obs` shows, byte for byte what the literal call sequence (step, render, ipm, reset_done,
render, ipm) gives on a twin BatchedSimulator; with final_obs=True info["final_ipm"] / info["final_ipm_valid"] hold, for the envs that
finished a step, the rows before the reset, and their rows of info["ipm"] their new episode's first frame; obs, reward, done and every other
info entry are bit-identical to an env built without the new options.  With final_obs, frame_stack, obs_shape=None (and chw=False: the
image is HWC), bev_shape beside it, domain_rand and camera_rand.
160 x 120 cameras, N = 66 (one full chunk of 64 and a tail of 2), max_steps = 3: every env finishes."""
import pytest

from dtsim import BatchedSimulator, DuckietownVecEnv, _ffi

pytestmark = pytest.mark.gpu

N, STEPS, MAX_STEPS = 66, 7, 3
CAM = dict(camera_width=160, camera_height=120)       # (the fisheye of a smaller camera shows no floor: the calibration is 640 x 480's)
MAP = "small_loop"
IPM = dict(ipm_shape=(40, 56), ipm_cell=0.015, ipm_rows_behind=4, ipm_valid=True)
NEW_KEYS = {"ipm", "ipm_valid", "final_ipm", "final_ipm_valid"}
CONFIGS = {
    # env arguments (also given to the env without the new options), simulator arguments
    "plain_bev": (dict(obs_shape=(24, 32), bev_shape=(40, 56), bev_cell=0.015, bev_rows_behind=4), dict(domain_rand=False)),
    "final_stack": (dict(obs_shape=(24, 32), final_obs=True, frame_stack=2), dict(domain_rand=True)),
    "raw_hwc": (dict(obs_shape=None, final_obs=True, chw=False), dict(domain_rand=False, distortion=True)),
    "camera_rand": (dict(obs_shape=(24, 32), final_obs=True), dict(domain_rand=False, camera_rand=True, distortion=True)),
}


def same(x, y):
    import torch
    return x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_the_ipm_rides_with_the_observation(cfg):
    import torch
    env_kw, sim_kw = CONFIGS[cfg]
    kw = dict(sim_kw, max_steps=MAX_STEPS, **CAM)
    A = DuckietownVecEnv(MAP, N, seed=4, **IPM, **env_kw, **kw)
    B = DuckietownVecEnv(MAP, N, seed=4, **env_kw, **kw)
    ref = BatchedSimulator(MAP, N, action_mode="vel_steer", seed=4, device_reset=True, auto_reset=False, do_reset=False, **kw)
    final, chw = bool(env_kw.get("final_obs")), env_kw.get("chw", True)
    (h, w), cell, rb = IPM["ipm_shape"], IPM["ipm_cell"], IPM["ipm_rows_behind"]

    def ref_pass():                                          # the literal sequence: the frames of the current state, then the pass
        ref.render()
        v = torch.empty((N, h, w), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        i = ref.ipm(h, w, cell=cell, rows_behind=rb, chw=chw, valid_out=v)
        ref.sync()
        return i.clone(), v.clone()

    oa, ob = A.reset(), B.reset()
    ref.reset()
    torch.cuda.synchronize()
    assert same(oa, ob) and B.ipm is None and B.ipm_valid is None
    assert A.ipm.shape == ((N, 3, h, w) if chw else (N, h, w, 3)) and A.ipm_valid.shape == (N, h, w)
    assert A.ipm.dtype == A.ipm_valid.dtype == torch.uint8
    ri, rv = ref_pass()
    assert torch.equal(A.ipm, ri) and torch.equal(A.ipm_valid, rv)               # the first frames' images: env.ipm / env.ipm_valid
    assert 0.2 < float(rv.float().mean()) < 0.9 and int(ri.max()) > 50           # a picture, not a blank
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    n_done, n_new = torch.zeros(N, device="cuda"), 0
    for t in range(STEPS):
        a = torch.rand((N, 2), device="cuda", generator=g) * 2 - 1
        oa, ra, da, ia = A.step(a)
        ob, rb_, db, ib = B.step(a)
        torch.cuda.synchronize()
        ref.step(a)
        before_i, before_v = ref_pass()
        ref_done = torch.as_tensor(ref.field_device(_ffi.FIELD_DONE), device="cuda").to(torch.bool).clone()
        ref.reset_done()
        after_i, after_v = ref_pass()
        # everything the env without the new options returns: bit-identical
        assert same(oa, ob) and same(ra, rb_) and same(da, db) and torch.equal(da, ref_done), (cfg, t)
        assert set(ia) - NEW_KEYS == set(ib) and not (set(ib) & NEW_KEYS), (cfg, sorted(ia), sorted(ib))
        for key in ib:
            if key.startswith("final_") and key != "final_obs_mask":
                assert same(ia[key][da], ib[key][db]), (cfg, t, key)
            else:
                assert same(ia[key], ib[key]), (cfg, t, key)
        assert ia["ipm"] is A.ipm and ia["ipm_valid"] is A.ipm_valid                # persistent tensors
        assert torch.equal(ia["ipm"], after_i) and torch.equal(ia["ipm_valid"], after_v), (cfg, t)   # the restarted envs' first frames included
        assert torch.equal(after_i[~da], before_i[~da])
        if final:
            assert same(ia["final_ipm"][da], before_i[da]) and same(ia["final_ipm_valid"][da], before_v[da]), (cfg, t, int(da.sum()))
            assert ia["final_ipm"].shape == A.ipm.shape and ia["final_ipm_valid"].shape == A.ipm_valid.shape
        else:
            assert "final_ipm" not in ia and "final_ipm_valid" not in ia
        n_new += int((after_i[da] != before_i[da]).flatten(1).any(dim=1).sum())
        n_done += da.float()
    assert float(n_done.min()) >= 2, cfg                     # every env finished at least twice
    assert n_new > 0, cfg                                    # restarts changed the picture
    for e in (A, B):
        e.close()
    ref.close()


def test_default_arguments_make_no_new_call(monkeypatch):
    import torch
    calls = []
    real = BatchedSimulator.ipm
    monkeypatch.setattr(BatchedSimulator, "ipm", lambda sim, *a, **k: (calls.append(1), real(sim, *a, **k))[1])
    env = DuckietownVecEnv(MAP, 4, obs_shape=(24, 32), seed=4, final_obs=True, bev_shape=(8, 8), max_steps=MAX_STEPS, domain_rand=False, **CAM)
    env.reset()
    for _ in range(4):
        _, _, _, info = env.step(torch.zeros((4, 2), device="cuda"))
        assert not NEW_KEYS & set(info)
    torch.cuda.synchronize()
    assert not calls and env.ipm is None and env.ipm_valid is None
    env.close()
    env = DuckietownVecEnv(MAP, 4, obs_shape=(24, 32), seed=4, ipm_shape=(8, 8), max_steps=MAX_STEPS, domain_rand=False, **CAM)
    env.reset()
    _, _, _, info = env.step(torch.zeros((4, 2), device="cuda"))
    torch.cuda.synchronize()
    assert len(calls) == 2 and "ipm" in info and "ipm_valid" not in info and env.ipm_valid is None     # one pass per shown frame, no flags
    env.close()


@pytest.mark.parametrize("kw", [
    dict(ipm_valid=True), dict(ipm_shape=(0, 8)), dict(ipm_shape=(8, 2000)), dict(ipm_shape=8), dict(ipm_shape=(8, 8), ipm_cell=0.0),
    dict(ipm_shape=(8, 8), ipm_cell=float("inf")), dict(ipm_shape=(8, 8), ipm_rows_behind=9), dict(ipm_shape=(8, 8), ipm_rows_behind=-1),
    dict(ipm_shape=(8, 8), motion_blur=True, action_mode="wheels"), dict(ipm_shape=(8, 8), undistort=True, distortion=True),
    dict(ipm_shape=(8, 8), render=False),
])
def test_the_constructor_refuses_bad_arguments_before_a_device_is_touched(kw, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the simulator was built")
    monkeypatch.setattr(BatchedSimulator, "__init__", no_device)
    with pytest.raises(ValueError):
        DuckietownVecEnv(MAP, 4, obs_shape=(24, 32), seed=4, max_steps=MAX_STEPS, **CAM, **kw)
