"""GPU: DuckietownVecEnv(frame_stack=4, grayscale=...) beside a plain DuckietownVecEnv of the same seed -- the stacked env's obs and
info["final_obs"] equal, bit for bit, the history a model keeps from the plain env's uint8 obs, done and final_obs (first observation of an
episode replicated, no frame crossing an episode border); reward / done / done_code / episode_steps are the plain env's."""
import numpy as np
import pytest

from dtsim import DuckietownVecEnv

pytestmark = pytest.mark.gpu

N, STEPS, MAX_STEPS, K = 96, 70, 30, 4
OBS = (60, 80)
KW = dict(domain_rand=False, max_steps=MAX_STEPS, camera_width=160, camera_height=120)


class Model:
    """The history in torch, exact by construction: grey in integer arithmetic, / 255 through a table numpy divided (float32, IEEE)."""

    def __init__(self, torch, gray, f32):
        self.t, self.gray, self.f32 = torch, gray, f32
        self.lut = torch.as_tensor(np.arange(256, dtype=np.float32) / np.float32(255.0), device="cuda")
        self.stack = None

    def convert(self, obs_u8):                              # [N, 3, h, w] uint8 -> [N, C, h, w]
        v = obs_u8.to(self.t.int64)
        if self.gray:
            v = ((19595 * v[:, 0] + 38470 * v[:, 1] + 7471 * v[:, 2] + 0x8000) >> 16)[:, None]
        return self.lut[v] if self.f32 else v.to(self.t.uint8)

    def restart(self, obs_u8, which=None):                  # the first observation of an episode, in every slot
        new = self.convert(obs_u8)[:, None].repeat(1, K, 1, 1, 1)
        if which is None:
            self.stack = new
        else:
            self.stack[which] = new[which]

    def shift(self, obs_u8):
        self.stack = self.t.cat([self.stack[:, 1:], self.convert(obs_u8)[:, None]], dim=1)

    def flat(self):
        return self.stack.flatten(1, 2)


@pytest.mark.parametrize("final_obs", [False, True], ids=["", "final_obs"])
@pytest.mark.parametrize("normalize", [False, True], ids=["u8", "f32"])
@pytest.mark.parametrize("gray", [False, True], ids=["rgb", "gray"])
def test_stacked_env_matches_the_model(gray, normalize, final_obs):
    import torch
    A = DuckietownVecEnv("small_loop", N, obs_shape=OBS, seed=4, normalize=normalize, final_obs=final_obs, frame_stack=K, grayscale=gray, **KW)
    B = DuckietownVecEnv("small_loop", N, obs_shape=OBS, seed=4, normalize=False, final_obs=final_obs, **KW)
    m = Model(torch, gray, normalize)
    oa, ob = A.reset(), B.reset()
    c = 1 if gray else 3
    assert oa.shape == (N, K * c, *OBS) and oa.dtype == (torch.float32 if normalize else torch.uint8) and oa.is_contiguous()
    m.restart(ob)
    assert torch.equal(oa, m.flat())
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    n_done, n_differ = torch.zeros(N, device="cuda"), 0
    for t in range(STEPS):
        a = torch.rand((N, 2), device="cuda", generator=g) * 2 - 1
        oa, ra, da, ia = A.step(a)
        ob, rb, db, ib = B.step(a)
        torch.cuda.synchronize()
        assert torch.equal(ra, rb) and torch.equal(da, db), t
        assert torch.equal(ia["done_code"], ib["done_code"]) and torch.equal(ia["episode_steps"], ib["episode_steps"]), t
        if final_obs:
            pre = ob.clone()
            pre[db] = ib["final_obs"][db]                  # what every env showed before the reset
            m.shift(pre)
            assert torch.equal(ia["final_obs_mask"], da) and ia["final_obs"].shape == oa.shape and ia["final_obs"].dtype == oa.dtype
            fa = ia["final_obs"][da]
            assert torch.equal(fa, m.flat()[db]), (t, int(da.sum()))
            n_differ += int((fa != oa[da]).flatten(1).any(dim=1).sum())
        else:
            before = m.flat()[db]
            m.shift(ob)
        m.restart(ob, db)
        assert torch.equal(oa, m.flat()), t
        if not final_obs:
            n_differ += int((before != oa[da]).flatten(1).any(dim=1).sum())   # (the last stack of the old episode against the new one)
        if bool(db.any()):                                  # a restarted env shows one frame K times
            r = oa[da].view(-1, K, c, *OBS)
            assert bool((r == r[:, :1]).all())
        n_done += da.float()
    assert float(n_done.min()) >= 2                         # every env finished at least twice
    assert n_differ > 0
    for e in (A, B):
        e.close()


@pytest.mark.parametrize("normalize", [False, True], ids=["u8", "f32"])
def test_frame_stack_1_colour_is_the_plain_env(normalize):
    import torch
    A = DuckietownVecEnv("small_loop", N, obs_shape=OBS, seed=4, normalize=normalize, final_obs=True, frame_stack=1, grayscale=False, **KW)
    B = DuckietownVecEnv("small_loop", N, obs_shape=OBS, seed=4, normalize=normalize, final_obs=True, **KW)
    assert not A._stacked and not hasattr(A, "_stack")
    oa, ob = A.reset(), B.reset()
    assert torch.equal(oa, ob) and oa.shape == (N, 3, *OBS)
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    seen = 0
    for t in range(MAX_STEPS + 2):
        a = torch.rand((N, 2), device="cuda", generator=g) * 2 - 1
        oa, ra, da, ia = A.step(a)
        ob, rb, db, ib = B.step(a)
        torch.cuda.synchronize()
        assert oa.shape == ob.shape and oa.dtype == ob.dtype and torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db), t
        assert sorted(ia) == sorted(ib)
        assert torch.equal(ia["final_obs"][da], ib["final_obs"][db]) and torch.equal(ia["done_code"], ib["done_code"])
        seen += int(da.sum())
    assert seen >= N
    for e in (A, B):
        e.close()


def test_grey_single_frame():
    """grayscale without a history: [N, 1, h, w], Pillow's L of the plain env's observation."""
    import torch
    A = DuckietownVecEnv("small_loop", N, obs_shape=OBS, seed=4, normalize=False, grayscale=True, **KW)
    B = DuckietownVecEnv("small_loop", N, obs_shape=OBS, seed=4, normalize=False, **KW)
    m = Model(torch, True, False)
    oa, ob = A.reset(), B.reset()
    assert oa.shape == (N, 1, *OBS) and torch.equal(oa, m.convert(ob))
    a = torch.full((N, 2), 0.5, device="cuda")
    for t in range(3):
        oa, _, _, _ = A.step(a)
        ob, _, _, _ = B.step(a)
        torch.cuda.synchronize()
        assert torch.equal(oa, m.convert(ob)), t
    for e in (A, B):
        e.close()
