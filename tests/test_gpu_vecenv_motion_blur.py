"""GPU: DuckietownVecEnv(motion_blur=...) beside the reference's MotionBlurWrapper.step driven LITERALLY on a second simulator of the same seed
and sub-step rate: clip, then `render(); step(STEP_ONE_UPDATE)` per sub-update and one more render, the blend in torch integers, reset_done and
a full render.  The env renders the window's first frame once (it is the previous window's last) and only the restarted envs after the reset;
its frames, observations, final observations, reward / done / done_code / episode_steps must equal the literal sequence's bit for bit.  The
device sampler is keyed by (seed, env, episode), so both restart alike."""
import numpy as np
import pytest

from dtsim import DuckietownVecEnv, _ffi

pytestmark = pytest.mark.gpu

N, STEPS, MAX_STEPS = 64, 25, 30                            # three sub-updates per step: an episode lasts at most 10 steps
OBS = (60, 80)
KW = dict(domain_rand=False, max_steps=MAX_STEPS, camera_width=160, camera_height=120, action_mode="wheels")


class Literal:
    """MotionBlurWrapper (learning/utils/wrappers.py:8-36) call for call on env.sim, for a window of len(weights) frames; env is a plain
    DuckietownVecEnv built with the sub-step frame_rate, used for its simulator, its stream and its field views only."""

    def __init__(self, torch, env, weights):
        self.t, self.env, self.sim, self.w = torch, env, env.sim, tuple(weights)

    def frames(self):
        self.sim.render()
        return self.env._frames.clone()

    def reset(self):
        self.t.cuda.synchronize()
        with self.t.cuda.stream(self.env.stream):
            self.sim.reset()
            first = self.frames()
        self.t.cuda.synchronize()
        return first

    def blend(self, window):
        S = sum(w * f.to(self.t.int32) for w, f in zip(self.w, window))
        D = sum(self.w)
        return self.t.div(2 * S + D, 2 * D, rounding_mode="floor").to(self.t.uint8)

    def step(self, action):
        """-> (the blurred frames, the newest sub-frame, reward, done, done_code, step_count after the last update, the frames after reset_done)"""
        t, env = self.t, self.env
        t.cuda.synchronize()
        with t.cuda.stream(env.stream):
            a = action.clamp(-1.0, 1.0).contiguous()
            window = []
            for _ in range(len(self.w) - 1):
                window.append(self.frames())
                self.sim.step(a, flags=_ffi.STEP_ONE_UPDATE)
            window.append(self.frames())
            blurred = self.blend(window)
            reward, done, code, steps = env._reward.to(t.float32), env._done.to(t.bool), env._code.clone(), env._steps.clone()
            self.sim.reset_done()
            first = self.frames()
        t.cuda.synchronize()
        return blurred, window[-1], reward, done, code, steps, first

    def observe(self, frames, **kw):
        """B.sim.observe of `frames` copied into the simulator's own frame buffer (the next step renders over it)."""
        t = self.t
        t.cuda.synchronize()
        with t.cuda.stream(self.env.stream):
            self.env._frames.copy_(frames)
            o = t.as_tensor(self.sim.observe(OBS[0], OBS[1], **kw), device="cuda").clone()
        t.cuda.synchronize()
        return o


def actions(torch, g):
    return torch.rand((N, 2), device="cuda", generator=g) * 3 - 1.5       # beyond [-1, 1]: the clip matters


@pytest.mark.parametrize("obs_shape,final_obs", [(None, False), (None, True), (OBS, True)], ids=["raw", "raw-final_obs", "obs-final_obs"])
def test_blurred_env_is_the_literal_wrapper(obs_shape, final_obs):
    import torch
    A = DuckietownVecEnv("small_loop", N, obs_shape=obs_shape, seed=4, final_obs=final_obs, motion_blur=True, **KW)
    B = DuckietownVecEnv("small_loop", N, obs_shape=None, seed=4, frame_rate=90, **KW)
    assert A.sim.frame_rate == 90 and A.sim.delay_steps == B.sim.delay_steps == 14 and A._blur == (80, 15, 4, 1)
    lit = Literal(torch, B, A._blur)
    view = (lambda f: f) if obs_shape is None else (lambda f: lit.observe(f, chw=True, normalize=True))
    oa, first = A.reset(), lit.reset()
    torch.cuda.synchronize()
    assert torch.equal(oa, view(first))                     # reset(): the plain frame
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    age = torch.zeros(N, dtype=torch.int32, device="cuda")
    n_done = n_blur = n_clip = 0
    for t in range(STEPS):
        a = actions(torch, g)
        n_clip += int((a.abs() > 1).sum())
        oa, ra, da, ia = A.step(a)
        blurred, newest, rb, db, cb, sb, first = lit.step(a)
        torch.cuda.synchronize()
        assert torch.equal(ra, rb) and torch.equal(da, db), t
        assert torch.equal(ia["done_code"], cb) and torch.equal(ia["episode_steps"], sb), t
        assert torch.equal(ia["truncated"], cb == _ffi.DONE_MAX_STEPS) and torch.equal(ia["terminated"], cb == _ffi.DONE_INVALID_POSE)
        age += 3
        assert torch.equal(sb, age), t                      # three sub-updates per step
        age[db] = 0
        want_blur, want_first = view(blurred), view(first)
        want = want_blur.clone()
        want[db] = want_first[db]                           # a restarted env shows its new episode's plain first frame
        assert oa.shape == want.shape and oa.dtype == want.dtype and torch.equal(oa, want), (t, int(db.sum()))
        if final_obs:
            assert torch.equal(ia["final_obs_mask"], da) and ia["final_obs"].shape == oa.shape and ia["final_obs"].dtype == oa.dtype
            assert torch.equal(ia["final_obs"][da], want_blur[db]), t
        else:
            assert "final_obs" not in ia
        n_done += int(db.sum())
        n_blur += int((blurred != newest).flatten(1).any(dim=1).sum())
    assert n_done >= N                                      # every env restarted (the time limit: 10 steps)
    assert n_blur > 0 and n_clip > 0
    for e in (A, B):
        e.close()


def test_a_window_of_two_is_one_sub_update():
    import torch
    A = DuckietownVecEnv("small_loop", N, obs_shape=None, seed=4, motion_blur=(1, 1), **KW)
    B = DuckietownVecEnv("small_loop", N, obs_shape=None, seed=4, frame_rate=30, **KW)
    assert A.sim.frame_rate == 30 and A._blur == (1, 1) and len(A._ring) == 2
    lit = Literal(torch, B, (1, 1))
    oa, first = A.reset(), lit.reset()
    torch.cuda.synchronize()
    assert torch.equal(oa, first)
    g = torch.Generator(device="cuda"); g.manual_seed(2)
    age = torch.zeros(N, dtype=torch.int32, device="cuda")
    for t in range(6):
        a = actions(torch, g)
        oa, ra, da, ia = A.step(a)
        blurred, newest, rb, db, cb, sb, first = lit.step(a)
        torch.cuda.synchronize()
        want = blurred.clone()
        want[db] = first[db]
        assert torch.equal(oa, want) and torch.equal(ra, rb) and torch.equal(da, db) and torch.equal(ia["episode_steps"], sb), t
        age += 1
        assert torch.equal(sb, age), t
        age[db] = 0
    for e in (A, B):
        e.close()


def test_numpy_actions_are_clipped_like_tensors():
    import torch
    A = DuckietownVecEnv("small_loop", N, obs_shape=OBS, seed=4, motion_blur=True, **KW)
    B = DuckietownVecEnv("small_loop", N, obs_shape=OBS, seed=4, motion_blur=True, **KW)
    assert torch.equal(A.reset(), B.reset())
    g = torch.Generator(device="cuda"); g.manual_seed(3)
    for t in range(4):
        a = actions(torch, g)
        oa, ra, da, ia = A.step(a)
        ob, rb, db, ib = B.step(a.cpu().numpy().astype(np.float64))          # (any float array: the env converts)
        torch.cuda.synchronize()
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db) and torch.equal(ia["episode_steps"], ib["episode_steps"]), t
    for e in (A, B):
        e.close()


class Model:
    """The observation history in torch (the model of tests/test_gpu_vecenv_stack.py, restated here for a depth K): grey in integer
    arithmetic, / 255 through a table numpy divided (float32, IEEE)."""

    def __init__(self, torch, depth, gray, f32):
        self.t, self.k, self.gray, self.f32 = torch, depth, gray, f32
        self.lut = torch.as_tensor(np.arange(256, dtype=np.float32) / np.float32(255.0), device="cuda")
        self.stack = None

    def convert(self, obs_u8):                              # [N, 3, h, w] uint8 -> [N, C, h, w]
        v = obs_u8.to(self.t.int64)
        if self.gray:
            v = ((19595 * v[:, 0] + 38470 * v[:, 1] + 7471 * v[:, 2] + 0x8000) >> 16)[:, None]
        return self.lut[v] if self.f32 else v.to(self.t.uint8)

    def restart(self, obs_u8, which=None):                  # the first observation of an episode, in every slot
        new = self.convert(obs_u8)[:, None].repeat(1, self.k, 1, 1, 1)
        if which is None:
            self.stack = new
        else:
            self.stack[which] = new[which]

    def shift(self, obs_u8):
        self.stack = self.t.cat([self.stack[:, 1:], self.convert(obs_u8)[:, None]], dim=1)

    def flat(self):
        return self.stack.flatten(1, 2)


@pytest.mark.parametrize("final_obs", [False, True], ids=["", "final_obs"])
def test_stacked_grey_blurred_env_matches_the_model(final_obs):
    """frame_stack=2, grayscale=True on top of the blur, beside an unstacked blurred env of the same seed (uint8, with final observations: they
    are what every env showed before the reset)."""
    import torch
    K = 2
    A = DuckietownVecEnv("small_loop", N, obs_shape=OBS, seed=4, normalize=True, final_obs=final_obs, frame_stack=K, grayscale=True,
                         motion_blur=True, **KW)
    B = DuckietownVecEnv("small_loop", N, obs_shape=OBS, seed=4, normalize=False, final_obs=True, motion_blur=True, **KW)
    m = Model(torch, K, True, True)
    oa, ob = A.reset(), B.reset()
    assert oa.shape == (N, K, *OBS) and oa.dtype == torch.float32 and oa.is_contiguous()
    m.restart(ob)
    assert torch.equal(oa, m.flat())
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    n_done = n_differ = 0
    for t in range(STEPS):
        a = actions(torch, g)
        oa, ra, da, ia = A.step(a)
        ob, rb, db, ib = B.step(a)
        torch.cuda.synchronize()
        assert torch.equal(ra, rb) and torch.equal(da, db) and torch.equal(ia["episode_steps"], ib["episode_steps"]), t
        pre = ob.clone()
        pre[db] = ib["final_obs"][db]                      # the blurred observation of every env before the reset
        m.shift(pre)
        if final_obs:
            assert torch.equal(ia["final_obs_mask"], da) and ia["final_obs"].shape == oa.shape
            fa = ia["final_obs"][da]
            assert torch.equal(fa, m.flat()[db]), t
            n_differ += int((fa != oa[da]).flatten(1).any(dim=1).sum())
        m.restart(ob, db)
        assert torch.equal(oa, m.flat()), t
        if bool(db.any()):                                  # a restarted env shows one frame K times
            r = oa[da]
            assert bool((r == r[:, :1]).all())
        n_done += int(db.sum())
    assert n_done >= N and (n_differ > 0 or not final_obs)
    for e in (A, B):
        e.close()
