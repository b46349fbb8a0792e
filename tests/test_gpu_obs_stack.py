"""GPU: dtsim_obs_push / BatchedSimulator.push_observation -- the per-env observation history kept in place on the device, held bit for bit
to the numpy model (obs_stack_model.push): element-wise and 16-byte paths, one and many workgroups per env, uint8 / float32, colour / grey,
`first` and `mask` in every combination, Pillow's grey on all 2^24 colours, the newest slot against the real observe, rejected calls."""
import ctypes as C

import numpy as np
import pytest

from dtsim import BatchedSimulator, _ffi
from obs_stack_model import gray_l, push

pytestmark = pytest.mark.gpu

SENTINEL = {np.uint8: 77, np.float32: 0.123}
# (h, w): 7 x 9 = 63 pixels -- no slot size is a multiple of 16 bytes, uint8 slots start misaligned: the element path;
# 12 x 16: the 16-byte path, one workgroup per env; 120 x 160: 16 workgroups per env, several items per thread
SMALL = [(7, 9), (12, 16)]
CASES = [(h, w, n, d) for (h, w) in SMALL for n in (5, 130) for d in (1, 2, 3, 16)] + [(120, 160, 5, 3), (120, 160, 130, 2)]


@pytest.fixture(scope="module")
def sims():
    """One small simulator per batch size (the push needs the handle's stream and N only), closed at the end of the module."""
    made = {}

    def get(n):
        if n not in made:
            made[n] = BatchedSimulator("small_loop", n, camera_width=160, camera_height=120, domain_rand=False, seed=2)
        return made[n]
    yield get
    for s in made.values():
        s.close()


def _selection(kind, n, rng):
    """kind 0: None (the NULL pointer); 1: some envs; 2: every env -- as a bool array."""
    if kind == 0:
        return None
    if kind == 1:
        m = rng.random(n) < 0.4
        m[0], m[n - 1] = True, False                       # both values occur, at the ends of the batch too
        return m
    return np.ones(n, bool)


@pytest.mark.parametrize("gray", [False, True], ids=["rgb", "gray"])
@pytest.mark.parametrize("f32", [False, True], ids=["u8", "f32"])
@pytest.mark.parametrize("h,w,n,depth", CASES)
def test_pushes_match_the_model(sims, h, w, n, depth, f32, gray):
    import torch
    sim = sims(n)
    dt = np.float32 if f32 else np.uint8
    rng = np.random.default_rng(1000 * h + 10 * depth + n)
    want = np.full((n, depth, 1 if gray else 3, h, w), SENTINEL[dt], dt)
    stack = torch.as_tensor(want, device="cuda")
    for t in range(max(2 * depth + 1, 9 + depth)):
        # the nine combinations first (first: none / some / all; mask: none selected -- the sentinel stays --, some, NULL), then plain pushes
        # with a few restarts, so that deep stacks shift all the way through
        fk, mk = (t % 3, t // 3) if t < 9 else (int(t % 5 == 0), 2)
        first = _selection(fk, n, rng)
        mask = _selection(1, n, rng) if mk == 1 else (None if mk == 2 else np.zeros(n, bool))
        obs = rng.integers(0, 256, (n, 3, h, w), dtype=np.uint8)
        d_obs = torch.as_tensor(obs, device="cuda")
        d_first = None if first is None else torch.as_tensor(first, device="cuda")
        d_mask = None if mask is None else torch.as_tensor(mask.astype(np.uint8), device="cuda")
        torch.cuda.synchronize()                           # (the library's stream does not wait for torch's)
        assert sim.push_observation(stack, d_obs, first=d_first, mask=d_mask, grayscale=gray) is stack
        sim.sync()
        want = push(want, obs, first, mask, gray, f32)
        got = stack.cpu().numpy()
        assert np.array_equal(got, want), (t, fk, mk)
        if t < 3:
            assert (got == np.asarray(SENTINEL[dt], dt)).all()
    if depth > 1:                                          # (the schedule ends with shifts: the last env's oldest and newest slots differ)
        assert not np.array_equal(want[n - 1, 0], want[n - 1, -1])


def test_unselected_envs_keep_the_sentinel_where_first_is_set(sims):
    import torch
    n, depth, h, w = 5, 3, 12, 16
    sim = sims(n)
    stack = torch.full((n, depth, 3, h, w), 77, dtype=torch.uint8, device="cuda")
    obs = torch.full((n, 3, h, w), 200, dtype=torch.uint8, device="cuda")
    first = torch.ones(n, dtype=torch.bool, device="cuda")
    mask = torch.as_tensor([0, 1, 0, 0, 1], dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    sim.push_observation(stack, obs, first=first, mask=mask)
    sim.sync()
    got = stack.cpu().numpy()
    assert (got[[0, 2, 3]] == 77).all() and (got[[1, 4]] == 200).all()


@pytest.mark.parametrize("f32", [False, True], ids=["u8", "f32"])
def test_grey_is_pillow_on_every_colour(sims, f32):
    """All 2^24 colours as one [64, 3, 512, 512] push at depth 1 (the pure conversion)."""
    import torch
    sim = sims(64)
    i = torch.arange(1 << 24, dtype=torch.int32, device="cuda").view(64, 1, 512, 512)
    obs = torch.cat([(i >> 16) & 255, (i >> 8) & 255, i & 255], dim=1).to(torch.uint8).contiguous()
    stack = torch.zeros((64, 1, 1, 512, 512), dtype=torch.float32 if f32 else torch.uint8, device="cuda")
    torch.cuda.synchronize()
    sim.push_observation(stack, obs, grayscale=True)
    sim.sync()
    j = np.arange(1 << 24, dtype=np.uint32)
    want = gray_l(np.stack([(j >> 16) & 255, (j >> 8) & 255, j & 255], axis=-1).astype(np.uint8))
    if f32:
        want = want.astype(np.float32) / np.float32(255.0)
    assert np.array_equal(stack.cpu().numpy().reshape(-1), want)


def test_newest_colour_float_slot_is_the_real_observe(sims):
    import torch
    sim = sims(5)
    sim.reset()
    sim.render()
    want = torch.as_tensor(sim.observe(60, 80, chw=True, normalize=True), device="cuda").clone()
    sim.sync()
    assert float(want.std()) > 0.01                        # a picture, not a constant
    o = sim.observe(60, 80, chw=True, normalize=False)
    stack = torch.full((5, 2, 3, 60, 80), 0.123, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    sim.push_observation(stack, o)
    sim.sync()
    assert torch.equal(stack[:, 1], want)
    assert bool((stack[:, 0] == 0.123).all())


def test_rejected_calls_change_nothing(sims):
    import torch
    n, h, w = 5, 12, 16
    sim = sims(n)
    stack = torch.full((n, 16, 3, h, w), 77, dtype=torch.uint8, device="cuda")
    obs = torch.full((n, 3, h, w), 200, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    sp, op = C.c_void_p(stack.data_ptr()), C.c_void_p(obs.data_ptr())
    call = sim._lib.dtsim_obs_push
    for depth, flags in ((0, _ffi.OBS_CHW), (17, _ffi.OBS_CHW), (-3, _ffi.OBS_CHW), (4, _ffi.OBS_HWC), (4, _ffi.OBS_F32 | _ffi.OBS_GRAY),
                         (4, _ffi.OBS_CHW | 8), (4, _ffi.OBS_CHW | 1 << 20)):
        assert call(sim._h, sp, op, depth, h, w, flags, None, None) == _ffi.E_INVALID, (depth, flags)
    for hh, ww in ((0, w), (h, -1)):
        assert call(sim._h, sp, op, 4, hh, ww, _ffi.OBS_CHW, None, None) == _ffi.E_INVALID
    assert call(sim._h, None, op, 4, h, w, _ffi.OBS_CHW, None, None) == _ffi.E_INVALID
    assert call(sim._h, sp, None, 4, h, w, _ffi.OBS_CHW, None, None) == _ffi.E_INVALID
    # the Python call: ValueError before a launch
    bad = [
        (torch.zeros((n, 17, 3, h, w), dtype=torch.uint8, device="cuda"), obs, {}),
        (torch.zeros((n, 4, 1, h, w), dtype=torch.uint8, device="cuda"), obs, {}),                      # grey stack, colour push
        (stack, obs, dict(grayscale=True)),
        (torch.zeros((n, 4, 3, h, w), dtype=torch.float16, device="cuda"), obs, {}),
        (stack, obs.float(), {}),
        (stack, obs[:, :, :, ::2], {}),
        (stack.cpu(), obs, {}),
        (stack, obs, dict(first=torch.ones(n + 1, dtype=torch.uint8, device="cuda"))),
        (stack, obs, dict(mask=np.ones(n, np.uint8))),
        (stack, stack.view(-1)[: n * 3 * h * w].view(n, 3, h, w), {}),                                  # overlap
    ]
    for st, ob, kw in bad:
        with pytest.raises(ValueError):
            sim.push_observation(st, ob, **kw)
    sim.sync()
    assert bool((stack == 77).all()) and bool((obs == 200).all())
