"""`not gpu`: the observation history's model (obs_stack_model) against Pillow and a naive deque, the declaration / export of dtsim_obs_push
with an unchanged ABI version, its argument check without a device, and DuckietownVecEnv's argument errors."""
import collections
import os
import re

import numpy as np
import pytest

from dtsim import DuckietownVecEnv, _ffi
from obs_stack_model import convert, gray_l, push

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gray_l_is_pillow_convert_L_on_every_colour():
    from PIL import Image
    i = np.arange(1 << 24, dtype=np.uint32).reshape(4096, 4096)
    rgb = np.stack([(i >> 16) & 255, (i >> 8) & 255, i & 255], axis=-1).astype(np.uint8)
    want = np.asarray(Image.fromarray(rgb, "RGB").convert("L"))
    assert np.array_equal(gray_l(rgb), want)


@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("depth", [1, 3])
def test_model_push_is_a_deque_per_env(gray, f32, depth):
    rng = np.random.default_rng(7)
    n, h, w = 6, 3, 5
    c = 1 if gray else 3
    dt = np.float32 if f32 else np.uint8
    stack = np.full((n, depth, c, h, w), 0.5 if f32 else 77, dt)
    hist = [collections.deque([stack[e, k].copy() for k in range(depth)], maxlen=depth) for e in range(n)]
    for t in range(2 * depth + 3):
        obs = rng.integers(0, 256, (n, 3, h, w), dtype=np.uint8)
        first = rng.random(n) < 0.3 if t % 3 else None
        mask = rng.random(n) < 0.6 if t % 2 else None
        stack = push(stack, obs, first, mask, gray, f32)
        for e in range(n):
            if mask is not None and not mask[e]:
                continue
            px = np.moveaxis(obs[e], 0, -1).astype(np.int64)                 # [h, w, 3]
            if gray:
                px = ((19595 * px[..., 0] + 38470 * px[..., 1] + 7471 * px[..., 2] + 0x8000) >> 16)[..., None]
            new = np.moveaxis(px, -1, 0).astype(np.uint8)
            new = (new.astype(np.float32) / np.float32(255)) if f32 else new
            if first is not None and first[e]:
                hist[e].clear()
                hist[e].extend([new] * depth)
            else:
                hist[e].append(new)                                          # (maxlen: the oldest leaves)
        want = np.stack([np.stack(list(d)) for d in hist])
        assert stack.dtype == dt and np.array_equal(stack, want), t
    assert convert(obs, gray, f32).shape == (n, c, h, w)


def test_obs_push_declared_mirrored_and_exported():
    src = open(os.path.join(ROOT, "include", "dtsim.h")).read()
    assert re.search(r"\bint dtsim_obs_push\s*\(", src)
    assert int(re.search(r"\bDTSIM_OBS_GRAY\s*=\s*(\d+)", src).group(1)) == _ffi.OBS_GRAY == 4
    assert int(re.search(r"#define DTSIM_OBS_MAX_DEPTH\s+(\d+)", src).group(1)) == _ffi.OBS_MAX_DEPTH == 16
    assert _ffi.OBS_GRAY & (_ffi.OBS_CHW | _ffi.OBS_F32) == 0
    assert "dtsim_obs_push" in _ffi.EXPORTS
    lib = _ffi.load()
    assert len(lib.dtsim_obs_push.argtypes) == 9
    assert _ffi.ABI_VERSION == 12 and lib.dtsim_abi_version() == 12
    assert "#define DTSIM_ABI_VERSION 12" in src


def test_obs_push_rejects_a_null_handle_without_a_device():
    lib = _ffi.load()
    assert lib.dtsim_obs_push(None, None, None, 4, 60, 80, _ffi.OBS_CHW, None, None) == _ffi.E_INVALID
    assert b"dtsim_obs_push" in lib.dtsim_last_error()


@pytest.mark.parametrize("kw", [
    dict(frame_stack=0), dict(frame_stack=17), dict(frame_stack=-1), dict(frame_stack=2.5),
    dict(frame_stack=0, grayscale=True),
    dict(frame_stack=4, obs_shape=None), dict(grayscale=True, obs_shape=None),
    dict(frame_stack=4, chw=False), dict(grayscale=True, chw=False),
    dict(frame_stack=17, obs_shape=None, chw=False),
])
def test_vecenv_argument_errors_come_before_the_simulator(kw):
    """(device 10 ** 6 does not exist: reaching the device or the simulator would raise something else than ValueError)"""
    with pytest.raises(ValueError, match="frame_stack"):
        DuckietownVecEnv("small_loop", 4, device=10 ** 6, **kw)
