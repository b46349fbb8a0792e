"""The observation history (dtsim_obs_push, DuckietownVecEnv(frame_stack=..., grayscale=...)) in numpy: the statement the GPU is held to,
bit for bit.  Helper, not a test."""
import numpy as np


def gray_l(rgb_u8):
    """Pillow's convert("L") of uint8 RGB, channel axis LAST ([..., 3] -> [...]): (19595 R + 38470 G + 7471 B + 0x8000) >> 16."""
    c = np.asarray(rgb_u8).astype(np.uint32)
    return ((19595 * c[..., 0] + 38470 * c[..., 1] + 7471 * c[..., 2] + 0x8000) >> 16).astype(np.uint8)


def convert(obs_u8, gray, f32):
    """[N, 3, h, w] uint8 -> one stack slot [N, C, h, w]: grey (C = 1) and / or float32 / 255 as the observe kernels normalise."""
    v = np.asarray(obs_u8)
    assert v.dtype == np.uint8 and v.ndim == 4 and v.shape[1] == 3
    if gray:
        v = gray_l(np.moveaxis(v, 1, -1))[:, None]
    return v.astype(np.float32) / np.float32(255.0) if f32 else v


def push(stack, obs_u8, first=None, mask=None, gray=False, f32=False):
    """A new [N, depth, C, h, w] stack: for every env selected by `mask` (None: all), with first[e] set every slot is the new observation,
    else the slots move one down (slot 0 is the oldest) and the last takes it; unselected envs keep their row, whatever `first` says."""
    out = np.array(stack, copy=True)
    new = convert(obs_u8, gray, f32)
    assert out.dtype == new.dtype and out.shape[0] == new.shape[0] and out.shape[2:] == new.shape[1:]
    n = out.shape[0]
    first = np.zeros(n, bool) if first is None else np.asarray(first).astype(bool)
    mask = np.ones(n, bool) if mask is None else np.asarray(mask).astype(bool)
    for e in range(n):
        if not mask[e]:
            continue
        if first[e]:
            out[e, :] = new[e]
        else:
            out[e, :-1] = stack[e, 1:]
            out[e, -1] = new[e]
    return out
