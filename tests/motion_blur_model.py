"""The weighted frame blend (dtsim_blend_frames, DuckietownVecEnv(motion_blur=...)) in numpy int64: the statement the GPU is held to, itself held
to the reference's own expression -- np.average(window, axis=0, weights=[0.8, 0.15, 0.04, 0.01]) -- in tests/test_motion_blur_host.py."""
import numpy as np

REF_WEIGHTS = (80, 15, 4, 1)                                # learning/utils/wrappers.py:29, in hundredths, oldest frame first


def sums(frames, weights):
    """(S, D): S = sum of weights[i] * frames[i] per element (int64), D = sum of the weights."""
    assert len(frames) == len(weights) and all(0 <= int(w) <= 255 for w in weights) and 1 <= sum(int(w) for w in weights) <= 256
    S = sum(int(w) * np.asarray(f).astype(np.int64) for f, w in zip(frames, weights))
    return S, sum(int(w) for w in weights)


def blend_u8(frames, weights):
    """S / D rounded half up: (2 S + D) // (2 D)."""
    S, D = sums(frames, weights)
    return ((2 * S + D) // (2 * D)).astype(np.uint8)


def blend_f32(frames, weights):
    """(float)S / (float)D: one IEEE float32 division (S <= 65280 and D <= 256 are exact in float32)."""
    S, D = sums(frames, weights)
    return S.astype(np.float32) / np.float32(D)


def blend(frames, weights, f32=False, out=None, mask=None):
    """What the call leaves in `out`: the blend in the rows of the selected envs (mask None: all), `out`'s own bytes in the others."""
    new = (blend_f32 if f32 else blend_u8)(frames, weights)
    if mask is None:
        return new
    res = np.array(out, copy=True)
    sel = np.asarray(mask).astype(bool)
    res[sel] = new[sel]
    return res


def device_round(S, D):
    """The kernel's division restated (csrc/observe.hip blend_round): ((S + D / 2) << 7) * (2^25 / D + 1) >> 32, in 64 bits here -- on the device the
    first factor is below 2^24, the second fits 32 bits and the shift is the high half of a 32 x 32 bit product."""
    S = np.asarray(S, dtype=np.uint64)
    x = (S + np.uint64(D // 2)) << np.uint64(7)
    assert int(x.max()) < 1 << 24 and (1 << 25) // D + 1 < 1 << 32
    return (x * np.uint64((1 << 25) // D + 1)) >> np.uint64(32)


def every_sum_window():
    """A window [4, 25501] uint8 whose column S realises the sum S = 80 a + 15 b + 4 c + d exactly, for every S in 0 .. 25500 (greedy from the
    heaviest weight, each byte capped at 255)."""
    r = np.arange(255 * 100 + 1, dtype=np.int64)
    cols = []
    for w in REF_WEIGHTS:
        b = np.minimum(r // w, 255)
        cols.append(b)
        r = r - w * b
    assert not r.any()
    return np.stack(cols).astype(np.uint8)
