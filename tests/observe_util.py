"""Helpers of the observation-resize tests: which kernel path of dtsim_observe a shape reaches (a restatement of the planner,
csrc/observe_plan.h dt_observe_plan, which tests/test_observe_paths_host.py holds it to, and of the branches inside csrc/observe.hip
k_observe), adversarial frame content, and injection of arbitrary frames into a handle's frame batch (GPU)."""
import zlib

import numpy as np

from dtsim import resample

PREC = resample.PRECISION_BITS
STAGE_ROWS = 8                 # DT_OBS_STAGE_ROWS (csrc/observe_plan.h)
PF_WORDS = 16 * 256            # k_observe's prefetch registers x threads per workgroup


def _uniform(bounds, taps, n_in, n_out, S):
    """dt_observe_uniform: every interior output coordinate has the same 2S small-integer taps starting at S*o - S/2.
    Returns the tap shift (22 - common trailing zeros) or None."""
    ksize = taps.shape[1]
    if n_out < 3 or n_out * S != n_in or 2 * S > ksize or 2 * S > 16:
        return None
    k1 = [int(v) for v in taps[1, :2 * S]]
    if min(k1) <= 0:
        return None
    common = min([22] + [(v & -v).bit_length() - 1 for v in k1])
    q = [v >> common for v in k1]
    if max(q) > 255 or sum(q) != 1 << (22 - common) or not 1 <= 22 - common <= 7:
        return None
    for o in range(1, n_out - 1):
        if bounds[o, 0] != S * o - S // 2 or bounds[o, 1] != 2 * S or [int(v) for v in taps[o, :2 * S]] != k1:
            return None
    return 22 - common


def fast_taps(W, H, ow, oh, generic=False):
    """(hfast, hn, vfast) of the plan: the power-of-two scales whose interior taps are uniform (0: none), and the dwords of a column window."""
    hfast = hn = vfast = 0
    if not generic:
        if ow != W and (W * 3) % 4 == 0:
            bx, kx = resample.coeffs(W, ow)
            for S in (4, 8):
                if _uniform(bx, kx, W, ow, S) is None:
                    continue
                start = -3 * S // 2
                hoff = start & ~3
                n = (3 * 2 * S + (start - hoff) + 3) // 4
                if n in (7, 12):
                    hfast, hn = S, n
                    break
        if oh != H and (ow * 3) % 4 == 0:
            by, ky = resample.coeffs(H, oh)
            for S in (2, 4, 8):
                if _uniform(by, ky, H, oh, S) is not None:
                    vfast = S
                    break
    return hfast, hn, vfast


def observe_path(W, H, ow, oh, staged=False, generic=False):
    """The kernel path dtsim_observe takes for camera W x H -> ow x oh (DTSIM_OBSERVE_STAGED / DTSIM_OBSERVE_GENERIC as flags).
    "pow2<HN,SY>/tail<t>" for k_observe_pow2 (+ k_observe_border), else "k_observe/h=<..>/v=<..>/PER=<..>/load=<..>"."""
    hfast, hn, vfast = fast_taps(W, H, ow, oh, generic)
    if hfast and vfast and ow >= 3 and oh >= 3 and not staged and hn in (7, 12) and vfast in (2, 4, 8):
        return f"pow2<{hn},{vfast}>/tail{(oh - 2) % 4}"
    kx_n = resample.coeffs(W, ow)[1].shape[1] if ow != W else 0
    if ow == W:
        h = "copy"
    elif hfast:
        h = "hfast"
    elif kx_n <= 9:
        h = "window9"
    else:
        h = "generic"
    per = 4 if (ow * 3) % 4 == 0 else 1
    if per == 4 and vfast:
        v = "twolane"
    elif oh == H:
        v = "copy"
    else:
        v = "table"
    aligned = (W * 3) % 4 == 0
    words = (W * 3 + 3) // 4
    load = ("pipelined" if STAGE_ROWS * words <= PF_WORDS else "staged") if aligned else "bytes"
    return f"k_observe/h={h}/v={v}/PER={per}/load={load}"


# (camera W, H, output ow, oh) -> the path it must reach.  Every branch of the selection is in here; the GPU tests run these shapes.
BILINEAR_CASES = {
    (640, 480, 160, 240): "pow2<7,2>/tail2",
    (640, 480, 160, 120): "pow2<7,4>/tail2",
    (640, 480, 160, 60): "pow2<7,8>/tail2",
    (640, 480, 80, 240): "pow2<12,2>/tail2",
    (32, 16, 4, 4): "pow2<12,4>/tail2",
    (640, 480, 80, 60): "pow2<12,8>/tail2",
    (800, 600, 200, 150): "pow2<7,4>/tail0",
    (64, 44, 16, 11): "pow2<7,4>/tail1",
    (64, 52, 16, 13): "pow2<7,4>/tail3",
    (16, 12, 4, 3): "pow2<7,4>/tail1",                                  # oh = 3: one interior row
    (640, 480, 160, 100): "k_observe/h=hfast/v=table/PER=4/load=pipelined",
    (12, 12, 3, 3): "k_observe/h=hfast/v=table/PER=1/load=pipelined",
    (800, 600, 200, 100): "k_observe/h=hfast/v=table/PER=4/load=staged",
    (800, 600, 200, 600): "k_observe/h=hfast/v=copy/PER=4/load=staged",
    (640, 480, 320, 240): "k_observe/h=window9/v=twolane/PER=4/load=pipelined",
    (640, 480, 200, 150): "k_observe/h=window9/v=table/PER=4/load=pipelined",
    (640, 480, 320, 480): "k_observe/h=window9/v=copy/PER=4/load=pipelined",
    (800, 600, 400, 300): "k_observe/h=window9/v=twolane/PER=4/load=staged",
    (640, 480, 84, 120): "k_observe/h=generic/v=twolane/PER=4/load=pipelined",
    (640, 480, 60, 45): "k_observe/h=generic/v=table/PER=4/load=pipelined",
    (640, 480, 85, 64): "k_observe/h=generic/v=table/PER=1/load=pipelined",
    (640, 480, 213, 160): "k_observe/h=window9/v=table/PER=1/load=pipelined",
    (126, 94, 37, 53): "k_observe/h=window9/v=table/PER=1/load=bytes",
    (640, 480, 640, 240): "k_observe/h=copy/v=twolane/PER=4/load=pipelined",
    (640, 480, 640, 480): "k_observe/h=copy/v=copy/PER=4/load=pipelined",
    (160, 120, 200, 150): "k_observe/h=window9/v=table/PER=4/load=pipelined",   # upscale
    (640, 480, 1, 1): "k_observe/h=generic/v=table/PER=1/load=pipelined",
    (640, 480, 2, 480): "k_observe/h=generic/v=copy/PER=1/load=pipelined",
    (640, 480, 3, 3): "k_observe/h=generic/v=table/PER=1/load=pipelined",
}

# (camera W, H, output ow, oh) of the cubic GPU tests: k_observe_cubic's dword / byte row loads, both replicated borders
CUBIC_CASES = [
    (640, 480, 160, 120),        # dword rows, integer down-scale
    (640, 480, 84, 84),          # dword rows, fractional down-scale
    (160, 120, 200, 150),        # dword rows, up-scale
    (126, 94, 37, 53),           # byte rows (126 * 3 % 4 != 0)
    (126, 94, 300, 7),           # byte rows, up along x, strong down along y
    (64, 48, 64, 48),            # identity
    (1, 9, 5, 4),                # 1-pixel source width
    (12, 1, 7, 3),               # 1-pixel source height
]

# what the GPU tests must reach between them (branch -> predicate on the path string)
REQUIRED_BRANCHES = {
    **{f"pow2<{hn},{sy}>": (lambda p, hn=hn, sy=sy: p.startswith(f"pow2<{hn},{sy}>")) for hn in (7, 12) for sy in (2, 4, 8)},
    **{f"pow2 tail {t}": (lambda p, t=t: p.startswith("pow2") and p.endswith(f"tail{t}")) for t in range(4)},
    **{f"h={h}": (lambda p, h=h: f"/h={h}/" in p) for h in ("copy", "hfast", "window9", "generic")},
    **{f"v={v}": (lambda p, v=v: f"/v={v}/" in p) for v in ("copy", "twolane", "table")},
    **{f"PER={n}": (lambda p, n=n: f"/PER={n}/" in p) for n in (1, 4)},
    **{f"load={ld}": (lambda p, ld=ld: p.endswith(f"load={ld}")) for ld in ("pipelined", "staged", "bytes")},
    "hfast + v=table": lambda p: "/h=hfast/v=table/" in p,
    "hfast + PER=1": lambda p: "/h=hfast/" in p and "/PER=1/" in p,
    "hfast + staged": lambda p: "/h=hfast/" in p and p.endswith("staged"),
    **{f"window9 + {v}": (lambda p, v=v: f"/h=window9/v={v}/" in p) for v in ("twolane", "table", "copy")},
    "copy + twolane": lambda p: "/h=copy/v=twolane/" in p,
    "window9 + staged": lambda p: "/h=window9/" in p and p.endswith("staged"),
    "generic + twolane": lambda p: "/h=generic/v=twolane/" in p,
    "generic + table": lambda p: "/h=generic/v=table/" in p,
}


# ---- adversarial frame content: uint8 [N, H, W, 3], seeded, every env different (an env-stride error shows) ---------------
def content(kind, N, H, W, seed=0):
    rng = np.random.default_rng([seed, N, H, W, zlib.crc32(kind.encode())])
    y = np.arange(H).reshape(1, H, 1, 1)
    x = np.arange(W).reshape(1, 1, W, 1)
    e = np.arange(N).reshape(N, 1, 1, 1)
    c = np.arange(3).reshape(1, 1, 1, 3)
    if kind == "noise":                        # independent uniform noise per pixel and channel
        return rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    if kind == "checker_x":                    # 1-px 0/255 period along x, each channel (and env) phase-shifted
        return (((x + e + c) % 2) * 255).astype(np.uint8) + np.zeros((N, H, W, 3), np.uint8)
    if kind == "checker_y":
        return (((y + e + c + 1) % 2) * 255).astype(np.uint8) + np.zeros((N, H, W, 3), np.uint8)
    if kind == "checker":
        return (((x + y + e + c * (c + 1) // 2) % 2) * 255).astype(np.uint8) + np.zeros((N, H, W, 3), np.uint8)
    if kind == "zeros":
        return np.zeros((N, H, W, 3), np.uint8)
    if kind == "full":
        return np.full((N, H, W, 3), 255, np.uint8)
    if kind == "const":                        # per-env / per-channel constants
        v = rng.integers(0, 256, (N, 1, 1, 3), dtype=np.uint8)
        v[0, 0, 0] = (0, 255, 1)
        return np.broadcast_to(v, (N, H, W, 3)).copy()
    if kind == "ramp_x":                       # an off-by-one tap origin becomes a systematic error
        return ((x + 17 * e + 85 * c) % 256).astype(np.uint8) + np.zeros((N, H, W, 3), np.uint8)
    if kind == "ramp_y":
        return ((7 * y + 17 * e + 85 * c) % 256).astype(np.uint8) + np.zeros((N, H, W, 3), np.uint8)
    if kind == "mixed":                        # saturated blocks, noise and a ramp in one frame
        f = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
        f[:, : H // 2, : W // 3] = (((x + y + c) % 2) * 255)[0, : H // 2, : W // 3]
        f[:, H // 2:, W // 3: 2 * W // 3] = 255
        f[:, : H // 2, 2 * W // 3:] = ((x + 85 * c) % 256)[0, 0, 2 * W // 3:]
        return f
    raise ValueError(kind)


CONSTANT_KINDS = ("zeros", "full", "const")


def cubic_headroom(N, H, W, oh, ow):
    """The int32-headroom worst case of the cubic resize: 255 where the product of the two axes' taps is positive (both on the
    centre taps or both on the negative lobes), 0 where it is negative -- as far as the windows of neighbouring outputs agree."""
    def sign(n_in, n_out):
        first, taps = resample.cubic_coeffs(n_in, n_out)
        s = np.zeros(n_in, np.int64)
        for d in range(n_out):
            for k in range(4):
                i = min(max(int(first[d]) + k, 0), n_in - 1)
                if s[i] == 0 or taps[d, k] > 0:
                    s[i] = 1 if taps[d, k] > 0 else -1
        s[s == 0] = 1
        return s
    sy, sx = sign(H, oh), sign(W, ow)
    f = ((sy[:, None] * sx[None, :]) > 0).astype(np.uint8) * 255
    out = np.broadcast_to(f[None, :, :, None], (N, H, W, 3)).copy()
    out[1::2] = 255 - out[1::2]                # odd envs: the most negative sum instead
    return out


# ---- plain float64 references -----------------------------------------------------------------------------------------
def keys_cubic_resize(img, out_h, out_w, A=-0.75):
    """float64 Keys-cubic resize (OpenCV INTER_CUBIC's geometry: fx = (d + 0.5) * in / out - 0.5, four taps at floor(fx) - 1 ..
    floor(fx) + 2, replicated borders), exact taps, rounded and clipped once at the end."""
    def kern(t):
        t = np.abs(t)
        return np.where(t <= 1, ((A + 2) * t - (A + 3)) * t * t + 1, np.where(t < 2, ((A * t - 5 * A) * t + 8 * A) * t - 4 * A, 0.0))

    def weights(n_in, n_out):
        fx = (np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5
        sx = np.floor(fx)
        t = fx - sx
        idx = sx.astype(np.int64)[:, None] + np.arange(-1, 3)[None, :]
        w = kern(t[:, None] - np.arange(-1, 3)[None, :])
        m = np.zeros((n_out, n_in))
        for k in range(4):
            np.add.at(m, (np.arange(n_out), np.clip(idx[:, k], 0, n_in - 1)), w[:, k])
        return m
    H, W = img.shape[:2]
    my, mx = weights(H, out_h), weights(W, out_w)
    v = my @ img.astype(np.float64).reshape(H, -1)                          # [out_h, W * C]
    v = np.einsum("pw,owc->opc", mx, v.reshape(out_h, W, -1))
    return np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8).reshape((out_h, out_w) + img.shape[2:])


def pil_bilinear(frames, oh, ow):
    from PIL import Image
    return np.stack([np.asarray(Image.fromarray(f).resize((ow, oh), Image.BILINEAR)) for f in frames])


def layouts(ref_u8_hwc):
    """The four output layouts of observe() from a uint8 [N, h, w, 3] result: {(chw, normalize): array}."""
    chw = np.ascontiguousarray(ref_u8_hwc.transpose(0, 3, 1, 2))
    return {(False, False): ref_u8_hwc, (True, False): chw,
            (False, True): ref_u8_hwc.astype(np.float32) / np.float32(255), (True, True): chw.astype(np.float32) / np.float32(255)}


# ---- GPU: arbitrary frames into the handle's frame batch ---------------------------------------------------------------
def inject(sim, frames):
    """Overwrite the handle's frame batch with `frames` (uint8 [N, H, W, 3]) and check the copy landed: the copy runs on torch's
    stream, the library on its own, so torch is synchronised before the next library call."""
    import torch
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    assert frames.shape == (sim.num_envs, sim.camera_height, sim.camera_width, 3)
    sim.sync()
    torch.as_tensor(sim.frames_device(), device=f"cuda:{sim.device_index}").copy_(torch.from_numpy(frames))
    torch.cuda.synchronize(sim.device_index)
    assert np.array_equal(sim.frames_host(), frames)


def observe_host(sim, h, w, **kw):
    """observe() on the injected frames, synchronised, as a host array."""
    import torch
    o = sim.observe(h, w, **kw)
    sim.sync()
    return torch.as_tensor(o, device=f"cuda:{sim.device_index}").cpu().numpy()
