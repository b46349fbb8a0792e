"""GPU: dtsim_blend_frames / BatchedSimulator.blend_frames -- the weighted sum of several frame batches, held bit for bit to the numpy model
(motion_blur_model): the 16-byte and the byte path (an odd frame size; an input base one byte off), one / several workgroups per env and more
than one chunk per thread, uint8 (rounded half up) and float32 (one division), the reference's window on every reachable sum, windows with
zero weights and with the largest divisor, `out` aliasing an input, a mask, guard bytes around every buffer, rejected calls.
Inputs are synthetic: nothing is rendered."""
import ctypes as C

import numpy as np
import pytest

from dtsim import BatchedSimulator, _ffi
from motion_blur_model import REF_WEIGHTS, blend, every_sum_window

pytestmark = pytest.mark.gpu

N = 3
# name -> (camera width, height, byte offset of the LAST input inside its allocation)
#   vec:   64 x 48 = 9216 bytes per frame, 576 chunks of 16 bytes: the 16-byte path, three workgroups per env
#   bytes: 66 x 17 = 3366 bytes per frame, not a multiple of 16: the byte path, a last chunk of 6 bytes
#   off1:  64 x 48 with one input base at 1 (mod 16): the byte path although the size would allow the other
#   big:   160 x 160 = 76800 bytes per frame, 4800 chunks for the 16 x 256 threads of an env: some threads take two chunks
KINDS = {"vec": (64, 48, 0), "bytes": (66, 17, 0), "off1": (64, 48, 1), "big": (160, 160, 0)}
WINDOWS = [REF_WEIGHTS, (1,), (1, 1, 1), (255, 1), (0, 7, 0, 3), (32,) * 8]
GUARD, GUARD_BYTE = 64, 0xA5                               # (64: the views stay 16-byte aligned unless a case offsets them)
CANARY = {np.uint8: 77, np.float32: 0.123}


@pytest.fixture(scope="module")
def sims():
    """One handle per camera size (the blend needs the handle's stream, N and frame size only), closed at the end of the module."""
    made = {}

    def get(kind):
        w, h, _ = KINDS[kind]
        if (w, h) not in made:
            made[(w, h)] = BatchedSimulator("small_loop", N, camera_width=w, camera_height=h, domain_rand=False, seed=2)
        return made[(w, h)]
    yield get
    for s in made.values():
        s.close()


def guarded(host, offset=0):
    """`host` on the device inside a larger uint8 allocation: GUARD + offset guard bytes, the data, GUARD guard bytes.  Returns (buffer, view)."""
    import torch
    raw = np.ascontiguousarray(host).view(np.uint8).reshape(-1)
    buf = torch.full((GUARD + offset + raw.size + GUARD,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    body = buf[GUARD + offset: GUARD + offset + raw.size]
    body.copy_(torch.as_tensor(raw))
    return buf, body.view({np.dtype(np.uint8): torch.uint8, np.dtype(np.float32): torch.float32}[host.dtype]).view(host.shape)


def guards_intact(buf, offset, nbytes):
    return bool((buf[:GUARD + offset] == GUARD_BYTE).all()) and bool((buf[GUARD + offset + nbytes:] == GUARD_BYTE).all())


def window_inputs(weights, shape, rng):
    """Rounds of len(weights) host frames of `shape`: the reference's window gets every reachable sum (over as many rounds as that takes),
    every window random bytes with all-0 and all-255 elements."""
    per = int(np.prod(shape))
    cols = np.zeros((len(weights), 0), np.uint8)
    if tuple(weights) == REF_WEIGHTS:
        cols = every_sum_window()
    rounds = max(1, -(-cols.shape[1] // per))
    fill = rng.integers(0, 256, (len(weights), rounds * per - cols.shape[1]), dtype=np.uint8)
    if fill.shape[1] >= 2:
        fill[:, 0], fill[:, -1] = 0, 255
    data = np.concatenate([cols, fill], axis=1)
    return [[data[k, r * per:(r + 1) * per].reshape(shape) for k in range(len(weights))] for r in range(rounds)]


def run(sim, out, frames, weights, mask=None):
    import torch
    torch.cuda.synchronize()                                # (the library's stream does not wait for torch's)
    assert sim.blend_frames(out, frames, weights, mask=mask) is out
    sim.sync()


@pytest.mark.parametrize("f32", [False, True], ids=["u8", "f32"])
@pytest.mark.parametrize("weights", WINDOWS, ids=lambda w: "w" + "_".join(map(str, w)))
@pytest.mark.parametrize("kind", list(KINDS))
def test_blend_matches_the_model(sims, kind, weights, f32):
    w, h, off = KINDS[kind]
    sim, shape = sims(kind), (N, h, w, 3)
    dt = np.float32 if f32 else np.uint8
    rng = np.random.default_rng(100 * w + len(weights) + int(f32))
    rounds = window_inputs(weights, shape, rng)
    assert kind in ("bytes", "big") or tuple(weights) != REF_WEIGHTS or len(rounds) == 1
    for host in rounds:
        offs = [0] * (len(weights) - 1) + [off]
        dev = [guarded(f, o) for f, o in zip(host, offs)]
        obuf, out = guarded(np.full(shape, CANARY[dt], dt))
        run(sim, out, [v for _, v in dev], weights)
        want = blend(host, weights, f32)
        got = out.cpu().numpy()
        assert got.dtype == want.dtype and np.array_equal(got, want)
        assert guards_intact(obuf, 0, want.nbytes)
        for (buf, v), f, o in zip(dev, host, offs):        # the inputs keep their bytes and their guards
            assert np.array_equal(v.cpu().numpy(), f) and guards_intact(buf, o, f.nbytes)
    if tuple(weights) == (32,) * 8:                         # D = 256: all-255 inputs give 255 (and 1.0 * 255)
        full = [guarded(np.full(shape, 255, np.uint8))[1] for _ in weights]
        _, out = guarded(np.full(shape, CANARY[dt], dt))
        run(sim, out, full, weights)
        assert bool((out == 255).all())
    if tuple(weights) == (1,):                              # the identity
        assert np.array_equal(got, host[0].astype(dt))


@pytest.mark.parametrize("which", [0, -1], ids=["first", "last"])
@pytest.mark.parametrize("weights", [REF_WEIGHTS, (32,) * 8], ids=["ref", "w32x8"])
@pytest.mark.parametrize("kind", ["vec", "bytes", "off1"])
def test_uint8_out_may_be_an_input(sims, kind, weights, which):
    """(off1 offsets the last input: aliased with it, `out` itself is the misaligned buffer)"""
    w, h, off = KINDS[kind]
    sim, shape = sims(kind), (N, h, w, 3)
    host = window_inputs(weights, shape, np.random.default_rng(7 + w))[0]
    offs = [0] * (len(weights) - 1) + [off]
    dev = [guarded(f, o) for f, o in zip(host, offs)]
    frames = [v for _, v in dev]
    run(sim, frames[which], frames, weights)
    want = blend(host, weights)
    assert np.array_equal(frames[which].cpu().numpy(), want)
    assert not np.array_equal(want, host[which])            # (the call changed it)
    for k, ((buf, v), f, o) in enumerate(zip(dev, host, offs)):
        assert guards_intact(buf, o, f.nbytes)
        if k != which % len(weights):
            assert np.array_equal(v.cpu().numpy(), f)


@pytest.mark.parametrize("f32", [False, True], ids=["u8", "f32"])
@pytest.mark.parametrize("kind", ["vec", "bytes", "off1"])
def test_mask_selects_env_1_only(sims, kind, f32):
    import torch
    w, h, off = KINDS[kind]
    sim, shape = sims(kind), (N, h, w, 3)
    dt = np.float32 if f32 else np.uint8
    host = window_inputs(REF_WEIGHTS, shape, np.random.default_rng(11 + w))[0]
    offs = [0, 0, 0, off]
    dev = [guarded(f, o) for f, o in zip(host, offs)]
    canary = np.full(shape, CANARY[dt], dt)
    obuf, out = guarded(canary)
    for mask in (torch.as_tensor([0, 1, 0], dtype=torch.uint8, device="cuda"), torch.as_tensor([False, True, False], device="cuda")):
        run(sim, out, [v for _, v in dev], REF_WEIGHTS, mask=mask)
        got = out.cpu().numpy()
        want = blend(host, REF_WEIGHTS, f32, out=canary, mask=[0, 1, 0])
        assert np.array_equal(got, want) and guards_intact(obuf, 0, want.nbytes)
        assert got[[0, 2]].tobytes() == canary[[0, 2]].tobytes()          # every byte of the unselected rows
        assert not np.array_equal(got[1], canary[1])
    none = torch.zeros(N, dtype=torch.uint8, device="cuda")
    obuf, out = guarded(canary)
    run(sim, out, [v for _, v in dev], REF_WEIGHTS, mask=none)
    assert out.cpu().numpy().tobytes() == canary.tobytes() and guards_intact(obuf, 0, canary.nbytes)


def test_rejected_calls_change_nothing(sims):
    import torch
    sim = sims("vec")
    w, h, _ = KINDS["vec"]
    shape = (N, h, w, 3)
    frames = [torch.full(shape, 200, dtype=torch.uint8, device="cuda") for _ in range(4)]
    out = torch.full(shape, 77, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    fp = (C.c_void_p * 9)(*[frames[0].data_ptr()] * 9)
    op = C.c_void_p(out.data_ptr())
    call = sim._lib.dtsim_blend_frames
    u32 = lambda *v: (C.c_uint32 * len(v))(*v)
    for wts, n, flags in ((u32(80, 15, 4, 1), 0, 0), (u32(*[1] * 9), 9, 0), (u32(80, 256, 4, 1), 4, 0), (u32(0, 0, 0, 0), 4, 0),
                          (u32(255, 1, 1, 0), 4, 0), (u32(80, 15, 4, 1), 4, _ffi.OBS_CHW), (u32(80, 15, 4, 1), 4, _ffi.OBS_F32 | _ffi.OBS_GRAY)):
        assert call(sim._h, op, fp, wts, n, flags, None) == _ffi.E_INVALID, (list(wts), n, flags)
    assert call(sim._h, None, fp, u32(80, 15, 4, 1), 4, 0, None) == _ffi.E_INVALID
    assert call(sim._h, op, (C.c_void_p * 4)(frames[0].data_ptr(), None, frames[2].data_ptr(), frames[3].data_ptr()), u32(80, 15, 4, 1), 4, 0,
                None) == _ffi.E_INVALID
    # the Python call: ValueError before a launch
    f32_inside = torch.zeros(N * h * w * 3 + 4, dtype=torch.float32, device="cuda")
    bad = [
        (out, frames, (80, 15, 4)),                                                   # one weight short
        (out, frames, (80, 256, 4, 1)), (out, frames, (0, 0, 0, 0)), (out, frames, (255, 1, 1, 0)), (out, frames, (80, -1, 4, 1)),
        (out, frames, (80.5, 15, 4, 1)), (out, frames, None),
        (out, [], ()), (out, frames * 3, (1,) * 12), (out, frames[0], (1,)),          # no / too many frames, a bare tensor
        (out, [f.float() for f in frames], REF_WEIGHTS),
        (out.to(torch.float16), frames, REF_WEIGHTS),
        (out.cpu(), frames, REF_WEIGHTS), (out, [frames[0].cpu()] + frames[1:], REF_WEIGHTS),
        (out[:, :, ::2], frames, REF_WEIGHTS), (out[:2], frames, REF_WEIGHTS),
        (out, frames[:3] + [frames[3].permute(0, 2, 1, 3)], REF_WEIGHTS),
        (f32_inside[:-4].view(shape), frames[:3] + [f32_inside.view(torch.uint8)[16:16 + N * h * w * 3].view(shape)], REF_WEIGHTS),   # float32 out over an input
        (frames[0].view(-1)[1:], frames, REF_WEIGHTS),
    ]
    for o, f, wts in bad:
        with pytest.raises(ValueError):
            sim.blend_frames(o, f, wts)
    with pytest.raises(ValueError):
        sim.blend_frames(out, frames, REF_WEIGHTS, mask=np.ones(N, np.uint8))
    with pytest.raises(ValueError):
        sim.blend_frames(out, frames, REF_WEIGHTS, mask=torch.ones(N + 1, dtype=torch.uint8, device="cuda"))
    sim.sync()
    assert bool((out == 77).all()) and all(bool((f == 200).all()) for f in frames)


def test_a_handle_without_render_is_refused():
    import torch
    sim = BatchedSimulator("small_loop", N, camera_width=64, camera_height=48, domain_rand=False, seed=2, render=False)
    f = torch.zeros((N, 48, 64, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = sim._lib.dtsim_blend_frames(sim._h, C.c_void_p(f.data_ptr()), (C.c_void_p * 1)(f.data_ptr()), (C.c_uint32 * 1)(1), 1, 0, None)
    assert rc == _ffi.E_STATE
    sim.close()
