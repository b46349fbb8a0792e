"""GPU: dtsim_observe_masked / dtsim_observe_cubic_masked / dtsim_copy_rows -- the rows of the selected envs are written exactly as the
unmasked call writes them, every other row keeps what was there (a sentinel), in all four output layouts."""
import numpy as np
import pytest

from dtsim import BatchedSimulator
from observe_util import content, inject

pytestmark = pytest.mark.gpu

N = 37
BILINEAR = [                       # a subset of observe_util.BILINEAR_CASES: both pow2 kernels + border, and k_observe's row paths
    (640, 480, 160, 120),          # k_observe_pow2<7, 4> + k_observe_border
    (640, 480, 80, 60),            # k_observe_pow2<12, 8>
    (640, 480, 160, 100),          # k_observe, h = hfast, v = table
    (640, 480, 84, 120),           # k_observe, generic taps
    (126, 94, 37, 53),             # k_observe, byte rows
    (160, 120, 200, 150),          # k_observe, up-scale
]
CUBIC = [(640, 480, 84, 84), (126, 94, 37, 53)]
LAYOUTS = [(False, False), (True, False), (False, True), (True, True)]


def _mask():
    m = np.zeros(N, bool)
    m[[0, 5, 6, 20, N - 1]] = True
    return m


def _check(sim, oh, ow, interpolation):
    import torch
    dev = f"cuda:{sim.device_index}"
    m = _mask()
    dm = torch.as_tensor(m, device=dev)
    for chw, norm in LAYOUTS:
        o = sim.observe(oh, ow, chw=chw, normalize=norm, interpolation=interpolation)
        sim.sync()
        full = torch.as_tensor(o, device=dev).clone()
        sentinel = 0.123 if norm else 77
        out = torch.full(full.shape, sentinel, dtype=full.dtype, device=dev)
        torch.cuda.synchronize()
        sim.observe(oh, ow, chw=chw, normalize=norm, out=out, interpolation=interpolation, mask=dm)
        sim.sync()
        got, want = out.cpu().numpy(), full.cpu().numpy()
        assert np.array_equal(got[m], want[m]), (oh, ow, chw, norm, interpolation)
        assert (got[~m] == np.asarray(sentinel, got.dtype)).all(), (oh, ow, chw, norm, interpolation)


@pytest.mark.parametrize("W,H,ow,oh", BILINEAR)
def test_masked_observe_bilinear(W, H, ow, oh):
    sim = BatchedSimulator("small_loop", N, camera_width=W, camera_height=H, domain_rand=False, seed=2)
    sim.reset()
    inject(sim, content("mixed", N, H, W, seed=3))
    _check(sim, oh, ow, "pil_bilinear")
    sim.close()


@pytest.mark.parametrize("W,H,ow,oh", CUBIC)
def test_masked_observe_cubic(W, H, ow, oh):
    sim = BatchedSimulator("small_loop", N, camera_width=W, camera_height=H, domain_rand=False, seed=2)
    sim.reset()
    inject(sim, content("noise", N, H, W, seed=4))
    _check(sim, oh, ow, "cv_cubic")
    sim.close()


@pytest.mark.parametrize("shape,dtype", [((N, 3, 60, 80), "float32"), ((N, 120, 160, 3), "uint8"), ((N, 7, 5), "uint8"), ((N, 1), "float64")])
def test_copy_rows(shape, dtype):
    """16-byte rows and rows of odd byte counts (the bytewise tail)."""
    import torch
    sim = BatchedSimulator("small_loop", N, camera_width=160, camera_height=120, domain_rand=False, seed=2)
    dt = getattr(torch, dtype)
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    src = (torch.rand(shape, device="cuda", generator=g) * 200).to(dt)
    dst = torch.full(shape, 3, dtype=dt, device="cuda")
    m = _mask()
    dm = torch.as_tensor(m, device="cuda")
    torch.cuda.synchronize()                               # (the library's stream does not wait for torch's)
    sim.copy_rows(dst, src, dm)
    sim.sync()
    d, s = dst.cpu().numpy(), src.cpu().numpy()
    assert np.array_equal(d[m], s[m])
    assert (d[~m] == 3).all()
    sim.close()
