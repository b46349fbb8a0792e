"""GPU: every kernel path of dtsim_observe / dtsim_observe_cubic, bit-exact on injected adversarial frames (independent per-channel
noise, 1-px 0/255 checkerboards, saturated constants, ramps), in all four output layouts.  Which path each shape reaches is
tests/observe_util.py observe_path, which tests/test_observe_paths_host.py holds the planner (csrc/observe_plan.h) to on the CPU."""
import ctypes as C

import numpy as np
import pytest

from dtsim import BatchedSimulator, _ffi, resample
from observe_util import (BILINEAR_CASES, CONSTANT_KINDS, CUBIC_CASES, content, cubic_headroom, inject, layouts, observe_host, observe_path,
                          pil_bilinear)

pytestmark = pytest.mark.gpu
pytest.importorskip("PIL.Image")

LAYOUTS = [(False, False), (True, False), (False, True), (True, True)]     # (chw, normalize)
PATTERNS = ("checker_x", "checker_y", "checker")
OTHERS = ("ramp_x", "ramp_y", "mixed", "const", "zeros")


def _n_envs(W, H):
    return 3 if W * H > 640 * 480 else 4


def _make(W, H, N):
    sim = BatchedSimulator("small_loop", N, camera_width=W, camera_height=H, distortion=False, domain_rand=False, seed=3)
    if min(W, H) > 1:                          # (the frames are overwritten anyway; a 1-pixel camera is not rendered)
        sim.render()
    sim.sync()
    return sim


@pytest.fixture(scope="module")
def sims():
    """One handle per camera size, shared by the tests of this module (the table cache is keyed by the tables themselves)."""
    cache = {}

    def get(W, H, N=None):
        key = (W, H, N or _n_envs(W, H))
        if key not in cache:
            cache[key] = _make(*key)
        return cache[key]
    yield get
    for s in cache.values():
        s.close()


def _check_layouts(sim, oh, ow, frames, ref, what, **kw):
    for (chw, norm), want in layouts(ref).items():
        got = observe_host(sim, oh, ow, chw=chw, normalize=norm, **kw)
        assert got.dtype == want.dtype and got.shape == want.shape, (what, chw, norm, got.shape)
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)
            raise AssertionError(f"{what} chw={chw} normalize={norm}: {len(bad)} values differ, first at {bad[0].tolist()}: "
                                 f"{got[tuple(bad[0])]} != {want[tuple(bad[0])]}")


@pytest.mark.parametrize("case", list(BILINEAR_CASES), ids=lambda c: "%dx%d-%dx%d" % c)
def test_bilinear_path_matches_pil(sims, case):
    W, H, ow, oh = case
    sim = sims(W, H)
    i = list(BILINEAR_CASES).index(case)
    for kind in ("noise", PATTERNS[i % 3], OTHERS[i % 5], "full"):
        frames = content(kind, sim.num_envs, H, W, seed=i)
        inject(sim, frames)
        ref = pil_bilinear(frames, oh, ow)
        if kind in CONSTANT_KINDS or kind == "full":        # a constant frame resamples to itself on every path (no PIL needed)
            assert np.array_equal(ref, np.broadcast_to(frames[:, :1, :1], ref.shape))
        _check_layouts(sim, oh, ow, frames, ref, f"{BILINEAR_CASES[case]} {kind}")


@pytest.mark.parametrize("switch", ["DTSIM_OBSERVE_STAGED", "DTSIM_OBSERVE_GENERIC"])
def test_ab_switches_give_the_same_bytes(sims, monkeypatch, switch):
    """The table-driven / staged kernels against k_observe_pow2 + k_observe_border on the power-of-two shapes.  The default path
    runs first, before the switch is set (GENERIC is read when a handle builds its tables: the switched handle is a fresh one)."""
    cases = [c for c, p in BILINEAR_CASES.items() if p.startswith("pow2")]
    runs = []
    for i, (W, H, ow, oh) in enumerate(cases):
        sim = sims(W, H)
        frames = content(("noise", "mixed", "checker")[i % 3], sim.num_envs, H, W, seed=100 + i)
        inject(sim, frames)
        runs.append((frames, {lay: observe_host(sim, oh, ow, chw=lay[0], normalize=lay[1]) for lay in LAYOUTS}))
    monkeypatch.setenv(switch, "1")
    for (W, H, ow, oh), (frames, default) in zip(cases, runs):
        sim = _make(W, H, len(frames))
        try:
            inject(sim, frames)
            for lay in LAYOUTS:
                got = observe_host(sim, oh, ow, chw=lay[0], normalize=lay[1])
                assert np.array_equal(got, default[lay]), ((W, H, ow, oh), lay)
            assert np.array_equal(default[(False, False)], pil_bilinear(frames, oh, ow)), (W, H, ow, oh)
        finally:
            sim.close()


@pytest.mark.parametrize("N", [37, 1024])
def test_batch_edges(sims, N):
    """Partial last workgroups of the pow2 and border grids (N = 37) and a large batch (N = 1024): every env at its own offset."""
    W, H, ow, oh = 640, 480, 160, 120
    sim = sims(W, H, N)
    base = content("noise", 1, H, W, seed=N)[0]
    frames = np.empty((N, H, W, 3), np.uint8)
    for e in range(N):                          # cheap per-env content: the noise frame shifted and XOR-ed per env
        frames[e] = np.roll(base, e, axis=1) ^ np.uint8((37 * e) % 256)
    frames[N // 2] = content("checker", 1, H, W)[0]
    frames[N - 1] = 255
    inject(sim, frames)
    sample = sorted({e for e in (0, 1, 63, 64, 65, 511, 512, N // 2, N - 1) if e < N})
    ref = layouts(pil_bilinear(frames[sample], oh, ow))
    for lay in LAYOUTS:
        got = observe_host(sim, oh, ow, chw=lay[0], normalize=lay[1])
        assert got.shape[0] == N
        assert np.array_equal(got[sample], ref[lay]), lay


def test_repeated_calls_on_one_handle(sims):
    """bilinear -> cubic -> bilinear at the same size on one handle: each call stays exact (the two table caches are separate)."""
    W, H, ow, oh = 640, 480, 160, 120
    sim = sims(W, H)
    frames = content("mixed", sim.num_envs, H, W, seed=5)
    inject(sim, frames)
    bil = pil_bilinear(frames, oh, ow)
    cub = np.stack([resample.resize_cubic(f, oh, ow) for f in frames])
    assert not np.array_equal(bil, cub)
    for want, kw in ((bil, {}), (cub, {"interpolation": "cv_cubic"}), (bil, {}), (cub, {"interpolation": "cv_cubic"})):
        assert np.array_equal(observe_host(sim, oh, ow, **kw), want), kw


def test_table_cache_is_keyed_by_the_tables():
    """dtsim_observe called twice at one output size with different (valid) tables uses the second call's tables."""
    import torch
    W, H, ow, oh = 640, 480, 320, 240
    sim = _make(W, H, 2)
    try:
        frames = content("noise", 2, H, W, seed=9)
        inject(sim, frames)
        out = torch.zeros((2, oh, ow, 3), dtype=torch.uint8, device=f"cuda:{sim.device_index}")
        torch.cuda.synchronize(sim.device_index)             # (torch's fill, then the library's stream)
        ip = C.POINTER(C.c_int32)

        def call(bx, kx, by, ky):
            tabs = [np.ascontiguousarray(a, dtype=np.int32) for a in (bx, kx, by, ky)]
            _ffi.check(sim._lib, sim._lib.dtsim_observe(sim._h, C.c_void_p(out.data_ptr()), oh, ow, 0,
                                                        tabs[0].ctypes.data_as(ip), tabs[1].ctypes.data_as(ip), tabs[1].shape[1],
                                                        tabs[2].ctypes.data_as(ip), tabs[3].ctypes.data_as(ip), tabs[3].shape[1]))
            sim.sync()
            return out.cpu().numpy()

        def nearest(n):                          # every second source pixel, one tap of weight 1.0
            return np.stack([2 * np.arange(n), np.ones(n, np.int64)], axis=1), np.full((n, 1), 1 << resample.PRECISION_BITS)
        assert np.array_equal(call(*nearest(ow), *nearest(oh)), frames[:, ::2, ::2])
        assert np.array_equal(call(*resample.coeffs(W, ow), *resample.coeffs(H, oh)), pil_bilinear(frames, oh, ow))
        assert np.array_equal(call(*nearest(ow), *nearest(oh)), frames[:, ::2, ::2])
    finally:
        sim.close()


def test_plans_replace_each_other_on_one_handle():
    """One handle through pow2 -> k_observe -> pow2 -> cubic -> masked pow2: every call rebuilds or reuses the plan of its slot and stays
    exact; a call whose tables are rejected changes nothing, so the next call with the earlier tables is exact too."""
    import torch
    W, H, N = 32, 16, 4
    assert observe_path(W, H, 4, 4).startswith("pow2") and observe_path(W, H, 7, 5).startswith("k_observe")
    sim = _make(W, H, N)
    try:
        frames = content("noise", N, H, W, seed=11)
        inject(sim, frames)
        small = pil_bilinear(frames, 4, 4)
        assert np.array_equal(observe_host(sim, 4, 4), small)
        assert np.array_equal(observe_host(sim, 5, 7), pil_bilinear(frames, 5, 7))
        assert np.array_equal(observe_host(sim, 4, 4), small)
        assert np.array_equal(observe_host(sim, 5, 6, interpolation="cv_cubic"), np.stack([resample.resize_cubic(f, 5, 6) for f in frames]))
        dev = f"cuda:{sim.device_index}"
        out = torch.full((N, 4, 4, 3), 0xA5, dtype=torch.uint8, device=dev)
        mask = torch.tensor([0, 1, 0, 1], dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(sim.device_index)             # (torch's fills, then the library's stream)
        got = observe_host(sim, 4, 4, out=out, mask=mask)
        assert np.array_equal(got[[1, 3]], small[[1, 3]]) and (got[[0, 2]] == 0xA5).all()
        ip = C.POINTER(C.c_int32)
        bx, kx = resample.coeffs(W, 4)
        by, ky = resample.coeffs(H, 4)
        by = by.copy()
        by[2, 0] = by[1, 0] - 1                               # in range, but before the row above
        tabs = [np.ascontiguousarray(a, dtype=np.int32) for a in (bx, kx, by, ky)]
        rc = sim._lib.dtsim_observe(sim._h, C.c_void_p(out.data_ptr()), 4, 4, 0, tabs[0].ctypes.data_as(ip), tabs[1].ctypes.data_as(ip), tabs[1].shape[1],
                                    tabs[2].ctypes.data_as(ip), tabs[3].ctypes.data_as(ip), tabs[3].shape[1])
        assert rc == _ffi.E_INVALID and b"not monotone" in sim._lib.dtsim_last_error()
        assert np.array_equal(observe_host(sim, 4, 4), small)
    finally:
        sim.close()


def test_observe_rejects_a_mismatched_out_buffer(sims):
    """observe(out=...) checks shape, dtype and contiguity before launching: the kernel writes one fixed layout from the data pointer.
    (Every buffer here is at least as large as the request, so nothing can be written out of bounds even without the check.)"""
    import torch
    W, H, ow, oh = 160, 120, 80, 60
    sim = sims(W, H)
    N, dev = sim.num_envs, f"cuda:{sim.device_index}"
    frames = content("noise", N, H, W, seed=3)
    inject(sim, frames)
    bad = [
        (torch.zeros((N, oh, ow, 3), dtype=torch.float32, device=dev), {}),                       # float32 for a uint8 request
        (torch.zeros((N, 3, oh, ow), dtype=torch.uint8, device=dev), {}),                         # CHW buffer, HWC request
        (torch.zeros((N, oh, ow, 3), dtype=torch.uint8, device=dev), {"chw": True}),              # HWC buffer, CHW request
        (torch.zeros((N, ow, oh, 3), dtype=torch.uint8, device=dev), {}),                         # transposed size
        (torch.zeros((N * oh, ow, 3), dtype=torch.uint8, device=dev), {}),                        # same bytes, other rank
        (torch.zeros((N, oh, ow, 6), dtype=torch.uint8, device=dev)[..., :3], {}),                # strided view
    ]
    torch.cuda.synchronize(sim.device_index)
    for buf, kw in bad:
        before = buf.clone()
        with pytest.raises(ValueError):
            sim.observe(oh, ow, out=buf, **kw)
        sim.sync()
        assert torch.equal(buf, before), (tuple(buf.shape), buf.dtype, kw)
    ref = layouts(pil_bilinear(frames, oh, ow))
    for chw, norm in LAYOUTS:
        shape = (N, 3, oh, ow) if chw else (N, oh, ow, 3)
        buf = torch.zeros(shape, dtype=torch.float32 if norm else torch.uint8, device=dev)
        torch.cuda.synchronize(sim.device_index)
        assert sim.observe(oh, ow, chw=chw, normalize=norm, out=buf) is buf
        sim.sync()
        assert np.array_equal(buf.cpu().numpy(), ref[(chw, norm)]), (chw, norm)
    whole = torch.zeros((2 * N, oh, ow, 3), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(sim.device_index)
    sim.observe(oh, ow, out=whole[N:])                                   # a contiguous slice (the sharding receive tensor's way)
    sim.sync()
    assert np.array_equal(whole[N:].cpu().numpy(), ref[(False, False)]) and not whole[:N].any()


@pytest.mark.parametrize("case", CUBIC_CASES, ids=lambda c: "%dx%d-%dx%d" % c)
def test_cubic_matches_the_opencv_statement(sims, case):
    """k_observe_cubic on adversarial frames against dtsim/resample.py resize_cubic (itself checked against a float64 Keys cubic on
    the host), including the int32-headroom worst case: 255 under the positive taps, 0 under the negative lobes."""
    W, H, ow, oh = case
    sim = sims(W, H)
    for i, kind in enumerate(("noise", "checker", "checker_x", "headroom", "full", "const")):
        N = sim.num_envs
        frames = cubic_headroom(N, H, W, oh, ow) if kind == "headroom" else content(kind, N, H, W, seed=i)
        inject(sim, frames)
        ref = np.stack([resample.resize_cubic(f, oh, ow) for f in frames])
        if kind in CONSTANT_KINDS or kind == "full":
            assert np.array_equal(ref, np.broadcast_to(frames[:, :1, :1], ref.shape))
        _check_layouts(sim, oh, ow, frames, ref, f"cubic {kind}", interpolation="cv_cubic")
