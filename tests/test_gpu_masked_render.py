"""GPU: dtsim_render_masked -- a render pass over the selected envs only.  Per pipeline: a full pass (frames A), a device-sampler reset of
the selected envs, the masked pass (B), a full pass (C).  The selected frames of B must be those of C byte for byte, the others those of A
(the masked quad-record passes never write them; the generic fallback re-renders unchanged state to the same bytes)."""
import numpy as np
import pytest

from dtsim import BatchedSimulator, _ffi

pytestmark = pytest.mark.gpu

W, H = 160, 120
# name -> (map, BatchedSimulator kwargs, render() kwargs, render_pipeline of the pass, DTSIM_RASTER_OLD)
PIPELINES = {
    "v3": ("small_loop", dict(domain_rand=False), {}, "k_raster_v3", None),
    "v3_light": ("small_loop", dict(domain_rand=False, light_capture=True), {}, "k_raster_v3+light", None),
    "v3_obj": ("small_loop_only_duckies", dict(domain_rand=False), {}, "k_raster_v3", None),
    "q": ("small_loop", dict(domain_rand=False), {}, "k_raster_q", "1"),
    "q_obj": ("small_loop_only_duckies", dict(domain_rand=False), {}, "k_raster_q", "1"),
    "v3dr": ("small_loop", dict(domain_rand=True), {}, "k_raster_v3dr", None),
    "v3dr_obj": ("small_loop_only_duckies", dict(domain_rand=True), {}, "k_raster_v3dr", None),
    "generic_segment": ("small_loop_only_duckies", dict(domain_rand=False), dict(segment=True), "k_raster_env", None),
}
SIZES = (1, 63, 64, 65, 1000)
MASKS = ("empty", "all", "first", "last", "third", "rand2pct", "one_bin")


def make_mask(kind, N):
    m = np.zeros(N, bool)
    if kind == "all":
        m[:] = True
    elif kind == "first":
        m[0] = True
    elif kind == "last":
        m[N - 1] = True
    elif kind == "third":
        m[::3] = True
    elif kind == "rand2pct":
        m[np.random.default_rng(N).random(N) < 0.02] = True
    elif kind == "one_bin":
        m[np.random.default_rng(N + 1).permutation(N)[:max(1, N // 10)]] = True
    return m


def frames(sim, **kw):
    sim.render(**kw)
    return sim.frames_host().copy()


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("pipe", list(PIPELINES))
def test_masked_render_writes_exactly_the_selected_frames(pipe, N, monkeypatch):
    import torch
    map_name, kw, rkw, want_pipe, old = PIPELINES[pipe]
    if old:
        monkeypatch.setenv("DTSIM_RASTER_OLD", old)
    sim = BatchedSimulator(map_name, N, camera_width=W, camera_height=H, distortion=True, seed=N + 7, max_steps=100000,
                           action_mode="vel_steer", device_reset=True, do_reset=False, **kw)
    sim.reset()
    sim.step(np.random.default_rng(N).uniform(0.2, 0.9, (3, N, 2)).astype(np.float32), n_steps=3)
    quad = want_pipe.startswith(("k_raster_v3", "k_raster_q"))
    for kind in MASKS:
        m = make_mask(kind, N)
        A = frames(sim, **rkw)
        assert sim.render_pipeline == want_pipe, (pipe, sim.render_pipeline)
        if m.any():
            sim.reset(m)                                   # device sampler, the selected envs only
        if kind == "one_bin":                              # every selected env on env sel[0]'s pose: one sort bin
            sel = np.flatnonzero(m)
            pos, ang = sim.read(_ffi.FIELD_POS).copy(), sim.read(_ffi.FIELD_ANGLE).copy()
            pos[sel] = pos[sel[0]]
            ang[sel] = ang[sel[0]]
            sim.write(_ffi.FIELD_POS, pos)
            sim.write(_ffi.FIELD_ANGLE, ang)
        dm = torch.as_tensor(m, device=f"cuda:{sim.device_index}")
        torch.cuda.synchronize()                           # (the library's stream does not wait for torch's)
        B = frames(sim, mask=dm, **rkw)
        assert sim.render_pipeline == want_pipe, (pipe, kind, sim.render_pipeline)
        rpos = sim.read(_ffi.FIELD_RENDER_POS).copy()
        if quad:                                           # the masked pass's order: the selected envs at [0, live), the others -1
            assert np.array_equal(np.sort(rpos[m]), np.arange(int(m.sum()))), (pipe, kind)
            assert (rpos[~m] == -1).all(), (pipe, kind)
        with pytest.raises(_ffi.DtsimError):               # the post-passes need a full pass
            sim.draw_lines(np.zeros((1, 9), np.float32))
        C = frames(sim, **rkw)
        assert np.array_equal(B[m], C[m]), (pipe, N, kind, np.flatnonzero((B != C).reshape(N, -1).any(axis=1) & m)[:8])
        assert np.array_equal(B[~m], A[~m]), (pipe, N, kind, np.flatnonzero((B != A).reshape(N, -1).any(axis=1) & ~m)[:8])
        if m.any() and kind != "all":
            assert (C[m] != A[m]).any(), (pipe, kind)      # the reset moved the selected envs: the test can see a missed frame
    sim.close()


@pytest.mark.parametrize("bad", ["numpy", "cpu", "int32", "short", "2d"])
def test_mask_validation_raises_before_any_launch(bad):
    import torch
    N = 8
    sim = BatchedSimulator("small_loop", N, camera_width=W, camera_height=H, domain_rand=False, seed=1)
    sim.reset()
    mask = {"numpy": np.ones(N, bool), "cpu": torch.ones(N, dtype=torch.bool), "int32": torch.ones(N, dtype=torch.int32, device="cuda"),
            "short": torch.ones(N - 1, dtype=torch.bool, device="cuda"), "2d": torch.ones((N, 1), dtype=torch.bool, device="cuda")}[bad]
    for call in (lambda: sim.render(mask=mask), lambda: sim.observe(60, 80, mask=mask),
                 lambda: sim.copy_rows(torch.empty((N, 4), device="cuda"), torch.empty((N, 4), device="cuda"), mask)):
        with pytest.raises(ValueError):
            call()
    sim.close()
