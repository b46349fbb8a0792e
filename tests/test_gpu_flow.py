"""`-m gpu`: dtsim_flow_mark / dtsim_flow / dtsim_flow_masked (k_flow_mark, k_flow_setup, k_flow) against the oracle-side model of
tests/flow_model.py: per pixel the device must lie within the derived tolerance of a CANDIDATE of the model -- on every plane-sure pixel,
with `valid` agreeing, without a cap; everywhere else on all but the case's cap of the pixels (tests/test_flow_model_host.py derives the
tolerances and states the constants read here; profiles/flow_parity.txt lists them).

Each case puts the PREVIOUS state on the device, renders, marks, moves to the current state (dtsim_write of the pose, or steps), renders and
asks for the flow; the object states of both times are read back from the device (frame_parity.obj_states).  The expected maps are the
host's, computed once per process and shared.

Measured on an MI355X: see PARITY.md section 4."""
import ctypes as C
import functools

import numpy as np
import pytest

import depth_model as dm
import flow_model as fm
import frame_parity as fp
import ipm_model as im
from dtsim import BatchedSimulator, _ffi
from test_flow_model_host import tolerances

pytestmark = pytest.mark.gpu
SENTINEL = 7.5


def host(sim, t):
    sim.sync()
    return t.cpu().numpy()


def make_prev(name, kind=None, n=None, period=None, **kw):
    """The PREVIOUS state of the case on the device (env e: state e % len(states), or (e % period) % len(states))."""
    dm_name, motion, moves = fm.CASES[name]
    c = dm.CASES[dm_name]
    n = len(c.states) if n is None else n
    args = dict(camera_width=c.W, camera_height=c.H, distortion=kind == "fisheye", domain_rand=c.dr, seed=1, max_steps=10 ** 6, do_reset=False)
    args.update(kw)
    if c.asset_tree:
        args["asset_root"] = fp.ASSETS
    sim = BatchedSimulator(c.map_name, n, **args)
    states = dm.init_states(c, n, period)
    for st in states:
        x, z, a = fm.prev_pose(float(st.pos[0]), float(st.pos[2]), float(st.angle), motion)
        st.pos[:] = [x, 0.0, z]
        st.angle = a
    sim.reset(states=states)
    if c.wait is not None:
        par = sim.read(_ffi.FIELD_OBJ_PARAMS)
        par[:, :, 1] = c.wait
        sim.write(_ffi.FIELD_OBJ_PARAMS, par)
    if moves:
        sim.step(np.zeros((fm.PED_PREV_STEPS, n, 2), np.float32), n_steps=fm.PED_PREV_STEPS)
    return sim


def to_current(sim, name, period=None):
    """From the previous state to the current one: the rest of the steps, then the pose by dtsim_write."""
    dm_name, motion, moves = fm.CASES[name]
    c = dm.CASES[dm_name]
    n = sim.num_envs
    if moves:
        k = c.steps - fm.PED_PREV_STEPS
        sim.step(np.zeros((k, n, 2), np.float32), n_steps=k)
    if motion != "still":
        cur = dm.init_states(c, n, period)
        sim.write(_ffi.FIELD_POS, np.array([list(st.pos) for st in cur], np.float64))
        sim.write(_ffi.FIELD_ANGLE, np.array([st.angle for st in cur], np.float64))


def objects_of(sim, name, e):
    sc = dm.scene_of(fm.CASES[name][0])
    return fp.obj_states(sim, e, sc) if sc.m.objects else None


def flow_of(sim, h=None, w=None, mask=None):
    """(flow, valid) on the host, from two buffers of the test's own."""
    import torch
    n = sim.num_envs
    h, w = sim.camera_height if h is None else h, sim.camera_width if w is None else w
    valid = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
    flow = sim.flow(h, w, valid_out=valid, mask=mask)
    return host(sim, flow).copy(), host(sim, valid).copy()


@functools.lru_cache(maxsize=None)
def cal_of(kind):
    return im.nominal_cal() if kind == "fisheye" else None


@pytest.mark.parametrize("kind", [None, "fisheye"])
@pytest.mark.parametrize("name", list(fm.CASES))
def test_the_flow_matches_the_model(name, kind):
    """Every case, rectilinear and through the fisheye: planes and per-env cameras moving forward, turning, backing up (points cross the
    previous near plane and image border) and across a tile border; walking duckies seen by a robot that stands or moves; static meshes, at a
    width that is no multiple of four too."""
    c = fm.case_of(name)
    n = len(c.states)
    sim = make_prev(name, kind)
    sim.render()
    sim.flow_mark()
    prev = [objects_of(sim, name, e) for e in range(n)]
    to_current(sim, name)
    sim.render()
    flow, valid = flow_of(sim)
    assert flow.shape == (n, 2, c.H, c.W) and flow.dtype == np.float32 and valid.shape == (n, c.H, c.W)
    depth = host(sim, sim.depth()).copy()
    tp, to, cap = tolerances(name)
    want_valid = []
    for e in range(n):
        cur = objects_of(sim, name, e)
        if cur is not None:                               # the device's objects are the ones the host's depth buffers were made with
            for got, want in zip(cur, dm.host_objects(fm.CASES[name][0])[e]):
                assert np.allclose(got["pos"], want["pos"], rtol=0, atol=1e-9) and abs(got["y_rot"] - want["y_rot"]) <= 1e-7, (name, e)
        exp = fm.expected(name, e, kind, cal_of(kind), None if cur is None else (cur, prev[e]))
        fm.hold(exp, flow[e], valid[e], tp, to, cap, (name, kind, e))
        want_valid.append(float(exp.valid.mean()))
        assert not valid[e][np.isinf(depth[e]) | (depth[e] == 0)].any(), (name, kind, e)         # sky and border pixels are never valid
    # a map, not a blank: as many valid pixels as the model has (the cap's share may differ; through the fisheye of a 90 x 62 camera, whose
    # calibration is a 640 x 480 camera's, a sixth of the pixels), and a flow of pixels
    assert abs(valid.mean() - np.mean(want_valid)) <= cap and np.mean(want_valid) > 0.1 and np.abs(flow).max() > 3.0
    sim.close()


@pytest.mark.parametrize("kind", [None, "fisheye"])
@pytest.mark.parametrize("name,steps", [("planes_dr-rotate", 0), ("pedestrians-still", 0), ("town-forward", 0)])
def test_nothing_moved_gives_exactly_zero(name, steps, kind):
    """The state equals its mark -- per-env cameras; duckies that wait; static meshes --: the flow is 0.0 in every bit and `valid` is
    exactly "a surface with a source": 0 where the depth is +inf or 0, 1 everywhere else."""
    dm_name = fm.CASES[name][0]
    c = dm.CASES[dm_name]
    args = dict(camera_width=c.W, camera_height=c.H, distortion=kind == "fisheye", domain_rand=c.dr, seed=1, max_steps=10 ** 6, do_reset=False)
    if c.asset_tree:
        args["asset_root"] = fp.ASSETS
    sim = BatchedSimulator(c.map_name, len(c.states), **args)
    sim.reset(states=dm.init_states(c))
    sim.render()
    sim.flow_mark()
    sim.render()
    flow, valid = flow_of(sim)
    depth = host(sim, sim.depth())
    assert not flow.any() and flow.tobytes() == np.zeros_like(flow).tobytes()
    assert np.array_equal(valid != 0, np.isfinite(depth) & (depth > 0))
    assert 0.3 < valid.mean() < 1.0
    sim.close()


def test_a_walking_duckie_moves_and_the_static_world_stands_exactly_still():
    """The robot still, the duckies walking: exactly 0 on every pixel no duckie owns, a flow on the duckies'."""
    name = "pedestrians-still"
    sim = make_prev(name)
    sim.render()
    sim.flow_mark()
    to_current(sim, name)
    sim.render()
    flow, valid = flow_of(sim)
    inst = host(sim, sim.instances()).copy()
    dyn = np.zeros(inst.shape, bool)
    sc = dm.scene_of("pedestrians")
    for k, o in enumerate(sc.m.objects):
        if not o.static:
            dyn |= inst == k + 1
    still = np.broadcast_to(~dyn[:, None], flow.shape)
    assert not flow[still].any()
    assert dyn.sum() > 500 and (np.abs(flow).max(axis=1)[dyn] > 0.05).mean() > 0.5
    sim.close()


@pytest.mark.parametrize("name", ["planes_dr-forward", "pedestrians-forward"])
def test_strides_env_positions_and_repeats_give_the_same_bytes(name):
    """N = 130: envs e, e + 64 and e + 128 share a state and a mark -- every position of the env loop, three chunks, the last with two envs;
    a second call and a second render give the same bytes; a strided map is the slice of the full one."""
    N = 130
    sim = make_prev(name, None, N, period=64)
    sim.render()
    sim.flow_mark()
    to_current(sim, name, period=64)
    sim.render()
    flow, valid = flow_of(sim)
    for a in (flow, valid):
        assert a[:64].tobytes() == a[64:128].tobytes() and a[:2].tobytes() == a[128:].tobytes()
    again = flow_of(sim)
    assert again[0].tobytes() == flow.tobytes() and again[1].tobytes() == valid.tobytes()
    for sy, sx in ((2, 2), (4, 8)):
        f, v = flow_of(sim, 120 // sy, 160 // sx)
        assert f.tobytes() == np.ascontiguousarray(dm.strided(flow, sy, sx)).tobytes() and v.tobytes() == np.ascontiguousarray(dm.strided(valid, sy, sx)).tobytes()
    sim.render()
    again = flow_of(sim)
    assert again[0].tobytes() == flow.tobytes() and again[1].tobytes() == valid.tobytes()
    assert np.abs(flow).max() > 3.0
    sim.close()


def test_the_masked_form_and_the_marks():
    """After a masked render only the masked form runs, and it leaves the unselected rows at the sentinel; a masked mark moves only the
    selected envs' marks; no mark, a mark of another episode, and marks dropped by dtsim_set_maps all give zeros."""
    import torch
    from dtsim import batched
    name = "planes-forward"
    c = fm.case_of(name)
    n = len(c.states)
    sim = make_prev(name)
    sim.render()
    f, v = flow_of(sim)
    assert not f.any() and not v.any()                                               # no mark yet
    sel = torch.tensor([1, 0, 1, 0, 0], dtype=torch.uint8, device="cuda")
    s = sel.cpu().numpy() != 0
    sim.flow_mark(mask=sel)                                                          # only envs 0 and 2 have one
    to_current(sim, name)
    sim.render()
    full, fv = flow_of(sim)
    assert not full[~s].any() and not fv[~s].any() and np.abs(full[s]).max() > 3.0 and fv[s].mean() > 0.3
    sim.render(mask=sel)
    out = torch.full((n, 2, c.H, c.W), SENTINEL, dtype=torch.float32, device="cuda")
    val = torch.full((n, c.H, c.W), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        sim.flow(out=out, valid_out=val)                                             # the unmasked form is refused
    sim.flow(out=out, valid_out=val, mask=sel)
    o, vv = host(sim, out), host(sim, val)
    assert (o[~s] == SENTINEL).all() and (vv[~s] == 9).all()
    assert o[s].tobytes() == full[s].tobytes() and vv[s].tobytes() == fv[s].tobytes()
    # another episode (a reset with host states keeps DTSIM_FIELD_EPISODE: the number is moved on by hand, as a device reset moves it)
    sim.write(_ffi.FIELD_EPISODE, sim.read(_ffi.FIELD_EPISODE) + 1)
    sim.render()
    f, v = flow_of(sim)
    assert not f.any() and not v.any()
    sim.flow_mark()
    f, v = flow_of(sim)
    assert not f.any() and v.any()                                                   # marked in this episode: valid, and nothing moved
    # dtsim_set_maps drops the marks
    sc = batched.load_scene(sim.library, sim.map_names, sim.map_datas)
    tarr, marr, farr, keep = batched.scene_ffi(sc)
    _ffi.check(sim._lib, sim._lib.dtsim_set_maps(sim._h, farr, len(sc.maps)))
    sim.reset(states=dm.init_states(c))                                              # (the episode and map numbers the dropped marks carried)
    sim.render()
    f, v = flow_of(sim)
    assert not f.any() and not v.any()
    sim.close()


def test_bad_arguments_and_refused_states_write_nothing():
    import torch
    name = "planes-forward"
    c = fm.case_of(name)
    n = len(c.states)
    sim = make_prev(name)
    lib, h = sim._lib, sim._h
    out = torch.full((n, 2, c.H, c.W), SENTINEL, dtype=torch.float32, device="cuda")
    val = torch.full((n, c.H, c.W), 9, dtype=torch.uint8, device="cuda")
    sel = torch.ones(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ptr, vp, mp = C.c_void_p(out.data_ptr()), C.c_void_p(val.data_ptr()), C.c_void_p(sel.data_ptr())

    def refused(code, full=True):
        if full:
            assert lib.dtsim_flow(h, ptr, vp, c.H, c.W, 0) == code
        assert lib.dtsim_flow_masked(h, ptr, vp, c.H, c.W, 0, mp) == code
        sim.sync()
        assert bool((out == SENTINEL).all()) and bool((val == 9).all())

    refused(_ffi.E_STATE)                                                            # no render yet
    sim.render()
    for args in ((None, ptr, vp, c.H, c.W, 0), (h, None, vp, c.H, c.W, 0), (h, ptr, ptr, c.H, c.W, 0), (h, ptr, vp, 0, c.W, 0), (h, ptr, vp, 7, c.W, 0),
                 (h, ptr, vp, c.H, 33, 0), (h, ptr, vp, c.H, c.W, 1), (h, ptr, vp, c.H, c.W, _ffi.MAP_ENV_TABLES)):
        assert lib.dtsim_flow(*args) == _ffi.E_INVALID, args
        assert lib.dtsim_flow_masked(*args, mp) == _ffi.E_INVALID, args
    assert lib.dtsim_flow_masked(h, ptr, vp, c.H, c.W, 0, None) == _ffi.E_INVALID
    assert lib.dtsim_flow_mark(None, None) == _ffi.E_INVALID
    sim.sync()
    assert bool((out == SENTINEL).all()) and bool((val == 9).all())
    for bad in (dict(height=50), dict(width=81), dict(out=out[:2]), dict(out=out.double()), dict(valid_out=val[:, :60]), dict(mask=sel.cpu())):
        with pytest.raises(ValueError):
            sim.flow(**bad)
    assert lib.dtsim_flow(h, ptr, None, c.H, c.W, 0) == _ffi.OK                      # `valid` is optional
    sim.sync()
    assert bool((val == 9).all()) and bool((out != SENTINEL).all())
    out.fill_(SENTINEL)
    torch.cuda.synchronize()
    sim.step(np.zeros((1, n, 2), np.float32))
    refused(_ffi.E_STATE)                                                            # the cameras describe the state before the step
    sim.render(segment=True)
    refused(_ffi.E_STATE)                                                            # the segment view
    sim.render()
    sim.write(_ffi.FIELD_ANGLE, sim.read(_ffi.FIELD_ANGLE))
    refused(_ffi.E_STATE)                                                            # dtsim_write invalidates
    sim.render(mask=sel)
    assert lib.dtsim_flow(h, ptr, vp, c.H, c.W, 0) == _ffi.E_STATE                   # after a masked pass: the masked form only
    sim.sync()
    assert bool((out == SENTINEL).all())
    sim.close()
    # a fisheye handle without a calibration; then per-env distortion tables
    sim = make_prev(name, "fisheye")
    sim.render()
    _ffi.check(sim._lib, sim._lib.dtsim_set_ipm_calibrations(sim._h, 0, None, None, None, None))
    lib, h = sim._lib, sim._h
    refused(_ffi.E_STATE)
    sim.close()
    sim = BatchedSimulator("small_loop", n, camera_width=c.W, camera_height=c.H, distortion=True, camera_rand=True, domain_rand=False, seed=3)
    sim.render()
    lib, h = sim._lib, sim._h
    refused(_ffi.E_STATE)
    with pytest.raises(ValueError):
        sim.flow()
    sim.close()
