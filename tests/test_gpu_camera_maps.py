"""`-m gpu`: dtsim_camera_maps / dtsim_camera_maps_masked (k_camera_maps) -- depth, labels, instances, flow and flow_valid of one size from
ONE classification of the pixel -- against the single passes of the same handle (dtsim_depth, dtsim_labels, dtsim_instances, dtsim_flow),
byte for byte in every case -- they all test a triangle by the pass's own box stream --, and against the oracle models of those passes after a
second render from another pose with mesh objects in view (tests/test_gpu_rerender_maps.py holds re-rendered handles to fresh ones).

The cases, cameras and batch sizes are the models' (tests/depth_model.py, label_model.py, instance_model.py, flow_model.py,
camera_rand_maps_model.py); tolerances and caps are read where tests/test_gpu_depth.py, test_gpu_labels.py and test_gpu_instances.py read
them.  The "parity" lines this file prints are the record of profiles/camera_maps_parity.txt."""
import ctypes as C

import numpy as np
import pytest

import camera_rand_maps_model as cm
import depth_model as dm
import flow_model as fm
import instance_model as im
import label_model as lm
from dtsim import BatchedSimulator, _ffi
from test_gpu_depth import TOL, want_full
from test_gpu_flow import make_prev, objects_of, to_current
from test_gpu_labels import fisheye_kw, make_sim

pytestmark = pytest.mark.gpu
NAMES = ("depth", "labels", "instances", "flow", "flow_valid")
SENTINEL = dict(depth=7.5, labels=99, instances=99, flow=7.5, flow_valid=9)


def fresh(sim, h, w, names=NAMES, depth_dtype="float32"):
    """Device tensors of the outputs `names`, each holding its sentinel, ready before the handle's stream writes."""
    import torch
    n = sim.num_envs
    spec = dict(depth=((n, h, w), getattr(torch, depth_dtype)), labels=((n, h, w), torch.uint8), instances=((n, h, w), torch.uint8),
                flow=((n, 2, h, w), torch.float32), flow_valid=((n, h, w), torch.uint8))
    out = {k: torch.full(spec[k][0], SENTINEL[k], dtype=spec[k][1], device="cuda") for k in names}
    torch.cuda.synchronize()
    return out


def host(sim, bufs):
    sim.sync()
    return {k: t.cpu().numpy().copy() for k, t in bufs.items()}


def single(sim, h, w, names=NAMES, depth_dtype="float32", mask=None):
    """The outputs `names` by the single passes of the handle, each into a sentinel-filled tensor of the test's own."""
    b = fresh(sim, h, w, names, depth_dtype)
    if "depth" in b:
        sim.depth(h, w, dtype=depth_dtype, out=b["depth"], mask=mask)
    if "labels" in b:
        sim.labels(h, w, out=b["labels"], mask=mask)
    if "instances" in b:
        sim.instances(h, w, out=b["instances"], mask=mask)
    if "flow" in b:
        sim.flow(h, w, out=b["flow"], mask=mask, valid_out=b.get("flow_valid"))
    return host(sim, b)


def fused(sim, h, w, names=NAMES, depth_dtype="float32", mask=None, bufs=None):
    """The outputs `names` by ONE camera_maps call, each into a sentinel-filled tensor of the test's own."""
    b = fresh(sim, h, w, names, depth_dtype) if bufs is None else bufs
    res = sim.camera_maps(h, w, depth_dtype=depth_dtype, mask=mask, **b)
    assert set(res) == set(b) and all(res[k] is b[k] for k in b)
    return host(sim, b)


def same(got, want, ctx, names=None):
    for k in (names or want):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (ctx, k)
        assert got[k].tobytes() == want[k].tobytes(), (ctx, k, int((got[k] != want[k]).sum()))


def has_objects(name):
    return bool(lm.scene_of(name).m.objects)


# ---- 1. one render, a fresh handle -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", [None, "fisheye"])
@pytest.mark.parametrize("name", list(lm.CASES))
def test_one_render_every_output_is_its_single_passes_bytes(name, kind):
    """Every case of label_model.CASES, rectilinear and through the fisheye: render, mark, all five outputs from one call -- each byte for byte
    its single pass's on the same handle, the flow of the unmoved state exactly 0 with dtsim_flow's flags; then three subsets (depth alone
    in float16; labels + instances; flow + valid), held to the same bytes."""
    c = lm.CASES[name]
    sim = make_sim(name, **fisheye_kw(kind))
    sim.render()
    sim.flow_mark()
    want = single(sim, c.H, c.W)
    got = fused(sim, c.H, c.W)
    same(got, want, (name, kind))
    assert not got["flow"].any() and got["flow"].tobytes() == np.zeros_like(got["flow"]).tobytes()
    assert np.array_equal(got["flow_valid"] != 0, np.isfinite(got["depth"]) & (got["depth"] > 0)) and got["flow_valid"].mean() > 0.1
    assert (got["labels"] != SENTINEL["labels"]).all() and (got["depth"] != SENTINEL["depth"]).all()
    half = single(sim, c.H, c.W, ("depth",), "float16")
    same(fused(sim, c.H, c.W, ("depth",), "float16"), half, (name, kind, "f16"))
    assert half["depth"].dtype == np.float16
    same(fused(sim, c.H, c.W, ("labels", "instances")), want, (name, kind, "labels + instances"), ("labels", "instances"))
    same(fused(sim, c.H, c.W, ("flow", "flow_valid")), want, (name, kind, "flow + valid"), ("flow", "flow_valid"))
    same(fused(sim, c.H, c.W, ("flow",)), want, (name, kind, "flow alone"), ("flow",))
    own = sim.camera_maps(depth=True, labels=True, instances=True, flow=True, flow_valid=True)      # the handle's own tensors
    same(host(sim, own), want, (name, kind, "own"))
    sim.close()


# ---- 2. two renders ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", [None, "fisheye"])
@pytest.mark.parametrize("name", list(fm.CASES))
def test_two_renders_flow_is_dtsim_flows_and_the_maps_hold(name, kind):
    """Every case of flow_model.CASES, as tests/test_gpu_flow.py runs it: every output is its single pass's bytes on every case -- all of them
    test a triangle by the second render's own box stream, so none sees a culled triangle's record of the first render
    (tests/test_gpu_rerender_maps.py) --, and with mesh objects depth, labels and instances are moreover held to the oracle models of the
    CURRENT state.  The printed line is the record of profiles/camera_maps_parity.txt."""
    dm_name = fm.CASES[name][0]
    c = fm.case_of(name)
    n = len(c.states)
    sim = make_prev(name, kind)
    sim.render()
    sim.flow_mark()
    to_current(sim, name)
    sim.render()
    want = single(sim, c.H, c.W)
    got = fused(sim, c.H, c.W)
    assert np.abs(got["flow"]).max() > 3.0 and got["flow_valid"].mean() > 0.1
    diff = {k: int((got[k] != want[k]).sum()) for k in ("depth", "labels", "instances")}
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.abs(1.0 / got["depth"].astype(np.float64) - 1.0 / want["depth"].astype(np.float64))
    inv = inv[np.isfinite(inv)]
    print(f"parity {name} {kind}: {n} x {c.H} x {c.W} px; differing from the single passes: depth {diff['depth']}, labels {diff['labels']}, "
          f"instances {diff['instances']}; largest |d(1/depth)| {inv.max() if inv.size else 0.0:.3e}")
    same(got, want, (name, kind))
    if has_objects(dm_name):
        for e in range(n):
            for g, w in zip(objects_of(sim, name, e), dm.host_objects(dm_name)[e]):     # the device holds the state the models were made from
                assert np.allclose(g["pos"], w["pos"], rtol=0, atol=1e-9) and abs(g["y_rot"] - w["y_rot"]) <= 1e-7, (name, e)
            dm.compare(got["depth"][e], want_full(dm_name, e, kind), TOL, c.cap, (name, kind, e, "depth"))
            wl, sl = lm.expected(dm_name, e, kind)
            lm.compare(got["labels"][e], wl, sl, lm.CASES[dm_name].cap, (name, kind, e, "labels"))
            wi, si = im.expected(dm_name, e, kind)
            im.compare(got["instances"][e], wi, si, im.CASES[dm_name].cap, (name, kind, e, "instances"))
        # one classification: where an object owns the pixel the label is its mesh's class, the depth finite, and nowhere else
        oc = sim.object_classes()[0]
        inst, lab = got["instances"], got["labels"]
        assert np.array_equal(lab[inst > 0], oc[inst[inst > 0].astype(np.int64) - 1])
        assert np.isfinite(got["depth"][inst > 0]).all() and (got["depth"][inst > 0] > 0).all()
    sim.close()


# ---- 3. one state, one result --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["planes_dr-forward", "pedestrians-forward"])
def test_env_positions_the_tail_chunk_and_repeats_give_the_same_bytes(name):
    """N = 130: envs e, e + 64 and e + 128 share a state and a mark -- every position of the env loop, three chunks, the last with two envs; a
    second call and a second render give the same bytes; a strided map is the slice of the full one."""
    N = 130
    sim = make_prev(name, None, N, period=64)
    sim.render()
    sim.flow_mark()
    to_current(sim, name, period=64)
    sim.render()
    got = fused(sim, 120, 160)
    for k, a in got.items():
        assert a[:64].tobytes() == a[64:128].tobytes() and a[:2].tobytes() == a[128:].tobytes(), (name, k)
    same(fused(sim, 120, 160), got, (name, "second call"))
    for sy, sx in ((2, 2), (4, 8)):
        small = fused(sim, 120 // sy, 160 // sx)
        for k in NAMES:
            assert small[k].tobytes() == np.ascontiguousarray(dm.strided(got[k], sy, sx)).tobytes(), (name, k, sy, sx)
    sim.render()
    same(fused(sim, 120, 160), got, (name, "second render"))
    assert np.abs(got["flow"]).max() > 3.0
    sim.close()


# ---- 4. the masked form ----------------------------------------------------------------------------------------------------------------------------

def test_the_masked_form_writes_the_selected_rows_only():
    import torch
    name = "pedestrians-forward"
    c = fm.case_of(name)
    sim = make_prev(name)
    n = sim.num_envs
    sim.render()
    sim.flow_mark()
    to_current(sim, name)
    sim.render()
    full = fused(sim, c.H, c.W)
    sel = torch.tensor([(e % 3) != 1 for e in range(n)], dtype=torch.uint8, device="cuda")
    s = sel.cpu().numpy() != 0
    assert s.any() and not s.all()
    sim.render(mask=sel)
    b = fresh(sim, c.H, c.W)
    with pytest.raises(RuntimeError):
        sim.camera_maps(c.H, c.W, **b)                                               # after a masked pass: the masked form only
    for k, a in host(sim, b).items():
        assert (a == SENTINEL[k]).all(), k
    got = fused(sim, c.H, c.W, mask=sel, bufs=b)
    for k in NAMES:
        assert (got[k][~s] == SENTINEL[k]).all() and got[k][s].tobytes() == full[k][s].tobytes(), k
    sim.close()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------------------

def test_bad_arguments_and_refused_states_write_nothing():
    import torch
    name = "planes-forward"
    c = fm.case_of(name)
    sim = make_prev(name)
    n = sim.num_envs
    lib, h = sim._lib, sim._h
    b = fresh(sim, c.H, c.W)
    sel = torch.ones(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    mp = C.c_void_p(sel.data_ptr())

    def arg(names=NAMES, **other):
        a = _ffi.CameraMapsOut()
        for k in names:
            setattr(a, k, b[k].data_ptr())
        for k, v in other.items():
            setattr(a, k, v)
        return a

    def untouched():
        for k, a in host(sim, b).items():
            assert (a == SENTINEL[k]).all(), k

    def refused(code, a=None, flags=0, full=True):
        a = arg() if a is None else a
        if full:
            assert lib.dtsim_camera_maps(h, C.byref(a), c.H, c.W, flags) == code
        assert lib.dtsim_camera_maps_masked(h, C.byref(a), c.H, c.W, flags, mp) == code
        untouched()

    sim._need_label_assets()
    sim.flow_mark()
    refused(_ffi.E_STATE)                                                            # no render yet
    sim.render()
    for a, hh, ww, fl in ((arg(()), c.H, c.W, 0), (arg(("depth", "flow_valid")), c.H, c.W, 0),        # no output; flow_valid without flow
                          (arg(labels=b["instances"].data_ptr()), c.H, c.W, 0),                        # labels and instances one buffer
                          (arg(depth=b["flow"].data_ptr() + 4 * n * c.H * c.W), c.H, c.W, 0),            # depth inside flow's second plane
                          (arg(flow_valid=b["labels"].data_ptr() + c.H * c.W), c.H, c.W, 0),            # valid across two rows of labels
                          (arg(), 0, c.W, 0), (arg(), 7, c.W, 0), (arg(), c.H, 33, 0), (arg(), c.H, c.W, 2), (arg(), c.H, c.W, 0x200)):
        assert lib.dtsim_camera_maps(h, C.byref(a), hh, ww, fl) == _ffi.E_INVALID
        assert lib.dtsim_camera_maps_masked(h, C.byref(a), hh, ww, fl, mp) == _ffi.E_INVALID
    assert lib.dtsim_camera_maps(None, C.byref(arg()), c.H, c.W, 0) == _ffi.E_INVALID
    assert lib.dtsim_camera_maps(h, None, c.H, c.W, 0) == _ffi.E_INVALID
    assert lib.dtsim_camera_maps_masked(h, C.byref(arg()), c.H, c.W, 0, None) == _ffi.E_INVALID
    untouched()
    for bad in (dict(), dict(flow_valid=b["flow_valid"]), dict(height=50, depth=True), dict(depth=b["depth"][:2]), dict(depth=b["depth"].double()),
                dict(depth=True, depth_dtype="float64"), dict(labels=b["labels"], instances=b["labels"]), dict(depth=True, mask=sel.cpu())):
        with pytest.raises(ValueError):
            sim.camera_maps(**bad)
    untouched()
    assert lib.dtsim_camera_maps(h, C.byref(arg()), c.H, c.W, 0) == _ffi.OK           # (the state is good: everything is written)
    for k, a in host(sim, b).items():
        assert (a != SENTINEL[k]).all(), k
    for k, t in b.items():
        t.fill_(SENTINEL[k])
    torch.cuda.synchronize()
    sim.step(np.zeros((1, n, 2), np.float32))
    refused(_ffi.E_STATE)                                                            # the cameras describe the state before the step
    sim.render(segment=True)
    refused(_ffi.E_STATE)                                                            # the segment view
    sim.render()
    sim.write(_ffi.FIELD_ANGLE, sim.read(_ffi.FIELD_ANGLE))
    refused(_ffi.E_STATE)                                                            # an invalidating call in between
    sim.render(mask=sel)
    assert lib.dtsim_camera_maps(h, C.byref(arg()), c.H, c.W, 0) == _ffi.E_STATE      # after a masked pass: the masked form only
    untouched()
    sim.close()
    # a fresh handle: no label tables with labels on, no mark with flow on -- and without them the other outputs are served
    sim = make_prev(name)
    lib, h = sim._lib, sim._h
    sim.render()
    refused(_ffi.E_STATE, arg(("depth", "labels")))
    refused(_ffi.E_STATE, arg(("depth", "flow", "flow_valid")))
    assert lib.dtsim_camera_maps(h, C.byref(arg(("depth", "instances"))), c.H, c.W, 0) == _ffi.OK
    sim.sync()
    assert bool((b["depth"] != SENTINEL["depth"]).all()) and bool((b["labels"] == SENTINEL["labels"]).all())
    b["depth"].fill_(SENTINEL["depth"]); b["instances"].fill_(SENTINEL["instances"])
    torch.cuda.synchronize()
    sim.close()
    # a fisheye handle without a calibration, flow on
    sim = make_prev(name, "fisheye")
    sim.render()
    sim.flow_mark()
    _ffi.check(sim._lib, sim._lib.dtsim_set_ipm_calibrations(sim._h, 0, None, None, None, None))
    lib, h = sim._lib, sim._h
    refused(_ffi.E_STATE, arg(("depth", "flow")))
    sim.close()
    # per-env distortion tables: refused without the flag; with flow refused with it too
    sim = BatchedSimulator("small_loop", n, camera_width=c.W, camera_height=c.H, distortion=True, camera_rand=True, domain_rand=False, seed=3)
    sim.render()
    sim.flow_mark()
    lib, h = sim._lib, sim._h
    refused(_ffi.E_STATE, arg(("depth", "instances")))
    refused(_ffi.E_STATE, arg(("depth", "flow", "flow_valid")))
    refused(_ffi.E_STATE, arg(("depth", "flow", "flow_valid")), flags=_ffi.MAP_ENV_TABLES)
    with pytest.raises(ValueError):
        sim.camera_maps(flow=True)
    untouched()
    assert lib.dtsim_camera_maps(h, C.byref(arg(("depth", "instances"))), c.H, c.W, _ffi.MAP_ENV_TABLES) == _ffi.OK
    sim.sync()
    sim.close()


# ---- 6. per-env tables -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["planes_dr", "pedestrians", "town"])
def test_per_env_tables_give_the_single_passes_bytes(name):
    """The six-table set-up of tests/test_gpu_camera_rand_maps.py (N = 72: a full chunk and a tail of 8, env e through table (e + e // 64) % 6):
    depth, labels and instances of one call are the single passes' bytes, each with DTSIM_MAP_ENV_TABLES; float16 and a strided size too."""
    sim = cm.make_sim(name)
    cm.install(sim)
    assert sim._env_tables_flag() == _ffi.MAP_ENV_TABLES
    sim.render()
    three = ("depth", "labels", "instances")
    want = single(sim, cm.H, cm.W, three)
    got = fused(sim, cm.H, cm.W, three)
    same(got, want, name)
    assert any(got["depth"][e].tobytes() != got["depth"][e + 64].tobytes() for e in range(cm.N - 64))      # the tables took effect
    same(fused(sim, cm.H // 2, cm.W // 2, ("depth", "instances"), "float16"), single(sim, cm.H // 2, cm.W // 2, ("depth", "instances"), "float16"),
         (name, "f16, strided"))
    with pytest.raises(ValueError):
        sim.camera_maps(depth=True, flow=True)
    sim.close()


# ---- the profiling slot ------------------------------------------------------------------------------------------------------------------------------

def test_the_kernel_has_its_own_profiling_slot():
    """DTSIM_KERNEL_CAMERA_MAPS counts the k_camera_maps launches of a handle created with DTSIM_F_PROFILE, and only them."""
    c = lm.CASES["planes"]
    sim = make_sim("planes", profile=True)
    sim.render()
    sim.flow_mark()
    assert sim.profile_read(_ffi.KERNEL_CAMERA_MAPS)[0] == 0
    fused(sim, c.H, c.W)
    fused(sim, c.H // 2, c.W // 2, ("depth",))
    single(sim, c.H, c.W)
    n, ms = sim.profile_read(_ffi.KERNEL_CAMERA_MAPS)
    assert n == 2 and ms > 0.0
    assert sim.profile_read(_ffi.KERNEL_CAMERA_MAPS)[0] == 0
    sim.close()
