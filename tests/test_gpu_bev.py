"""`-m gpu`: dtsim_bev (k_bev) against the model of tests/bev_model.py -- the egocentric bird's-eye class and id maps of N = 130 envs (two
full chunks of 64 and a tail of 2) on handles with a 32 x 24 camera that never render, except in the one test that proves a render changes
nothing.  On the model's SURE cells (one candidate within M = 1e-4 m of the cell's point) the class and the id are EQUAL to the model's; on
every other cell they are a member of the cell's candidate set: no capped share, a wrong class anywhere fails at one cell.  The model takes
the rectangles from object_footprints(), which each case first holds to the oracle's own physics (tests/bev_model.py host_footprints).

Measured on an MI355X: profiles/bev_parity.txt."""
import ctypes as C
import math

import numpy as np
import pytest

import bev_model as bm
import crowd_scenes as cs
import depth_model as dm
import frame_parity as fp
import label_model as lm
import multimap_scenes as ms
from dtsim import BatchedSimulator, _ffi, assets, labels as L
from oracle import sim as osim

pytestmark = pytest.mark.gpu
N = bm.N
SENTINEL = 99                                                # no default class, no id in use
CAM = dict(camera_width=32, camera_height=24)


@pytest.fixture(scope="module", autouse=True)
def own_maps():
    """The crowd map and multimap_scenes' own maps as fixtures of the asset library, so that a simulator can hold them by name."""
    added = {"crowd": cs.crowd_map(), **{n: ms.map_data(n) for n in ms.OWN_MAPS}}
    before = {n: assets.MAPS.get(n) for n in added}
    assets.MAPS.update(added)
    yield
    for n, v in before.items():
        if v is None:
            assets.MAPS.pop(n, None)
        else:
            assets.MAPS[n] = v


def init_states(case, n):
    out = (_ffi.InitState * n)()
    for e in range(n):
        st = out[e]
        st.pos[:] = [bm.START[0], 0.0, bm.START[1]]
        st.angle, st.map_id, st.wheel_dist = bm.START[2], bm.map_of(case, e), osim.WHEEL_DIST
        st.cam_height, st.cam_angle_deg, st.cam_fov_y_deg = osim.CAMERA_FLOOR_DIST, osim.CAMERA_ANGLE, float(osim.CAMERA_FOV_Y)
        st.horizon_color[:] = list(dm.BLUE_SKY); st.ground_color[:] = [0.15, 0.15, 0.15]
        st.light_pos[:] = [0.0, 3.0, 0.0, 1.0]; st.light_ambient[:] = [0.25] * 3; st.light_diffuse[:] = [0.35] * 3
    return out


def make_sim(name, n=N, **kw):
    """The case on the device: every env stands at START while the case's zero-action steps run, then takes its pose through dtsim_write."""
    case = bm.CASES[name]
    args = dict(CAM, distortion=False, domain_rand=False, seed=1, max_steps=10 ** 6, do_reset=False)
    args.update(kw)
    if case.asset_tree:
        args["asset_root"] = fp.ASSETS
    sim = BatchedSimulator(list(case.maps) if len(case.maps) > 1 else case.maps[0], n, **args)
    sim.reset(states=init_states(case, n))
    if case.wait is not None:
        par = sim.read(_ffi.FIELD_OBJ_PARAMS)
        par[:, :, 1] = case.wait
        sim.write(_ffi.FIELD_OBJ_PARAMS, par)
    if case.steps:
        sim.step(np.zeros((case.steps, n, 2), np.float32), n_steps=case.steps)
    if case.hidden:
        vis = sim.read(_ffi.FIELD_OBJ_VISIBLE)
        vis[:, list(case.hidden)] = 0
        sim.write(_ffi.FIELD_OBJ_VISIBLE, vis)
    pos, ang = sim.read(_ffi.FIELD_POS), sim.read(_ffi.FIELD_ANGLE)
    for e in range(n):
        x, z, a = bm.pose_of(case, e)
        pos[e], ang[e] = (x, 0.0, z), a
    sim.write(_ffi.FIELD_POS, pos)
    sim.write(_ffi.FIELD_ANGLE, ang)
    return sim


_SIMS = {}


@pytest.fixture(scope="module")
def sims():
    """One simulator per case, made at first use and shared by the tests that leave its state and tables alone."""
    def get(name):
        if name not in _SIMS:
            sim = make_sim(name)
            _SIMS[name] = (sim, check_state(sim, name))
        return _SIMS[name]
    yield get
    for sim, _ in _SIMS.values():
        sim.close()
    _SIMS.clear()


def check_state(sim, name):
    """The device holds what the model is computed from: the written poses, the default tables of the host, and footprints that are the
    oracle's (the static ones the map's, the walkers' after the case's steps).  Returns (corners, drawn) per resident map."""
    case = bm.CASES[name]
    pos, ang, mid = sim.read(_ffi.FIELD_POS), sim.read(_ffi.FIELD_ANGLE), sim.read(_ffi.FIELD_MAP_ID)
    for e in range(N):
        x, z, a = bm.pose_of(case, e)
        assert (pos[e, 0], pos[e, 2], ang[e], mid[e]) == (x, z, a, bm.map_of(case, e)), (name, e)
    corners, drawn = sim.object_footprints()
    assert corners.shape == (N, _ffi.MAX_OBJECTS, 4, 2) and corners.dtype == np.float64 and drawn.shape == (N, _ffi.MAX_OBJECTS) and drawn.dtype == bool
    texel, mesh = sim.label_assets()
    out = []
    for mi, mname in enumerate(case.maps):
        mm = bm.map_model(mname)
        want_c, want_d = bm.host_footprints(name)[mi]
        k = len(want_c)
        for e in range(mi, N, len(case.maps)):
            assert np.allclose(corners[e, :k], want_c, rtol=0, atol=1e-9), (name, e, float(np.abs(corners[e, :k] - want_c).max()))
            assert np.array_equal(drawn[e, :k], want_d) and not drawn[e, k:].any() and not corners[e, k:].any(), (name, e)
            assert corners[e].tobytes() == corners[mi].tobytes()              # envs of one map went through one history
        for kd, t in mm.tiles.items():
            assert texel[sim.texture_kinds.index(kd)].tobytes() == t.tobytes(), (name, kd)
        per_obj = [int(mesh[sim._mesh_order.index(o.mesh_kind)]) for o in sim.maps[mi].objects]
        assert per_obj == [int(v) for v in mm.obj_cls], (name, mname)
        out.append((corners[mi, :k].copy(), drawn[mi, :k].copy()))
    return out


def host(sim, t):
    sim.sync()
    return t.cpu().numpy()


def filled(shape, value=SENTINEL):
    import torch
    out = torch.full(shape, value, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return out


def model_of(name, foot, e, shape, cache, tables=None):
    case = bm.CASES[name]
    k, mi = (e % 64) % len(case.poses), bm.map_of(case, e)
    if (k, mi) not in cache:
        cache[k, mi] = bm.expected(bm.map_model(case.maps[mi]), case.poses[k], *foot[mi], shape, tables=None if tables is None else tables[mi])
    return cache[k, mi]


def hold_to_model(name, foot, cls, inst, shape, tables=None):
    """Every env's maps against the model; returns dict(differ, fell_back, sure_cls, sure_id, cells)."""
    case = bm.CASES[name]
    cache, tot = {}, dict(differ=0, fell_back=0, cells=0, sure_cls=0, sure_id=0)
    hidden = {h + 1 for h in case.hidden}
    for e in range(N):
        want = model_of(name, foot, e, shape, cache, tables)
        r = bm.compare(None if cls is None else cls[e], None if inst is None else inst[e], want, (name, shape, e))
        tot["differ"] += r["differ"]; tot["fell_back"] += r["fell_back"]
        tot["cells"] += want.cls.size; tot["sure_cls"] += int(want.sure_cls.sum()); tot["sure_id"] += int(want.sure_id.sum())
        if inst is not None:
            seen = set(np.unique(inst[e]).tolist())
            assert not seen & hidden, (name, shape, e, "a hidden object's id", seen & hidden)
            must = set(np.unique(want.inst[want.sure_id]).tolist()) - {0}     # every drawn object that covers a sure cell appears
            assert must <= seen, (name, shape, e, must - seen)
    return tot


# ---- the maps against the model ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", bm.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}@{s[2]}b{s[3]}")
@pytest.mark.parametrize("name", list(bm.CASES))
def test_bev_matches_the_model(sims, name, shape):
    """Planes only, walked duckies, the asset-tree town, the 64-object crowd with every third object hidden, two resident maps of different
    tile sizes and object lists alternating per slot -- at every shape: 64 x 64, 37 x 53 (no multiple of four), one cell, the agent inside a
    128 x 96 window, the whole window behind it.  No render() has run on these handles."""
    sim, foot = sims(name)
    oh, ow, cell, rb = shape
    inst_t = filled((N, oh, ow))
    cls = host(sim, sim.bev(oh, ow, cell=cell, rows_behind=rb, instances_out=inst_t)).copy()
    inst = host(sim, inst_t)
    assert cls.shape == (N, oh, ow) and cls.dtype == np.uint8
    tot = hold_to_model(name, foot, cls, inst, shape)
    print(f"bev {name:17s} {oh:3d} x {ow:3d} cell {cell:.3f} behind {rb:3d}: cells {tot['cells']} sure class {tot['sure_cls'] / tot['cells']:.4f} "
          f"sure id {tot['sure_id'] / tot['cells']:.4f} differed {tot['differ']} fell back on the candidate set {tot['fell_back']}")
    # the class-only and the id-only launch give the same bytes per map, and so does a second call
    only_cls = host(sim, sim.bev(oh, ow, cell=cell, rows_behind=rb, out=filled((N, oh, ow))))
    assert only_cls.tobytes() == cls.tobytes()
    only_inst = filled((N, oh, ow))
    _ffi.check(sim._lib, sim._lib.dtsim_bev(sim._h, None, C.c_void_p(only_inst.data_ptr()), oh, ow, cell, rb, 0, None))
    assert host(sim, only_inst).tobytes() == inst.tobytes()
    again_i = filled((N, oh, ow))
    assert host(sim, sim.bev(oh, ow, cell=cell, rows_behind=rb, instances_out=again_i)).tobytes() == cls.tobytes() and host(sim, again_i).tobytes() == inst.tobytes()
    # envs e, e + 64 and e + 128 hold one state (the tail chunk's two envs included): the same bytes
    assert cls[:64].tobytes() == cls[64:128].tobytes() and cls[:2].tobytes() == cls[128:].tobytes()
    assert inst[:64].tobytes() == inst[64:128].tobytes() and inst[:2].tobytes() == inst[128:].tobytes()


def test_a_render_changes_nothing_and_none_is_needed():
    """A fresh handle: the map before any render(), after a render() and after a masked one -- the same bytes."""
    import torch
    sim = make_sim("loop_pedestrians")
    shape = bm.SHAPES[0]
    oh, ow, cell, rb = shape
    i0 = filled((N, oh, ow))
    c0 = host(sim, sim.bev(oh, ow, cell=cell, rows_behind=rb, instances_out=i0)).copy()
    i0 = host(sim, i0)
    hold_to_model("loop_pedestrians", check_state(sim, "loop_pedestrians"), c0, i0, shape)
    sim.render()
    i1 = filled((N, oh, ow))
    assert host(sim, sim.bev(oh, ow, cell=cell, rows_behind=rb, instances_out=i1)).tobytes() == c0.tobytes() and host(sim, i1).tobytes() == i0.tobytes()
    m = (torch.arange(N, device="cuda") % 3 == 0).to(torch.uint8)
    sim.render(mask=m)
    assert host(sim, sim.bev(oh, ow, cell=cell, rows_behind=rb)).tobytes() == c0.tobytes()
    sim.close()


def test_a_masked_call_leaves_the_other_rows(sims):
    import torch
    sim, _ = sims("crowd")
    oh, ow, cell, rb = bm.SHAPES[1]
    fi = filled((N, oh, ow))
    full = host(sim, sim.bev(oh, ow, cell=cell, rows_behind=rb, instances_out=fi)).copy()
    fi = host(sim, fi)
    for mask in ((torch.arange(N, device="cuda") % 3 == 1), torch.zeros(N, dtype=torch.uint8, device="cuda"),
                 (torch.arange(N, device="cuda") >= 127).to(torch.uint8)):
        out, oi = filled((N, oh, ow)), filled((N, oh, ow), 77)
        torch.cuda.synchronize()
        sim.bev(oh, ow, cell=cell, rows_behind=rb, out=out, instances_out=oi, mask=mask)
        out, oi, sel = host(sim, out), host(sim, oi), mask.cpu().numpy().astype(bool)
        assert out[sel].tobytes() == full[sel].tobytes() and oi[sel].tobytes() == fi[sel].tobytes()
        assert (out[~sel] == SENTINEL).all() and (oi[~sel] == 77).all()


def test_a_user_table_changes_exactly_its_cells():
    """set_label_assets with one tile texture -> 200 and one mesh -> 201: the cells on that texture's tiles and under that mesh's objects, no other."""
    sim = make_sim("loop_pedestrians")
    foot = check_state(sim, "loop_pedestrians")
    shape = bm.SHAPES[0]
    oh, ow, cell, rb = shape
    i0 = filled((N, oh, ow))
    c0 = host(sim, sim.bev(oh, ow, cell=cell, rows_behind=rb, instances_out=i0)).copy()
    i0 = host(sim, i0)
    texel, mesh = sim.label_assets()
    kind, mkey = "straight", "duckie"
    texel[sim.texture_kinds.index(kind)] = np.full_like(texel[sim.texture_kinds.index(kind)], 200)
    mesh = mesh.copy(); mesh[sim._mesh_order.index(mkey)] = 201
    sim.set_label_assets(texel, mesh)
    i1 = filled((N, oh, ow))
    c1 = host(sim, sim.bev(oh, ow, cell=cell, rows_behind=rb, instances_out=i1)).copy()
    i1 = host(sim, i1)
    assert i1.tobytes() == i0.tobytes()                                  # the ids know no table
    changed = c1 != c0
    assert np.array_equal(changed, (c1 == 200) | (c1 == 201)) and (c1 == 200).sum() > 1000 and (c1 == 201).sum() > 20
    mm = bm.map_model("loop_pedestrians")
    duckie = mm.obj_cls == L.CLASS_IDS["duckie"]
    assert duckie.any() and np.array_equal(c1 == 201, np.isin(i1, np.nonzero(duckie)[0] + 1))      # under the duckies, nowhere else
    tiles = dict(mm.tiles); tiles[kind] = np.full_like(tiles[kind], 200)
    hold_to_model("loop_pedestrians", foot, c1, i1, shape, tables=[(tiles, np.where(duckie, 201, mm.obj_cls))])
    sim.close()


def test_bad_arguments_raise_before_a_launch_and_leave_the_last_result(sims):
    import torch
    sim, _ = sims("small_loop")
    good = sim.bev(16, 24, cell=0.02, rows_behind=16)
    keep = host(sim, good).copy()
    other = torch.zeros((N, 16, 24), dtype=torch.uint8, device="cuda")
    for kw in (dict(height=0), dict(height=1025), dict(width=0), dict(width=1025), dict(height=16.5), dict(cell=0.0), dict(cell=-0.02),
               dict(cell=float("nan")), dict(cell=float("inf")), dict(cell="a"), dict(rows_behind=-1), dict(rows_behind=17), dict(rows_behind=0.5),
               dict(out=torch.zeros((N, 16, 25), dtype=torch.uint8, device="cuda")), dict(out=torch.zeros((N, 16, 24), dtype=torch.int8, device="cuda")),
               dict(out=np.zeros((N, 16, 24), np.uint8)), dict(instances_out=torch.zeros((N, 24, 16), dtype=torch.uint8, device="cuda")),
               dict(out=other, instances_out=other), dict(mask=torch.ones(N - 1, dtype=torch.uint8, device="cuda")),
               dict(mask=np.ones(N, np.uint8)), dict(mask=torch.ones(N, dtype=torch.float32, device="cuda"))):
        args = dict(height=16, width=24, cell=0.02, rows_behind=16)
        args.update(kw)
        with pytest.raises(ValueError):
            sim.bev(**args)
    # what the wrapper cannot send: the library's own refusals, DTSIM_E_INVALID with a text, before any launch
    p, q, lib = C.c_void_p(good.data_ptr()), C.c_void_p(other.data_ptr()), sim._lib
    for args in ((p, q, 16, 24, 0.02, 16, 1, None), (None, None, 16, 24, 0.02, 16, 0, None), (p, p, 16, 24, 0.02, 16, 0, None),
                 (p, q, 0, 24, 0.02, 0, 0, None), (p, q, 16, 1025, 0.02, 16, 0, None), (p, q, 16, 24, float("nan"), 16, 0, None),
                 (p, q, 16, 24, -1.0, 16, 0, None), (p, q, 16, 24, 0.02, 17, 0, None), (p, q, 16, 24, 0.02, -1, 0, None)):
        assert lib.dtsim_bev(sim._h, *args) == _ffi.E_INVALID and b"dtsim_bev" in lib.dtsim_last_error(), args
    assert host(sim, good).tobytes() == keep.tobytes() and not host(sim, other).any()
    # a handle without render tables, and a class map before any label table
    bare = BatchedSimulator("small_loop", 2, render=False, seed=1)
    with pytest.raises(ValueError):
        bare.bev(4, 4)
    small = torch.zeros((2, 4, 4), dtype=torch.uint8, device="cuda")
    assert bare._lib.dtsim_bev(bare._h, C.c_void_p(small.data_ptr()), None, 4, 4, 0.02, 0, 0, None) == _ffi.E_INVALID
    bare.close()
    fresh = BatchedSimulator("small_loop", 2, seed=1, **CAM)
    assert fresh._lib.dtsim_bev(fresh._h, C.c_void_p(small.data_ptr()), None, 4, 4, 0.02, 0, 0, None) == _ffi.E_INVALID     # no label tables yet
    assert b"dtsim_set_label_assets" in fresh._lib.dtsim_last_error()
    ids = torch.full((2, 4, 4), SENTINEL, dtype=torch.uint8, device="cuda")
    assert fresh._lib.dtsim_bev(fresh._h, None, C.c_void_p(ids.data_ptr()), 4, 4, 0.02, 0, 0, None) == _ffi.OK                # the ids need none
    assert not host(fresh, ids).any() and not host(fresh, small).any()
    fresh.close()


def test_the_camera_labels_and_the_bev_name_one_class_at_one_world_point():
    """One render of the marking close-ups of the town (160 x 120, rectilinear) and a 256 x 256 map of 2 mm cells -- finer than a texel, so
    a label pixel's world hit lies within the 3 x 3 texel neighbourhood of its cell's centre.  For the label pixels that are sure in
    label_model, show a tile and hit the window on a cell that is sure and no object's, the two device outputs agree."""
    name = "marks_town"
    c = lm.CASES[name]
    n = len(c.states)
    sim = BatchedSimulator(c.map_name, n, camera_width=c.W, camera_height=c.H, distortion=False, domain_rand=c.dr, seed=1, max_steps=10 ** 6,
                           do_reset=False, asset_root=fp.ASSETS)
    sim.reset(states=dm.init_states(c, n))
    sim.render()
    lab = host(sim, sim.labels()).copy()
    shape = (256, 256, 0.002, 0)
    oh, ow, cell, rb = shape
    bev = host(sim, sim.bev(oh, ow, cell=cell, rows_behind=rb)).copy()
    corners, drawn = sim.object_footprints()
    mm = bm.map_model("test_town")
    assert mm.texel > cell
    k = len(mm.obj_cls)
    compared, red = 0, 0
    for e in range(n):
        x, z, th = c.states[e][:3]
        want = bm.expected(mm, (x, z, th), corners[e, :k], drawn[e, :k], shape)
        bm.compare(bev[e], None, want, (name, e))
        exp_lab, sure = lm.expected(name, e)
        depths, srf = lm.host_buffers(name, e)
        tile = (srf == -1).all(axis=0) & sure
        wx, wz = lm.world_hit(dm.host_camera(c, e), depths[0], tile, 0)
        dx, dz = wx - x, wz - z
        f, s = (dx * math.cos(th) - dz * math.sin(th)) / cell, (dx * math.sin(th) + dz * math.cos(th)) / cell
        i, j = np.floor(oh - rb - f).astype(np.int64), np.floor(s + ow / 2).astype(np.int64)
        ok = tile & (i >= 0) & (i < oh) & (j >= 0) & (j < ow)
        i, j = np.where(ok, i, 0), np.where(ok, j, 0)
        ok &= want.sure_cls[i, j] & want.sure_id[i, j] & (want.inst[i, j] == 0)
        assert np.array_equal(lab[e][ok], exp_lab[ok])
        assert np.array_equal(lab[e][ok], bev[e][i, j][ok]), (name, e, int((lab[e][ok] != bev[e][i, j][ok]).sum()))
        compared += int(ok.sum()); red += int((lab[e][ok] == L.MARK_RED).sum())
    print(f"bev against the camera's labels: {compared} pixels compared, {red} of them on the red line")
    assert compared > 3000 and red > 300
    sim.close()
