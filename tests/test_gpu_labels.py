"""`-m gpu`: dtsim_labels / dtsim_labels_masked / dtsim_set_label_assets (k_labels) against the oracle's per-sample surfaces
(tests/label_model.py): per pixel the class of the nearest of the four MSAA samples of the frame's source pixel -- 0 = a pixel without a
source, 1 sky, 2 ground, a tile by the nearest texel's class, a mesh object by its mesh's; point-sampled smaller maps.

Exact equality on the model's SURE pixels (the four samples on one surface in the oracle's run and its nudged run, and no class edge within a
texel of any sample); elsewhere a different class on at most Case.cap of the pixels (frame_parity.ORACLE_PLANE.gt1 / ORACLE_MESH.gt1: the
shares allowed for samples whose coverage flips; the oracle against its nudged self stays within a quarter of it,
tests/test_label_model_host.py).  The expected maps are the host's (computed once per process, shared, read-only); each test first checks
that the device holds the state and the tables they were computed from.

Measured on an MI355X: PARITY.md section 4."""
import ctypes as C

import numpy as np
import pytest

import depth_model as dm
import frame_parity as fp
import label_model as lm
from dtsim import BatchedSimulator, _ffi, labels as L

pytestmark = pytest.mark.gpu
SENTINEL = 99                                                # no default class


def make_sim(name, n=None, period=None, **kw):
    """The case's states on the device (env e: state e % len(states), or (e % period) % len(states)), stepped as the case says."""
    c = lm.CASES[name]
    n = len(c.states) if n is None else n
    args = dict(camera_width=c.W, camera_height=c.H, distortion=False, domain_rand=c.dr, seed=1, max_steps=10 ** 6, do_reset=False)
    args.update(kw)
    if c.asset_tree:
        args["asset_root"] = fp.ASSETS
    sim = BatchedSimulator(c.map_name, n, **args)
    sim.reset(states=dm.init_states(c, n, period))
    if c.wait is not None:
        par = sim.read(_ffi.FIELD_OBJ_PARAMS)                 # [N, MAX_DYNAMIC, (vel, wait_time, wiggle)]
        par[:, :, 1] = c.wait
        sim.write(_ffi.FIELD_OBJ_PARAMS, par)
    if c.steps:
        sim.step(np.zeros((c.steps, n, 2), np.float32), n_steps=c.steps)
    return sim


def check_state(sim, name):
    """The device holds what the host's expected maps were computed from: the poses, the objects as the oracle's physics left them (the
    cases of dm.CASES), and the default tables of the host (label_assets() == the model's host_tables, byte for byte)."""
    c, sc = lm.CASES[name], lm.scene_of(name)
    pos, ang = sim.read(_ffi.FIELD_POS), sim.read(_ffi.FIELD_ANGLE)
    objs = dm.host_objects(name) if name in dm.CASES else None
    for e in range(len(c.states)):
        x, z, a = c.states[e][:3]
        if c.steps:
            assert max(abs(pos[e, 0] - x), abs(pos[e, 2] - z), abs(ang[e] - a)) <= 1e-9, (name, e)
        else:
            assert (pos[e, 0], pos[e, 2], ang[e]) == (x, z, a), (name, e)
        if sc.m.objects:
            want = objs[e] if objs is not None else [dict(pos=np.asarray(o.pos, np.float64), y_rot=float(o.y_rot), visible=True) for o in sc.m.objects]
            for got, w in zip(fp.obj_states(sim, e, sc), want):
                assert np.allclose(got["pos"], w["pos"], rtol=0, atol=1e-9) and abs(got["y_rot"] - w["y_rot"]) <= 1e-7 and got["visible"] == w["visible"], (name, e)
    tiles, obj_cls = lm.host_tables(name)
    texel, mesh = sim.label_assets()
    assert len(texel) == len(sim.textures) and mesh.shape == (len(sim._mesh_order),) and mesh.dtype == np.uint8
    for i, kd in enumerate(sim.texture_kinds):
        assert texel[i].tobytes() == tiles[kd].tobytes() and texel[i].shape == tiles[kd].shape, (name, kd)
    per_obj = [int(mesh[sim._mesh_order.index(o.mesh_kind)]) for o in sim.maps[0].objects]
    assert per_obj == [int(v) for v in obj_cls], (name, per_obj, obj_cls)


def host(sim, t):
    sim.sync()
    return t.cpu().numpy()


def dev(sim, t):
    sim.sync()
    return t.clone()


def filled(like, value=SENTINEL):
    import torch
    out = torch.full_like(like, value)
    torch.cuda.synchronize()
    return out


def fisheye_kw(kind):
    return {None: {}, "fisheye": dict(distortion=True), "undistort": dict(distortion=True, undistort=True)}[kind]


def run_case(name, kind, strides=dm.STRIDES):
    """Render the case and hold its label maps to the model at every stride; returns (the full maps, the sim's depth of the same render)."""
    c = lm.CASES[name]
    n = len(c.states)
    sim = make_sim(name, **fisheye_kw(kind))
    check_state(sim, name)
    sim.render()
    full = host(sim, sim.labels()).copy()
    assert full.shape == (n, c.H, c.W) and full.dtype == np.uint8
    assert host(sim, sim.labels()).tobytes() == full.tobytes()                      # a second call: the same bytes
    depth = host(sim, sim.depth()).copy()
    for e in range(n):
        want, sure = lm.expected(name, e, kind)
        r = lm.compare(full[e], want, sure, c.cap, (name, kind, e))
        print(f"{name} {kind} env {e}: off {r['off']:.2e} ({r['n_off']} px, all off the sure mask), unsure {r['unsure']:.3f}")
        if kind is not None:                                                        # class 0 sits exactly on the border set
            rx, ry = dm.rmap(c.W, c.H, kind)
            sx, sy = np.rint(rx.astype(np.float64)), np.rint(ry.astype(np.float64))
            assert np.array_equal(full[e] == 0, ~((sx >= 0) & (sx < c.W) & (sy >= 0) & (sy < c.H)))
        else:
            assert not (full[e] == 0).any()
        # every class the expected map holds in more than a handful of pixels appears on the device (a kernel that never emits markings ...)
        ids, cnt = np.unique(want, return_counts=True)
        for k, v in zip(ids.tolist(), cnt.tolist()):
            if v > 8:
                assert (full[e] == k).sum() >= v // 2, (name, kind, e, k, v)
        # consistent with depth on the same render: sky <=> inf, no source <=> 0, both exact
        assert np.array_equal(full[e] == L.SKY, np.isinf(depth[e])) and np.array_equal(full[e] == 0, depth[e] == 0), (name, kind, e)
    for sy, sx in strides:
        if (sy, sx) == (1, 1) or c.H % sy or c.W % sx:
            continue
        small = host(sim, sim.labels(c.H // sy, c.W // sx)).copy()
        assert small.tobytes() == np.ascontiguousarray(dm.strided(full, sy, sx)).tobytes(), (name, kind, sy, sx)    # exactly the slice
        for e in range(n):
            want, sure = lm.expected(name, e, kind)
            lm.compare(small[e], dm.strided(want, sy, sx), dm.strided(sure, sy, sx), c.cap, (name, kind, e, sy, sx))
    sim.close()
    return full


@pytest.mark.parametrize("kind", [None, "fisheye", "undistort"])
@pytest.mark.parametrize("name", list(lm.CASES))
def test_labels_match_the_model(name, kind):
    """Every case of depth_model.CASES (160 x 120 planes, per-env cameras, walking duckies after 14 steps, the asset-tree town, 90 x 62) and
    the marking close-ups: without a source map, through the fisheye, and through the rectify map with its border; the full map and the
    strided ones (90 x 62: the strides that divide it, i.e. (2, 2) -- 45 columns: no multiple of four)."""
    full = run_case(name, kind)
    if name == "marks_straight" and kind is None:
        assert (full[0] == L.MARK_WHITE).sum() > 1500 and (full[1] == L.MARK_YELLOW).sum() > 500
    if name == "marks_town" and kind is None:
        assert (full[0] == L.MARK_RED).sum() > 1500
    if kind == "undistort":
        assert (full[0] == 0).sum() > (300 if full.shape[1:] == (120, 160) else 80)


@pytest.mark.parametrize("name", ["planes_dr", "pedestrians", "marks_town"])
def test_env_positions_and_the_tail_chunk_give_the_same_bytes(name):
    """N = 130: envs e, e + 64 and e + 128 share a state -- every position of the env loop, three chunks, the last with two envs; a second
    call and a second render give the same bytes."""
    N = 130
    sim = make_sim(name, N, period=64)
    sim.render()
    a = host(sim, sim.labels()).copy()
    small = host(sim, sim.labels(30, 20)).copy()
    for m in (a, small):
        assert m[:64].tobytes() == m[64:128].tobytes() and m[:2].tobytes() == m[128:].tobytes()
    c = lm.CASES[name]
    for e in (0, 63, 64, 127, 128, 129):
        want, sure = lm.expected(name, (e % 64) % len(c.states))
        lm.compare(a[e], want, sure, c.cap, (name, e))
    assert host(sim, sim.labels()).tobytes() == a.tobytes()
    sim.render()
    assert host(sim, sim.labels()).tobytes() == a.tobytes()                         # and after another render of the same state
    sim.close()


def test_masked_call_writes_the_selected_rows_only():
    """9 envs, 3 selected: the other rows keep a sentinel; the selected rows equal the unmasked call's -- after a full render, and after
    render(mask=) with the same mask (only the masked form is valid then)."""
    import torch
    N = 9
    sim = make_sim("pedestrians", N)
    sel = torch.zeros(N, dtype=torch.uint8, device="cuda")
    sel[[1, 4, 8]] = 1
    keep = ~sel.bool()
    torch.cuda.synchronize()
    sim.render()
    ref = dev(sim, sim.labels())
    for size in ((None, None), (60, 80)):
        want = dev(sim, sim.labels(*size))
        out = filled(want)
        assert sim.labels(*size, out=out, mask=sel) is out
        sim.sync()
        assert bool((out[keep] == SENTINEL).all()) and torch.equal(out[sel.bool()], want[sel.bool()])
    pos = sim.read(_ffi.FIELD_POS)
    pos[[1, 4, 8], 0] += 0.05
    sim.write(_ffi.FIELD_POS, pos)
    sim.render(mask=sel)
    out = filled(ref)
    with pytest.raises(_ffi.DtsimError) as ei:
        sim.labels(out=out)                                  # the plain call: the unselected envs' records describe the older pass
    assert ei.value.code == _ffi.E_STATE
    sim.labels(out=out, mask=sel)
    sim.sync()
    assert bool((out[keep] == SENTINEL).all()) and not bool((out[sel.bool()] == SENTINEL).any())
    sim.render()
    full = dev(sim, sim.labels())
    assert torch.equal(out[sel.bool()], full[sel.bool()]) and torch.equal(full[keep], ref[keep])
    assert not torch.equal(full[sel.bool()], ref[sel.bool()])
    sim.close()


def test_refusals_leave_out_untouched():
    """Before label assets are installed; no preceding render; a step since the render; the segment view; dtsim_labels after a masked
    pass; per-env distortion tables: DTSIM_E_STATE.  A size that does not divide the camera's, a nonzero flag, a null out or mask:
    DTSIM_E_INVALID.  Nothing is written: return codes and the sentinel only."""
    import torch
    N = 3
    sim = make_sim("pedestrians", N)
    lib, h = sim._lib, sim._h
    c = lm.CASES["pedestrians"]
    out = torch.full((N, c.H, c.W), SENTINEL, dtype=torch.uint8, device="cuda")
    ptr = C.c_void_p(out.data_ptr())
    sel = torch.ones(N, dtype=torch.uint8, device="cuda")
    mp = C.c_void_p(sel.data_ptr())
    torch.cuda.synchronize()

    def refused(code):
        assert lib.dtsim_labels(h, ptr, c.H, c.W, 0) == code
        assert lib.dtsim_labels_masked(h, ptr, c.H, c.W, 0, mp) == code
    refused(_ffi.E_STATE)                                    # nothing rendered yet (and no tables)
    sim.render()
    refused(_ffi.E_STATE)                                    # rendered, but no label assets installed
    assert "dtsim_set_label_assets" in lib.dtsim_last_error().decode()
    sim.set_label_assets()
    assert lib.dtsim_labels(h, ptr, 50, c.W, 0) == _ffi.E_INVALID and lib.dtsim_labels(h, ptr, c.H, 81, 0) == _ffi.E_INVALID
    assert lib.dtsim_labels(h, ptr, 0, c.W, 0) == _ffi.E_INVALID and lib.dtsim_labels(h, ptr, 2 * c.H, c.W, 0) == _ffi.E_INVALID
    assert lib.dtsim_labels(h, ptr, c.H, c.W, 1) == _ffi.E_INVALID and lib.dtsim_labels(h, None, c.H, c.W, 0) == _ffi.E_INVALID
    assert lib.dtsim_labels_masked(h, ptr, c.H, c.W, 0, None) == _ffi.E_INVALID
    for bad in (dict(height=50), dict(width=81), dict(out=out[:2]), dict(out=out.float()), dict(mask=sel.cpu())):
        with pytest.raises(ValueError):
            sim.labels(**bad)
    sim.step(np.zeros((1, N, 2), np.float32))
    refused(_ffi.E_STATE)                                    # the cameras describe the state before the step
    sim.render(segment=True)
    refused(_ffi.E_STATE)                                    # the segment view
    sim.render(mask=sel)
    assert lib.dtsim_labels(h, ptr, c.H, c.W, 0) == _ffi.E_STATE     # after a masked pass: the masked form only
    sim.sync()
    assert bool((out == SENTINEL).all())
    assert lib.dtsim_labels_masked(h, ptr, c.H, c.W, 0, mp) == _ffi.OK
    sim.sync()
    assert bool((out != SENTINEL).all())
    sim.close()
    # per-env distortion tables (camera_rand with the fisheye)
    sim = BatchedSimulator("small_loop", N, camera_width=c.W, camera_height=c.H, distortion=True, camera_rand=True, domain_rand=False, seed=3)
    sim.render()
    sim.set_label_assets()
    out.fill_(SENTINEL)
    torch.cuda.synchronize()
    assert sim._lib.dtsim_labels(sim._h, ptr, c.H, c.W, 0) == _ffi.E_STATE
    assert sim._lib.dtsim_labels_masked(sim._h, ptr, c.H, c.W, 0, mp) == _ffi.E_STATE
    sim.sync()
    assert bool((out == SENTINEL).all())
    sim.close()


def _user_tables(sim, kind, mesh_key):
    texel, mesh = sim.label_assets()
    t = sim.texture_kinds.index(kind)
    texel = list(texel)
    texel[t] = np.full_like(texel[t], 200)
    mesh = mesh.copy()
    mesh[sim._mesh_order.index(mesh_key)] = 201
    return texel, mesh


def test_user_tables_and_failed_setters():
    """A user's tables -- every texel of the `straight` texture -> 200, the cone's mesh -> 201 -- show up exactly where the default map had
    that tile / that object, and nothing else changes; a failed dtsim_set_label_assets (wrong count; through the
    Python layer also a wrong size or type) leaves the previous tables in force: the same bytes before and after."""
    name = "town"
    sim = make_sim(name)
    check_state(sim, name)
    sim.render()
    default = host(sim, sim.labels()).copy()
    texel, mesh = _user_tables(sim, "straight", "cone")
    sim.set_label_assets(texel, mesh)
    user = host(sim, sim.labels()).copy()
    tiles, obj_cls = lm.host_tables(name)
    tiles = dict(tiles, straight=np.full_like(tiles["straight"], 200))
    cone = L.CLASS_IDS["cone"]
    obj_cls = np.where(obj_cls == cone, 201, obj_cls)
    c = lm.CASES[name]
    for e in range(len(c.states)):
        want, sure = lm.expected_with(name, e, None, False, (tiles, obj_cls))
        lm.compare(user[e], want, sure, c.cap, (name, "user", e))
    changed = user != default
    assert np.array_equal(changed, (user == 200) | (user == 201))                   # nothing else moved
    assert np.array_equal(user == 201, default == cone) and (user == 201).sum() > 200
    assert np.isin(default[user == 200], (L.ROAD, L.MARK_WHITE, L.MARK_YELLOW)).all() and (user == 200).sum() > 5000
    assert (default[~changed] == user[~changed]).all() and (user == L.ROAD).sum() > 1000     # the other tiles' road is still road
    # failed setters: the user tables stay in force
    lib, h = sim._lib, sim._h
    u8p = C.POINTER(C.c_uint8)
    ok_t = [np.ascontiguousarray(a) for a in sim.label_assets()[0]]
    parr = (u8p * len(ok_t))(*[a.ctypes.data_as(u8p) for a in ok_t])
    ok_m = sim.label_assets()[1]
    mp = ok_m.ctypes.data_as(u8p)
    assert lib.dtsim_set_label_assets(h, parr, len(ok_t) - 1, mp, len(ok_m)) == _ffi.E_INVALID      # wrong texture count
    assert lib.dtsim_set_label_assets(h, parr, len(ok_t), mp, len(ok_m) + 1) == _ffi.E_INVALID      # wrong mesh count
    assert lib.dtsim_set_label_assets(h, None, len(ok_t), mp, len(ok_m)) == _ffi.E_INVALID
    assert lib.dtsim_set_label_assets(h, parr, len(ok_t), None, len(ok_m)) == _ffi.E_INVALID
    hole = (u8p * len(ok_t))(*[a.ctypes.data_as(u8p) for a in ok_t])
    hole[1] = None
    assert lib.dtsim_set_label_assets(h, hole, len(ok_t), mp, len(ok_m)) == _ffi.E_INVALID
    for bad in (dict(texel_class=ok_t[:-1]), dict(texel_class=[ok_t[0][:64]] + ok_t[1:]), dict(texel_class=[a.astype(np.int32) for a in ok_t]),
                dict(mesh_class=ok_m[:-1]), dict(mesh_class=ok_m.astype(np.int64))):
        with pytest.raises(ValueError):                                             # wrong count, wrong size, wrong type
            sim.set_label_assets(**bad)
    assert host(sim, sim.labels()).tobytes() == user.tobytes()                      # still valid (no render needed), the same bytes
    sim.set_label_assets()                                                          # and back to the defaults
    assert host(sim, sim.labels()).tobytes() == default.tobytes()
    sim.close()


def test_set_assets_drops_the_tables():
    """dtsim_set_assets drops the label tables (the list they mirror is gone): after new assets and maps, dtsim_labels waits for
    dtsim_set_label_assets."""
    import torch
    from dtsim import batched
    sim = make_sim("planes", 2)
    sim.render()
    first = host(sim, sim.labels()).copy()
    c = lm.CASES["planes"]
    out = torch.full((2, c.H, c.W), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    sc = batched.load_scene(sim.library, sim.map_names, sim.map_datas)
    tarr, marr, farr, keep = batched.scene_ffi(sc)
    _ffi.check(sim._lib, sim._lib.dtsim_set_assets(sim._h, tarr, len(sc.textures), marr, len(sc.mesh_order)))
    _ffi.check(sim._lib, sim._lib.dtsim_set_maps(sim._h, farr, len(sc.maps)))
    sim.reset(states=dm.init_states(c, 2))
    sim.render()
    assert sim._lib.dtsim_labels(sim._h, C.c_void_p(out.data_ptr()), c.H, c.W, 0) == _ffi.E_STATE
    sim.sync()
    assert bool((out == SENTINEL).all())
    sim.set_label_assets()
    assert host(sim, sim.labels()).tobytes() == first.tobytes()
    sim.close()
