"""`-m gpu`: dtsim_instances / dtsim_instances_masked (k_labels<LAB, INST>) against the oracle's per-sample surfaces (tests/instance_model.py):
per pixel o + 1 where the nearest of the four MSAA samples of the frame's source pixel shows mesh object o of the env's own map, 0 on every
other surface and where a pixel has no source; point-sampled smaller maps; with a label map from the same launch.

Exact equality on the model's SURE pixels (the four samples on one surface in the oracle's run and its nudged run); elsewhere another id on
at most Case.cap of the pixels (frame_parity.ORACLE_PLANE.gt1 / ORACLE_MESH.gt1, the label tests' caps; the oracle against its nudged self
stays within a quarter of it, tests/test_instance_model_host.py).  The expected maps are the host's (computed once per process, shared,
read-only); im.make_sim checks that the device holds the object states they were computed from.

160 x 120 or smaller, N <= 130.  Measured on an MI355X: PARITY.md section 4."""
import ctypes as C

import numpy as np
import pytest

import crowd_scenes as cs
import depth_model as dm
import instance_model as im
from dtsim import BatchedSimulator, _ffi, assets, labels as L

pytestmark = pytest.mark.gpu
SENTINEL = 99                                                # no object id (ids end at 64) and no default class


@pytest.fixture(autouse=True)
def crowd_map(monkeypatch):
    """The crowd map as a fixture of the asset library, so that a simulator can hold it by name."""
    monkeypatch.setitem(assets.MAPS, "crowd", cs.crowd_map())


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


MODEL_RUNS = [(n, k) for n in im.DM_CASES for k in (None, "fisheye", "undistort")] + [(n, k) for n in im.CROWD_CASES for k in (None, "fisheye")]


@pytest.mark.parametrize("name,kind", MODEL_RUNS)
def test_instances_match_the_model(name, kind):
    """"planes" (all zero), the walking duckies after 14 steps, the asset-tree town, 90 x 62, and the crowd views: without a source map,
    through the fisheye, and (the dm cases) through the rectify map with its border; the full map against the model, the strided ones byte
    for byte its slices (90 x 62: the strides that divide it, i.e. (2, 2) -- 45 columns: no multiple of four)."""
    c = im.CASES[name]
    sim = im.make_sim(name, kind=kind)
    sim.render()
    full = host(sim, sim.instances()).copy()
    assert full.shape == (c.n_envs, c.H, c.W) and full.dtype == np.uint8
    assert host(sim, sim.instances()).tobytes() == full.tobytes()                   # a second call: the same bytes
    for e in range(c.n_envs):
        want, sure = im.expected(name, e, kind)
        r = im.compare(full[e], want, sure, c.cap, (name, kind, e))
        print(f"{name} {kind} env {e}: off {r['off']:.2e} ({r['n_off']} px, all off the sure mask), unsure {r['unsure']:.3f}, "
              f"ids {im.crowding(full[e])[0]} (expected {im.crowding(want)[0]})")
        if kind is not None:                                                        # a pixel without a source holds 0
            rx, ry = dm.rmap(c.W, c.H, kind)
            sx, sy = np.rint(rx.astype(np.float64)), np.rint(ry.astype(np.float64))
            assert not full[e][~((sx >= 0) & (sx < c.W) & (sy >= 0) & (sy < c.H))].any()
        # every id the expected map holds in more than a handful of sure pixels appears on the device (a kernel that never emits ids ...)
        ids, cnt = np.unique(want[sure], return_counts=True)
        for k, v in zip(ids.tolist(), cnt.tolist()):
            if k and v > 8:
                assert (full[e] == k).sum() >= v, (name, kind, e, k, v)
    if name == "planes":
        assert not full.any()
    if name == "crowd_inside2":
        assert not np.isin(full, np.array(cs.HIDDEN) + 1).any()
    for sy, sx in dm.STRIDES:
        if (sy, sx) == (1, 1) or c.H % sy or c.W % sx:
            continue
        small = host(sim, sim.instances(c.H // sy, c.W // sx)).copy()
        assert small.tobytes() == np.ascontiguousarray(dm.strided(full, sy, sx)).tobytes(), (name, kind, sy, sx)    # exactly the slice
    sim.close()


def test_a_hidden_object_never_appears():
    """"inside2": every third object is invisible -- it has no triangles in the pass, so its id is nowhere in the device map.  Exact: not a
    share of the pixels.  The visible ones are there."""
    for kind in (None, "fisheye"):
        sim = im.make_sim("crowd_inside2", kind=kind)
        vis = sim.read(_ffi.FIELD_OBJ_VISIBLE)[0]
        assert not vis[list(cs.HIDDEN)].any() and vis.sum() == im.MAX_OBJECTS - len(cs.HIDDEN)
        sim.render()
        for size in ((None, None), (60, 80), (30, 20)):
            m = host(sim, sim.instances(*size))
            assert not np.isin(m, np.array(cs.HIDDEN) + 1).any(), (kind, size)
        full = host(sim, sim.instances())
        assert len(np.unique(full[full > 0])) >= 5 and full.max() <= im.MAX_OBJECTS
        sim.close()


@pytest.mark.parametrize("name,kind", [("town", None), ("pedestrians", "undistort"), ("crowd_side", "fisheye")])
def test_one_classification_fills_both_maps(name, kind):
    """The same render, every pixel: the instance map with a label map beside it is the instance map without; the label map of that launch is
    dtsim_labels'; where inst is k + 1 the label is the class of object k of the env's map, where it is 0 a plane's, a texel's or none; an
    object pixel has a finite, non-zero depth."""
    import torch
    c = im.CASES[name]
    sim = im.make_sim(name, kind=kind)
    sim.render()
    for size in ((None, None), (c.H // 2, c.W // 2)):
        alone = dev(sim, sim.instances(*size))
        inst, lab = filled(alone), filled(alone)
        assert sim.instances(*size, out=inst, labels_out=lab) is inst
        ref = dev(sim, sim.labels(*size))
        depth = dev(sim, sim.depth(*size))
        sim.sync()
        assert torch.equal(inst, alone) and torch.equal(lab, ref), (name, size)
        inst, lab, depth = inst.cpu().numpy(), lab.cpu().numpy(), depth.cpu().numpy()
        oc = sim.object_classes()
        assert oc.shape == (1, im.MAX_OBJECTS) and oc.dtype == np.uint8 and not oc[0, len(sim.maps[0].objects):].any()
        assert (oc[0, :len(sim.maps[0].objects)] >= L.OBJECT_FIRST).all()
        on = inst > 0
        assert on.sum() > 50
        assert np.array_equal(lab[on], oc[0][inst[on].astype(np.int64) - 1])
        assert (lab[~on] < L.OBJECT_FIRST).all()
        assert np.isfinite(depth[on]).all() and (depth[on] > 0).all()
        assert not inst[lab == 0].any() and not inst[depth == 0].any()
    sim.close()


@pytest.mark.parametrize("name", ["pedestrians", "crowd_far"])
def test_env_positions_and_the_tail_chunk_give_the_same_bytes(name):
    """N = 130 with period 64: envs e, e + 64 and e + 128 share a state -- every position of the env loop, three chunks, the last with two
    envs; a second call and a second render give the same bytes, with and without the label map beside."""
    N = 130
    c = im.CASES[name]
    sim = im.make_sim(name, N, period=64)
    sim.render()
    a = host(sim, sim.instances()).copy()
    small = host(sim, sim.instances(30, 20)).copy()
    for m in (a, small):
        assert m[:64].tobytes() == m[64:128].tobytes() and m[:2].tobytes() == m[128:].tobytes()
    for e in (0, 1, 2, 63, 64, 127, 128, 129):
        case = name if c.view is None else "crowd_" + sim.views[e]
        want, sure = im.expected(case, im.case_of_env(name, e, 64) if c.view is None else 0)
        im.compare(a[e], want, sure, c.cap, (name, e))
    assert any(a[e].any() for e in range(3))
    assert host(sim, sim.instances()).tobytes() == a.tobytes()
    lab = filled(sim.instances())
    assert host(sim, sim.instances(labels_out=lab)).tobytes() == a.tobytes()
    lab = host(sim, lab)
    assert lab[:64].tobytes() == lab[64:128].tobytes() and lab[:2].tobytes() == lab[128:].tobytes() and (lab != SENTINEL).all()
    sim.render()
    assert host(sim, sim.instances()).tobytes() == a.tobytes()                      # and after another render of the same state
    sim.close()


def test_masked_call_writes_the_selected_rows_only():
    """9 envs, 3 selected: the other rows of both maps keep a sentinel; the selected rows equal the unmasked call's -- after a full render,
    and after render(mask=) with the same mask (only the masked form is valid then)."""
    import torch
    N = 9
    sim = im.make_sim("pedestrians", N)
    sel = torch.zeros(N, dtype=torch.uint8, device="cuda")
    sel[[1, 4, 8]] = 1
    keep = ~sel.bool()
    torch.cuda.synchronize()
    sim.render()
    ref = dev(sim, sim.instances())
    assert bool(ref[sel.bool()].any())
    for size in ((None, None), (60, 80)):
        want = dev(sim, sim.instances(*size))
        want_lab = dev(sim, sim.labels(*size))
        out, lab = filled(want), filled(want)
        assert sim.instances(*size, out=out, mask=sel, labels_out=lab) is out
        sim.sync()
        assert bool((out[keep] == SENTINEL).all()) and torch.equal(out[sel.bool()], want[sel.bool()])
        assert bool((lab[keep] == SENTINEL).all()) and torch.equal(lab[sel.bool()], want_lab[sel.bool()])
        out = filled(want)
        sim.instances(*size, out=out, mask=sel)
        sim.sync()
        assert bool((out[keep] == SENTINEL).all()) and torch.equal(out[sel.bool()], want[sel.bool()])
    pos = sim.read(_ffi.FIELD_POS)
    pos[[1, 4, 8], 0] += 0.05
    sim.write(_ffi.FIELD_POS, pos)
    sim.render(mask=sel)
    out = filled(ref)
    with pytest.raises(_ffi.DtsimError) as ei:
        sim.instances(out=out)                               # the plain call: the unselected envs' records describe the older pass
    assert ei.value.code == _ffi.E_STATE
    sim.instances(out=out, mask=sel)
    sim.sync()
    assert bool((out[keep] == SENTINEL).all()) and not bool((out[sel.bool()] == SENTINEL).any())
    sim.render()
    full = dev(sim, sim.instances())
    assert torch.equal(out[sel.bool()], full[sel.bool()]) and torch.equal(full[keep], ref[keep])
    assert not torch.equal(full[sel.bool()], ref[sel.bool()])
    sim.close()


def test_refusals_leave_both_maps_untouched():
    """No preceding render; a step since the render; the segment view; dtsim_instances after a masked pass; per-env distortion tables; a
    label map asked for without label tables (never installed, or dropped by dtsim_set_assets): DTSIM_E_STATE.  A size that does not divide
    the camera's, a nonzero flag, a null inst or mask: DTSIM_E_INVALID.  Nothing is written: return codes and the sentinel only."""
    import torch
    from dtsim import batched
    N = 3
    sim = im.make_sim("pedestrians", N)
    lib, h = sim._lib, sim._h
    c = im.CASES["pedestrians"]
    out = torch.full((N, c.H, c.W), SENTINEL, dtype=torch.uint8, device="cuda")
    lab = torch.full((N, c.H, c.W), SENTINEL, dtype=torch.uint8, device="cuda")
    ptr, lp = C.c_void_p(out.data_ptr()), C.c_void_p(lab.data_ptr())
    sel = torch.ones(N, dtype=torch.uint8, device="cuda")
    mp = C.c_void_p(sel.data_ptr())
    torch.cuda.synchronize()

    def untouched():
        sim.sync()
        return bool((out == SENTINEL).all()) and bool((lab == SENTINEL).all())

    def refused(code, labels=(None, lp)):
        for l in labels:
            assert lib.dtsim_instances(h, ptr, l, c.H, c.W, 0) == code
            assert lib.dtsim_instances_masked(h, ptr, l, c.H, c.W, 0, mp) == code
    refused(_ffi.E_STATE)                                    # nothing rendered yet
    sim.render()
    refused(_ffi.E_STATE, (lp,))                             # rendered, but a label map without label tables
    assert "dtsim_set_label_assets" in lib.dtsim_last_error().decode()
    assert untouched()
    sim.set_label_assets()
    for l in (None, lp):
        assert lib.dtsim_instances(h, ptr, l, 50, c.W, 0) == _ffi.E_INVALID and lib.dtsim_instances(h, ptr, l, c.H, 81, 0) == _ffi.E_INVALID
        assert lib.dtsim_instances(h, ptr, l, 0, c.W, 0) == _ffi.E_INVALID and lib.dtsim_instances(h, ptr, l, 2 * c.H, c.W, 0) == _ffi.E_INVALID
        assert lib.dtsim_instances(h, ptr, l, c.H, c.W, 1) == _ffi.E_INVALID and lib.dtsim_instances(h, None, l, c.H, c.W, 0) == _ffi.E_INVALID
        assert lib.dtsim_instances_masked(h, ptr, l, c.H, c.W, 0, None) == _ffi.E_INVALID
    for bad in (dict(height=50), dict(width=81), dict(out=out[:2]), dict(out=out.float()), dict(mask=sel.cpu()), dict(labels_out=lab[:2]),
                dict(labels_out=lab.float()), dict(out=out, labels_out=out)):
        with pytest.raises(ValueError):
            sim.instances(**bad)
    sim.step(np.zeros((1, N, 2), np.float32))
    refused(_ffi.E_STATE)                                    # the cameras describe the state before the step
    sim.render(segment=True)
    refused(_ffi.E_STATE)                                    # the segment view
    sim.render(mask=sel)
    for l in (None, lp):
        assert lib.dtsim_instances(h, ptr, l, c.H, c.W, 0) == _ffi.E_STATE      # after a masked pass: the masked form only
    assert untouched()
    assert lib.dtsim_instances_masked(h, ptr, lp, c.H, c.W, 0, mp) == _ffi.OK
    sim.sync()
    assert bool((out != SENTINEL).all()) and bool((lab != SENTINEL).all())
    # dtsim_set_assets drops the label tables: the instance map alone is still to be had, a label map beside it is not
    out.fill_(SENTINEL); lab.fill_(SENTINEL)
    torch.cuda.synchronize()
    sc = batched.load_scene(sim.library, sim.map_names, sim.map_datas)
    tarr, marr, farr, keep = batched.scene_ffi(sc)
    _ffi.check(lib, lib.dtsim_set_assets(h, tarr, len(sc.textures), marr, len(sc.mesh_order)))
    _ffi.check(lib, lib.dtsim_set_maps(h, farr, len(sc.maps)))
    sim.reset(states=dm.init_states(c.dm_case, N))
    sim.render()
    refused(_ffi.E_STATE, (lp,))
    assert untouched()
    assert lib.dtsim_instances(h, ptr, None, c.H, c.W, 0) == _ffi.OK
    sim.sync()
    assert bool((out != SENTINEL).all()) and bool((lab == SENTINEL).all())
    sim.close()
    # per-env distortion tables (camera_rand with the fisheye)
    sim = BatchedSimulator("small_loop", N, camera_width=c.W, camera_height=c.H, distortion=True, camera_rand=True, domain_rand=False, seed=3)
    sim.render()
    sim.set_label_assets()
    out.fill_(SENTINEL)
    torch.cuda.synchronize()
    for l in (None, lp):
        assert sim._lib.dtsim_instances(sim._h, ptr, l, c.H, c.W, 0) == _ffi.E_STATE
        assert sim._lib.dtsim_instances_masked(sim._h, ptr, l, c.H, c.W, 0, mp) == _ffi.E_STATE
    sim.sync()
    assert bool((out == SENTINEL).all()) and bool((lab == SENTINEL).all())
    sim.close()


@pytest.mark.parametrize("kind", [None, "fisheye"])
def test_two_maps_each_env_indexes_its_own_object_list(kind):
    """loop_only_duckies (8 objects) and small_loop_only_duckies (4) resident in one simulator, envs alternating: each env's ids are indices
    into ITS map's list, held to the oracle of that map; the classes of object_classes() go by map."""
    sim, envs = im.make_two_map_sim(kind)
    assert [len(m.objects) for m in sim.maps] == [8, 4]
    sim.render()
    lab = filled(sim.instances())
    full = host(sim, sim.instances(labels_out=lab)).copy()
    lab = host(sim, lab)
    oc = sim.object_classes()
    assert oc.shape == (2, im.MAX_OBJECTS) and (oc[0, :8] == L.CLASS_IDS["duckie"]).all() and (oc[1, :4] == L.CLASS_IDS["duckie"]).all()
    assert not oc[0, 8:].any() and not oc[1, 4:].any()
    for e, (case, ce) in enumerate(envs):
        c = im.CASES[case]
        want, sure = im.expected(case, ce, kind)
        r = im.compare(full[e], want, sure, c.cap, (case, kind, e))
        print(f"{case} {kind} env {e}: off {r['off']:.2e} ({r['n_off']} px), ids {sorted(np.unique(full[e]).tolist())}")
        own = im.TWO_PICKS[e % 2][ce] + 1
        assert (full[e] == own).sum() > 50 and full[e].max() <= len(sim.maps[e % 2].objects)
        assert np.array_equal(lab[e][full[e] > 0], oc[e % 2][full[e][full[e] > 0].astype(np.int64) - 1])
    assert max(full[e].max() for e in range(0, len(envs), 2)) > 4                    # map 0's envs show ids map 1 does not have
    small = host(sim, sim.instances(60, 80))
    assert small.tobytes() == np.ascontiguousarray(dm.strided(full, 2, 2)).tobytes()
    sim.close()
