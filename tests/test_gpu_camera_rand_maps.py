"""`-m gpu`: dtsim_depth / dtsim_labels / dtsim_instances and their masked forms with DTSIM_MAP_ENV_TABLES while per-env distortion tables are
installed (k_depth<F16, true>, k_labels<LAB, INST, true>): the map of env e at camera pixel p is the pass's value at rectilinear pixel
src_index[env_cal[e]][p] of that env, 0 where the table names no source.

Against the oracle through tests/camera_rand_maps_model.py (the existing models' rectilinear maps gathered through the env's table, with their
tolerances and caps); against the device itself, byte for byte (a twin handle with an identity table, its full maps gathered on the host);
against the folded fisheye with the nominal calibration for every env; one state, one result; the masked forms; the ABI's edges.
160 x 120 cameras, six tables, N = 72: a full chunk of the env loop and a tail of 8.  Measured on an MI355X: PARITY.md section 4,
profiles/camera_rand_maps_parity.txt."""
import ctypes as C

import numpy as np
import pytest

import camera_rand_maps_model as cm
import crowd_scenes as cs
import depth_model as dm
import instance_model as im
import label_model as lm
from dtsim import _ffi, assets
from dtsim import distortion as pdist

pytestmark = pytest.mark.gpu
FLAG = _ffi.MAP_ENV_TABLES
SENTINEL = 99                                                # no object id, no default class, no depth of these scenes
ip = C.POINTER(C.c_int32)


@pytest.fixture(autouse=True)
def crowd_map(monkeypatch):
    """The crowd map as a fixture of the asset library, so that a simulator can hold it by name."""
    monkeypatch.setitem(assets.MAPS, "crowd", cs.crowd_map())


def host(sim, t):
    sim.sync()
    return t.cpu().numpy().copy()


def maps_of(sim, h=None, w=None, mask=None, out=None):
    """(depth, labels, instances) of the simulator's own calls, as host arrays; out: three device tensors to write into."""
    o = out or (None, None, None)
    return (host(sim, sim.depth(h, w, out=o[0], mask=mask)), host(sim, sim.labels(h, w, out=o[1], mask=mask)),
            host(sim, sim.instances(h, w, out=o[2], mask=mask)))


def raw(sim, what, out, flags, mask=None, labels=None):
    """The C entry point itself: its return code.  out / labels / mask: device tensors."""
    lib, hd = sim._lib, sim._h
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())       # noqa: E731
    hh, ww = int(out.shape[1]), int(out.shape[2])
    if what == "depth":
        return lib.dtsim_depth(hd, p(out), hh, ww, flags) if mask is None else lib.dtsim_depth_masked(hd, p(out), hh, ww, flags, p(mask))
    if what == "labels":
        return lib.dtsim_labels(hd, p(out), hh, ww, flags) if mask is None else lib.dtsim_labels_masked(hd, p(out), hh, ww, flags, p(mask))
    if mask is None:
        return lib.dtsim_instances(hd, p(out), p(labels), hh, ww, flags)
    return lib.dtsim_instances_masked(hd, p(out), p(labels), hh, ww, flags, p(mask))


def fresh(n, h, w, value=SENTINEL):
    """(depth float32, labels uint8, instances uint8) device tensors [n, h, w] holding the sentinel."""
    import torch
    out = (torch.full((n, h, w), float(value), dtype=torch.float32, device="cuda"), torch.full((n, h, w), value, dtype=torch.uint8, device="cuda"),
           torch.full((n, h, w), value, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    return out


def raw_maps(sim, flags, h, w):
    """The three maps through the C entry points with `flags`, as host arrays."""
    sim._need_label_assets()
    d, l, i = fresh(sim.num_envs, h, w)
    for what, t in (("depth", d), ("labels", l), ("instances", i)):
        assert raw(sim, what, t, flags) == _ffi.OK, (what, sim._lib.dtsim_last_error())
    return host(sim, d), host(sim, l), host(sim, i)


def hold_to_the_oracle(tag, got, who, cal):
    """got = (depth, labels, instances) [n, H, W] of a batch, env e showing case env who[e] = (case, env of the case) through table cal[e]:
    each map against the model at every stride.  Prints the worst figures (profiles/camera_rand_maps_parity.txt)."""
    depth, lab, inst = got
    worst = dict(depth_beyond=0.0, depth_max_within=0.0, labels_off=0.0, instances_off=0.0)
    for e, (name, ce) in enumerate(who):
        cap, c = cm.case_of(name)[3], int(cal[e])
        wd = cm.expected("depth", name, ce, c)
        wi, si = cm.expected("instances", name, ce, c)
        wl, sl = cm.expected("labels", name, ce, c) if name in lm.CASES else (None, None)
        for sy, sx in dm.STRIDES:
            r = dm.compare(dm.strided(depth[e], sy, sx), dm.strided(wd, sy, sx), dm.INV_DEPTH_TOL, cap, (tag, "depth", e, name, ce, c, sy, sx))
            worst["depth_beyond"] = max(worst["depth_beyond"], r["beyond"]); worst["depth_max_within"] = max(worst["depth_max_within"], r["max_within"])
            r = im.compare(dm.strided(inst[e], sy, sx), dm.strided(wi, sy, sx), dm.strided(si, sy, sx), cap, (tag, "instances", e, name, ce, c, sy, sx))
            worst["instances_off"] = max(worst["instances_off"], r["off"])
            if wl is not None:
                r = lm.compare(dm.strided(lab[e], sy, sx), dm.strided(wl, sy, sx), dm.strided(sl, sy, sx), cap, (tag, "labels", e, name, ce, c, sy, sx))
                worst["labels_off"] = max(worst["labels_off"], r["off"])
    print(f"parity {tag}: {len(who)} envs x 3 strides: depth beyond tol {worst['depth_beyond']:.2e} (worst env), max |d(1/d)| within {worst['depth_max_within']:.3e}; "
          f"labels off {worst['labels_off']:.2e}; instances off {worst['instances_off']:.2e} (worst env; all off the sure masks)")


def all_strides(sim, full):
    """The simulator's three maps at every stride: each is byte for byte the slice of `full` (depth, labels, instances)."""
    for sy, sx in dm.STRIDES[1:]:
        small = maps_of(sim, cm.H // sy, cm.W // sx)
        for s, f in zip(small, full):
            assert s.tobytes() == np.ascontiguousarray(dm.strided(f, sy, sx)).tobytes(), (sy, sx, f.dtype)


# ---- 1. against the oracle ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", cm.LABEL_CASES + (cm.CROWD_CASE,))
def test_maps_match_the_oracle_through_each_envs_own_table(name):
    """N = 72, env e through table (e + e // 64) % 6: envs e and e + 64 show one state through two tables."""
    sim = cm.make_sim(name)
    cal = cm.install(sim)
    sim.render()
    full = maps_of(sim)
    assert full[0].shape == (cm.N, cm.H, cm.W) and full[0].dtype == np.float32 and full[1].dtype == full[2].dtype == np.uint8
    who = [(cm.case_name(name, e), cm.case_env(name, e)) for e in range(cm.N)]
    hold_to_the_oracle(name, full, who, cal)
    src = cm.tables()[0]
    for e in range(cm.N):                                     # no source: depth 0, class 0, id 0 -- exactly there
        none = (src[cal[e]] < 0).reshape(cm.H, cm.W)
        assert np.array_equal(full[0][e] == 0, none) and np.array_equal(full[1][e] == 0, none) and not full[2][e][none].any(), e
    assert any(full[0][e].tobytes() != full[0][e + 64].tobytes() for e in range(cm.N - 64))      # the tables took effect
    all_strides(sim, full)
    inst = sim.instances()
    boxes = host(sim, sim.boxes(inst))
    assert np.array_equal(boxes, im.box_model(host(sim, inst)))                   # boxes: exactly those of the device's own map
    if name != "planes_dr" and name != "marks_straight":
        assert full[2].any()
    sim.close()


def test_two_maps_each_env_through_its_own_table_and_object_list():
    sim, who = im.make_two_map_sim("fisheye")
    cal = cm.install(sim)
    assert cal.tolist() == list(range(6))
    sim.render()
    full = maps_of(sim)
    hold_to_the_oracle("two_maps", full, who, cal)
    for e, (name, ce) in enumerate(who):                     # its own object, by its index in its own map's list
        k = im.TWO_PICKS[e % 2][ce]
        assert (full[2][e] == k + 1).sum() > 50, (e, name, k)
    all_strides(sim, full)
    inst = sim.instances()
    assert np.array_equal(host(sim, sim.boxes(inst)), im.box_model(host(sim, inst)))
    sim.close()


# ---- 2. against the device itself ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["pedestrians", "planes_dr"])
def test_maps_are_the_rectilinear_maps_of_the_device_gathered_through_the_tables(name):
    """Handle b: the same states, ONE identity table (src_index[p] = p) for every env -- its frames and maps are the rectilinear ones, and its
    maps run the per-env-table instantiation too.  Every map of handle a, at every stride, is b's full map gathered on the host."""
    a, b = cm.make_sim(name), cm.make_sim(name)
    cal = cm.install(a)
    ident, zeros = np.arange(cm.H * cm.W, dtype=np.int32), np.zeros(cm.N, np.int32)
    assert b._lib.dtsim_set_distortion_luts(b._h, 1, ident.ctypes.data_as(ip), zeros.ctypes.data_as(ip), 0) == _ffi.OK
    a.render()
    b.render()
    rect = raw_maps(b, FLAG, cm.H, cm.W)
    src = cm.tables()[0]
    want = [np.stack([cm.gather(m[e], src[cal[e]], 0) for e in range(cm.N)]) for m in rect]
    for sy, sx in dm.STRIDES:
        got = maps_of(a, cm.H // sy, cm.W // sx)
        for g, w, what in zip(got, want, ("depth", "labels", "instances")):
            w = np.ascontiguousarray(dm.strided(w, sy, sx))
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (name, what, sy, sx, int((g != w).sum()))
    print(f"parity device {name}: {cm.N} envs x 3 maps x 3 strides byte-identical to the identity-table handle's full maps gathered on the host")
    # the frames are gathered the same way: map and frame stay pixel-aligned
    fa, fb = a.frames_host(), b.frames_host()
    for e in (0, 5, 64, 71):
        assert np.array_equal(fa[e], cm.gather(np.moveaxis(fb[e], -1, 0), src[cal[e]], 0).transpose(1, 2, 0)), e
    a.close()
    b.close()


def test_a_table_without_a_source_gives_the_no_source_values():
    """The sampled calibrations leave no pixel of a 160 x 120 frame without a source, so the -1 entries are hand-made: table 0 the identity
    inside a 7-pixel border of -1, table 1 a mirror image with every fifth pixel -1; envs alternate.  The maps are the identity-table maps of
    the same handle gathered on the host, 0 where the table says -1 -- and so are the frames, black there."""
    n = 66
    sim = cm.make_sim("pedestrians", n)
    lib, hd = sim._lib, sim._h
    ident = np.arange(cm.H * cm.W, dtype=np.int32)
    assert lib.dtsim_set_distortion_luts(hd, 1, ident.ctypes.data_as(ip), np.zeros(n, np.int32).ctypes.data_as(ip), 0) == _ffi.OK
    sim.render()
    rect, frames = raw_maps(sim, FLAG, cm.H, cm.W), sim.frames_host()
    t0 = ident.reshape(cm.H, cm.W).copy()
    t0[:7] = t0[-7:] = -1; t0[:, :7] = t0[:, -7:] = -1
    t1 = ident.reshape(cm.H, cm.W)[:, ::-1].copy()
    t1.reshape(-1)[::5] = -1
    src = np.ascontiguousarray(np.stack([t0.reshape(-1), t1.reshape(-1)]))
    cal = (np.arange(n) % 2).astype(np.int32)
    assert lib.dtsim_set_distortion_luts(hd, 2, src.ctypes.data_as(ip), cal.ctypes.data_as(ip), 0) == _ffi.OK
    sim.render()
    for sy, sx in dm.STRIDES:
        got = raw_maps(sim, FLAG, cm.H // sy, cm.W // sx)
        for g, m, what in zip(got, rect, ("depth", "labels", "instances")):
            w = np.ascontiguousarray(dm.strided(np.stack([cm.gather(m[e], src[cal[e]], 0) for e in range(n)]), sy, sx))
            assert g.tobytes() == w.tobytes(), (what, sy, sx, int((g != w).sum()))
    full = raw_maps(sim, FLAG, cm.H, cm.W)
    none = (src[cal] < 0).reshape(n, cm.H, cm.W)
    assert none[0].sum() > 3000 and none[1].sum() == cm.H * cm.W // 5
    assert not full[0][none].any() and not full[1][none].any() and not full[2][none].any() and (full[1][~none] > 0).all()
    fr = sim.frames_host()
    for e in (0, 1, 64, 65):
        assert np.array_equal(fr[e], cm.gather(np.moveaxis(frames[e], -1, 0), src[cal[e]], 0).transpose(1, 2, 0)), e
    sim.close()


# ---- 3. anchor ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["pedestrians", "planes_dr"])
def test_anchor_nominal_tables_give_the_folded_fisheyes_maps(name):
    """The nominal calibration for every env, maps under the flag, against the same handle's maps with the folded fisheye (flags 0) before
    the install.  Labels and instances equal; depth equal, or -- the two instantiations contracted differently -- within INV_DEPTH_TOL on
    every pixel, the count printed."""
    sim = cm.make_sim(name)
    sim.render()
    fold = maps_of(sim)
    sim.set_camera_calibrations(pdist.CAMERA_MATRIX[None], pdist.DIST_COEFS[None], np.zeros(cm.N, np.int32))
    sim.render()
    got = maps_of(sim)
    assert got[1].tobytes() == fold[1].tobytes() and got[2].tobytes() == fold[2].tobytes(), name
    n_diff = int((got[0].view(np.int32) != fold[0].view(np.int32)).sum())
    assert np.array_equal(got[0] == 0, fold[0] == 0)
    err = np.abs(dm.inv(np.where(got[0] == 0, 1.0, got[0])) - dm.inv(np.where(fold[0] == 0, 1.0, fold[0])))
    print(f"parity anchor {name}: labels and instances equal; depth differs on {n_diff} of {got[0].size} pixels, max |d(1/d)| {float(err.max()):.3e}")
    assert float(err.max()) <= dm.INV_DEPTH_TOL, (name, n_diff, float(err.max()))
    sim.close()


# ---- 4. one state, one result ----------------------------------------------------------------------------------------------------------------

def test_one_state_and_one_table_give_the_same_bytes_at_every_env_position():
    """Envs e, e + 64 and e + 70 hold one state and read one table: a position inside the full chunk, the first of the tail chunk and its
    last but one.  The same bytes in all three maps, on a second call, and after a second render."""
    e = 1
    c = lm.CASES["pedestrians"]
    st = dm.init_states(c, cm.N, cm.PERIOD)
    st[e + 70] = st[e]
    sim = cm.make_sim("pedestrians", states=st)
    cal = cm.env_cal()
    cal[e + 64] = cal[e + 70] = cal[e]
    cm.install(sim, cal)
    sim.render()
    first = maps_of(sim)
    small = maps_of(sim, 30, 20)
    half = host(sim, sim.depth(dtype="float16"))
    for m in first + small + (half,):
        assert m[e].tobytes() == m[e + 64].tobytes() == m[e + 70].tobytes(), m.dtype
    assert first[0][e].tobytes() != first[0][e + 1].tobytes() and first[2][e].any()
    again = maps_of(sim)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(first, again))
    sim.render()
    again = maps_of(sim)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(first, again))
    sim.close()


# ---- 5. the masked forms ---------------------------------------------------------------------------------------------------------------------

def test_masked_forms_write_the_selected_rows_only():
    import torch
    sim = cm.make_sim("pedestrians")
    cm.install(sim)
    sel = torch.zeros(cm.N, dtype=torch.uint8, device="cuda")
    sel[1::3] = 1
    on = sel.bool().cpu().numpy()
    torch.cuda.synchronize()
    sim.render()
    for size in ((cm.H, cm.W), (30, 20)):
        ref = maps_of(sim, *size)
        got = maps_of(sim, *size, mask=sel, out=fresh(cm.N, *size))                 # after a full render both forms are valid
        for g, r in zip(got, ref):
            assert (g[~on] == SENTINEL).all() and g[on].tobytes() == r[on].tobytes()
    ref = maps_of(sim)
    sim.render(mask=sel)                                     # the same state: the selected rows come out as before
    d, l, i = fresh(cm.N, cm.H, cm.W)
    for what, t in (("depth", d), ("labels", l), ("instances", i)):
        assert raw(sim, what, t, FLAG) == _ffi.E_STATE       # after a masked pass: the masked form only, with the flag as without
    got = maps_of(sim, mask=sel, out=(d, l, i))
    for g, r in zip(got, ref):
        assert (g[~on] == SENTINEL).all() and g[on].tobytes() == r[on].tobytes() and not (g[on] == SENTINEL).all()
    sim.close()


# ---- 6. the ABI's edges ----------------------------------------------------------------------------------------------------------------------

def test_the_flag_is_opt_in_and_changes_nothing_without_tables():
    import torch
    n = 8
    sim = cm.make_sim("pedestrians", n, None)
    sim.render()
    # without tables: the bytes of flags 0 (the folded fisheye), and DEPTH_F16 beside it
    assert all(x.tobytes() == y.tobytes() for x, y in zip(raw_maps(sim, 0, cm.H, cm.W), raw_maps(sim, FLAG, cm.H, cm.W)))
    d, l, i = fresh(n, cm.H, cm.W)
    for what, t in (("depth", d), ("labels", l), ("instances", i)):      # the flag beside an unknown bit: 2 for depth, 1 for the byte maps, a high one
        for bad in (2 if what == "depth" else 1, 0x200, 0x80000000):
            assert raw(sim, what, t, FLAG | bad) == _ffi.E_INVALID, (what, bad)
    sim.sync()
    assert bool((d == SENTINEL).all()) and bool((l == SENTINEL).all()) and bool((i == SENTINEL).all())
    cm.install(sim)
    sim.render()
    sel = torch.ones(n, dtype=torch.uint8, device="cuda")
    for what, t in (("depth", d), ("labels", l), ("instances", i)):      # tables installed, flags 0: the refusal stays
        assert raw(sim, what, t, 0) == _ffi.E_STATE and raw(sim, what, t, 0, mask=sel) == _ffi.E_STATE, what
        assert raw(sim, what, t, FLAG | 0x200) == _ffi.E_INVALID
    assert raw(sim, "depth", d, _ffi.DEPTH_F16) == _ffi.E_STATE
    sim.sync()
    assert bool((d == SENTINEL).all()) and bool((l == SENTINEL).all()) and bool((i == SENTINEL).all())
    assert raw(sim, "depth", d, FLAG) == _ffi.OK
    h16 = torch.full((n, cm.H, cm.W), float(SENTINEL), dtype=torch.float16, device="cuda")
    assert raw(sim, "depth", h16, _ffi.DEPTH_F16 | FLAG) == _ffi.OK
    sim.sync()
    assert torch.equal(h16.view(torch.int16), d.half().view(torch.int16))          # the half rounding of the float32 result, inf included
    assert not bool((d == SENTINEL).any())
    lab2 = torch.full_like(l, SENTINEL)                                         # one classification fills both maps under the flag too
    assert raw(sim, "instances", i, FLAG, labels=lab2) == _ffi.OK and raw(sim, "labels", l, FLAG) == _ffi.OK
    sim.sync()
    assert torch.equal(l, lab2) and bool((i > 0).any())
    sim.close()
