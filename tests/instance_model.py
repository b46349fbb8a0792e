"""The expected instance map of dtsim_instances (include/dtsim.h), from the oracle alone; a numpy model of dtsim_boxes; and the inputs the
instance tests share.

The quantity: per camera pixel the owner of the sample that sets the depth -- of the four per-sample depth buffers of the oracle the sample
with the smallest depth (np.argmin: the lowest index on ties; a sky sample is inf, so it wins only when all four are sky); where its surface
(depth_model.surfaces) is object k >= 0 the value is k + 1, else 0.  k is the object's index in the scene's object list, hidden objects
included (they keep their slot and never appear).  Through the fisheye and the rectify map by dm.remap_nearest(fill=0), smaller maps by
dm.strided.

SURE pixels, where the device must agree exactly: the four samples lie on one surface, in the oracle's run and in its nudged run (the
float32-rounded pose scaled by 1 + 2e-7), and on the same one in both -- the `agree` term of label_model.expected_with.  Elsewhere
(silhouettes, and where two meshes share a depth range) another id is allowed on at most Case.cap of ALL the map's pixels, the cap the label
tests use: fp.ORACLE_MESH.gt1 with meshes in view, fp.ORACLE_PLANE.gt1 without.  tests/test_instance_model_host.py holds the oracle against its
nudged self to a quarter of that on every case (profiles/instances_parity.txt).

The cases: "planes" (no object: all zero), "pedestrians", "town", "town_odd" (90 x 62) of dm.CASES; three crowd views of tests/crowd_scenes.py
at 160 x 120 -- "far" (64 objects, dozens per raster tile), "side" (two meshes sharing a depth range), "inside2" (every third object hidden);
and two maps whose object lists differ, for the envs of one simulator that stand on different maps."""
import functools
from typing import NamedTuple, Optional

import numpy as np

import crowd_scenes as cs
import depth_model as dm
import frame_parity as fp
import label_model as lm  # noqa: F401  (the label tests' model: the sure mask's `agree` term is stated there)
from dtsim import _ffi

MAX_OBJECTS = _ffi.MAX_OBJECTS
CROWD_W, CROWD_H = 160, 120
DM_CASES = ("planes", "pedestrians", "town", "town_odd")
CROWD_VIEWS = ("far", "side", "inside2")
# one simulator, two resident maps, envs alternating: env e stands on TWO_MAPS[e % 2], 0.40 m in front of object TWO_PICKS[e % 2][e // 2] of it
TWO_MAPS = ("loop_only_duckies", "small_loop_only_duckies")
TWO_PICKS = ((5, 7, 2), (1, 3, 0))


class Case(NamedTuple):
    W: int
    H: int
    n_envs: int
    cap: float
    view: Optional[str] = None          # a crowd view
    dm_case: Optional[dm.Case] = None    # a case in depth_model's form (dm.CASES, or one of TWO_MAPS)
    dm_name: Optional[str] = None        # its name in dm.CASES


def _two_map_case(m):
    objs = fp.scene(TWO_MAPS[m]).m.objects
    states = tuple(p + dm.DEFAULT_CAM for p in dm._facing(objs, TWO_PICKS[m], 0.40))
    return dm.Case(TWO_MAPS[m], dm.W, dm.H, False, states, mesh=True)


def _cases():
    out = {n: Case(dm.CASES[n].W, dm.CASES[n].H, len(dm.CASES[n].states), dm.CASES[n].cap, dm_case=dm.CASES[n], dm_name=n) for n in DM_CASES}
    for v in CROWD_VIEWS:
        out["crowd_" + v] = Case(CROWD_W, CROWD_H, 1, fp.ORACLE_MESH.gt1, view=v)
    for m, name in enumerate(TWO_MAPS):
        c = _two_map_case(m)
        out["two_" + name] = Case(c.W, c.H, len(c.states), c.cap, dm_case=c)
    return out


CASES = _cases()
MODEL_CASES = tuple(n for n in CASES if not n.startswith("two_"))          # the cases of the issue's lists; the two-map pair has its own test
CROWD_CASES = tuple("crowd_" + v for v in CROWD_VIEWS)


def case_of(name):
    """A name of CASES, or a dm.Case of the caller's own (dm.case_of), in this module's form."""
    if isinstance(name, dm.Case):
        return Case(name.W, name.H, len(name.states), name.cap, dm_case=name, dm_name=name)
    return CASES[name]


@functools.lru_cache(maxsize=None)
def host_buffers(name, e, nudge=False):
    """(depths [4, H, W], surfaces [4, H, W]) of env e of the case, on the oracle alone; cached, read-only."""
    c = case_of(name)
    if c.dm_name is not None:
        return dm.host_buffers(c.dm_name, e, nudge)
    if c.view is not None:
        cam, sc, objs = cs.camera(c.view, c.W, c.H, False, nudge), cs.scene(), cs.obj_states(c.view)
    else:
        sc = fp.scene(c.dm_case.map_name)
        cam = dm.host_camera(c.dm_case, e, nudge)
        objs = [dict(pos=np.array(o.pos, dtype=np.float64), y_rot=float(o.y_rot), visible=True) for o in sc.m.objects]
    depths, ids = dm.oracle_buffers(cam, sc, objs)
    srf = dm.surfaces(cam, depths, ids)
    depths.setflags(write=False); srf.setflags(write=False)
    return depths, srf


def instances_of(depths, srf):
    """[H, W] int64: k + 1 of the nearest sample's surface where it is object k, else 0."""
    k = np.take_along_axis(srf, np.argmin(depths, axis=0)[None], axis=0)[0]
    return np.where(k >= 0, k + 1, 0)


@functools.lru_cache(maxsize=None)
def expected(name, e, kind=None, nudge=False):
    """(instances [H, W] uint8, sure [H, W] bool) of env e of the case: full size, through the source map `kind` (None / "fisheye" /
    "undistort") by nearest source pixel with id 0 -- and sure -- where a pixel has no source.  Cached, read-only."""
    c = case_of(name)
    d0, s0 = host_buffers(name, e, False)
    d1, s1 = host_buffers(name, e, True)
    inst = instances_of(d1, s1) if nudge else instances_of(d0, s0)
    sure = (s0 == s0[0]).all(axis=0) & (s1 == s1[0]).all(axis=0) & (s0[0] == s1[0])
    assert inst.min() >= 0 and inst.max() <= MAX_OBJECTS
    if kind is not None:
        rm = dm.rmap(c.W, c.H, kind)
        inst = dm.remap_nearest(inst, rm, fill=0)
        sure = dm.remap_nearest(sure, rm, fill=True)
    inst = inst.astype(np.uint8)
    inst.setflags(write=False); sure.setflags(write=False)
    return inst, sure


def compare(got, want, sure, cap, ctx=None):
    """A device map against the expected one: exact equality on the sure pixels; elsewhere a different id on at most `cap` of ALL the map's
    pixels.  Returns dict(off=share of pixels that differ, n_off, unsure=share of pixels not sure)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape == sure.shape and got.dtype == np.uint8, (ctx, got.shape, want.shape, got.dtype)
    diff = got != want
    out = dict(off=float(diff.mean()), n_off=int(diff.sum()), unsure=float((~sure).mean()))
    assert not (diff & sure).any(), (ctx, out, "sure pixels differ", [(int(y), int(x), int(got[y, x]), int(want[y, x])) for y, x in np.argwhere(diff & sure)[:8]])
    assert out["off"] <= cap, (ctx, out, [(int(y), int(x), int(got[y, x]), int(want[y, x])) for y, x in np.argwhere(diff)[:8]])
    return out


def nudge_share(name, e):
    """The oracle's map of env e against its nudged self: dict(off = share of ALL pixels with another id, unsure = share not sure,
    sure_off = differing pixels ON the sure mask)."""
    a, sure = expected(name, e)
    b, _ = expected(name, e, None, True)
    diff = a != b
    return dict(off=float(diff.mean()), n_off=int(diff.sum()), unsure=float((~sure).mean()), sure_off=int((diff & sure).sum()), pixels=int(diff.size))


def crowding(inst):
    """(the number of distinct non-zero ids of an [H, W] map, the number of 4-adjacent pixel pairs that hold two different non-zero ids):
    how many objects a view shows, and how much of their outline is against another object."""
    a = np.asarray(inst).astype(np.int64)
    pairs = int(((a[:, 1:] != a[:, :-1]) & (a[:, 1:] > 0) & (a[:, :-1] > 0)).sum() + ((a[1:] != a[:-1]) & (a[1:] > 0) & (a[:-1] > 0)).sum())
    return int(len(np.unique(a[a > 0]))), pairs


# What the oracle shows in the crowd views at 160 x 120 (distinct ids, adjacent pairs of two ids), as tests/test_instance_model_host.py prints
# it; that test asserts at least half of each, so that a change to crowd_scenes.py cannot silently take the occlusions out of the views.
CROWD_ORACLE = {"far": (56, 495), "side": (49, 619), "inside2": (9, 25)}


# ---- the cases on a device (the GPU tests) ------------------------------------------------------------------------------------------------

def fisheye_kw(kind):
    return {None: {}, "fisheye": dict(distortion=True), "undistort": dict(distortion=True, undistort=True)}[kind]


def case_of_env(name, e, period=None):
    """Which env of the case's oracle runs env e of a device batch shows: e % n_envs, or with `period` (e % period) % n_envs."""
    return (e if period is None else e % period) % CASES[name].n_envs


def make_sim(name, n=None, period=None, kind=None):
    """The case's states on a device, env e showing case_of_env(name, e, period), through the source map `kind`; stepped as a dm case says.
    A crowd case needs the map "crowd" (cs.crowd_map()) registered in dtsim.assets.MAPS; with a crowd case and n > 1, env e shows view
    CROWD_VIEWS[case_of_env] -- `name` then only sets the size.  Checked: the device holds the object states the oracle's runs were made from."""
    from dtsim import BatchedSimulator
    c = CASES[name]
    n = c.n_envs if n is None else n
    args = dict(camera_width=c.W, camera_height=c.H, distortion=False, domain_rand=False, seed=1, max_steps=10 ** 6, do_reset=False)
    args.update(fisheye_kw(kind))
    if c.view is not None:
        views = [c.view if n == 1 else CROWD_VIEWS[(e if period is None else e % period) % len(CROWD_VIEWS)] for e in range(n)]
        sim = BatchedSimulator("crowd", n, **args)
        sim.reset(states=cs.init_states(views))
        cs.write_env_state(sim, views)
        sim.views = views
        for e in sorted({0, n - 1}):
            dev, want = fp.obj_states(sim, e, cs.scene()), cs.obj_states(views[e])
            assert all(np.array_equal(a["pos"], b["pos"]) and a["y_rot"] == b["y_rot"] and a["visible"] == b["visible"] for a, b in zip(dev, want)), (name, e)
        return sim
    d = c.dm_case
    if d.asset_tree:
        args["asset_root"] = fp.ASSETS
    sim = BatchedSimulator(d.map_name, n, **args)
    sim.reset(states=dm.init_states(d, n, period))
    if d.wait is not None:
        par = sim.read(_ffi.FIELD_OBJ_PARAMS)                 # [N, MAX_DYNAMIC, (vel, wait_time, wiggle)]
        par[:, :, 1] = d.wait
        sim.write(_ffi.FIELD_OBJ_PARAMS, par)
    if d.steps:
        sim.step(np.zeros((d.steps, n, 2), np.float32), n_steps=d.steps)
    sc = dm._scene(d.map_name, d.asset_tree)
    if sc.m.objects and c.dm_name is not None:
        objs = dm.host_objects(c.dm_name)
        for e in range(min(n, c.n_envs)):
            for got, w in zip(fp.obj_states(sim, e, sc), objs[e]):
                assert np.allclose(got["pos"], w["pos"], rtol=0, atol=1e-9) and abs(got["y_rot"] - w["y_rot"]) <= 1e-7 and got["visible"] == w["visible"], (name, e)
    return sim


def make_two_map_sim(kind=None):
    """One simulator holding both TWO_MAPS, 6 envs: env e on map e % 2 at state e // 2 of that map's case.  Returns (sim, [(case name, env
    of the case)] per device env)."""
    from dtsim import BatchedSimulator
    cases = [CASES["two_" + m].dm_case for m in TWO_MAPS]
    n = 2 * len(cases[0].states)
    st = (_ffi.InitState * n)()
    per = [dm.init_states(c) for c in cases]
    for e in range(n):
        st[e] = per[e % 2][e // 2]
        st[e].map_id = e % 2
    args = dict(camera_width=dm.W, camera_height=dm.H, distortion=False, domain_rand=False, seed=1, max_steps=10 ** 6, do_reset=False)
    args.update(fisheye_kw(kind))
    sim = BatchedSimulator(list(TWO_MAPS), n, **args)
    sim.reset(states=st)
    assert [m for m in sim.map_names] == list(TWO_MAPS)
    return sim, [("two_" + TWO_MAPS[e % 2], e // 2) for e in range(n)]


# ---- dtsim_boxes -------------------------------------------------------------------------------------------------------------------------

def box_model(inst):
    """[..., MAX_OBJECTS, 5] int32 of an [..., h, w] id map: row k = x0, y0, x1, y1, n of id k + 1 -- n pixels, columns [x0, x1), rows
    [y0, y1) their tight bound; all 0 when the id is absent.  Id 0 and ids above MAX_OBJECTS are ignored."""
    a = np.asarray(inst)
    lead = a.shape[:-2]
    flat = a.reshape((-1,) + a.shape[-2:])
    big = np.iinfo(np.int32).max
    out = np.zeros((flat.shape[0], MAX_OBJECTS, 5), np.int32)
    for e, m in enumerate(flat):
        ys, xs = np.nonzero((m >= 1) & (m <= MAX_OBJECTS))
        k = m[ys, xs].astype(np.int64) - 1
        lo = np.full((2, MAX_OBJECTS), big, np.int64)
        hi = np.zeros((2, MAX_OBJECTS), np.int64)
        np.minimum.at(lo[0], k, xs); np.minimum.at(lo[1], k, ys)
        np.maximum.at(hi[0], k, xs + 1); np.maximum.at(hi[1], k, ys + 1)
        n = np.bincount(k, minlength=MAX_OBJECTS)
        out[e] = np.where(n[:, None] > 0, np.stack([lo[0], lo[1], hi[0], hi[1], n], axis=1), 0)
    return out.reshape(lead + (MAX_OBJECTS, 5))


def box_brute(m):
    """box_model of one [h, w] map by a plain loop over its pixels."""
    out = np.zeros((MAX_OBJECTS, 5), np.int64)
    h, w = m.shape
    for y in range(h):
        for x in range(w):
            k = int(m[y, x])
            if k < 1 or k > MAX_OBJECTS:
                continue
            r = out[k - 1]
            if r[4] == 0:
                r[:4] = (x, y, x + 1, y + 1)
            else:
                r[:4] = (min(r[0], x), min(r[1], y), max(r[2], x + 1), max(r[3], y + 1))
            r[4] += 1
    return out.astype(np.int32)


def check_boxes_against_oracle(boxes, want, sure, ctx=None):
    """A device box table [MAX_OBJECTS, 5] of one env against the oracle's map: for every id the box contains the bounding box of the sure
    pixels of that id, and n lies between the number of sure pixels of the id and the number of expected pixels of it plus ALL unsure pixels."""
    unsure = int((~sure).sum())
    for k in range(MAX_OBJECTS):
        x0, y0, x1, y1, n = (int(v) for v in boxes[k])
        core = (want == k + 1) & sure
        lo, hi = int(core.sum()), int((want == k + 1).sum()) + unsure
        assert lo <= n <= hi, (ctx, k + 1, n, lo, hi)
        if lo:
            ys, xs = np.nonzero(core)
            assert x0 <= xs.min() and y0 <= ys.min() and x1 >= xs.max() + 1 and y1 >= ys.max() + 1, (ctx, k + 1, (x0, y0, x1, y1))


def parity_report():
    """The text of profiles/instances_parity.txt."""
    lines = ["dtsim_instances: what tests/test_gpu_instances.py allows off the sure mask, checked on the oracle by tests/test_instance_model_host.py "
             "(python -c 'import instance_model as m; print(m.parity_report())')",
             "oracle/raster.py against itself from the float32-rounded pose scaled by 1 + 2e-7",
             "off:    share of ALL pixels whose id differs between the two runs; bound: a quarter of the cap",
             "unsure: share of pixels off the sure mask (the four samples on several surfaces in either run)",
             "ids:    distinct non-zero ids in the expected map;  pairs: 4-adjacent pixel pairs holding two different non-zero ids", ""]
    for name, c in CASES.items():
        for e in range(c.n_envs):
            r = nudge_share(name, e)
            ids, pairs = crowding(expected(name, e)[0])
            lines.append(f"{name:28s} env {e}  {c.W:3d} x {c.H:3d}  off {r['off']:.2e} ({r['n_off']:2d} px)  sure_off {r['sure_off']}  unsure {r['unsure']:.3f}  "
                         f"(cap / 4 = {c.cap / 4:.2e})  ids {ids:2d}  pairs {pairs:4d}")
    return "\n".join(lines)
