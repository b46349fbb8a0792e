"""The expected depth map of dtsim_depth (include/dtsim.h), from the oracle as it stands, and the inputs both depth tests share.

The quantity: per camera pixel the smallest, over the four MSAA samples of the frame's source pixel, of the eye depth of the nearest opaque
surface -- np.minimum.reduce of the four per-sample depth buffers raster.render_rectilinear(return_depth=True) returns (inf = clear colour);
through the fisheye by nearest source pixel, as raster.distort_ids moves ids, with 0 where a pixel has no source; a smaller map is the slice
full[sy // 2::sy, sx // 2::sx].

Comparisons are in INVERSE depth (1 / d, 1 / inf = 0): 1 / t of a plane hit is linear in the ray direction, so float32 error does not blow
up at the horizon the way t does.  Border pixels (depth 0) are compared for exact equality, not inverted.

The cases (scene, frame size, one init state per env, steps, walking duckies' wait) are stated here once: tests/test_depth_model_host.py
runs the oracle on them twice to DERIVE the tolerance (INV_DEPTH_NUDGE_MAX below is its recorded result, which that test holds to the
derivation), tests/test_gpu_depth.py puts the same states on the device."""
import functools
import math
from typing import NamedTuple, Optional

import numpy as np

import frame_parity as fp
from dtsim import _ffi, assets
from dtsim import distortion as pdist
from oracle import raster, sim as osim
from util import EXT

W, H = 160, 120
STRIDES = ((1, 1), (2, 2), (4, 8))         # (sy, sx): the full map, 60 x 80 and 30 x 20
BLUE_SKY = (0.45, 0.82, 1.0)

# Largest |delta(1 / d)| (1 / m) between the oracle's map of a case and its map from the float32-rounded pose scaled by 1 + 2e-7, over the
# pixels whose four samples agree on the surface in both runs, over every case below (profiles/depth_parity.txt has the per-case values).
# test_depth_model_host.py recomputes it and fails if this line no longer states it.  The device is held to 4 x this: the factor covers its
# float32 ray set-up against the oracle's float64.
INV_DEPTH_NUDGE_MAX = 1.090720e-04          # ("pedestrians" env 1: a duckie's steep triangles 0.4 m away; every plane pixel: 0)
INV_DEPTH_TOL = 4 * INV_DEPTH_NUDGE_MAX
# The share of pixels that may lie beyond the tolerance: a sample whose coverage flips at a silhouette or a tile seam.
CAP_PLANE, CAP_MESH = fp.ORACLE_PLANE.gt1, fp.ORACLE_MESH.gt1


# ---- the model -----------------------------------------------------------------------------------------------------------------------

def min_depth(depths):
    """[H, W] depth of the four per-sample buffers: the smallest."""
    return np.minimum.reduce(depths)


def remap_nearest(a, rmap, fill=0.0):
    """`a` through the fisheye as raster.distort_ids moves ids (nearest source pixel), `fill` where the source lies outside the frame."""
    rmapx, rmapy = rmap
    h, w = a.shape
    sx = np.rint(rmapx.astype(np.float64)).astype(np.int64)
    sy = np.rint(rmapy.astype(np.float64)).astype(np.int64)
    ok = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
    out = np.full_like(a, fill)
    out[ok] = a[sy[ok], sx[ok]]
    return out


def strided(full, sy, sx):
    """The small map of a full one ([..., H, W]): output pixel (i, j) is camera pixel (i sy + sy // 2, j sx + sx // 2)."""
    return full[..., sy // 2::sy, sx // 2::sx]


def oracle_buffers(cam, scene, obj_states):
    """(the four per-sample depth buffers, the four per-sample object-id arrays) of the rectilinear frame."""
    _, depths, ids = raster.render_rectilinear(cam, scene, "pixel", obj_states, return_depth=True, return_ids=True)
    return np.stack(depths), np.stack(ids)


def expected(cam, scene, obj_states, rmap=None):
    """The full-size expected map of one env."""
    d = min_depth(oracle_buffers(cam, scene, obj_states)[0])
    return d if rmap is None else remap_nearest(d, rmap)


def surfaces(cam, depths, ids):
    """Per sample [4, H, W] which surface owns it: k >= 0 object k, -1 the tile plane, -2 the ground quad, -3 the clear colour.  Tile and
    ground (which the ids do not tell apart) by the height the hit lies below the camera: depth x the ray's downward slope is the camera's
    height above the tile plane, or 8 mm more."""
    Wc, Hc = cam.W, cam.H
    cols, rows = np.meshgrid(np.arange(Wc, dtype=np.float64), np.arange(Hc, dtype=np.float64))
    out = np.empty(depths.shape, np.int64)
    for q, (ox, oy) in enumerate(raster.SAMPLE_OFFSETS):
        ny = 1 - 2 * (rows + 0.5) / Hc - 2 * oy / Hc
        yla = ny * cam.ty * cam.cth - cam.sth
        with np.errstate(invalid="ignore"):
            below = depths[q] * -yla
        s = np.where(np.abs(below - cam.C[1]) < 0.5 * abs(raster.GROUND_Y), -1, -2)
        s = np.where(np.isinf(depths[q]), -3, s)
        out[q] = np.where(ids[q] >= 0, ids[q], s)
    return out


def silhouette(depths, srf):
    """Pixels with one to three samples on a mesh object, the nearest of them nearer than every other sample of the pixel by far more than
    the tolerance (in inverse depth): where the minimum and a vote differ."""
    k = (srf >= 0).sum(axis=0)
    on = np.where(srf >= 0, depths, np.inf).min(axis=0)
    off = np.where(srf < 0, depths, np.inf).min(axis=0)
    with np.errstate(invalid="ignore"):
        return (k >= 1) & (k <= 3) & (inv(on) - inv(off) > 100 * INV_DEPTH_TOL)


def inv(d):
    """1 / d with 1 / inf = 0; a border pixel (d = 0) gives inf, which compare() never reads."""
    with np.errstate(divide="ignore"):
        return 1.0 / np.asarray(d, dtype=np.float64)


def compare(got, want, tol, cap, ctx=None):
    """A device map against the expected one (same shape): border pixels (0) the same set on both sides; elsewhere |1/got - 1/want| <= tol on
    all but `cap` of the pixels.  Returns dict(beyond=share of pixels beyond tol, worst=largest difference within the tolerated pixels...)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (ctx, got.shape, want.shape)
    border = want == 0
    assert np.array_equal(got == 0, border), (ctx, "border pixels differ", int((got == 0).sum()), int(border.sum()))
    assert not np.isnan(got).any() and (got >= 0).all(), ctx
    err = np.where(border, 0.0, np.abs(inv(np.where(border, 1.0, got)) - inv(np.where(border, 1.0, want))))
    beyond = err > tol
    share = float(beyond.mean())
    out = dict(beyond=share, n_beyond=int(beyond.sum()), max_within=float(err[~beyond].max()), max=float(err.max()))
    assert share <= cap, (ctx, out, [tuple(int(v) for v in yx) for yx in np.argwhere(beyond)[:8]])
    return out


# ---- the cases -----------------------------------------------------------------------------------------------------------------------

class Case(NamedTuple):
    map_name: str
    W: int
    H: int
    dr: bool                       # per-env camera (domain randomisation)
    states: tuple                  # per env (x, z, angle, cam_height, cam_angle_deg, cam_fov_y_deg, (camera noise x, y, z))
    steps: int = 0                 # zero-action steps before the frame
    wait: Optional[float] = None   # the walking duckies' wait before their first walk, s (None: the map's)
    asset_tree: bool = False       # the test_town asset tree (frame_parity.asset_scene)
    mesh: bool = False

    @property
    def cap(self):
        return CAP_MESH if self.mesh else CAP_PLANE


DEFAULT_CAM = (osim.CAMERA_FLOOR_DIST, osim.CAMERA_ANGLE, float(osim.CAMERA_FOV_Y), (0.0, 0.0, 0.0))
# small_loop (5 x 5 tiles of 0.585 m): on the road, at a curve, and two looking off the map edge (the ground quad out to 50 m, then sky)
PLANE_POSES = ((1.0, 0.9, 0.3), (2.0, 1.1, -1.2), (0.9, 2.0, 2.2), (0.3, 1.5, math.pi), (2.6, 2.6, -0.8))


def _dr_cams(n, seed):
    """Per-env cameras as domain randomisation draws them: height, pitch and fov within +-10 %, a camera noise of millimetres."""
    rng = np.random.default_rng(seed)
    return [(DEFAULT_CAM[0] * rng.uniform(0.9, 1.1), DEFAULT_CAM[1] * rng.uniform(0.9, 1.1), DEFAULT_CAM[2] * rng.uniform(0.9, 1.1),
             tuple(float(v) for v in rng.uniform(-0.005, 0.005, 3))) for _ in range(n)]


def _facing(objs, picks, dist):
    """Poses `dist` in front of objects objs[k], k in picks, facing them, each from another side."""
    out = []
    for e, k in enumerate(picks):
        a = 0.7 * e + 0.2
        out.append((float(objs[k].pos[0] - dist * math.cos(a)), float(objs[k].pos[2] + dist * math.sin(a)), a))
    return out


@functools.lru_cache(maxsize=None)
def _town():
    return fp.asset_scene()                          # (scene, map data, mesh extents)


@functools.lru_cache(maxsize=None)
def _scene(map_name, asset_tree):
    return _town()[0] if asset_tree else fp.scene(map_name)


def case_of(ref):
    """The Case a model function is asked about: a name of CASES, or a Case of the caller's own (tests/rerender_model.py keeps its cases out
    of CASES, whose members test_depth_model_host.py derives the tolerance over).  A Case is hashable, so the caches below take either."""
    return ref if isinstance(ref, Case) else CASES[ref]


def scene_of(case_name):
    return _scene(case_of(case_name).map_name, case_of(case_name).asset_tree)


def _cases():
    planes = tuple(p + DEFAULT_CAM for p in PLANE_POSES)
    planes_dr = tuple(p + cam for p, cam in zip(PLANE_POSES, _dr_cams(len(PLANE_POSES), 11)))
    ped = _scene("loop_pedestrians", False).m.objects
    town = _town()[0].m.objects
    ped_states = tuple(p + DEFAULT_CAM for p in _facing(ped, (0, 1, 3, 6), 0.40))
    town_states = tuple(p + DEFAULT_CAM for p in _facing(town, range(len(town)), 0.45))
    return {
        "planes": Case("small_loop", W, H, False, planes),
        "planes_dr": Case("small_loop", W, H, True, planes_dr),
        "pedestrians": Case("loop_pedestrians", W, H, False, ped_states, steps=14, wait=0.2, mesh=True),
        "town": Case("test_town", W, H, False, town_states, asset_tree=True, mesh=True),
        "town_odd": Case("test_town", 90, 62, False, town_states[:4], asset_tree=True, mesh=True),
    }


CASES = _cases()


def init_states(case, n=None, period=None):
    """(_ffi.InitState * n): env e takes state e % len(case.states) -- with `period`, state (e % period) % len(case.states), so that envs e,
    e + period, e + 2 period ... share one."""
    n = len(case.states) if n is None else n
    out = (_ffi.InitState * n)()
    for e in range(n):
        x, z, ang, ch, ca, cf, noise = case.states[(e if period is None else e % period) % len(case.states)]
        st = out[e]
        st.pos[:] = [x, 0.0, z]
        st.angle, st.map_id, st.wheel_dist = ang, 0, osim.WHEEL_DIST
        st.cam_height, st.cam_angle_deg, st.cam_fov_y_deg = ch, ca, cf
        st.camera_noise[:] = list(noise)
        st.horizon_color[:] = list(BLUE_SKY)
        st.ground_color[:] = [0.15, 0.15, 0.15]
        st.light_pos[:] = [0.0, 3.0, 0.0, 1.0]
        st.light_ambient[:] = [0.25, 0.25, 0.25]
        st.light_diffuse[:] = [0.35, 0.35, 0.35]
    return out


@functools.lru_cache(maxsize=None)
def rmap(Wc, Hc, kind="fisheye"):
    """The per-pixel source map of BatchedSimulator(distortion=True): the simulator's fisheye, whose sources all lie inside the frame at these
    sizes (no border), or with kind="undistort" the rectify map of undistort=True (UndistortWrapper), which leaves a border without a source."""
    return (pdist.undistort_wrapper_maps if kind == "undistort" else pdist.distortion_maps)(Wc, Hc)


def _map_data(case):
    return _town()[1] if case.asset_tree else assets.get_map(case.map_name)


@functools.lru_cache(maxsize=None)
def host_objects(case_name):
    """Per env the oracle's object states (frame_parity.obj_states' form) after the case's steps, from the oracle's own physics: every env
    starts from the map's object poses, the walking duckies' wait shortened to case.wait, and stands still (zero actions)."""
    import copy
    case, sc = case_of(case_name), scene_of(case_name)
    if not sc.m.objects:
        return tuple(None for _ in case.states)
    if case.steps == 0:                              # nothing has moved: the map's own poses
        return tuple([dict(pos=np.array(ob.pos, dtype=np.float64), y_rot=float(ob.y_rot), visible=True) for ob in sc.m.objects] for _ in case.states)
    ext = _town()[2] if case.asset_tree else EXT
    out = []
    for (x, z, ang, *_rest) in case.states:
        o = osim.OracleSim(copy.deepcopy(_map_data(case)), ext, do_reset=False, max_steps=10 ** 6)
        o.wheel_dist = osim.WHEEL_DIST
        o.set_pose([x, 0.0, z], ang)
        for ob in o.map.objects:
            if case.wait is not None and not ob.static and ob.kind == "duckie":
                ob.pedestrian_wait_time = case.wait
        for _ in range(case.steps):
            o.step(np.zeros(2))
        st = []
        for ob in o.map.objects:
            p = ob.pos if ob.static else np.array([ob.center[0], ob.pos[1], ob.center[2]])
            st.append(dict(pos=np.array(p, dtype=np.float64), y_rot=float(ob.y_rot), visible=bool(ob.visible)))
        out.append(st)
    return tuple(out)


def host_camera(case, e, nudge=False):
    """The oracle's camera of env e of the case.  nudge: from the pose a float32 holds, the position scaled by 1 + 2e-7 (the perturbation
    of tests/crowd_scenes.py: of the size of the device's own rounding)."""
    st = init_states(case)[e]
    pos, ang = np.array(st.pos[:], dtype=np.float64), float(st.angle)
    if nudge:
        pos, ang = pos.astype(np.float32).astype(np.float64) * (1 + 2e-7), float(np.float32(ang))
    return fp.camera_of_state(st, pos, ang, case.W, case.H, case.dr)


@functools.lru_cache(maxsize=None)
def host_buffers(case_name, e, nudge=False):
    """(depths [4, H, W], surfaces [4, H, W]) of env e of the case on the oracle alone; cached and read-only."""
    case = case_of(case_name)
    cam = host_camera(case, e, nudge)
    depths, ids = oracle_buffers(cam, scene_of(case_name), host_objects(case_name)[e])
    srf = surfaces(cam, depths, ids)
    depths.setflags(write=False); srf.setflags(write=False)
    return depths, srf


def nudge_stats(case_name, e, tol=None):
    """The oracle's map of env e against its nudged self: dict(agree_max = largest |delta(1 / d)| over the pixels whose four samples agree
    on the surface in both runs, agree = how many such pixels, beyond = share of ALL pixels beyond `tol` (when given))."""
    d0, s0 = host_buffers(case_name, e)
    d1, s1 = host_buffers(case_name, e, True)
    agree = (s0 == s0[0]).all(axis=0) & (s1 == s1[0]).all(axis=0) & (s0[0] == s1[0])
    err = np.abs(inv(min_depth(d0)) - inv(min_depth(d1)))
    out = dict(agree_max=float(err[agree].max()), agree=int(agree.sum()), pixels=int(agree.size))
    if tol is not None:
        out["beyond"] = float((err > tol).mean())
    return out


def parity_report():
    """The text of profiles/depth_parity.txt: per case and env the oracle against its nudged self, the maximum and the tolerance."""
    lines = ["dtsim_depth: the tolerance of tests/test_gpu_depth.py, derived by tests/test_depth_model_host.py (python -c 'import depth_model as m; print(m.parity_report())')",
             "oracle/raster.py against itself from the float32-rounded pose scaled by 1 + 2e-7; inverse depth, 1 / m",
             "agree_max: largest |delta(1/d)| over the pixels whose four samples agree on the surface (tile / ground / sky / object k) in both runs",
             "beyond:    share of ALL pixels beyond the tolerance (4 x the maximum of agree_max); bound: a quarter of the cap", ""]
    rows, worst = [], 0.0
    for name, c in CASES.items():
        for e in range(len(c.states)):
            worst = max(worst, nudge_stats(name, e)["agree_max"])
    tol = 4 * worst
    for name, c in CASES.items():
        for e in range(len(c.states)):
            r = nudge_stats(name, e, tol)
            rows.append(f"{name:12s} env {e}  {c.W:3d} x {c.H:3d}  agree_max {r['agree_max']:.3e}  agreeing pixels {r['agree']:5d} / {r['pixels']:5d}  "
                        f"beyond {r['beyond']:.2e}  (cap / 4 = {c.cap / 4:.2e})")
    return "\n".join(lines + rows + ["", f"maximum   {worst:.6e}", f"tolerance {tol:.6e}  (4 x the maximum)"])
