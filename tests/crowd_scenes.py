"""Deterministic crowd views shared by tests/test_crowd_scenes_host.py (the oracle alone: do the inputs reach what they are meant to
reach?) and tests/test_gpu_crowd.py (k_obj_setup -> the <OBJ> rasters -> k_resolve_obj against the oracle, object by object).

Map "crowd": the small_loop tiles with the per-map object limits of include/dtsim.h -- 56 static duckies seeded into the patch
x in [1.2, 2.6], z in [1.1, 1.9] (tile units) with seeded rotations, heights mixed over 0.04 / 0.06 / 0.12 m and four of 0.30 m (tall
enough for a close one to be cut by the top border), and 8 walking duckies on the line z = 1.5, x = 1.3 + 0.15 k (objects 56 .. 63).  Several
interpenetrate: the z-buffer, not the draw order, decides between them.  Map "empty": the plain small_loop.
What is arranged so that "far" -- a camera 0.108 m above the floor looking over the whole crowd -- still sees most objects with a countable
interior: the seeded x is denser towards that camera (2.6 - 1.4 u^1.5), a duckie's height goes by its x (the small ones in front, 0.12 m
-- taller than the camera stands, so it hides whatever stands behind it -- only in the last third, the 0.30 m ones in the last quarter), and
the walkers, which stand in one line along the view axis, grow with their distance so that each looks over the one in front of it.

Four views, explicit poses (no reset() sampling):
  "far"      from outside the patch along -x: every object of the map is live, up to dozens of boxes in one raster tile;
  "side"     across the patch from the lane below it; two walkers are moved onto static duckies and turned (DTSIM_FIELD_OBJ_CENTER /
             DTSIM_FIELD_OBJ_YROT), so two meshes share their depth range;
  "inside"   from the middle of the patch: close-ups that fill most of the frame, triangles across the near plane and behind the camera;
  "inside2"  another close-up, with every third object hidden (DTSIM_FIELD_OBJ_VISIBLE).
The oracle's frames and per-sample object ids are computed once per (view, mode, size, fisheye, domain randomisation) and cached: treat
them as read-only.
"""
import functools
import math

import numpy as np

import frame_parity as fp
from dtsim import _ffi, assets
from dtsim import distortion as pdist
from oracle import raster, sim as osim
from util import EXT

TS = 0.585
VIEWS = ("far", "side", "inside", "inside2")
POSES = {"far": (3.4, 1.5, math.pi), "side": (1.9, 0.6, -math.pi / 2), "inside": (1.9, 1.5, math.pi), "inside2": (1.6, 1.3, 0.7)}   # x, z (tiles), angle
N_STATIC, N_WALKERS = _ffi.MAX_STATIC, _ffi.MAX_DYNAMIC
HEIGHTS = (0.04, 0.06, 0.12)                            # static heights: 0.12 where x < X_BIG, 0.04 where x > X_SMALL
SEED, X_BIG, X_SMALL, X_POWER = 31, 1.67, 2.13, 1.5
WALKER_H = (0.208, 0.168, 0.134, 0.104, 0.080, 0.0615, 0.048, 0.04)     # from "far": the top of walker k stands 0.03 rad above that of walker k + 1
TALL, TALL_AT = 0.30, (7, 20, 33, 46)                   # static objects of 0.30 m
HIDDEN = tuple(range(0, N_STATIC + N_WALKERS, 3))       # "inside2": these objects are invisible
MOVED = {5: (13, 90.0), 6: (25, 65.0)}                  # "side": walker slot -> (the static duckie it stands in, its y_rot relative to that one's)

# per-view domain randomisation (the "v3dr" case): camera height / angle / fov factors within the ranges reset() draws from, camera noise,
# a directional light (w = 0, as reset() draws it), per-channel ambient / diffuse / ground / horizon
DR = {
    "far": dict(cam=(1.05, 0.85, 1.10), noise=(0.004, -0.003, 0.002), light=(120.0, 180.0, -90.0), ambient=(0.22, 0.27, 0.30), diffuse=(0.55, 0.30, 0.12),
                ground=(0.12, 0.17, 0.19), horizon=(0.60, 0.70, 0.30)),
    "side": dict(cam=(0.93, 1.15, 0.90), noise=(-0.005, 0.005, -0.001), light=(-140.0, 215.0, 30.0), ambient=(0.30, 0.20, 0.25), diffuse=(0.10, 0.45, 0.65),
                 ground=(0.18, 0.11, 0.15), horizon=(0.45, 0.85, 0.95)),
    "inside": dict(cam=(1.08, 1.05, 1.20), noise=(0.001, 0.002, 0.005), light=(10.0, 171.0, 149.0), ambient=(0.25, 0.31, 0.18), diffuse=(0.35, 0.02, 0.60),
                   ground=(0.15, 0.15, 0.12), horizon=(0.14, 0.20, 0.10)),
    "inside2": dict(cam=(0.92, 0.80, 0.82), noise=(-0.002, -0.004, -0.005), light=(-60.0, 200.0, -120.0), ambient=(0.19, 0.19, 0.32), diffuse=(0.69, 0.50, 0.33),
                    ground=(0.10, 0.19, 0.16), horizon=(0.95, 0.80, 1.00)),
}


def crowd_map():
    rng = np.random.default_rng(SEED)
    md = assets.get_map("small_loop")
    objs = []
    for i in range(N_STATIC):
        x, z, rot = 2.6 - 1.4 * float(rng.uniform(0, 1)) ** X_POWER, float(rng.uniform(1.1, 1.9)), float(rng.uniform(0, 360))
        if i in TALL_AT:                    # at the end of the patch that is far from "far" and in front of "inside": they hide little, and one is close
            x, h = 1.2 + (x - 1.2) * 0.25, TALL
        else:                               # the small ones towards "far"'s camera, so that most objects keep a countable interior there
            h = HEIGHTS[2] if x < X_BIG else HEIGHTS[0] if x > X_SMALL else HEIGHTS[1]
        objs.append(dict(kind="duckie", pos=[x, z], rotate=rot, height=h, static=True))
    objs += [dict(kind="duckie", pos=[1.3 + 0.15 * k, 1.5], rotate=90.0, height=WALKER_H[k], static=False) for k in range(N_WALKERS)]
    md["objects"] = objs
    return md


def map_data(name):
    return crowd_map() if name == "crowd" else assets.get_map("small_loop")


@functools.lru_cache(maxsize=None)
def scene(name="crowd"):
    om = osim.OracleMap(map_data(name), EXT)
    tex = {k: assets.get_texture(k) for k in {t["kind"] for t in om.grid if t is not None}}
    return raster.Scene(om, tex, {"duckie": assets.get_mesh("duckie"), "*": assets.get_mesh("*")})


def init_state(view, dr=False, map_id=0):
    st = _ffi.InitState()
    x, z, ang = POSES[view]
    st.pos[:] = [x * TS, 0.0, z * TS]
    st.angle, st.map_id, st.wheel_dist = ang, map_id, osim.WHEEL_DIST
    st.cam_height, st.cam_angle_deg, st.cam_fov_y_deg = osim.CAMERA_FLOOR_DIST, osim.CAMERA_ANGLE, float(osim.CAMERA_FOV_Y)
    st.horizon_color[:] = [0.45, 0.82, 1.0]; st.ground_color[:] = [0.15, 0.15, 0.15]
    st.light_pos[:] = [0.0, 3.0, 0.0, 1.0]; st.light_ambient[:] = [0.25] * 3; st.light_diffuse[:] = [0.35] * 3
    if dr:
        d = DR[view]
        st.cam_height, st.cam_angle_deg, st.cam_fov_y_deg = (a * b for a, b in zip((st.cam_height, st.cam_angle_deg, st.cam_fov_y_deg), d["cam"]))
        st.camera_noise[:] = d["noise"]
        st.light_pos[:] = list(d["light"]) + [0.0]
        st.light_ambient[:], st.light_diffuse[:] = d["ambient"], d["diffuse"]
        st.ground_color[:], st.horizon_color[:] = d["ground"], d["horizon"]
    return st


def init_states(views, dr=False, map_ids=None):
    """(_ffi.InitState * len(views)): env e looks through views[e], on map map_ids[e] (default 0)."""
    out = (_ffi.InitState * len(views))()
    for e, view in enumerate(views):
        out[e] = init_state(view, dr, 0 if map_ids is None else int(map_ids[e]))
    return out


def obj_states(view):
    """The oracle's per-object render state in `view`: what frame_parity.obj_states reads back from a device after write_env_state."""
    objs = scene().m.objects
    out = [dict(pos=np.array(o.pos, dtype=np.float64), y_rot=float(o.y_rot), visible=True) for o in objs]
    if view == "inside2":
        for k in HIDDEN:
            out[k]["visible"] = False
    if view == "side":
        for slot, (onto, turn) in MOVED.items():
            w = out[N_STATIC + slot]
            w["pos"] = np.array([objs[onto].pos[0], w["pos"][1], objs[onto].pos[2]])
            w["y_rot"] = float(objs[onto].y_rot + turn)
    return out


def write_env_state(sim, views):
    """The per-env part of the views, through the C-ABI: env e gets views[e]'s (None: an env that is not on the crowd map, left alone)."""
    vis, cen, yrot = sim.read(_ffi.FIELD_OBJ_VISIBLE), sim.read(_ffi.FIELD_OBJ_CENTER), sim.read(_ffi.FIELD_OBJ_YROT)
    for e, view in enumerate(views):
        if view is None:
            continue
        for k, s in enumerate(obj_states(view)):
            vis[e, k] = 1 if s["visible"] else 0
            if k >= N_STATIC:
                cen[e, k - N_STATIC] = s["pos"][[0, 2]]
                yrot[e, k - N_STATIC] = s["y_rot"]
    sim.write(_ffi.FIELD_OBJ_VISIBLE, vis)
    sim.write(_ffi.FIELD_OBJ_CENTER, cen)
    sim.write(_ffi.FIELD_OBJ_YROT, yrot)


def camera(view, W, H, dr=False, nudge=False):
    """The oracle's camera of `view`.  nudge: the pose a float32 would hold, the position scaled by (1 + 2e-7) -- a perturbation of the
    size of the device's own rounding, for measuring how far the oracle's frame moves under it."""
    st = init_state(view, dr)
    pos, ang = np.array(st.pos[:], dtype=np.float64), float(st.angle)
    if nudge:
        pos, ang = pos.astype(np.float32).astype(np.float64) * (1 + 2e-7), float(np.float32(ang))
    return fp.camera_of_state(st, pos, ang, W, H, dr)


@functools.lru_cache(maxsize=None)
def rmap(W, H):
    return pdist.distortion_maps(W, H)


@functools.lru_cache(maxsize=None)
def oracle_view(view, mode, W, H, fisheye, dr=False, nudge=False):
    """(frame uint8 [H, W, 3], the four per-sample object-id arrays) of the crowd map in `view`; cached and read-only."""
    img, ids = raster.render_obs(camera(view, W, H, dr, nudge), scene(), mode, rmap(W, H) if fisheye else None, obj_states=obj_states(view), return_ids=True)
    ids = np.stack(ids)
    img.setflags(write=False); ids.setflags(write=False)
    return img, ids


# ---- what the views reach (the host test's measurements) ---------------------------------------------------------------------------

def screen_geometry(view, W, H):
    """Of every visible object in `view`, without the fisheye: (boxes {object: (x0, y0, x1, y1) of its drawn triangles' screen box in pixels, inclusive,
    clipped to the frame, only where it meets the frame}, the number of its mesh triangles that straddle the near plane: a vertex nearer than it,
    another beyond)."""
    cam = camera(view, W, H)
    boxes, straddle = {}, 0
    for Vw, _, _, _, _, k in raster._object_instances(scene(), obj_states(view)):
        Pe = cam.to_eye(Vw)
        w = -Pe[..., 2]
        straddle += int(((w > raster.NEAR).any(axis=1) & (w <= raster.NEAR).any(axis=1)).sum())
        ok = (w > raster.NEAR).all(axis=1)
        if not ok.any():
            continue
        sx = (Pe[ok][..., 0] / w[ok] / cam.tx + 1) * 0.5 * W
        sy = (1 - Pe[ok][..., 1] / w[ok] / cam.ty) * 0.5 * H
        x0, x1 = max(int(math.floor(sx.min())), 0), min(int(math.ceil(sx.max())) - 1, W - 1)
        y0, y1 = max(int(math.floor(sy.min())), 0), min(int(math.ceil(sy.max())) - 1, H - 1)
        if x0 <= x1 and y0 <= y1:
            boxes[k] = (x0, y0, x1, y1)
    return boxes, straddle


def box_pixels(boxes, W, H):
    """[H, W] bool: inside some object's screen box."""
    m = np.zeros((H, W), bool)
    for x0, y0, x1, y1 in boxes.values():
        m[y0:y1 + 1, x0:x1 + 1] = True
    return m


def per_tile(a, th, tw, fn=np.sum):
    """fn over each th x tw tile of the [H, W] array `a` (partial tiles at the right / bottom padded with zeros)."""
    H, W = a.shape
    p = np.zeros((-(-H // th) * th, -(-W // tw) * tw), a.dtype)
    p[:H, :W] = a
    return fn(p.reshape(p.shape[0] // th, th, p.shape[1] // tw, tw), axis=(1, 3))
