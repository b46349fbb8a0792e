"""Frame parity, stated once: the statistics of a frame pair, the tolerance table (DESIGN.md section 4 / PARITY.md quote these rows by
name; the tests assert exactly these), the readers that turn device state into the oracle's inputs, and the per-env comparison loop."""
import os
from typing import NamedTuple, Optional

import numpy as np

from dtsim import _ffi, assets
from oracle import raster, sim as osim
from util import EXT, oracle_mode

ASSETS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "assets")


# ---- statistics --------------------------------------------------------------------------------------------------------------------

def stats(a, b, mask=None):
    """|a - b| of two uint8 frames in 1/255: `mean` over all channel values; `gt1` / `gt2` / `gt8` the fraction of pixels whose largest
    channel error is beyond 1 / 2 / 8, `max` the largest.  `mask`: pixels left OUT (gl_golden.line_mask)."""
    e = np.abs(a.astype(np.int32) - b.astype(np.int32))
    if mask is not None:
        e = e[~mask]
    m = e.max(axis=-1)
    return dict(mean=float(e.mean()), gt1=float((m > 1).mean()), gt2=float((m > 2).mean()), gt8=float((m > 8).mean()), max=int(m.max()))


# ---- tolerances --------------------------------------------------------------------------------------------------------------------

class Tol(NamedTuple):
    """Upper bounds (<=) on stats()' gt1, gt2 and mean; None: not asserted at the sites of this row."""
    gt1: Optional[float]
    gt2: Optional[float]
    mean: Optional[float]


def assert_within(s, tol, ctx=None):
    for key, bound in zip(Tol._fields, tol):
        assert bound is None or s[key] <= bound, (ctx, key, bound, s)


# The rows of DESIGN.md section 4, "Tolerances" (the comment quotes the row's first words).  HIP raster against the oracle restating
# the SAME pipeline (util.oracle_mode):
ORACLE_PLANE = Tol(1e-3, 5e-4, 0.02)         # "frames, plane-only scenes"
ORACLE_MESH = Tol(2e-3, 1e-3, 0.03)          # "frames, scenes with mesh objects"
ORACLE_MESH_GT1 = Tol(2e-3, None, 0.03)      # the same row where beyond +-2 is not asserted (checkerboard, the facade's free camera), and
#                                              "the generic raster in GL-filter mode" against the reference's frames
ORACLE_TINY = Tol(4e-3, None, 0.05)          # "tiny frames with mesh objects"
GOURAUD_CROSS = Tol(None, 1e-2, 0.5)         # "the same frames against the oracle's GL-faithful per-vertex ("gouraud") tile light"
# against the reference's own frames (Mesa 23.2.1 llvmpipe):
REFERENCE_GL = Tol(1e-2, 4e-3, 0.35)         # "frames against the reference's own frames": every HIP pipeline; the oracle's byte-weight filter
ORACLE_GL = Tol(2e-3, None, 0.02)            # "the oracle's GL-faithful mode against the same frames" (CPU)
ORACLE_PIXEL_GL = Tol(2e-3, None, 0.2)       # "the oracle with per-fragment tile light" (CPU)
GL_FILTER_DIFFER = 2.5e-2                    # "the generic raster in GL-filter mode": fraction of pixels that differ AT ALL (its own assert)
# "frames the drop-in facade returns, against the oracle":
FACADE_LIGHT = Tol(None, 1e-3, 0.05)         # second-episode light
FACADE_TOP_DOWN = Tol(3e-3, None, 0.05)      # top-down view
FACADE_OVERLAY = Tol(None, 3e-3, 0.1)        # draw_curve / enable_leds frames
FACADE_BBOX = Tol(None, 1e-2, 0.3)           # draw_bbox view (the lines are drawn over the meshes: no depth test against them)


# one HIP raster against another on the same batch:
class PairTol(NamedTuple):
    """Upper bounds (<=) on the fraction of pixels that differ at all, and that differ by more than 1."""
    differ: float
    gt1: float


Q_VS_V3 = PairTol(2e-3, 1e-5)                # "k_raster_q against k_raster_v3": same records, same snapped coordinates, same byte-weight filter; the exact
#                                              paths differ in form, which may move a rounding tie on a queued pixel


def assert_pair(a, b, tol, ctx=None):
    """Frames a against b (uint8, same shape) within PairTol `tol`; returns (fraction that differ, fraction beyond 1, the largest difference)."""
    d = np.abs(a.astype(np.int32) - b.astype(np.int32)).max(axis=-1)
    out = (float((d > 0).mean()), float((d > 1).mean()), int(d.max()))
    assert out[0] <= tol.differ and out[1] <= tol.gt1, (ctx, out)
    return out


class ObjTol(NamedTuple):
    """The bounds of compare_objects: `frame` on the whole frame; of an object's interior pixels at most obj_share of them + obj_slack
    beyond +-2; of the pixels away from every object at most outside_gt2 x W x H beyond +-2."""
    frame: Tol
    obj_share: float
    obj_slack: float
    outside_gt2: float


OBJ_MIN_INTERIOR = 16                        # an object is judged on its own from this many interior pixels in the oracle
# "crowded frames, per object": ORACLE_MESH on the frame; per object the 5 % of the touched pixels that overlay_lines_tol / leds_tol
# allow, + 2 pixels; away from the objects ORACLE_PLANE's beyond-2 share of the frame
ORACLE_OBJECTS = ObjTol(ORACLE_MESH, 0.05, 2.0, ORACLE_PLANE.gt2)


def tighter(tol, k):
    """`tol` with every bound divided by k (the oracle's own headroom under a row: tests/test_crowd_scenes_host.py)."""
    if isinstance(tol, ObjTol):
        return ObjTol(tighter(tol.frame, k), tol.obj_share / k, tol.obj_slack / k, tol.outside_gt2 / k)
    return Tol(*(None if b is None else b / k for b in tol))


def overlay_lines_tol(n_line, W, H):
    """"`draw_curve` / `draw_bbox` overlays", through the fisheye: ORACLE_PLANE's beyond-2 bound plus 5 % of the n_line line pixels of a W x H frame."""
    return Tol(None, 5e-4 + 0.05 * n_line / (W * H), 0.05)


def leds_tol(touched, W, H):
    """"`enable_leds` spheres", through the fisheye: 5 % of the `touched` pixels of a W x H frame on top of 2e-3."""
    return Tol(None, 2e-3 + 0.05 * touched / (W * H), 0.1)


# ---- readers: device state -> oracle inputs ----------------------------------------------------------------------------------------

def scene(map_name):
    om = osim.OracleMap(assets.get_map(map_name), EXT)
    kinds = {t["kind"] for t in om.grid if t is not None}
    tex = {k: assets.get_texture(k) for k in kinds}
    meshes = {"duckie": assets.get_mesh("duckie"), "*": assets.get_mesh("*")}
    return raster.Scene(om, tex, meshes)


def asset_scene():
    """Oracle scene of the real-asset fixture (tests/golden/assets): per-kind meshes with textures."""
    lib = assets.AssetLibrary(ASSETS)
    md = lib.map_data("test_town")
    meshes = {"*": assets.get_mesh("*")}
    for desc in md["objects"]:
        meshes[desc["kind"]] = lib.object_mesh(desc)[1]
    ext = {k: (m.min_coords, m.max_coords) for k, m in meshes.items()}
    om = osim.OracleMap(md, ext)
    kinds = {t["kind"] for t in om.grid if t is not None}
    sc = raster.Scene(om, {k: lib.tile_texture(k) for k in kinds}, meshes)
    sc.light_cards = lib.light_cards()              # TrafficLightObj.texs (objects.py:438-441)
    return sc, md, ext


def camera(sim, e, W, H, dr, colors=None):
    """Env e's camera.  Colours and light come from its init state ((0, 3, 0, 1) unless the facade captured the light through a
    model-view) -- or, for device-side resets that moved them since, from `colors`: env e's row of DTSIM_FIELD_COLORS
    (horizon, ground, ambient, diffuse, light xyzw)."""
    return camera_of_state(sim.init_states[e], sim.read(_ffi.FIELD_POS)[e], sim.read(_ffi.FIELD_ANGLE)[e], W, H, dr, colors)


def camera_of_state(st, pos, ang, W, H, dr, colors=None):
    """The camera of an env with init state `st` standing at (pos, ang): what camera() builds from a device's state."""
    if colors is None:
        horizon, ground, ambient, diffuse, light = (list(v) for v in (st.horizon_color, st.ground_color, st.light_ambient, st.light_diffuse, st.light_pos))
    else:
        horizon, ground, ambient, diffuse, light = ([float(v) for v in colors[i:j]] for i, j in ((0, 3), (3, 6), (6, 9), (9, 12), (12, 16)))
    if not dr:
        return raster.Camera(pos, ang, width=W, height=H, horizon_color=horizon, ground_color=ground, light_pos=light)
    return raster.Camera(pos, ang, cam_height=st.cam_height, cam_angle_deg=st.cam_angle_deg,
                         cam_fov_y_deg=st.cam_fov_y_deg, camera_noise=list(st.camera_noise), domain_rand=True,
                         horizon_color=horizon, ground_color=ground, light_pos=light, light_ambient=ambient,
                         light_diffuse=diffuse, width=W, height=H)


def obj_states(sim, e, sc):
    """Per-object render state of env e (static: map pose; DuckieObj: device centre / y_rot)."""
    cen, yrot = sim.read(_ffi.FIELD_OBJ_CENTER)[e], sim.read(_ffi.FIELD_OBJ_YROT)[e]
    cy = sim.read(_ffi.FIELD_OBJ_Y)[e]
    vis = sim.read(_ffi.FIELD_OBJ_VISIBLE)[e]
    out, slot = [], 0
    for k, o in enumerate(sc.m.objects):
        if o.static:
            out.append(dict(pos=o.pos, y_rot=o.y_rot, visible=bool(vis[k])))
        else:
            out.append(dict(pos=np.array([cen[slot, 0], cy[slot], cen[slot, 1]]), y_rot=float(yrot[slot]), visible=bool(vis[k])))
            slot += 1
    return out


def stratified_picks(sim, N, n_min, seed):
    """Env indices of an N-env batch that exercise the raster's work decomposition.  The decomposition goes by POSITION in the
    render order of the pass that just ran (DTSIM_FIELD_RENDER_POS: k_env_sort's order on the quad-record paths, the identity
    elsewhere): 64 consecutive positions (32 before round 6) share a workgroup chunk, XCD x owns the x-th eighth of the chunks (raster_common.h:
    XCD-affine workgroup map).  Picked positions: the first / last of the order, both sides of chunk borders, the middle of
    every XCD's eighth (a chunk border there), the tail chunk -- mapped back to env indices -- plus envs 0 and N - 1."""
    pos = sim.read(_ffi.FIELD_RENDER_POS)
    assert sorted(pos.tolist()) == list(range(N))          # a permutation of the batch
    env_at = np.argsort(pos, kind="stable")                # position -> env
    at = [0, 1, 31, 32, 33, 63, 64, N - 1, N - 2, N - 32, N - 33]
    for x in range(8):
        m = x * (N // 8) + N // 16
        at += [m - 1, m]
    picks = [int(env_at[p]) for p in at if 0 <= p < N] + [0, N - 1]
    rng = np.random.default_rng(seed)
    while len(set(picks)) < n_min:
        picks.append(int(rng.integers(N)))
    return sorted(set(picks))


def frames_of(sim, picks):
    import torch
    frames = torch.as_tensor(sim.frames_device(), device="cuda:0")
    return frames[torch.as_tensor(np.array(picks), device="cuda:0")].cpu().numpy()


# ---- the comparison ----------------------------------------------------------------------------------------------------------------

def object_pixels(ref, no_obj):
    """Pixels of `ref` that the mesh objects own: those that change when the objects are hidden."""
    return int((np.abs(ref.astype(int) - no_obj.astype(int)).max(-1) > 0).sum())


def oracle_frame(sim, e, sc, rmap, *, dr, mode=None, objects=True, colors=None, **overlay):
    """The oracle's frame of env e as the device holds it; `mode` defaults to the pipeline `sim` renders with (util.oracle_mode);
    objects=False hides the mesh objects; `overlay`: render_obs' lines= / leds=."""
    st = obj_states(sim, e, sc) if sc.m.objects else None
    if st and not objects:
        st = [dict(s, visible=False) for s in st]
    return raster.render_obs(camera(sim, e, sim.camera_width, sim.camera_height, dr, colors), sc, oracle_mode(sim) if mode is None else mode,
                             rmap, obj_states=st, **overlay)


def compare_envs(sim, frames, envs, scene_of, rmap, tol, *, dr, mode=None, count_objects=0, colors=None):
    """frames[k] against the oracle's frame of env envs[k], each asserted within `tol`.  scene_of: the Scene, or env -> Scene where the
    batch holds several maps; colors: the [N][16] DTSIM_FIELD_COLORS array where the cameras take colours and light from it (camera).
    Returns (worst gt1 / gt2 / mean over the envs, object pixels of the first `count_objects` envs)."""
    worst, n_obj_px = dict(gt1=0.0, gt2=0.0, mean=0.0), 0
    for k, e in enumerate(envs):
        kw = dict(dr=dr, mode=mode, colors=None if colors is None else colors[e])
        sc = scene_of(e) if callable(scene_of) else scene_of
        ref = oracle_frame(sim, e, sc, rmap, **kw)
        if k < count_objects:
            n_obj_px += object_pixels(ref, oracle_frame(sim, e, sc, rmap, objects=False, **kw))
        s = stats(frames[k], ref)
        assert_within(s, tol, e)
        worst = {f: max(worst[f], s[f]) for f in worst}
    return worst, n_obj_px


def interior(ids, k):
    """Pixels whose four samples all carry object k's id (`ids`: the four per-sample arrays of raster.render_obs(return_ids=True))."""
    return (ids[0] == k) & (ids[1] == k) & (ids[2] == k) & (ids[3] == k)


def away_from_objects(ids):
    """Pixels none of whose samples, nor any sample of their 3 x 3 neighbourhood, belongs to an object."""
    obj = (ids[0] >= 0) | (ids[1] >= 0) | (ids[2] >= 0) | (ids[3] >= 0)
    H, W = obj.shape
    p = np.zeros((H + 2, W + 2), bool)
    p[1:-1, 1:-1] = obj
    near = np.zeros((H, W), bool)
    for dy in range(3):
        for dx in range(3):
            near |= p[dy:dy + H, dx:dx + W]
    return ~near


def compare_objects(frame, ref, ids, tol=ORACLE_OBJECTS, ctx=None):
    """`frame` against the oracle's `ref` with the oracle's per-sample object ids, asserted in this order: (a) the whole frame within
    tol.frame; (b) for every object with >= OBJ_MIN_INTERIOR interior pixels, the interior pixels beyond +-2 are at most
    tol.obj_share of them + tol.obj_slack -- a dropped object, a dropped slice of its triangles, the wrong winner between two objects
    or an unqueued box pixel move far more; (c) away from the objects (away_from_objects) at most tol.outside_gt2 x W x H pixels are
    beyond +-2: nothing leaks outside a silhouette.  `ctx` (the env, the case) leads every message.
    Returns dict(frame=stats(), judged=objects judged, obj_share=the worst share of an object's interior pixels beyond +-2,
    obj_worst=(object, beyond +-2, interior pixels) of that object, outside=pixels beyond +-2 away from the objects)."""
    H, W = frame.shape[:2]
    s = stats(frame, ref)
    assert_within(s, tol.frame, ctx)
    bad = np.abs(frame.astype(np.int32) - ref.astype(np.int32)).max(axis=-1) > 2
    out = dict(frame=s, judged=0, obj_share=0.0, obj_worst=None, outside=0)
    for k in np.unique(np.stack(ids)):
        if k < 0:
            continue
        inner = interior(ids, k)
        n = int(inner.sum())
        if n < OBJ_MIN_INTERIOR:
            continue
        n_bad = int((bad & inner).sum())
        out["judged"] += 1
        if out["obj_worst"] is None or n_bad / n > out["obj_share"]:
            out["obj_share"], out["obj_worst"] = n_bad / n, (int(k), n_bad, n)
        assert n_bad <= tol.obj_share * n + tol.obj_slack, (ctx, f"object {int(k)}: {n_bad} of its {n} interior pixels beyond +-2",
                                                            [tuple(int(v) for v in yx) for yx in np.argwhere(bad & inner)[:8]])
    out["outside"] = int((bad & away_from_objects(ids)).sum())
    assert out["outside"] <= tol.outside_gt2 * W * H, (ctx, f"{out['outside']} pixels beyond +-2 away from every object",
                                                        [tuple(int(v) for v in yx) for yx in np.argwhere(bad & away_from_objects(ids))[:8]])
    return out
