"""The expected optical-flow map of dtsim_flow (include/dtsim.h), in float64 on the oracle's side alone, and the inputs the flow tests share.

The quantity, per MSAA sample of a rectilinear source pixel: the depth buffers and surfaces are depth_model's (oracle_buffers / surfaces of
the CURRENT state); the world hit P is rebuilt from the sample's depth and ray as label_model.world_hit rebuilds it, with the height too;
a point of mesh object k moves with it, P_prev = pos_prev(k) + Ry(yrot_prev(k)) Ry(yrot_cur(k))^-1 (P - pos_cur(k)), from two lists of
object states (frame_parity.obj_states' form); both points go through ipm_model.project with their state's camera and, on fisheye frames,
ipm_model.forward at (u - 0.5, v - 0.5).  flow = A(prev) - A(cur); valid iff the sample is not sky, w_prev >= 0.04 and the previous
rectilinear (u, v) lies in [0, W) x [0, H).  Through the fisheye the map moves by nearest source pixel (dm.remap_nearest: flow 0, invalid
where a pixel has no source).

A pixel's CANDIDATE SET: the (flow, valid) of every sample whose inverse depth lies within dm.INV_DEPTH_TOL of the pixel's largest (its
minimum depth), taken in the oracle's run and in its run from the float32-rounded poses scaled by 1 + 2e-7 (dm.host_camera(nudge=True); both
states' poses).  A pixel is SURE when all four samples lie on one surface in both runs (the same one) and every candidate's validity
conditions are farther from their limits than MARGIN.  PLANE-SURE: sure, and that surface is a plane or the sky.

The cases are depth_model's, whose states are the CURRENT ones (so its cached buffers are reused); MOTIONS says how the previous state
differs."""
import copy
import functools
import math
from typing import NamedTuple

import numpy as np

import depth_model as dm
import frame_parity as fp
import ipm_model as im
from oracle import raster, sim as osim
from util import EXT

MARGIN = 1e-2          # px (u, v against the image border) and 1e-4 m (w against the near plane): far more than any tolerance below
MARGIN_W = 1e-4

# (forward metres, dtheta): the CURRENT pose is the previous one moved `forward` along the previous heading, then turned by dtheta.
MOTIONS = {"forward": (0.03, 0.02), "rotate": (0.0, 0.08), "backward": (-0.05, -0.03), "tile": (0.45, 0.05), "still": (0.0, 0.0)}
PED_PREV_STEPS = 8     # "pedestrians": the previous state is 8 zero-action steps in (the duckies walk from step 6 on), the current one dm's 14
# name -> (depth_model case, motion, the objects move)
CASES = {}
for _c in ("planes", "planes_dr"):
    for _m in ("forward", "rotate", "backward", "tile"):
        CASES[f"{_c}-{_m}"] = (_c, _m, False)
CASES["pedestrians-still"] = ("pedestrians", "still", True)
CASES["pedestrians-forward"] = ("pedestrians", "forward", True)
CASES["town-forward"] = ("town", "forward", False)
CASES["town_odd-rotate"] = ("town_odd", "rotate", False)


def case_of(name):
    return dm.CASES[CASES[name][0]]


def prev_pose(x, z, ang, motion):
    """The previous pose of a current one."""
    f, dth = MOTIONS[motion]
    a0 = ang - dth
    return x - f * math.cos(a0), z + f * math.sin(a0), a0


def cameras(name, e, nudge=False):
    """(current, previous) oracle cameras of env e."""
    c = case_of(name)
    cur = dm.host_camera(c, e, nudge)
    st = dm.init_states(c)[e]
    px, pz, pa = prev_pose(float(st.pos[0]), float(st.pos[2]), float(st.angle), CASES[name][1])
    pos, ang = np.array([px, 0.0, pz]), pa
    if nudge:
        pos, ang = pos.astype(np.float32).astype(np.float64) * (1 + 2e-7), float(np.float32(ang))
    return cur, fp.camera_of_state(st, pos, ang, c.W, c.H, c.dr)


@functools.lru_cache(maxsize=None)
def host_objects_at(dm_name, steps):
    """dm.host_objects with another number of zero-action steps (the oracle's own physics)."""
    case, sc = dm.CASES[dm_name], dm.scene_of(dm_name)
    if steps == case.steps or not sc.m.objects:
        return dm.host_objects(dm_name)
    ext = dm._town()[2] if case.asset_tree else EXT
    out = []
    for (x, z, ang, *_rest) in case.states:
        o = osim.OracleSim(copy.deepcopy(dm._map_data(case)), ext, do_reset=False, max_steps=10 ** 6)
        o.wheel_dist = osim.WHEEL_DIST
        o.set_pose([x, 0.0, z], ang)
        for ob in o.map.objects:
            if case.wait is not None and not ob.static and ob.kind == "duckie":
                ob.pedestrian_wait_time = case.wait
        for _ in range(steps):
            o.step(np.zeros(2))
        out.append([dict(pos=np.array(ob.pos if ob.static else [ob.center[0], ob.pos[1], ob.center[2]], dtype=np.float64),
                         y_rot=float(ob.y_rot), visible=bool(ob.visible)) for ob in o.map.objects])
    return tuple(out)


def host_objects(name, e):
    """(current, previous) object states of env e on the oracle alone."""
    dm_name, _, moves = CASES[name]
    cur = dm.host_objects(dm_name)[e]
    return cur, (host_objects_at(dm_name, PED_PREV_STEPS)[e] if moves else cur)


def _ry(deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])          # glRotatef(y_rot, 0, 1, 0), as raster places a mesh


def world_hits(cam, depth, q):
    """World (x, y, z) [H, W, 3] of sample q's hit: label_model.world_hit's rebuild, with the height; where depth is inf, the camera's centre."""
    cols, rows = np.meshgrid(np.arange(cam.W, dtype=np.float64), np.arange(cam.H, dtype=np.float64))
    ox, oy = raster.SAMPLE_OFFSETS[q]
    nx = 2 * (cols + 0.5) / cam.W - 1 + 2 * ox / cam.W
    ny = 1 - 2 * (rows + 0.5) / cam.H - 2 * oy / cam.H
    xe, ye, yla, fwd = raster._rays(cam, nx, ny)
    t = np.where(np.isfinite(depth), depth, 0.0)
    rr, ff = t * xe, t * fwd
    return np.stack([cam.C[0] + rr * cam.sa + ff * cam.ca, cam.C[1] + t * yla, cam.C[2] + rr * cam.ca - ff * cam.sa], axis=-1)


def image(cam, P, cal):
    """(w, u, v, ax, ay) of world points: ipm_model.project, then A."""
    w, u, v = im.project(cam, P)
    if cal is None:
        return w, u, v, u, v
    ax, ay = im.forward(cal, u - 0.5, v - 0.5)
    return w, u, v, ax, ay


def sample_flows(cam_c, cam_p, depths, srf, objs_c, objs_p, cal=None):
    """Per sample: (flow [4, H, W, 2], valid [4, H, W] bool, clear [4, H, W] bool: the validity conditions are farther than MARGIN from their limits)."""
    Hc, Wc = depths.shape[1:]
    flow = np.zeros((4, Hc, Wc, 2))
    valid = np.zeros((4, Hc, Wc), bool)
    clear = np.ones((4, Hc, Wc), bool)
    for q in range(4):
        P = world_hits(cam_c, depths[q], q)
        Pp = P.copy()
        for k in (np.unique(srf[q][srf[q] >= 0]) if objs_c else ()):
            sel = srf[q] == k
            R = _ry(objs_p[k]["y_rot"]) @ _ry(objs_c[k]["y_rot"]).T
            Pp[sel] = np.asarray(objs_p[k]["pos"], np.float64) + (P[sel] - np.asarray(objs_c[k]["pos"], np.float64)) @ R.T
        _, _, _, ax0, ay0 = image(cam_c, P, cal)
        w, u, v, ax1, ay1 = image(cam_p, Pp, cal)
        hit = np.isfinite(depths[q])
        with np.errstate(invalid="ignore"):
            ok = hit & (w >= raster.NEAR) & (u >= 0) & (u < Wc) & (v >= 0) & (v < Hc)
            near = (np.abs(w - raster.NEAR) <= MARGIN_W) | (np.abs(u) <= MARGIN) | (np.abs(u - Wc) <= MARGIN) | (np.abs(v) <= MARGIN) | (np.abs(v - Hc) <= MARGIN)
        f = np.stack([ax1 - ax0, ay1 - ay0], axis=-1)
        flow[q] = np.where(ok[..., None], f, 0.0)
        valid[q], clear[q] = ok, ~(hit & near)
    return flow, valid, clear


class Run(NamedTuple):
    flow: np.ndarray        # [4, H, W, 2] per sample
    valid: np.ndarray       # [4, H, W]
    clear: np.ndarray       # [4, H, W]
    cand: np.ndarray        # [4, H, W] the sample is a candidate of its pixel
    srf: np.ndarray         # [4, H, W]
    pick: np.ndarray        # [H, W] label_model.nearest_sample


def run(name, e, nudge=False, cal=None, objects=None):
    """One run of the model in rectilinear source-pixel space.  objects: (current, previous) object states in place of the oracle's own."""
    dm_name = CASES[name][0]
    depths, srf = dm.host_buffers(dm_name, e, nudge)
    cam_c, cam_p = cameras(name, e, nudge)
    oc, op = host_objects(name, e) if objects is None else objects
    flow, valid, clear = sample_flows(cam_c, cam_p, depths, srf, oc, op, cal)
    inv = dm.inv(depths)
    cand = inv >= inv.max(axis=0) - dm.INV_DEPTH_TOL
    return Run(flow, valid, clear, cand, srf, np.argmin(depths, axis=0))


class Expected(NamedTuple):
    flow: np.ndarray        # [H, W, 2] the oracle's own value (its nearest sample's)
    valid: np.ndarray       # [H, W] bool
    cflow: np.ndarray       # [8, H, W, 2] the candidates: four of the oracle's run, four of the nudged one
    cvalid: np.ndarray      # [8, H, W]
    cand: np.ndarray        # [8, H, W] which of them are members
    sure: np.ndarray        # [H, W]
    plane: np.ndarray       # [H, W] sure, and a plane or the sky
    source: np.ndarray      # [H, W] the pixel has a source pixel


def _take(a, pick):
    return np.take_along_axis(a, pick[None, ..., None] if a.ndim == 4 else pick[None], axis=0)[0]


def expected(name, e, kind=None, cal=None, objects=None) -> Expected:
    """The expected map of env e: full size, through the source map `kind` (None / "fisheye") by nearest source pixel.  With kind, pass
    the calibration whose forward model the frames go through (ipm_model.nominal_cal())."""
    c = case_of(name)
    r0, r1 = run(name, e, False, cal, objects), run(name, e, True, cal, objects)
    flow, valid = _take(r0.flow, r0.pick), _take(r0.valid, r0.pick)
    cflow, cvalid, cand = np.concatenate([r0.flow, r1.flow]), np.concatenate([r0.valid, r1.valid]), np.concatenate([r0.cand, r1.cand])
    one = (r0.srf == r0.srf[0]).all(axis=0) & (r1.srf == r1.srf[0]).all(axis=0) & (r0.srf[0] == r1.srf[0])
    clear = np.where(cand, np.concatenate([r0.clear, r1.clear]), True).all(axis=0)
    sure = one & clear
    plane = sure & (r0.srf[0] < 0)
    source = np.ones(sure.shape, bool)
    if kind is not None:
        rm = dm.rmap(c.W, c.H, kind)
        mv = lambda a, fill: np.stack([dm.remap_nearest(np.ascontiguousarray(p), rm, fill) for p in a.reshape(-1, *sure.shape)]).reshape(a.shape)
        planes = lambda a: np.moveaxis(mv(np.moveaxis(a, -1, 0), 0.0), 0, -1)
        flow, cflow = planes(flow), np.stack([planes(f) for f in cflow])
        valid, cvalid, cand = (mv(a[None], False)[0] if a.ndim == 2 else mv(a, False) for a in (valid, cvalid, cand))
        source = dm.remap_nearest(source, rm, False)
        sure, plane = dm.remap_nearest(sure, rm, True), dm.remap_nearest(plane, rm, True)
        cand[0] |= ~source                                  # a pixel without a source: one candidate, flow 0, invalid
    return Expected(flow, valid, cflow, cvalid, cand, sure, plane, source)


def nearest_candidate(exp: Expected, got_flow, got_valid):
    """[H, W] the distance (max of |du|, |dv|, px) from the device's value to the nearest candidate with the device's `valid`; inf where
    no candidate has it.  got_flow: [2, H, W], got_valid: [H, W]."""
    g = np.moveaxis(np.asarray(got_flow, np.float64), 0, -1)
    d = np.abs(exp.cflow - g[None]).max(axis=-1)
    d = np.where(exp.cand & (exp.cvalid == (np.asarray(got_valid) != 0)[None]), d, np.inf)
    return d.min(axis=0)


def hold(exp: Expected, got_flow, got_valid, tol_plane, tol_obj, cap, ctx=None):
    """The check of the issue: on every plane-sure pixel within tol_plane of a candidate and agreeing on valid (no cap); everywhere else
    within tol_obj of a candidate on all but `cap` of ALL pixels.  Returns dict(plane_max, other_beyond, other_max_within, n_plane)."""
    got_flow, got_valid = np.asarray(got_flow), np.asarray(got_valid)
    assert got_flow.shape == (2, *exp.sure.shape) and got_flow.dtype == np.float32 and got_valid.dtype == np.uint8, (ctx, got_flow.shape, got_flow.dtype)
    assert np.isfinite(got_flow).all() and set(np.unique(got_valid)) <= {0, 1}, ctx
    assert (got_flow[:, got_valid == 0] == 0).all(), (ctx, "an invalid pixel with a flow")
    d = nearest_candidate(exp, got_flow, got_valid)
    out = dict(n_plane=int(exp.plane.sum()), plane_max=float(d[exp.plane].max()) if exp.plane.any() else 0.0)
    rest = ~exp.plane
    beyond = rest & ~(d <= tol_obj)
    within = d[rest & (d <= tol_obj)]
    out.update(other_beyond=float(beyond.sum() / d.size), n_beyond=int(beyond.sum()), other_max_within=float(within.max()) if within.size else 0.0)
    print(f"{ctx}: plane-sure {out['n_plane']} px, max {out['plane_max']:.3e} (tol {tol_plane:.3e}); others beyond {out['n_beyond']} px "
          f"({out['other_beyond']:.2e}, cap {cap:.2e}), max within {out['other_max_within']:.3e} (tol {tol_obj:.3e})")
    bad = exp.plane & ~(d <= tol_plane)
    assert not bad.any(), (ctx, out, [(int(y), int(x), float(d[y, x])) for y, x in np.argwhere(bad)[:8]])
    assert out["other_beyond"] <= cap, (ctx, out, [(int(y), int(x), float(d[y, x])) for y, x in np.argwhere(beyond)[:8]])
    return out


def nudge_stats(name, e):
    """The oracle's map against its nudged self (each run's own nearest sample): dict(plane_max = largest |dflow| over the plane-sure
    pixels, err = [H, W] |dflow| (inf where `valid` differs), sure = share of sure pixels, valid = share of valid pixels, flow_max)."""
    exp = expected(name, e)
    r0, r1 = run(name, e, False), run(name, e, True)
    f0, f1 = _take(r0.flow, r0.pick), _take(r1.flow, r1.pick)
    v0, v1 = _take(r0.valid, r0.pick), _take(r1.valid, r1.pick)
    err = np.where(v0 == v1, np.abs(f0 - f1).max(axis=-1), np.inf)
    return dict(plane_max=float(err[exp.plane].max()) if exp.plane.any() else 0.0, err=err, sure=float(exp.sure.mean()), valid=float(v0.mean()),
                flow_max=float(np.abs(f0).max()), n_plane=int(exp.plane.sum()), plane=exp.plane)


def expected_loop(name, e, cal=None):
    """The same quantity pixel by pixel in plain Python floats, from the issue's statement: (flow [H, W, 2], valid [H, W]) of the
    oracle's run (no candidates)."""
    c = case_of(name)
    depths, srf = dm.host_buffers(CASES[name][0], e)
    cc, cp = cameras(name, e)
    oc, op = host_objects(name, e)
    flow, valid = np.zeros((c.H, c.W, 2)), np.zeros((c.H, c.W), bool)

    def proj(cam, P):
        rel = [P[i] - float(cam.C[i]) for i in range(3)]
        xla, yla, zla = rel[0] * cam.sa + rel[2] * cam.ca, rel[1], -(rel[0] * cam.ca - rel[2] * cam.sa)
        xe, ye, w = xla, yla * cam.cth - zla * cam.sth, -(yla * cam.sth + zla * cam.cth)
        if w == 0:
            return w, math.inf, math.inf
        return w, (xe / w / cam.tx + 1) * cam.W / 2, (1 - ye / w / cam.ty) * cam.H / 2

    def A(u, v):
        if cal is None:
            return u, v
        x, y = im.forward(cal, u - 0.5, v - 0.5)
        return float(x), float(y)

    for r in range(c.H):
        for col in range(c.W):
            q = min(range(4), key=lambda k: (depths[k, r, col], k))
            d = float(depths[q, r, col])
            if math.isinf(d):
                continue
            ox, oy = raster.SAMPLE_OFFSETS[q]
            nx, ny = 2 * (col + 0.5 + ox) / c.W - 1, 1 - 2 * (r + 0.5 + oy) / c.H
            xe, ye = nx * cc.tx, ny * cc.ty
            yla, fwd = ye * cc.cth - cc.sth, ye * cc.sth + cc.cth
            P = [float(cc.C[0]) + d * xe * cc.sa + d * fwd * cc.ca, float(cc.C[1]) + d * yla, float(cc.C[2]) + d * xe * cc.ca - d * fwd * cc.sa]
            Pp = P
            k = int(srf[q, r, col])
            if k >= 0:
                rel = np.array(P) - np.asarray(oc[k]["pos"], np.float64)
                Pp = list(np.asarray(op[k]["pos"], np.float64) + _ry(op[k]["y_rot"]) @ (_ry(-oc[k]["y_rot"]) @ rel))
            _, u0, v0 = proj(cc, P)
            w, u1, v1 = proj(cp, Pp)
            if w >= 0.04 and 0 <= u1 < c.W and 0 <= v1 < c.H:
                a0, a1 = A(u0, v0), A(u1, v1)
                flow[r, col], valid[r, col] = (a1[0] - a0[0], a1[1] - a0[1]), True
    return flow, valid
