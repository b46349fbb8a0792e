"""What a handle that has rendered BEFORE must not show: a numpy statement of k_obj_setup's survive / cull rule (csrc/render_setup.hip) and of
what a reader of the ScreenTri records sees if it tests a triangle by the box inside its record instead of the pass's own box stream.

The rule.  A pass projects the triangles of every object that is visible and passes the object-level frustum cull (else ObjBox.count = 0 and
nothing of the object is tested by anyone).  A triangle SURVIVES when every vertex has w > NEAR_Z, its screen area is not 0 and its box, padded
by DT_TRI_PAD, meets the frame; the pass rewrites the record of a survivor only, and writes every triangle's box -- inverted for a culled one --
to its box stream.  A triangle culled now that survived an earlier pass is STALE: its record is the earlier pass's.  A reader that goes by the
record's box z-buffers it where it stood then, at every pixel inside the object's current ObjBox +- 1 px; a reader that goes by the box stream
skips it.  The maps of the second reader are those of a fresh handle in the same state, and those the oracle gives.

The pairs (map, object, prime pose, current pose) are stated here once and kept out of dm.CASES, lm.CASES, im.CASES and fm.CASES: the model
functions of depth_model.py, label_model.py and instance_model.py take the Case objects built here.  tests/test_rerender_model_host.py asserts
that every pair would show far more wrong pixels than the comparisons' caps forgive, so that tests/test_gpu_rerender_maps.py cannot pass
over a reader of stale records; the projection runs in float32 as the kernel's does, the coverage test in float64 at the four sample
positions of oracle/raster.py."""
import functools
import math
from typing import NamedTuple

import numpy as np

import depth_model as dm
import instance_model as im
import label_model as lm
from led_model import led_share, sphere_set  # noqa: F401  (led_share: read through this module by the two re-render tests)
from oracle import raster

NEAR_Z = np.float32(raster.NEAR)
TRI_PAD = np.float32(0.5)                   # DT_TRI_PAD
F = np.float32


class Pair(NamedTuple):
    group: str                               # GROUPS' key: the pairs of one group are the envs of one handle
    obj: int                                 # the object the poses look at
    prime: tuple                             # (x, z, angle) of the render that leaves the records
    cur: tuple                               # (x, z, angle) of the render the maps are asked of


class Group(NamedTuple):
    map_name: str
    W: int
    H: int
    asset_tree: bool


GROUPS = {"town": Group("test_town", dm.W, dm.H, True), "town_odd": Group("test_town", 90, 62, True),
          "ped": Group("loop_pedestrians", dm.W, dm.H, False)}


def _objects(group):
    g = GROUPS[group]
    return dm._scene(g.map_name, g.asset_tree).m.objects


def on_line(group, k, d, a=0.2, turn=0.0):
    """The pose d m in front of object k of the group's map on heading a, turned by `turn`."""
    p = _objects(group)[k].pos
    return (float(p[0] - d * math.cos(a)), float(p[2] + d * math.sin(a)), a + turn)


def _pair(group, k, d, turn, d0=0.45):
    return Pair(group, k, on_line(group, k, d0), on_line(group, k, d, turn=turn))


# test_town: 0 a cone, 2 a tree, 3 a duckiebot.  The prime pose faces the object from d0 m (0.45 unless given); the current pose stands closer
# on the same line and looks past it, so that part of the object leaves the frame or crosses the near plane while the rest stays in view.
# Every pair meets every condition of tests/test_rerender_model_host.py.  What the model says of their neighbours, for whoever moves one:
#   the cone from d0 = 0.45 m (0.12 m, -0.45) shows 111 wrong depth pixels, under 3 x the cap; from 0.28 m it shows 389, with 2 cm of room
#   between the stale surface and the real one; from 0.22 m (0.13 m, -0.50) 224, but 4 mm of room, too little for a sphere between them; and
#   at (0.13 m, -0.35) the ORACLE moves beyond the depth tolerance on 139 pixels under its own nudge (the cone's steep side 10 cm away);
#   loop_pedestrians' 6 cm duckies (standing: no step is taken) show nothing from 0.45 m; primed from 0.14 m they do.
PAIRS = {
    "bot_left": _pair("town", 3, 0.20, +0.50),
    "bot_right": _pair("town", 3, 0.12, -0.70),
    "tree": _pair("town", 2, 0.12, +0.25),
    "cone": _pair("town", 0, 0.12, -0.45, d0=0.28),
    "odd_bot": _pair("town_odd", 3, 0.20, +0.50),
    "odd_tree": _pair("town_odd", 2, 0.12, +0.25),
    "duckie6": _pair("ped", 6, 0.11, +0.20, d0=0.14),
    "duckie0": _pair("ped", 0, 0.11, -0.15, d0=0.14),
}
# Three earlier poses for the handle that is primed three times (the last is the pair's own prime pose): from further away and from two sides.
def prime3(name):
    p = PAIRS[name]
    return (on_line(p.group, p.obj, 0.70, a=-0.4), on_line(p.group, p.obj, 0.55, a=0.9), p.prime)


def names(group):
    return tuple(n for n, p in PAIRS.items() if p.group == group)


@functools.lru_cache(maxsize=None)
def case(group, which="cur"):
    """The dm.Case of a group: env e stands at pair e's pose `which` ("prime", "cur", or 0..2 of prime3)."""
    g = GROUPS[group]
    poses = [getattr(PAIRS[n], which) if isinstance(which, str) else prime3(n)[which] for n in names(group)]
    return dm.Case(g.map_name, g.W, g.H, False, tuple(tuple(p) + dm.DEFAULT_CAM for p in poses), asset_tree=g.asset_tree, mesh=True)


def env_of(name):
    return names(PAIRS[name].group).index(name)


# ---- k_obj_setup ----------------------------------------------------------------------------------------------------------------------------

class ObjPass(NamedTuple):
    live: bool               # ObjBox.count > 0: visible, inside the frustum, and at least one triangle survived
    ok: np.ndarray           # [T] the triangle survived
    sx: np.ndarray           # [T, 3] float32 screen x of its vertices (pixels)
    sy: np.ndarray
    iw: np.ndarray           # [T, 3] 1 / w
    box: np.ndarray          # [T, 4] bx0, bx1, by0, by1: padded
    obox: tuple              # the union of the survivors' boxes


def setup_pass(cam, scene, obj_states, W, H):
    """One pass of k_obj_setup over the objects of the scene, in float32: a list of ObjPass, one per object of scene.m.objects."""
    C = cam.C.astype(F)
    sa, ca, sth, cth, tx, ty = (F(v) for v in (cam.sa, cam.ca, cam.sth, cam.cth, cam.tx, cam.ty))
    Wf, Hf = F(W), F(H)
    out = []
    for k, o in enumerate(scene.m.objects):
        st = obj_states[k]
        mesh = scene.meshes.get(o.kind) or scene.meshes.get("*")
        V = mesh.verts.astype(F) * F(o.scale)
        T = V.shape[0]
        pos = np.asarray(st["pos"], dtype=np.float64).astype(F)
        ang = F(st["y_rot"]) * F(0.017453292519943295)
        co, so = np.cos(ang, dtype=F), np.sin(ang, dtype=F)

        def eye(P):
            rx, ry, rz = (P[..., 0] * co + P[..., 2] * so + pos[0]) - C[0], (P[..., 1] + pos[1]) - C[1], (-P[..., 0] * so + P[..., 2] * co + pos[2]) - C[2]
            xla, zla = rx * sa + rz * ca, -(rx * ca - rz * sa)
            return xla, ry * cth - zla * sth, -(ry * sth + zla * cth)

        # the object-level frustum cull: the eight corners of the mesh's box against near, left, right, bottom, top
        mn, mx = mesh.min_coords.astype(F) * F(o.scale), mesh.max_coords.astype(F) * F(o.scale)
        corners = np.array([[(mx if i & 1 else mn)[0], (mx if i & 2 else mn)[1], (mx if i & 4 else mn)[2]] for i in range(8)], dtype=F)
        xe, ye, w = eye(corners)
        lx, ly = w * tx, w * ty
        sx_, sy_ = np.abs(w) * tx * (F(4) / Wf), np.abs(w) * ty * (F(4) / Hf)
        outside = np.stack([w <= NEAR_Z, xe < -lx - sx_, xe > lx + sx_, ye < -ly - sy_, ye > ly + sy_])
        in_frustum = bool(st.get("visible", True)) and not outside.all(axis=1).any()
        xe, ye, w = eye(V)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            iw = F(1) / w
            sx = (xe * iw / tx + F(1)) * F(0.5) * Wf
            sy = (F(1) - ye * iw / ty) * F(0.5) * Hf
            area = (sx[:, 1] - sx[:, 0]) * (sy[:, 2] - sy[:, 0]) - (sx[:, 2] - sx[:, 0]) * (sy[:, 1] - sy[:, 0])
            box = np.stack([sx.min(axis=1) - TRI_PAD, sx.max(axis=1) + TRI_PAD, sy.min(axis=1) - TRI_PAD, sy.max(axis=1) + TRI_PAD], axis=1)
            ok = (w > NEAR_Z).all(axis=1) & (area != 0)
            ok &= ~((box[:, 1] < 0) | (box[:, 0] > Wf) | (box[:, 3] < 0) | (box[:, 2] > Hf))
        ok &= in_frustum
        live = bool(ok.any())
        obox = (box[ok, 0].min(), box[ok, 1].max(), box[ok, 2].min(), box[ok, 3].max()) if live else None
        assert ok.shape == (T,)
        out.append(ObjPass(live, ok, sx, sy, iw, box, obox))
    return out


def stale_triangles(history, cur):
    """Per object of the current pass `cur` the triangles a record reader would still test, as (pass they last survived, [T] mask): culled now,
    survivors of an earlier pass of `history` (oldest first) -- the LAST such pass is the one whose record stands.  Nothing of an object that
    is not live now: its ObjBox.count is 0."""
    out = []
    for k, now in enumerate(cur):
        last = np.full(now.ok.shape, -1)
        for i, h in enumerate(history):
            last[h[k].ok] = i
        out.append(np.where(now.live & ~now.ok, last, -1))
    return out


def stale_buffers(history, cur, W, H):
    """(depth [4, H, W], owner [4, H, W]) of the stale triangles alone at the four samples: inf / -1 where none covers the sample.  A triangle is
    tested at the pixels whose centre lies in its record's padded box and in the object's current ObjBox +- 1 px."""
    depth = np.full((4, H, W), np.inf)
    owner = np.full((4, H, W), -1, np.int64)
    cols, rows = np.meshgrid(np.arange(W, dtype=np.float64) + 0.5, np.arange(H, dtype=np.float64) + 0.5)
    for k, last in enumerate(stale_triangles(history, cur)):
        if not (last >= 0).any():
            continue
        b = cur[k].obox
        gate = (cols >= b[0] - 1) & (cols <= b[1] + 1) & (rows >= b[2] - 1) & (rows <= b[3] + 1)
        for t in np.flatnonzero(last >= 0):
            rec = history[last[t]][k]
            sx, sy, iw, bx = rec.sx[t].astype(np.float64), rec.sy[t].astype(np.float64), rec.iw[t].astype(np.float64), rec.box[t]
            cand = gate & (cols >= bx[0]) & (cols <= bx[1]) & (rows >= bx[2]) & (rows <= bx[3])
            if not cand.any():
                continue
            area = (sx[1] - sx[0]) * (sy[2] - sy[0]) - (sx[2] - sx[0]) * (sy[1] - sy[0])
            for q, (ox, oy) in enumerate(raster.SAMPLE_OFFSETS):
                qx, qy = cols + ox, rows + oy
                b0 = ((sx[1] - qx) * (sy[2] - qy) - (sx[2] - qx) * (sy[1] - qy)) / area
                b1 = ((sx[2] - qx) * (sy[0] - qy) - (sx[0] - qx) * (sy[2] - qy)) / area
                b2 = 1 - b0 - b1
                wq = b0 * iw[0] + b1 * iw[1] + b2 * iw[2]
                with np.errstate(divide="ignore", invalid="ignore"):
                    d = 1.0 / wq
                win = cand & (b0 >= 0) & (b1 >= 0) & (b2 >= 0) & (d >= raster.NEAR) & (d <= raster.FAR) & (d < depth[q])
                depth[q][win] = d[win]
                owner[q][win] = k
    return depth, owner


# ---- what a reader of stale records would return ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def passes(group, which):
    """setup_pass of every env of the group at its pose `which`: a tuple over envs of lists over objects."""
    c = case(group, which)
    sc = dm.scene_of(c)
    return tuple(setup_pass(dm.host_camera(c, e), sc, dm.host_objects(c)[e], c.W, c.H) for e in range(len(c.states)))


class Wrong(NamedTuple):
    stale: int               # stale triangles of the pair's object
    tris: int                # all its triangles
    depth: np.ndarray        # [H, W] bool: the depth map moves by more than INV_DEPTH_TOL
    labels: np.ndarray       # [H, W] bool: the label changes on a sure pixel of lm.expected
    instances: np.ndarray    # [H, W] bool: the id changes on a sure pixel of im.expected
    stale_depth: np.ndarray  # [H, W] the stale reader's depth map
    true_depth: np.ndarray   # [H, W] the oracle's


@functools.lru_cache(maxsize=None)
def predicted(name, kind=None, history=("prime",)):
    """The pixels of pair `name` a reader of stale records gets wrong after rendering the poses `history` and then the current one; through the
    source map `kind` (None / "fisheye") as the GPU tests run it."""
    p = PAIRS[name]
    e, c = env_of(name), case(p.group)
    cur = passes(p.group, "cur")[e]
    hist = [passes(p.group, h)[e] for h in history]
    sd, so = stale_buffers(hist, cur, c.W, c.H)
    d0, s0 = dm.host_buffers(c, e)
    wins = sd < d0
    d, srf = np.where(wins, sd, d0), np.where(wins, so, s0)
    cls0, _ = lm.sample_classes(c, e)
    obj_cls = lm.host_tables(c)[1]
    cls = np.where(wins, obj_cls[np.maximum(so, 0)], cls0)
    maps = [(dm.min_depth(d), dm.min_depth(d0), 0.0), (lm.labels_of(d, cls), lm.labels_of(d0, cls0), 0), (im.instances_of(d, srf), im.instances_of(d0, s0), 0)]
    sure_l, sure_i = lm.expected(c, e, kind)[1], im.expected(c, e, kind)[1]
    if kind is not None:
        rm = dm.rmap(c.W, c.H, kind)
        maps = [(dm.remap_nearest(a, rm, fill), dm.remap_nearest(b, rm, fill), fill) for a, b, fill in maps]
    (ds, dt, _), (ls, lt, _), (is_, it, _) = maps
    live = dt != 0
    with np.errstate(invalid="ignore"):
        wd = live & (np.abs(dm.inv(np.where(live, ds, 1.0)) - dm.inv(np.where(live, dt, 1.0))) > dm.INV_DEPTH_TOL)
    last = stale_triangles(hist, cur)[p.obj]
    return Wrong(int((last >= 0).sum()), int(last.size), wd, (ls != lt) & sure_l, (is_ != it) & sure_i, ds, dt)


def culled_now(cam, scene, obj_states, W, H):
    """How many triangles of LIVE objects one pass culls: what a drive must show at some step to prove anything."""
    return sum(int((~o.ok).sum()) for o in setup_pass(cam, scene, obj_states, W, H) if o.live)


# ---- a sphere the stale surface would hide ----------------------------------------------------------------------------------------------------

def hidden_sphere(name, pixels=7.0):
    """A world-space LED sphere (dtsim_draw_leds' row: centre, radius, colour, alpha) and its pixel: on the ray through a wrong depth pixel near
    the centroid of the pair's wrong depth pixels -- one of the quarter of them with the most room --, at a depth between the stale surface and
    the real one (their harmonic mean): in front of the scene, behind what a reader of stale records believes is there.  Its radius shows as
    `pixels` px of a 160-wide frame, and is at most 0.4 of the room to either surface; a pair that leaves it less than 5 mm is no pair for the
    LED test (asserted)."""
    p = PAIRS[name]
    c = case(p.group)
    cam = dm.host_camera(c, env_of(name))
    w = predicted(name)
    with np.errstate(invalid="ignore", divide="ignore"):
        mid = 2.0 / (1.0 / w.stale_depth + 1.0 / w.true_depth)
        room = np.where(w.depth, np.minimum(mid - w.stale_depth, w.true_depth - mid), 0.0)
    cy, cx = (float(v.mean()) for v in np.nonzero(w.depth))
    ys, xs = np.nonzero(room >= np.percentile(room[w.depth], 75))
    i = int(np.argmin((ys - cy) ** 2 + (xs - cx) ** 2))
    y, x = int(ys[i]), int(xs[i])
    t = float(mid[y, x])
    radius = min(pixels * (c.W / 160.0) * t * cam.tx / (0.5 * c.W), 0.4 * float(room[y, x]))
    assert radius >= 0.005, (name, radius)
    xe, ye, _, _ = raster._rays(cam, 2 * (x + 0.5) / c.W - 1, 1 - 2 * (y + 0.5) / c.H)
    # eye (t xe, t ye, -t) back to the world: the inverse of Camera.to_eye
    ex, ey, ez = t * xe, t * ye, -t
    yla, zla = ey * cam.cth + ez * cam.sth, -ey * cam.sth + ez * cam.cth
    rx, rz = ex * cam.sa - zla * cam.ca, ex * cam.ca + zla * cam.sa
    centre = cam.C + np.array([rx, yla, rz])
    assert np.allclose(cam.to_eye(centre), [ex, ey, ez], atol=1e-12)
    return np.array([*centre, radius, 1.0, 1.0, 1.0, 1.0], np.float32), (y, x)


def led_spheres(name):
    """The spheres dtsim_draw_leds is given for the pair's env: the hidden sphere first, then the usual set of tests/led_model.py at
    the current pose."""
    p = PAIRS[name]
    e, c = env_of(name), case(p.group)
    x, z, a = p.cur
    usual = sphere_set([x, 0.0, z], a, dm.host_objects(c)[e], 90 + e)
    return np.concatenate([hidden_sphere(name)[0][None], usual])


def hidden_pixels(name, sphere):
    """(hidden, shown): the pixels `sphere` changes of a black frame over the oracle's depth buffers and no longer changes over the stale
    reader's; and all those it changes over the oracle's."""
    p = PAIRS[name]
    e, c = env_of(name), case(p.group)
    cam = dm.host_camera(c, e)
    sd, _ = stale_buffers([passes(p.group, "prime")[e]], passes(p.group, "cur")[e], c.W, c.H)
    d0 = dm.host_buffers(c, e)[0]
    black = np.zeros((c.H, c.W, 3), np.uint8)
    true = raster.overlay_leds(black, cam, list(d0), sphere[None]).any(-1)
    stale = raster.overlay_leds(black, cam, list(np.minimum(d0, sd)), sphere[None]).any(-1)
    return true & ~stale, true


def parity_report():
    """The model's half of profiles/rerender_parity.txt: per pair and source map the stale triangles and the predicted wrong pixels."""
    lines = ["pair        map       size       stale / all triangles   predicted wrong pixels: depth  labels  instances   (rectilinear | fisheye)"]
    for n, p in PAIRS.items():
        g = GROUPS[p.group]
        a, b = predicted(n), predicted(n, "fisheye")
        lines.append(f"{n:10s}  {g.map_name:9s} {g.W:3d} x {g.H:3d}  {a.stale:3d} / {a.tris:3d}            "
                     f"{int(a.depth.sum()):5d} {int(a.labels.sum()):5d} {int(a.instances.sum()):5d}  |  {int(b.depth.sum()):5d} {int(b.labels.sum()):5d} {int(b.instances.sum()):5d}")
    return "\n".join(lines)
