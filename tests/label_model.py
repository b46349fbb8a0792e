"""The expected label map of dtsim_labels (include/dtsim.h), from the oracle alone, and the inputs both label tests share.

The quantity: per camera pixel the class of the surface that sets the depth -- of the four per-sample depth buffers of
depth_model.host_buffers the sample with the smallest depth (np.argmin: the lowest index on ties; a sky sample is inf, so it wins only when all
four are sky); its surface (depth_model.surfaces) gives the class: object k -> the class of k's mesh, the ground quad -> 2, the clear colour -> 1,
a tile -> the class of the nearest texel of the tile's texture, where the world hit is rebuilt from the sample's depth and ray in float64 and
goes through the ORACLE's tile texture coordinates (raster._tile_uv on the tile fraction, the tile's angle from raster.Scene).  Through the
fisheye by dm.remap_nearest(fill=0), smaller maps by dm.strided.

The host tables (tile kind -> [h, w] classes, object -> class) are built here from dtsim/labels.py without a device; the GPU test checks that
BatchedSimulator.label_assets() gives the same bytes.

SURE pixels, where the device must agree exactly: the four samples agree on the surface in the oracle's run and in its nudged run
(dm.host_camera(nudge=True)) and on the same one, and for a tile pixel every texel of the 3 x 3 neighbourhood of every sample's texel -- taken
in the world, one texel's width to each side of the hit, so that the neighbourhood of a texel on a tile seam lies on the next tile -- holds one
class, in both runs.  Elsewhere (silhouettes, tile seams, the edge texels of a marking) a disagreement is allowed on at most Case.cap of the
pixels: the shares frame parity allows for samples whose coverage flips, fp.ORACLE_PLANE.gt1 / fp.ORACLE_MESH.gt1.  tests/test_label_model_host.py
holds the oracle against its nudged self to a quarter of that on every case (profiles/labels_parity.txt)."""
import functools
import math
import os

import numpy as np

import depth_model as dm
import frame_parity as fp
from dtsim import assets, labels as L
from oracle import raster

# Lane markings filling the view (the 160 x 120 road poses of dm.CASES put a few hundred marking pixels in a frame): a camera 5 cm over the
# road, pitched 55 degrees down -- a footprint of some 10 cm -- through per-env camera records, as dm's "planes_dr".  small_loop, the straight
# at tile (2, 1): along its white line (3100 pixels of it), along the dashed yellow one (1000), and slanting across the other white line.
# test_town (the asset tree): over the red stop line of the 4way at tile (2, 3) coming from the west (3500 pixels), its east stop line and
# corner, and the yellow line of the straight north of it.
LOW_CAM = (0.05, 55.0, 75.0, (0.0, 0.0, 0.0))
_TS = 0.585
CASES = dict(dm.CASES)
CASES["marks_straight"] = dm.Case("small_loop", dm.W, dm.H, True, tuple(p + LOW_CAM for p in (
    (1.3, _TS + 0.06 * _TS, 0.0), (1.3, _TS + 0.5 * _TS, 0.15), (1.35, 1.12, -0.35))))
CASES["marks_town"] = dm.Case("test_town", dm.W, dm.H, True, tuple(p + LOW_CAM for p in (
    (1.15, 2.25, 0.0), (1.9, 1.9, math.pi), (1.46, 1.62, -math.pi / 2))), asset_tree=True, mesh=True)
OWN = tuple(n for n in CASES if n not in dm.CASES)


def case_of(name):
    """A name of CASES, or a dm.Case of the caller's own (dm.case_of)."""
    return name if isinstance(name, dm.Case) else CASES[name]


def scene_of(name):
    return dm._scene(case_of(name).map_name, case_of(name).asset_tree)


@functools.lru_cache(maxsize=None)
def host_buffers(name, e, nudge=False):
    """dm.host_buffers for every case of CASES: (depths [4, H, W], surfaces [4, H, W]) of env e on the oracle alone; read-only."""
    if isinstance(name, dm.Case) or name in dm.CASES:
        return dm.host_buffers(name, e, nudge)
    case, sc = CASES[name], scene_of(name)
    assert case.steps == 0
    cam = dm.host_camera(case, e, nudge)
    objs = [dict(pos=np.array(ob.pos, dtype=np.float64), y_rot=float(ob.y_rot), visible=True) for ob in sc.m.objects] or None
    depths, ids = dm.oracle_buffers(cam, sc, objs)
    srf = dm.surfaces(cam, depths, ids)
    depths.setflags(write=False); srf.setflags(write=False)
    return depths, srf


# ---- the host tables -------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def host_tables(name):
    """(tile kind -> [h, w] uint8 classes of its texture, [n_objects] class of every map object) of the case's scene: dtsim/labels.py's
    defaults, built as BatchedSimulator.label_assets() builds them."""
    case, sc = case_of(name), scene_of(name)
    lib = assets.AssetLibrary(fp.ASSETS) if case.asset_tree else assets.AssetLibrary(None)
    tiles = {}
    for kd, tex in sc.textures.items():
        p = lib.tile_texture_file(kd) if lib.root else None
        seg = assets.segment_texture(tex, p if p else os.path.join("tiles-processed", lib.style, kd, "texture.png"))
        tiles[kd] = L.texel_classes(tex, seg, kd)
    md = dm._map_data(case)
    keys = [lib.object_mesh(desc)[0] for desc in md.get("objects", [])]
    assert len(keys) == len(sc.m.objects)
    return tiles, L.mesh_classes(keys).astype(np.int64)


# ---- the model -------------------------------------------------------------------------------------------------------------------------

def nearest_sample(depths):
    """[H, W] index of the sample with the smallest depth; the lowest index on ties (all four sky: 0)."""
    return np.argmin(depths, axis=0)


def tile_class_at(sc, tiles, wx, wz):
    """The class of the texel a tile-plane hit (wx, wz) shows, or -1 off the grid / on an absent tile; an untextured tile: GROUND."""
    ts = sc.m.tile_size
    fi, fj = np.floor(wx / ts), np.floor(wz / ts)
    gh, gw = sc.present.shape
    ok = (fi >= 0) & (fj >= 0) & (fi < gw) & (fj < gh) & np.isfinite(wx) & np.isfinite(wz)
    i, j = np.where(ok, fi, 0).astype(np.int64), np.where(ok, fj, 0).astype(np.int64)
    ok &= sc.present[j, i]
    u, v = raster._tile_uv(sc.angle[j, i], wx / ts - i, wz / ts - j)            # the oracle's tile texture coordinates
    out = np.full(wx.shape, -1, np.int64)
    kinds = np.array([[hash(k) for k in row] for row in sc.kinds])[j, i]
    for kd in {k for row in sc.kinds for k in row if k is not None}:
        sel = ok & (kinds == hash(kd))
        if not sel.any():
            continue
        t = tiles.get(kd)
        if t is None:
            out[sel] = L.GROUND
            continue
        h, w = t.shape
        x = np.floor(u[sel] * w).astype(np.int64) % w                          # nearest texel, GL_REPEAT
        y = np.floor(v[sel] * h).astype(np.int64) % h
        out[sel] = t[y, x]
    return out


def world_hit(cam, depth, tile, q):
    """World (x, z) [H, W] of sample q's hit on the tile plane, rebuilt in float64 from the sample's depth and ray; the camera's own (x, z) where
    `tile` (the sample's surface is the tile plane) is False."""
    cols, rows = np.meshgrid(np.arange(cam.W, dtype=np.float64), np.arange(cam.H, dtype=np.float64))
    ox, oy = raster.SAMPLE_OFFSETS[q]
    nx = 2 * (cols + 0.5) / cam.W - 1 + 2 * ox / cam.W
    ny = 1 - 2 * (rows + 0.5) / cam.H - 2 * oy / cam.H
    xe, ye, yla, fwd = raster._rays(cam, nx, ny)
    t = np.where(tile, depth, 0.0)
    rr, ff = t * xe, t * fwd
    return cam.C[0] + rr * cam.sa + ff * cam.ca, cam.C[2] + rr * cam.ca - ff * cam.sa


def sample_classes(name, e, nudge=False, tables=None):
    """(cls [4, H, W] the class of every sample's surface, same [4, H, W] bool: the 3 x 3 texel neighbourhood of a tile sample holds one
    class; True for the other surfaces).  tables: (tile kind -> classes, object -> class) in place of host_tables(name)."""
    case, sc = case_of(name), scene_of(name)
    depths, srf = host_buffers(name, e, nudge)
    return sample_classes_of(dm.host_camera(case, e, nudge), sc, host_tables(name) if tables is None else tables, depths, srf)


def sample_classes_of(cam, sc, tables, depths, srf):
    """sample_classes' rule on any camera, scene, tables (tile kind -> classes, object -> class) and per-sample (depths, surfaces): a state read
    back from a device has no case."""
    tiles, obj_cls = tables
    cls = np.empty(srf.shape, np.int64)
    same = np.ones(srf.shape, bool)
    texel = sc.m.tile_size / max(t.shape[0] for t in tiles.values())
    for q in range(len(raster.SAMPLE_OFFSETS)):
        tile = srf[q] == -1
        wx, wz = world_hit(cam, depths[q], tile, q)
        c = tile_class_at(sc, tiles, wx, wz)
        ok = np.ones(tile.shape, bool)
        for dx in (-texel, 0.0, texel):
            for dz in (-texel, 0.0, texel):
                ok &= tile_class_at(sc, tiles, wx + dx, wz + dz) == c
        ok &= c >= 0
        k = srf[q]
        c = np.where(tile, c, np.where(k >= 0, obj_cls[np.maximum(k, 0)] if len(obj_cls) else 0, np.where(k == -2, L.GROUND, L.SKY)))
        cls[q], same[q] = c, np.where(tile, ok, True)
    return cls, same


def labels_of(depths, cls):
    """[H, W] the class of the nearest sample."""
    return np.take_along_axis(cls, nearest_sample(depths)[None], axis=0)[0]


@functools.lru_cache(maxsize=None)
def expected(name, e, kind=None, nudge=False):
    """(labels [H, W] uint8, sure [H, W] bool) of env e of the case: full size, through the source map `kind` (None / "fisheye" /
    "undistort") by nearest source pixel with class 0 -- and sure -- where a pixel has no source.  Cached, read-only."""
    return expected_with(name, e, kind, nudge, None)


def expected_with(name, e, kind=None, nudge=False, tables=None):
    """expected() under a user's tables (sample_classes' `tables`); not cached."""
    case = case_of(name)
    d0, s0 = host_buffers(name, e, False)
    d1, s1 = host_buffers(name, e, True)
    c0, same0 = sample_classes(name, e, False, tables)
    c1, same1 = sample_classes(name, e, True, tables)
    lab = labels_of(d1 if nudge else d0, c1 if nudge else c0)
    agree = (s0 == s0[0]).all(axis=0) & (s1 == s1[0]).all(axis=0) & (s0[0] == s1[0])
    one = (c0 == c0[0]).all(axis=0) & (c1 == c1[0]).all(axis=0) & (c0[0] == c1[0])
    sure = agree & one & same0.all(axis=0) & same1.all(axis=0)
    assert lab.min() >= 1 and lab.max() <= 255
    if kind is not None:
        rm = dm.rmap(case.W, case.H, kind)
        lab = dm.remap_nearest(lab, rm, fill=0)
        sure = dm.remap_nearest(sure, rm, fill=True)
    lab = lab.astype(np.uint8)
    lab.setflags(write=False); sure.setflags(write=False)
    return lab, sure


def compare(got, want, sure, cap, ctx=None):
    """A device map against the expected one: class 0 on exactly the same set; exact equality on the sure pixels; elsewhere a different class
    on at most `cap` of ALL the map's pixels.  Returns dict(off=share of pixels that differ, n_off, unsure=share of pixels not sure)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape == sure.shape and got.dtype == np.uint8, (ctx, got.shape, want.shape, got.dtype)
    assert np.array_equal(got == 0, want == 0), (ctx, "border pixels differ", int((got == 0).sum()), int((want == 0).sum()))
    diff = got != want
    out = dict(off=float(diff.mean()), n_off=int(diff.sum()), unsure=float((~sure).mean()))
    assert not (diff & sure).any(), (ctx, out, "sure pixels differ", [(int(y), int(x), int(got[y, x]), int(want[y, x])) for y, x in np.argwhere(diff & sure)[:8]])
    assert out["off"] <= cap, (ctx, out, [(int(y), int(x), int(got[y, x]), int(want[y, x])) for y, x in np.argwhere(diff)[:8]])
    return out


def nudge_share(name, e):
    """The oracle's map of env e against its nudged self: dict(off = share of ALL pixels with another class, unsure = share not sure,
    sure_off = differing pixels ON the sure mask (0 by construction of the mask))."""
    a, sure = expected(name, e)
    b, _ = expected(name, e, None, True)
    diff = a != b
    return dict(off=float(diff.mean()), n_off=int(diff.sum()), unsure=float((~sure).mean()), sure_off=int((diff & sure).sum()), pixels=int(diff.size))


def parity_report():
    """The text of profiles/labels_parity.txt."""
    lines = ["dtsim_labels: what tests/test_gpu_labels.py allows off the sure mask, checked on the oracle by tests/test_label_model_host.py "
             "(python -c 'import label_model as m; print(m.parity_report())')",
             "oracle/raster.py against itself from the float32-rounded pose scaled by 1 + 2e-7",
             "off:    share of ALL pixels whose class differs between the two runs; bound: a quarter of the cap",
             "unsure: share of pixels off the sure mask (samples on several surfaces, or a class edge within a texel of a sample)", ""]
    for name, c in CASES.items():
        for e in range(len(c.states)):
            r = nudge_share(name, e)
            lab, _ = expected(name, e)
            lines.append(f"{name:14s} env {e}  {c.W:3d} x {c.H:3d}  off {r['off']:.2e} ({r['n_off']:2d} px)  unsure {r['unsure']:.3f}  (cap / 4 = {c.cap / 4:.2e})  "
                         f"classes {' '.join(f'{int(k)}:{int(n)}' for k, n in zip(*np.unique(lab, return_counts=True)))}")
    return "\n".join(lines)
