"""The expected bird's-eye maps of dtsim_bev (include/dtsim.h), from the oracle's side alone, and the inputs both BEV tests share.

The quantity: cell (i, j) of env e stands for the world point P = (x, z) + f d + s r of the AGENT's pose (x, z, theta), d = (cos theta,
-sin theta), r = (sin theta, cos theta), f = (oh - rows_behind - i - 0.5) cell, s = (j + 0.5 - ow / 2) cell; its class is that of the mesh of the
lowest-indexed drawn object (visible, with a mesh) whose collision rectangle holds P, else that of the nearest texel of the tile under P --
label_model.tile_class_at: the oracle's raster._tile_uv on the tile fraction, the tile's angle from raster.Scene --, else GROUND; its id is
o + 1 or 0.  Everything here is numpy in float64; the rectangles come in the shape of BatchedSimulator.object_footprints().

The CANDIDATE SET of a cell: every class (id) it could take if P moved by up to M in any direction --
  * the classes over the 3 x 3 texel neighbourhood of P's texel, taken in the world (one texel's width to each side: across tile seams and
    the grid's border, where the alternative is GROUND);
  * the class (id) of every drawn object whose rectangle's border comes within M of P, inside or outside;
  * the class (id) of the lowest-indexed object that holds P more than M from its border, and only when there is none the tile alternative
    (id 0).
A cell is SURE when its set has one member: there the device must agree exactly; elsewhere it must name a member of the set.

M = 1e-4 m is derived, not chosen: coordinates stay below 32 m (a 24 x 32 padded grid of tiles of at most 0.585 m), where a float32 ulp is at
most 2^-19 m; fewer than 16 roundings lie between the double pose and the device's comparison, i.e. at most 3.1e-5 m; M is three times that.
A texel is 2.3e-3 m, so the texel neighbourhood is wider still."""
import copy
import functools
import math
import os
from typing import NamedTuple, Optional

import numpy as np

import crowd_scenes as cs
import depth_model as dm
import frame_parity as fp
import label_model as lm
import multimap_scenes as ms
from dtsim import assets, labels as L
from oracle import sim as osim
from util import EXT

M = 1e-4                                # metres a cell's point may move: 3 * 16 * 2^-19 = 9.2e-5, rounded up
assert 3 * 16 * 2.0 ** -19 <= M < 1.1 * 3 * 16 * 2.0 ** -19
TS = 0.585
N_IDS = 65                              # ids 0 .. 64

# ---- the cases ------------------------------------------------------------------------------------------------------------------------
# (oh, ow, cell, rows_behind): 64 x 64; neither size a multiple of four; one cell; the agent inside the window; the whole window behind it
SHAPES = ((64, 64, 0.02, 0), (37, 53, 0.013, 0), (1, 1, 0.02, 0), (128, 96, 0.01, 32), (16, 24, 0.02, 16))
# x, z (metres), theta: on the road; on a tile border (x = 2 tiles exactly) looking along it; at the grid's corner looking outward (most of
# the window off the grid); negative coordinates; theta beyond 2 pi; theta negative beyond -2 pi
COMMON = ((1.0, 0.9, 0.3), (2 * TS, 0.9, math.pi / 2), (0.05, 0.04, 3 * math.pi / 4), (-0.3, -0.2, -0.7), (1.9, 1.5, 40.5), (2.0, 1.1, -7.5))
START = (1.0, 0.9, 0.3)                 # where every env stands while the case's steps run (zero actions: it stays)


class Case(NamedTuple):
    maps: tuple                         # resident maps; env e is on map e % len(maps)
    poses: tuple                        # env e takes pose (e % 64) % len(poses)
    steps: int = 0                      # zero-action steps before the poses are written (the walking duckies move)
    wait: Optional[float] = None        # the walking duckies' wait before their first walk, s
    hidden: tuple = ()                  # object indices made invisible in every env
    asset_tree: bool = False


def _xyz(states):
    return tuple((float(s[0]), float(s[1]), float(s[2])) for s in states)


CASES = {
    "small_loop": Case(("small_loop",), COMMON),
    "loop_pedestrians": Case(("loop_pedestrians",), COMMON + _xyz(dm.CASES["pedestrians"].states), steps=40, wait=0.2),
    "test_town": Case(("test_town",), COMMON + _xyz(dm.CASES["town"].states) + _xyz(lm.CASES["marks_town"].states), asset_tree=True),
    "crowd": Case(("crowd",), COMMON + tuple((x * TS, z * TS, a) for x, z, a in cs.POSES.values()), hidden=tuple(range(0, 64, 3))),
    "two_maps": Case(("loop_pedestrians", "mm_t47"), COMMON),
}
N = 130                                 # two full chunks of 64 and a tail of 2


def pose_of(case, e):
    return case.poses[(e % 64) % len(case.poses)]


def map_of(case, e):
    return e % len(case.maps)


def map_data(name):
    if name == "test_town":
        return fp.asset_scene()[1]
    if name == "crowd":
        return cs.crowd_map()
    return ms.map_data(name)


class MapModel(NamedTuple):
    sc: object                          # raster.Scene
    tiles: dict                         # tile kind -> [h, w] uint8 classes
    obj_cls: np.ndarray                 # [n_objects] class of every object's mesh
    texel: float                        # metres per texel


@functools.lru_cache(maxsize=None)
def map_model(name):
    """The oracle's scene of map `name` and the default tables of dtsim/labels.py on it, built as label_model.host_tables builds them."""
    town = name == "test_town"
    sc = fp.asset_scene()[0] if town else cs.scene("crowd") if name == "crowd" else ms.scene(name)
    lib = assets.AssetLibrary(fp.ASSETS) if town else assets.AssetLibrary(None)
    tiles = {}
    for kd, tex in sc.textures.items():
        p = lib.tile_texture_file(kd) if lib.root else None
        seg = assets.segment_texture(tex, p if p else os.path.join("tiles-processed", lib.style, kd, "texture.png"))
        tiles[kd] = L.texel_classes(tex, seg, kd)
    keys = [lib.object_mesh(d)[0] for d in (map_data(name).get("objects") or []) if d["kind"] != "floor_tag"]
    assert len(keys) == len(sc.m.objects)
    return MapModel(sc, tiles, L.mesh_classes(keys).astype(np.int64), sc.m.tile_size / max(t.shape[0] for t in tiles.values()))


@functools.lru_cache(maxsize=None)
def host_footprints(case_name):
    """Per resident map (corners [K, 4, 2] float64, drawn [K] bool) of the case on the oracle alone: the objects' collision rectangles after
    the case's zero-action steps from START (the oracle's own physics: the duckies walk), every object with a mesh, the hidden ones not drawn."""
    case = CASES[case_name]
    out = []
    for name in case.maps:
        ext = fp.asset_scene()[2] if case.asset_tree else EXT
        o = osim.OracleSim(copy.deepcopy(map_data(name)), ext, do_reset=False, max_steps=10 ** 6)
        o.wheel_dist = osim.WHEEL_DIST
        o.set_pose([START[0], 0.0, START[1]], START[2])
        for ob in o.map.objects:
            if case.wait is not None and not ob.static and ob.kind == "duckie":
                ob.pedestrian_wait_time = case.wait
        for _ in range(case.steps):
            o.step(np.zeros(2))
        corners = np.array([np.asarray(ob.obj_corners, np.float64).reshape(4, 2) for ob in o.map.objects], np.float64).reshape(-1, 4, 2)
        drawn = np.array([k not in case.hidden for k in range(len(corners))], bool)
        corners.setflags(write=False); drawn.setflags(write=False)
        out.append((corners, drawn))
    return tuple(out)


# ---- the model ------------------------------------------------------------------------------------------------------------------------

def cell_points(pose, oh, ow, cell, rows_behind):
    """(wx, wz) [oh, ow] float64: the world point of every cell."""
    x, z, th = pose
    f = (oh - rows_behind - np.arange(oh, dtype=np.float64) - 0.5)[:, None] * cell
    s = (np.arange(ow, dtype=np.float64) + 0.5 - ow / 2)[None, :] * cell
    c, sn = math.cos(th), math.sin(th)
    return x + f * c + s * sn, z - f * sn + s * c


def inside(quad, px, pz):
    """P in the convex quadrilateral quad [4, 2] (its border included): on one side of all four edges."""
    pos = np.ones(np.shape(px), bool)
    neg = np.ones(np.shape(px), bool)
    for k in range(4):
        ax, az = quad[k]
        bx, bz = quad[(k + 1) % 4]
        cr = (bx - ax) * (pz - az) - (bz - az) * (px - ax)
        pos &= cr >= 0
        neg &= cr <= 0
    return pos | neg


def border_distance(quad, px, pz):
    """Distance from P to the quadrilateral's border (its four edge segments)."""
    d = np.full(np.shape(px), np.inf)
    for k in range(4):
        ax, az = quad[k]
        ex, ez = quad[(k + 1) % 4][0] - ax, quad[(k + 1) % 4][1] - az
        ll = ex * ex + ez * ez
        t = np.clip(((px - ax) * ex + (pz - az) * ez) / ll, 0.0, 1.0) if ll > 0 else np.zeros(np.shape(px))
        d = np.minimum(d, np.hypot(px - (ax + t * ex), pz - (az + t * ez)))
    return d


def tile_class(mm, wx, wz):
    """label_model's world hit -> _tile_uv -> nearest texel on the host tables; off the grid and on absent tiles: GROUND."""
    c = lm.tile_class_at(mm.sc, mm.tiles, wx, wz)
    return np.where(c < 0, L.GROUND, c)


class Expected(NamedTuple):
    cls: np.ndarray                     # [oh, ow] uint8
    inst: np.ndarray                    # [oh, ow] uint8
    cand_cls: np.ndarray                # [oh, ow, 256] bool
    cand_id: np.ndarray                 # [oh, ow, N_IDS] bool
    sure_cls: np.ndarray                # [oh, ow] bool: one candidate class
    sure_id: np.ndarray                 # [oh, ow] bool


def expected(mm, pose, corners, drawn, shape, tables=None, m=M):
    """The maps of one env: mm its map's MapModel, corners [K, 4, 2] / drawn [K] its row of object_footprints(), shape = (oh, ow, cell,
    rows_behind).  tables: (tile kind -> classes, object -> class) in place of mm's."""
    oh, ow, cell, rb = shape
    if tables is not None:
        mm = mm._replace(tiles=tables[0], obj_cls=np.asarray(tables[1], np.int64))
    wx, wz = cell_points(pose, oh, ow, cell, rb)
    tile = tile_class(mm, wx, wz)
    cand_cls = np.zeros((oh, ow, 256), bool)
    cand_id = np.zeros((oh, ow, N_IDS), bool)
    ii, jj = np.indices((oh, ow))
    tile_alt = np.zeros((oh, ow, 256), bool)
    for dx in (-mm.texel, 0.0, mm.texel):
        for dz in (-mm.texel, 0.0, mm.texel):
            tile_alt[ii, jj, tile_class(mm, wx + dx, wz + dz)] = True
    cls, inst = tile.copy(), np.zeros((oh, ow), np.int64)
    owned = np.zeros((oh, ow), bool)    # a lower-indexed object holds P
    deep = np.zeros((oh, ow), bool)     # ... more than m from its border
    for o in range(min(len(corners), len(mm.obj_cls))):
        if not drawn[o]:
            continue
        q = np.asarray(corners[o], np.float64)
        ins, bd = inside(q, wx, wz), border_distance(q, wx, wz)
        first = ins & ~owned
        cls[first], inst[first] = mm.obj_cls[o], o + 1
        owned |= ins
        cand = (bd <= m) | (ins & ~deep)                      # near its border, or the lowest one that holds P deeply (and those before it)
        cand_cls[cand, mm.obj_cls[o]] = True
        cand_id[cand, o + 1] = True
        deep |= ins & (bd > m)
    cand_cls |= tile_alt & ~deep[..., None]
    cand_id[..., 0] |= ~deep
    assert cand_cls[ii, jj, cls].all() and cand_id[ii, jj, inst].all()
    assert cls.min() >= 2
    return Expected(cls.astype(np.uint8), inst.astype(np.uint8), cand_cls, cand_id, cand_cls.sum(-1) == 1, cand_id.sum(-1) == 1)


def loop_expected(mm, pose, corners, drawn, shape):
    """(cls, inst) by a plain double loop over the cells, one scalar point at a time."""
    oh, ow, cell, rb = shape
    x, z, th = pose
    cls, inst = np.zeros((oh, ow), np.uint8), np.zeros((oh, ow), np.uint8)
    for i in range(oh):
        for j in range(ow):
            f, s = (oh - rb - i - 0.5) * cell, (j + 0.5 - ow / 2) * cell
            px = x + f * math.cos(th) + s * math.sin(th)
            pz = z - f * math.sin(th) + s * math.cos(th)
            for o in range(len(corners)):
                if drawn[o] and bool(inside(np.asarray(corners[o]), np.float64(px), np.float64(pz))):
                    cls[i, j], inst[i, j] = mm.obj_cls[o], o + 1
                    break
            else:
                cls[i, j] = tile_class(mm, np.array([px]), np.array([pz]))[0]
    return cls, inst


def compare(got_cls, got_inst, want, ctx=None):
    """Device maps of one env against `want` (either may be None): equal on the sure cells, a member of the candidate set elsewhere, no 0 / 1
    class.  Returns dict(differ = cells whose value is not the model's, fell_back = of those the ones a candidate set admitted)."""
    out = dict(differ=0, fell_back=0)
    ii, jj = np.indices(want.cls.shape)
    for got, exp, cand, sure, what in ((got_cls, want.cls, want.cand_cls, want.sure_cls, "class"), (got_inst, want.inst, want.cand_id, want.sure_id, "id")):
        if got is None:
            continue
        got = np.asarray(got)
        assert got.shape == exp.shape and got.dtype == np.uint8, (ctx, what, got.shape, exp.shape, got.dtype)
        if what == "class":
            assert got.min() >= 2, (ctx, "class 0 / 1 occurs", np.argwhere(got < 2)[:4].tolist())
        else:
            assert got.max() < N_IDS, (ctx, "id beyond 64")
        diff = got != exp
        bad = diff & sure
        assert not bad.any(), (ctx, what, "sure cells differ", [(int(i), int(j), int(got[i, j]), int(exp[i, j])) for i, j in np.argwhere(bad)[:8]])
        member = cand[ii, jj, got]
        assert member.all(), (ctx, what, "not a candidate", [(int(i), int(j), int(got[i, j]), int(exp[i, j])) for i, j in np.argwhere(~member)[:8]])
        out["differ"] += int(diff.sum())
        out["fell_back"] += int((diff & member).sum())
    return out


@functools.lru_cache(maxsize=None)
def host_expected(case_name, k, shape):
    """expected() of pose k of the case on the host's footprints, per resident map: a tuple over the maps."""
    case = CASES[case_name]
    return tuple(expected(map_model(name), case.poses[k], *host_footprints(case_name)[mi], shape) for mi, name in enumerate(case.maps))


def sure_shares(case_name, shape):
    """(share of cells with a sure class, share with a sure id) over every pose and map of the case at `shape`."""
    case = CASES[case_name]
    ex = [e for k in range(len(case.poses)) for e in host_expected(case_name, k, shape)]
    return float(np.mean([e.sure_cls.mean() for e in ex])), float(np.mean([e.sure_id.mean() for e in ex]))


def parity_report():
    """The host's part of profiles/bev_parity.txt."""
    lines = ["dtsim_bev: the share of SURE cells (one candidate class / id within M = 1e-4 m) of every case of tests/test_gpu_bev.py, from the "
             "model alone (python -c 'import bev_model as m; print(m.parity_report())'); tests/test_bev_model_host.py holds each to >= 0.80", ""]
    for name, c in CASES.items():
        for shape in SHAPES:
            a, b = sure_shares(name, shape)
            lines.append(f"{name:17s} {shape[0]:3d} x {shape[1]:3d} cell {shape[2]:.3f} behind {shape[3]:3d}  poses {len(c.poses):2d} x maps {len(c.maps)}  "
                         f"sure class {a:.4f}  sure id {b:.4f}")
    return "\n".join(lines)
