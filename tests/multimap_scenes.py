"""Map sets at the limits of the raster dispatch (csrc/render.hip dt_raster_pipe), shared by tests/test_multimap_scenes_host.py (the packer and
the oracle alone: do the sets sit where they are meant to sit, do the poses reach the far table entries?) and tests/test_gpu_multimap_render.py.

k_raster_v3 / k_raster_v3dr keep the tile tables of all resident maps side by side in one LDS row -- 32 columns a map, at most 4 maps -- and
need a padded grid (map + 4 tiles of ring each side) of at most 24 rows x 32 columns: a map of 24 x 16 tiles.  Past either limit the shared
camera falls to k_raster_q and domain randomisation to the generic per-env raster.  The sets:

  S3, S4, S5   three, four and five of the library's maps (S4 fills the row: columns 96 .. 127; S5 is one map past it)
  P4           four object-free 5 x 5 maps, so that the OBJ = false instantiations reach map ids 2 and 3
  L1, L2, L4   edge(24, 16) -- a padded grid of exactly 24 x 32 -- alone, first of two, and LAST of four (columns 96 .. 127, rows up to 23;
               there with four duckies at its far corner)
  Lw, Lh       edge(25, 16) and edge(24, 17): one column / one row past the limit (Lh with the duckies)
  T2           small_loop at 0.585 m and the same tiles at 0.47 m: q_per_m is the larger of the two

edge(w, h): a road ring along the border (drivable corner cells), grass and asphalt inside with two empty cells, and next to the far corner one
tile in the last column and one in the last row of a kind that appears nowhere else in the map (SPECIAL: a dark plain texture of its own).

Eight poses per map, each at least MARGIN inside the outer border: from the first tile along the z = 0 border (5e-5 rad off the axis) and
diagonally outward; from the last tile along the last row (5e-5 rad off the axis), along the last column and diagonally inward; outward over
the last column and over the last row from the tiles next to the far corner (edge(): the SPECIAL ones); the centre.  The outward views show a
sliver of their tile, then ring and ground.

The batch: N = 130 -- two chunks of 64 envs and a tail of 2.  Envs 0 .. 63 interleave the maps (e % n_maps); envs 64 .. 129 all stand on the
highest map id.  Env e takes pose pose_of(mode)[e]; env e + 65 repeats env e's pose, so wherever env e stands on the highest map id -- every env
of a one-map set -- the state appears twice, at e and e + 65 (replicas()).  The quad-record rasters run in k_env_sort's order, so which envs
share a workgroup chunk is the sort's business: the GPU test holds EVERY env to its one-map handle, and the oracle to the envs picks() names.
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
W, H, N = 160, 120, 130
QRING, V3_MAX_ROWS, V3_MAP_COLS, V3_TAB_PITCH = 4, 24, 32, 256     # csrc/scene_tables.h DT_QRING; csrc/raster_common.h; csrc/render_records.h
MARGIN = 0.1                                                       # metres from the outer border to the nearest pose
# ... of the outward views, on an object-free map and on a map with objects: the tile under the camera fills 3 % / 7 % of the frame.  At the
# far corner of the 24 x 16 map the oracle's byte-weight filter moves by +-1 on a tenth of the tile pixels when the pose moves by a float32's
# worth; these shares keep that within a quarter of ORACLE_PLANE's / ORACLE_MESH's mean (tests/test_multimap_scenes_host.py).
OUT_MARGIN = {False: 0.134, True: 0.143}
SEED = 47

_G, _A, _F = "grass", "asphalt", "floor"
_P1 = [[_A] * 5,
       [_A, "curve_left/W", "straight/E", "curve_left/N", _A],
       [_A, "straight/S", _F, "straight/S", _A],
       [_A, "curve_left/S", "straight/E", "curve_left/E", _A],
       [_A] * 5]
_P2 = [[_G, _G, "straight/N", _G, _G],
       [_G, _F, "straight/N", _F, _G],
       ["straight/W", "straight/W", "4way", "straight/E", "straight/E"],
       [_G, _F, "straight/S", _F, _G],
       [_G, _G, "straight/S", _G, _G]]
_P3 = [[_G] * 5,
       [_G, "3way_left/S", "straight/E", "3way_left/N", _G],
       [_G, "straight/N", _F, "straight/N", _G],
       [_G, "3way_right/W", "straight/W", "3way_right/E", _G],
       [_G] * 5]
SPECIAL = "tarmac"                                                  # edge(): the kind of tiles (w - 1, h - 2) and (w - 2, h - 1) only


def edge(w, h, objects=False):
    """The w x h map of the module docstring.  objects: four static duckies within a tile of the far corner (w - 1, h - 1)."""
    rows = [[(_G if (i // 2 + j // 3) % 2 else _A) for i in range(w)] for j in range(h)]
    for i in range(w):
        rows[0][i] = rows[h - 1][i] = "straight/E"
    for j in range(h):
        rows[j][0] = rows[j][w - 1] = "straight/S"
    rows[0][0], rows[0][w - 1], rows[h - 1][0], rows[h - 1][w - 1] = "curve_right/N", "curve_right/E", "curve_right/W", "curve_right/S"
    rows[h - 2][w - 1] = rows[h - 1][w - 2] = SPECIAL
    rows[2][2] = rows[h - 3][w - 3] = "empty"
    objs = []
    if objects:
        spec = (((w - 1.6, h - 0.5), 40, 0.06), ((w - 0.5, h - 1.7), 130, 0.08), ((w - 1.35, h - 1.3), 250, 0.07), ((w - 0.45, h - 0.62), 10, 0.05))
        objs = [dict(kind="duckie", pos=list(p), rotate=r, height=ht, static=True, optional=False) for p, r, ht in spec]
    return dict(tiles=rows, objects=objs, tile_size=TS)


OWN_MAPS = {
    "mm_p1": dict(tiles=_P1, objects=[], tile_size=TS), "mm_p2": dict(tiles=_P2, objects=[], tile_size=TS), "mm_p3": dict(tiles=_P3, objects=[], tile_size=TS),
    "mm_L": edge(24, 16), "mm_Lo": edge(24, 16, True), "mm_Lw": edge(25, 16), "mm_Lh": edge(24, 17, True),
    "mm_t47": dict(assets.get_map("small_loop"), tile_size=0.47),
}
_S3 = ["small_loop", "loop_only_duckies", "small_loop_only_duckies"]
SETS = {
    "S3": _S3, "S4": _S3 + ["loop_pedestrians"], "S5": _S3 + ["loop_pedestrians", "loop_dyn_duckiebots"],
    "P4": ["small_loop", "mm_p1", "mm_p2", "mm_p3"],
    "L1": ["mm_L"], "L2": ["mm_L", "small_loop"], "L4": ["small_loop", "small_loop_only_duckies", "loop_only_duckies", "mm_Lo"],
    "Lw": ["mm_Lw"], "Lh": ["mm_Lh"],
    "T2": ["small_loop", "mm_t47"],
}
V3_SETS = ("S3", "S4", "P4", "L1", "L2", "L4", "T2")               # the issue's table: these stay on the v3 kernels, the others fall off
MODES = ("shared", "dr", "light")


def map_data(name):
    import copy
    return copy.deepcopy(OWN_MAPS[name]) if name in OWN_MAPS else assets.get_map(name)


def patch_maps(monkeypatch):
    """The module's own maps as fixtures of the asset library, so that one simulator can hold them by name."""
    for name in OWN_MAPS:
        monkeypatch.setitem(assets.MAPS, name, map_data(name))


def dims(name):
    md = map_data(name)
    return len(md["tiles"][0]), len(md["tiles"])


def has_objects(set_name):
    return any(map_data(n)["objects"] for n in SETS[set_name])


@functools.lru_cache(maxsize=None)
def scene(name):
    om = osim.OracleMap(map_data(name), EXT)
    tex = {k: assets.get_texture(k) for k in {t["kind"] for t in om.grid if t is not None}}
    return raster.Scene(om, tex, {"duckie": assets.get_mesh("duckie"), "*": assets.get_mesh("*")})


# ---- the dispatch, restated ----------------------------------------------------------------------------------------------------------

def set_tables(names, tex_side=256):
    """What dtsim_set_maps keeps of a set (csrc/scene_tables.h dt_pack_maps): dict(qlog2, n_qtiles, grid_rows, grid_cols, n_maps)."""
    d = [dims(n) for n in names]
    rows, cols = max(h for _, h in d) + 2 * QRING, max(w for w, _ in d) + 2 * QRING
    qlog2 = int(math.log2(tex_side)) if tex_side >= 2 and tex_side & (tex_side - 1) == 0 else 0
    if max(rows, cols) * tex_side >= 32768:
        qlog2 = 0
    return dict(qlog2=qlog2, n_qtiles=sum((w + 2 * QRING) * (h + 2 * QRING) for w, h in d) if qlog2 else 0, grid_rows=rows, grid_cols=cols, n_maps=len(names))


def expected_pipeline(set_name, dr=False, light=False, raster_old=False, width=W):
    """BatchedSimulator.render_pipeline of a plain pass over the set: dt_raster_pipe, restated."""
    t = set_tables(SETS[set_name])
    light = light and not dr
    v3 = t["qlog2"] == 8 and t["grid_rows"] <= V3_MAX_ROWS and t["grid_cols"] <= V3_MAP_COLS and t["n_maps"] * V3_MAP_COLS <= V3_TAB_PITCH // 2 and not raster_old
    records = t["qlog2"] > 0 and width % 4 == 0
    if records and not dr and t["n_qtiles"] * 8 <= 32768 and not (t["qlog2"] == 8 and max(t["grid_rows"], t["grid_cols"]) >= 256):
        name = "k_raster_v3" if v3 else "k_raster_q"
    elif records and dr and v3:
        name = "k_raster_v3dr"
    else:
        name = "k_raster_env" if (dr or light) else "k_raster"
    return name + ("+light" if light else "")


# ---- poses, layout, states -----------------------------------------------------------------------------------------------------------

def poses(name):
    """The eight (x, z, angle) of the module docstring on map `name` (direction of view: (cos a, -sin a))."""
    (w, h), ts = dims(name), map_data(name)["tile_size"]
    x1, z1, out = w * ts - MARGIN, h * ts - MARGIN, OUT_MARGIN[bool(map_data(name)["objects"])]
    return ((MARGIN, MARGIN, 5e-5),                                        # 0 first tile, along the z = 0 border (+x), a hair off the axis
            (out, out, 0.75 * math.pi),                                    # 1 first tile, diagonally outward: a sliver of the tile, then ring and ground
            (x1, z1, math.pi - 5e-5),                                      # 2 last tile, along the last row (-x), a hair off the axis
            (x1, z1, math.pi / 2 + 0.03),                                  # 3 last tile, along the last column (-z)
            (x1, z1, 0.75 * math.pi),                                      # 4 last tile, diagonally inward
            (w * ts - out, (h - 1.5) * ts, 0.2),                           # 5 last column, the tile above the corner (edge(): SPECIAL), outward (+x)
            ((w - 1.5) * ts, h * ts - out, -math.pi / 2 - 0.2),            # 6 last row, the tile left of the corner (edge(): SPECIAL), outward (+z)
            (0.5 * w * ts + 0.11, 0.5 * h * ts + 0.07, 0.6))               # 7 the centre
N_POSES = 8
OUTWARD = (1, 5, 6)
# Poses 2, 3, 4 and 7 fill the frame with tiles metres from the origin.  On the SHARED camera (and with light_capture) the oracle's byte-weight
# filter with the lit factor folded into the weights ("pixel") moves there, under a float32 nudge of the pose, by more than a frame-parity row
# allows the DEVICE (tests/test_multimap_scenes_host.py): in those modes picks() names envs on poses 0, 1, 5 and 6 only, and the other envs are
# held to their one-map handle byte for byte.  The per-env filters ("pixel-dr", "pixel-gl") stay within a quarter of the row on those poses
# too: under domain randomisation envs 64 / 129 stand on pose 3 -- from the last tile along the last column, the far duckies in view -- and
# picks() adds env 6, on pose 3 as well.
_rng = np.random.default_rng(SEED)
_POSE_OF = np.concatenate([_rng.integers(0, N_POSES, 65)] * 2)     # env e + 65 repeats env e's pose
_POSE_OF[:12] = _POSE_OF[65:77] = [0, 0, 0, 1, 0, 2, 3, 4, 5, 6, 6, 7]   # (every pose is in the batch; envs 0 .. 4: a tile-filled view of every map id)
_POSE_OF[[63, 128]], _POSE_OF[[64, 129]] = 5, 6                    # the envs picks() always names: on the highest map id, outward over the last column / row
assert len(_POSE_OF) == N


def pose_of(mode="shared", fisheye=False):
    """[N] the pose of every env.  Envs 64 / 129 (one side of the chunk border, the tail): pose 6; under domain randomisation pose 3; through the
    fisheye pose 5 (there the oracle's frame of the large map's last-row sliver moves by a mean of 0.012 under the float32 nudge, past
    ORACLE_MESH's quarter)."""
    out = _POSE_OF.copy()
    if mode == "dr":
        out[[64, 129]] = 3
    elif fisheye:
        out[[64, 129]] = 5
    return out


def map_ids(set_name):
    n = len(SETS[set_name])
    return np.where(np.arange(N) < 64, np.arange(N) % n, n - 1).astype(np.int32)


def replicas(set_name):
    """[(e, e + 65)] holding one state: env e on the highest map id."""
    mid = map_ids(set_name)
    return [(e, e + 65) for e in range(65) if mid[e] == mid[e + 65]]


# per-pose domain randomisation (mode "dr"): camera height / angle / fov factors within reset()'s ranges, a camera noise, a directional light
# (w = 0, as reset() draws it), per-channel ambient / diffuse / ground / horizon; per-pose eye-space positional lights (mode "light")
_dr = np.random.default_rng(SEED + 1)
DR = [dict(cam=_dr.uniform(0.9, 1.1, 3), noise=_dr.uniform(-0.005, 0.005, 3), light=np.append(_dr.uniform(-1, 1, 3) * (150, 0, 150) + (0, 180, 0), 0.0),
           ambient=_dr.uniform(0.18, 0.32, 3), diffuse=_dr.uniform(0.1, 0.7, 3), ground=_dr.uniform(0.1, 0.2, 3), horizon=_dr.uniform(0.3, 1.0, 3))
      for _ in range(N_POSES)]
LIGHTS = [np.append(_dr.uniform(-1, 1, 3) * (1.5, 1.0, 2.0) + (0, 2.5, -1.0), 1.0) for _ in range(N_POSES)]


def init_state(name, k, mode, map_id=0):
    """Pose k of map `name` as a dtsim_init_state of `mode` ("shared" / "dr" / "light")."""
    st = _ffi.InitState()
    x, z, ang = poses(name)[k]
    st.pos[:] = [x, 0.0, z]
    st.angle, st.map_id, st.wheel_dist = ang, int(map_id), osim.WHEEL_DIST
    st.cam_height, st.cam_angle_deg, st.cam_fov_y_deg = osim.CAMERA_FLOOR_DIST, osim.CAMERA_ANGLE, float(osim.CAMERA_FOV_Y)
    st.horizon_color[:] = [0.45, 0.82, 1.0]; st.ground_color[:] = [0.15, 0.15, 0.15]
    st.light_pos[:] = [0.0, 3.0, 0.0, 1.0]; st.light_ambient[:] = [0.25] * 3; st.light_diffuse[:] = [0.35] * 3
    if mode == "dr":
        d = DR[k]
        st.cam_height, st.cam_angle_deg, st.cam_fov_y_deg = (float(a * b) for a, b in zip((st.cam_height, st.cam_angle_deg, st.cam_fov_y_deg), d["cam"]))
        st.camera_noise[:] = [float(v) for v in d["noise"]]
        st.light_pos[:] = [float(v) for v in d["light"]]
        st.light_ambient[:], st.light_diffuse[:] = [float(v) for v in d["ambient"]], [float(v) for v in d["diffuse"]]
        st.ground_color[:], st.horizon_color[:] = [float(v) for v in d["ground"]], [float(v) for v in d["horizon"]]
    elif mode == "light":
        st.light_pos[:] = [float(v) for v in LIGHTS[k]]
    return st


def init_states(set_name, mode, fisheye=False, envs=None, one_map=False):
    """(_ffi.InitState * len(envs)) of the set's batch (envs: default all N); one_map: the same states for a handle that holds the env's map alone."""
    envs = range(N) if envs is None else list(envs)
    mid, POSE_OF = map_ids(set_name), pose_of(mode, fisheye)
    out = (_ffi.InitState * len(envs))()
    for i, e in enumerate(envs):
        out[i] = init_state(SETS[set_name][mid[e]], int(POSE_OF[e]), mode, 0 if one_map else mid[e])
    return out


def picks(set_name, mode="shared"):
    """Six envs at most for the oracle: both sides of the border between the two 64-env chunks, the tail, every map id; then, while there is
    room, under domain randomisation env 6 (pose 3: the tile-filled view along the last column -- on the large map in every set but L4, where
    envs 64 / 129 show it), the outward views of envs 8 and 10 (poses 5 and 6), the first tile's two views."""
    mid = map_ids(set_name)
    out = [63, 64, N - 1]
    for m in range(len(SETS[set_name])):
        if m not in {int(mid[e]) for e in out}:
            out.append(int(np.flatnonzero(mid == m)[0]))
    out += [e for e in ((6,) if mode == "dr" else ()) + (8, 10, 0, 3) if e not in out][:6 - len(out)]
    assert len(out) <= 6
    return sorted(out)


def tolerance(set_name):
    """The row of tests/frame_parity.py a set is held to: object-free sets ORACLE_PLANE, the others ORACLE_MESH."""
    return fp.ORACLE_MESH if has_objects(set_name) else fp.ORACLE_PLANE


ORACLE_MODES = {"k_raster_v3": "pixel", "k_raster_q": "pixel", "k_raster_v3dr": "pixel-dr", "k_raster_env": "pixel-gl", "k_raster": "pixel-gl"}


def oracle_mode_of(pipeline):
    """The `lighting` of oracle.raster.render_obs that restates `pipeline`: what util.oracle_mode must answer after such a pass."""
    return ORACLE_MODES[pipeline.split("+")[0]]


@functools.lru_cache(maxsize=None)
def rmap(fisheye):
    return pdist.distortion_maps(W, H) if fisheye else None


def camera(name, k, mode, nudge=False):
    """The oracle's camera of pose k on map `name`.  nudge: from the pose a float32 holds, the position scaled by 1 + 2e-7."""
    st = init_state(name, k, mode)
    pos, ang = np.array(st.pos[:], dtype=np.float64), float(st.angle)
    if nudge:
        pos, ang = pos.astype(np.float32).astype(np.float64) * (1 + 2e-7), float(np.float32(ang))
    return fp.camera_of_state(st, pos, ang, W, H, mode == "dr")


def obj_states(name):
    objs = scene(name).m.objects
    return [dict(pos=np.array(o.pos, dtype=np.float64), y_rot=float(o.y_rot), visible=True) for o in objs] or None


@functools.lru_cache(maxsize=None)
def oracle_frame(name, k, mode, lighting, fisheye=False, nudge=False):
    """The oracle's frame of pose k on map `name` with every object at its map pose; cached and read-only."""
    img = raster.render_obs(camera(name, k, mode, nudge), scene(name), lighting, rmap(fisheye), obj_states=obj_states(name))
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def hits(name, k, mode="shared"):
    """What the rectilinear frame of pose k on map `name` sees, per sample [4, H, W]: (surface -- k >= 0 object k, -1 the tile plane, -2 the
    ground quad, -3 the clear colour: depth_model.surfaces --, tile column, tile row of the hit; columns and rows outside the grid where the
    surface is not the tile plane)."""
    import depth_model as dm
    import label_model as lm
    cam, sc = camera(name, k, mode), scene(name)
    depths, ids = dm.oracle_buffers(cam, sc, obj_states(name))
    srf = dm.surfaces(cam, depths, ids)
    ti, tj = np.full(srf.shape, -1, np.int64), np.full(srf.shape, -1, np.int64)
    for q in range(len(raster.SAMPLE_OFFSETS)):
        tile = srf[q] == -1
        wx, wz = lm.world_hit(cam, depths[q], tile, q)              # (the hit reconstruction of the label model)
        ti[q] = np.where(tile, np.floor(wx / sc.m.tile_size), -1)
        tj[q] = np.where(tile, np.floor(wz / sc.m.tile_size), -1)
    return srf, ti, tj
