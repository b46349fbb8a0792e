"""Inputs of tests/test_gpu_render_order.py, in plain numpy: agent states on and off the borders of k_env_sort's sort key, the slot -> state
layout of a large batch, the host statement of the key with the check of an order against it, and a restatement of the quad-record
rasters' workgroup map.  tests/test_render_order_scenes_host.py holds all of it to its purpose on a CPU.

k_env_sort (csrc/render_setup.hip) bins env e by the tile under its camera centre (x + 0.066 cos a, z - 0.066 sin a) and its heading quadrant
floor(a 2/pi + 0.5) & 3, in float32.  The bins of the first 8192 envs stay in registers between the histogram and the scatter; every env
past them has its bin computed twice.  Only an env ON a border of the key can get two different bins from two evaluations, so the states
here come in two kinds: border states, which sit within a float32 ulp of a border, and clear states, which keep the distance CLEAR_POS /
CLEAR_ANG from every border and whose float64 host key therefore IS the device's bin."""
import math

import numpy as np

TILE = 0.585                    # tile_size of small_loop, small_loop_only_duckies and loop_only_duckies
CAM_FWD = 0.066                 # DT_CAMERA_FORWARD_DIST
KEEP_ENVS = 8 * 1024            # k_env_sort: KEEP * 1024 envs keep their bin in registers
ENVS_PER_CHUNK = 64             # DT_ENVS_PER_BLOCK: positions of the order that one raster workgroup loops over
SORT_BINS = 4096
COORD_MAX = 4.0                 # every coordinate of every state, and of its camera centre, is below this in magnitude
ANGLE_MAX = 7.2                 # every heading, in magnitude (2 pi + pi / 4 = 7.07 is the largest)
SEED = 20240

# ---- the margin of the clear states ------------------------------------------------------------------------------------------------
# The device's camera centre differs from the float64 one by roundings of the size of two terms:
ULP_COORD = float(np.spacing(np.float32(np.nextafter(np.float32(COORD_MAX), np.float32(0)))))   # a float32 ulp of the largest coordinate: 2^-22
SINCOS_ABS_ERR = 2.0 ** -21.19  # __sincosf: the larger of the documented absolute errors of __sinf (2^-21.41) and __cosf (2^-21.19) on [-pi, pi]
# Counted in units of (ULP_COORD + CAM_FWD * SINCOS_ABS_ERR) = 2.7e-7 m: the float64 -> float32 conversion of the coordinate (1/2), the
# rounding of the sum (1/2), the product with inv_tile_size (1/2 ulp of a tile index up to 7, under one ulp of the coordinate), inv_tile_size's own
# rounding (tile index x 2^-24 relative: under one), the sine / cosine (one), and once more for headings beyond [-pi, pi], where the argument's
# conversion to revolutions alone costs |a| 2^-24: about five units.  CLEAR_MULT leaves an order of magnitude above that, and is still
# 30000 times smaller than a tile.
CLEAR_MULT = 64
CLEAR_POS = CLEAR_MULT * (ULP_COORD + CAM_FWD * SINCOS_ABS_ERR)          # metres between a clear camera centre and any tile border: 1.7e-5
# The quadrant is floor(a * (2 / pi) + 0.5): the conversion of a (1/2 ulp), the constant's rounding (relative 2^-24), the product and the
# sum (1/2 ulp each, or one for a fused multiply-add) -- under three ulps of the largest value of the sum, which lies in [4, 8).
ULP_QUAD = float(np.spacing(np.float32(ANGLE_MAX * 2 / math.pi + 0.5)))  # 2^-21
CLEAR_ANG = CLEAR_MULT * ULP_QUAD * math.pi / 2                           # radians between a clear heading and any quadrant border: 4.8e-5
# How far (in float32 ulps of each input) the host test moves x, z and a around a state when it asks which bins float32 arithmetic can give:
# the device's value is within two ulps of the float64 one (above), so three reach both sides of a border that a state sits on.
REACH = 3

BORDER_KINDS = ("quad", "tile_x", "tile_z", "both")
KINDS = BORDER_KINDS + ("offgrid", "clear")


# ---- the sort key ------------------------------------------------------------------------------------------------------------------

def host_key(x, z, a, mid=0):
    """The float64 statement of k_env_sort's bin (the one test_c3_full_size_batch_matches_oracle_directly restates), with the map term."""
    x, z, a = (np.asarray(v, dtype=np.float64) for v in (x, z, a))
    cx, cz = x + CAM_FWD * np.cos(a), z - CAM_FWD * np.sin(a)
    ti, tj = np.clip(np.floor(cx / TILE), 0, 31).astype(np.int64), np.clip(np.floor(cz / TILE), 0, 31).astype(np.int64)
    quad = np.floor(a * (2.0 / np.pi) + 0.5).astype(np.int64) & 3
    return ((((tj << 5) | ti) << 2) | quad) ^ ((np.asarray(mid, dtype=np.int64) * 1237) & (SORT_BINS - 1))


def key32(x, z, a, mid=0, fused=False):
    """The bin in float32 with round-to-nearest, operation by operation as bin_of writes it (sine and cosine rounded from float64);
    fused: the two multiply-adds contracted, as the compiler may."""
    f = np.float32
    x, z, a = (np.asarray(v, dtype=np.float64).astype(f) for v in (x, z, a))
    its = f(1.0 / TILE)
    sa, ca = np.sin(a.astype(np.float64)).astype(f), np.cos(a.astype(np.float64)).astype(f)
    if fused:
        px = (x.astype(np.float64) + np.float64(f(CAM_FWD)) * ca).astype(f)
        pz = (z.astype(np.float64) - np.float64(f(CAM_FWD)) * sa).astype(f)
        u = (a.astype(np.float64) * np.float64(f(2.0 / math.pi)) + 0.5).astype(f)
    else:
        px, pz = x + f(CAM_FWD) * ca, z - f(CAM_FWD) * sa
        u = a * f(2.0 / math.pi) + f(0.5)
    ti = np.clip(np.floor(px * its), 0, 31).astype(np.int64)
    tj = np.clip(np.floor(pz * its), 0, 31).astype(np.int64)
    quad = np.floor(u).astype(np.int64) & 3
    return ((((tj << 5) | ti) << 2) | quad) ^ ((np.asarray(mid, dtype=np.int64) * 1237) & (SORT_BINS - 1))


def _nudged(v, steps):
    """float32(v) moved by `steps` float32 ulps."""
    v = np.float32(v)
    for _ in range(abs(steps)):
        v = np.nextafter(v, np.float32(math.inf if steps > 0 else -math.inf))
    return v


def bins32(x, z, a, reach=REACH):
    """Every bin that float32 arithmetic gives for the state and for its neighbours within `reach` ulps of each input, plain and fused."""
    r = range(-reach, reach + 1)
    xs, zs, as_ = np.meshgrid([_nudged(x, i) for i in r], [_nudged(z, i) for i in r], [_nudged(a, i) for i in r], indexing="ij")
    return set(np.unique(np.concatenate([key32(xs, zs, as_, fused=fu).ravel() for fu in (False, True)])).tolist())


def border_distance(x, z, a):
    """(metres from the float64 camera centre to the nearest tile border of the key, radians from the heading to the nearest quadrant
    border).  The key clamps the tile to 0..31, so the borders are k * TILE for k = 1..31: none at 0, and none below it."""
    x, z, a = (np.asarray(v, dtype=np.float64) for v in (x, z, a))
    cx, cz = x + CAM_FWD * np.cos(a), z - CAM_FWD * np.sin(a)
    k = np.arange(1, 32) * TILE
    d_pos = np.minimum(np.abs(cx[..., None] - k).min(axis=-1), np.abs(cz[..., None] - k).min(axis=-1))
    u = a * (2.0 / np.pi) + 0.5
    return d_pos, np.abs(u - np.round(u)) * (np.pi / 2)


def is_clear(x, z, a):
    d_pos, d_ang = border_distance(x, z, a)
    return (d_pos > CLEAR_POS) & (d_ang > CLEAR_ANG)


# ---- the state list ----------------------------------------------------------------------------------------------------------------

def _ulp(v):
    return float(np.spacing(np.float32(v)))


def _build_states():
    """[(kind, x, z, a)], border states first.  Headings of the tile-border states and positions of the quadrant-border states are clear."""
    out = []

    def centre_at(cx, cz, a):                          # the agent position that puts the camera centre at (cx, cz)
        return cx - CAM_FWD * math.cos(a), cz + CAM_FWD * math.sin(a)

    # the heading on a quadrant border: pi/4 + k pi/2, all four quadrants, negative headings, headings beyond +-pi and beyond +-2 pi
    for k in range(-5, 5):
        out.append(("quad", 1.0 + 0.13 * (k + 5), 0.8 + 0.17 * (k + 5), math.pi / 4 + k * math.pi / 2))
    for k in range(4):                                 # ... and one and two float32 ulps to either side
        a = math.pi / 4 + k * math.pi / 2
        for s in (-2, -1, 1, 2):
            out.append(("quad", 0.9 + 0.4 * k, 2.2 - 0.3 * k, float(_nudged(a, s))))
    # the camera centre on a tile border: half a float32 ulp below it, half above, and on the float32 nearest to it; the borders inside
    # the 5 x 5 grid, its high edge (5) and one beyond (6)
    for axis, ks, headings in (("tile_x", (1, 3, 5), (0.3, 2.0, -1.2)), ("tile_z", (2, 4, 6), (-0.4, 1.1, 2.9))):
        for k, a in zip(ks, headings):
            b = k * TILE
            for c in (b - 0.5 * _ulp(b), b + 0.5 * _ulp(b), float(np.float32(b))):
                other = 0.31 + 0.4 * k
                x, z = centre_at(c, other, a) if axis == "tile_x" else centre_at(other, c, a)
                out.append((axis, x, z, a))
    # both at once
    for k in range(4):
        a = math.pi / 4 + k * math.pi / 2
        x, z = centre_at(float(np.float32(2 * TILE)), 0.4 + 0.5 * k, a)
        out.append(("both", x, z, a))
    for k in (0, 2):
        a = math.pi / 4 + k * math.pi / 2 - 2 * math.pi
        x, z = centre_at(1.9 + 0.2 * k, 3 * TILE + 0.5 * _ulp(3 * TILE), a)
        out.append(("both", x, z, a))
    # off the grid: the low side (a negative tile coordinate, clamped to tile 0) and the high side (tiles the map does not have), each looking back at the map
    for cx, cz, a in ((-0.21, 1.3, 0.1), (1.6, -0.18, -1.5), (-0.12, -0.09, -0.6), (3.3, 1.0, 3.0), (1.2, 3.4, 1.5), (3.2, 3.3, 2.4)):
        x, z = centre_at(cx, cz, a)
        out.append(("offgrid", x, z, a))
    # clear states on the map, a centimetre and a hundredth of a radian from every border at least
    rng = np.random.default_rng(SEED)
    while len(out) < N_STATES:
        x, z, a = rng.uniform(0.1, 5 * TILE - 0.1), rng.uniform(0.1, 5 * TILE - 0.1), rng.uniform(-math.pi, math.pi)
        d_pos, d_ang = border_distance(x, z, a)
        if d_pos > 0.01 and d_ang > 0.01:
            out.append(("clear", float(x), float(z), float(a)))
    # state 0, which the layout gives the first slot past KEEP_ENVS: a quadrant-border state whose float32 quadrant changes when 1e-7f is
    # added to its heading -- two evaluations of the bin that differ by that much disagree on it
    sharp = next(i for i, (kind, x, z, a) in enumerate(out) if kind == "quad" and moves_under_1e7(x, z, a))
    out.insert(0, out.pop(sharp))
    return out


def moves_under_1e7(x, z, a):
    moved = np.float32(a) + np.float32(1e-7)
    return all(key32(x, z, a, fused=fu) != key32(x, z, moved, fused=fu) for fu in (False, True))


N_STATES = 96
_STATES = _build_states()
KIND = np.array([s[0] for s in _STATES])
X, Z, A = (np.array([s[i] for s in _STATES], dtype=np.float64) for i in (1, 2, 3))
BORDER = np.isin(KIND, BORDER_KINDS)                   # the device chooses these states' bins
N_BORDER = int(BORDER.sum())
# One state of each kind for the oracle: two clear, two on a tile border, one on a quadrant border, one off the grid -- picked by the ORACLE's
# own behaviour at ORACLE_SIZE: all six see a duckie of small_loop_only_duckies, and the oracle's frame of each moves a quarter of the
# comparison's bounds at most under a float32 nudge of the pose (tests/test_render_order_scenes_host.py; half of the 96 states do)
ORACLE_SIZE = (160, 120)
ORACLE_STATES = tuple(int(np.flatnonzero(KIND == k)[i]) for k, i in (("clear", 26), ("clear", 20), ("tile_x", 0), ("tile_z", 6), ("quad", 1), ("offgrid", 1)))


# ---- the layout --------------------------------------------------------------------------------------------------------------------

BATCH_SIZES = (65, 577, 1025, 8192, 8193, 9217, 16385)


def segments(N):
    """The slot ranges whose borders the layout respects: [0, 8192), the envs past it, the last 1024-slot stride of k_env_sort's
    loops, the tail chunk of the render order."""
    cuts = {0, N, 1024 * ((N - 1) // 1024), ENVS_PER_CHUNK * ((N - 1) // ENVS_PER_CHUNK)}
    if N > KEEP_ENVS:
        cuts.add(KEEP_ENVS)
    cuts = sorted(cuts)
    return list(zip(cuts[:-1], cuts[1:]))


def layout(N, K=N_STATES, seed=SEED):
    """state of slot e, [N].  Counted from the LAST slot the states run 0, 1, .., K - 1, 0, .. -- so the last r slots hold the first
    min(r, K) states, the border states first among them -- and a seeded permutation then shuffles the slots inside each of segments(N).
    Every suffix of the batch that starts on a segment border keeps its set of states: the envs past slot 8192, the last stride and the tail
    chunk each hold as many distinct states as they have room for, and every state they have room for twice, twice."""
    rng = np.random.default_rng([seed, N, K])
    out = (N - 1 - np.arange(N)) % K
    for lo, hi in segments(N):
        out[lo:hi] = out[lo:hi][rng.permutation(hi - lo)]
    return out


# ---- the order check ---------------------------------------------------------------------------------------------------------------

def order_fault(rpos, key, clear, selected=None):
    """None if `rpos` (DTSIM_FIELD_RENDER_POS) is a valid render order, else what is wrong with it.  Valid: a permutation of 0..N-1 --
    for a masked pass (`selected`: bool [N]) a permutation of 0..live-1 on the selected envs and exactly -1 elsewhere --, along which the
    keys of the clear envs never decrease."""
    rpos, key, clear = np.asarray(rpos).astype(np.int64), np.asarray(key), np.asarray(clear, dtype=bool)
    sel = np.ones(len(rpos), bool) if selected is None else np.asarray(selected, dtype=bool)
    if (rpos[~sel] != -1).any():
        e = int(np.flatnonzero(~sel & (rpos != -1))[0])
        return f"unselected env {e} at position {int(rpos[e])}"
    live = int(sel.sum())
    p = rpos[sel]
    out_of_range = (p < 0) | (p >= live)
    if out_of_range.any():
        e = int(np.flatnonzero(sel)[np.flatnonzero(out_of_range)[0]])
        return f"selected env {e} at position {int(rpos[e])}, outside [0, {live})"
    count = np.bincount(p, minlength=live)
    if (count != 1).any():
        shared, empty = np.flatnonzero(count > 1), np.flatnonzero(count == 0)
        return (f"not a permutation: {len(shared)} positions shared (the first: {shared[:1].tolist()}, envs "
                f"{np.flatnonzero(sel & np.isin(rpos, shared[:1]))[:4].tolist()}), {len(empty)} empty (the first: {empty[:1].tolist()})")
    env_at = np.flatnonzero(sel)[np.argsort(p)]
    env_at = env_at[clear[env_at]]
    down = np.flatnonzero(np.diff(key[env_at]) < 0)
    if len(down):
        a, b = int(env_at[down[0]]), int(env_at[down[0] + 1])
        return (f"clear env {a} (key {int(key[a])}, position {int(rpos[a])}) comes before clear env {b} (key {int(key[b])}, "
                f"position {int(rpos[b])}); {len(down)} such steps down")
    return None


def order_is_sorted(rpos, key, clear, selected=None):
    return order_fault(rpos, key, clear, selected) is None


# ---- the workgroup map of the quad-record rasters ----------------------------------------------------------------------------------
# Written from the comment block above raster_wg in csrc/raster_common.h: workgroup b runs on XCD b % 8; XCD x is given the x-th eighth of the
# chunks, ceil(n_chunks / 8) of them; within an XCD, groups of dt_q_tile_group() frame tiles (half the frame, the last group padded), all
# chunks of the slice for one group before the next group.

Q_TILE_SPLIT = 2                                       # DT_Q_TILE_SPLIT
TILE_W, TILE_H = 128, 8                                # DT_TILE_W x DT_TILE_H: a raster workgroup's pixel tile


def n_raster_tiles(W, H):
    """dt_raster_tiles"""
    return -(-W // TILE_W) * -(-H // TILE_H)


def tile_group(n_tiles):
    """dt_q_tile_group"""
    return -(-n_tiles // Q_TILE_SPLIT)


def raster_wg_grid(n_tiles, n_chunks):
    """raster_wg_grid: ((n_tiles + q_tg - 1) / q_tg) * q_tg * ((n_chunks + 7) / 8) * 8"""
    q_tg = tile_group(n_tiles)
    return -(-n_tiles // q_tg) * q_tg * -(-n_chunks // 8) * 8


def raster_wg(b, n_tiles, n_chunks, sub=False):
    """raster_wg for workgroups `b` (array): (tile, chunk, live).  n_chunks: the chunks of the pass (sub: the live chunks of a masked
    pass, whose grid is still sized for all N envs)."""
    b = np.asarray(b, dtype=np.int64)
    if sub:                                            # tile = bx % n_tiles, chunk = bx / n_tiles, live = chunk < n_chunks
        tile, chunk = b % n_tiles, b // n_tiles
        return tile, chunk, chunk < n_chunks
    cpx = -(-n_chunks // 8)                            # cpx = (n_chunks + 7) / 8
    xcd, bi = b & 7, b >> 3                            # xcd = bx & 7, bi = bx >> 3
    q_tg = tile_group(n_tiles)                         # q_tg = dt_q_tile_group(n_tiles)
    per_group = q_tg * cpx                             # per_group = q_tg * cpx
    grp, gi = bi // per_group, bi % per_group          # grp = bi / per_group, gi = bi % per_group
    g_tiles = np.minimum(q_tg, n_tiles - grp * q_tg)   # g_tiles = min(q_tg, n_tiles - grp * q_tg)
    g_safe = np.maximum(g_tiles, 1)                    # (a group past the frame's tiles: no launch has one, see the host test)
    tile = grp * q_tg + gi % g_safe                    # tile = grp * q_tg + gi % g_tiles
    chunk = xcd * cpx + gi // g_safe                   # chunk = xcd * cpx + gi / g_tiles
    live = (gi < g_tiles * cpx) & (chunk < n_chunks)   # live = gi < g_tiles * cpx && chunk < n_chunks
    return tile, chunk, live


def empty_slices(n_chunks):
    """The XCDs whose slice of the chunks is empty."""
    cpx = -(-n_chunks // 8)
    return [x for x in range(8) if x * cpx >= n_chunks]
