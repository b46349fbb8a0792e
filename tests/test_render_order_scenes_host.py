"""tests/render_order_scenes.py on a CPU: the states are where they claim to be (on a border of k_env_sort's key, or clear of all of them),
the layout puts them where the sort's second code path and the raster's last chunks are, the order check rejects what it must, the
restated workgroup map covers every (tile, chunk) exactly once -- and the oracle, at the small frame of tests/test_gpu_render_order.py,
moves a quarter of the comparison's bounds at most under a float32 nudge of the pose."""
import math

import numpy as np
import pytest

import frame_parity as fp
import render_order_scenes as ro
from dtsim import distortion as pdist
from oracle import raster

W, H = 128, 48                                         # the frame of tests/test_gpu_render_order.py


# ---- the states --------------------------------------------------------------------------------------------------------------------

def test_the_list_has_every_kind_of_state():
    assert len(ro.KIND) == ro.N_STATES == 96 and set(ro.KIND) == set(ro.KINDS)
    assert ro.N_BORDER >= ro.N_STATES // 3 and (ro.BORDER[:ro.N_BORDER]).all()           # border states first: the layout's priority
    assert len({(x, z, a) for x, z, a in zip(ro.X, ro.Z, ro.A)}) == ro.N_STATES         # distinct
    assert np.abs(ro.X).max() < ro.COORD_MAX and np.abs(ro.Z).max() < ro.COORD_MAX and np.abs(ro.A).max() < ro.ANGLE_MAX
    cx, cz = ro.X + ro.CAM_FWD * np.cos(ro.A), ro.Z - ro.CAM_FWD * np.sin(ro.A)
    assert np.abs(cx).max() < ro.COORD_MAX and np.abs(cz).max() < ro.COORD_MAX
    quad = ro.KIND == "quad"
    u = ro.A[quad] * 2 / math.pi + 0.5
    assert set(np.round(u).astype(int) & 3) == {0, 1, 2, 3}                             # all four borders
    assert (ro.A[quad] < -math.pi).any() and (ro.A[quad] > math.pi).any() and ((ro.A[quad] < 0) & (ro.A[quad] > -math.pi)).any()
    assert (np.floor(u) < 0).any()                                                      # a negative number goes through & 3
    off = ro.KIND == "offgrid"
    assert (cx[off] < 0).any() and (cz[off] < 0).any() and (cx[off] > 5 * ro.TILE).any() and (cz[off] > 5 * ro.TILE).any()
    both = ro.KIND == "both"
    d_pos, d_ang = ro.border_distance(ro.X, ro.Z, ro.A)
    assert (d_pos[both] < 2 * ro.ULP_COORD).all() and (d_ang[both] < 2 * ro.ULP_QUAD).all()
    for kind, axis_c in (("tile_x", cx), ("tile_z", cz)):                               # below, above and on the float32 nearest to k * TILE
        c = axis_c[ro.KIND == kind]
        k = np.round(c / ro.TILE)
        d = c - k * ro.TILE
        ulp = np.spacing((k * ro.TILE).astype(np.float32)).astype(np.float64)
        assert (np.abs(d) <= ulp).all() and (d < 0).any() and (d > 0).any(), kind
        nearest = (k * ro.TILE).astype(np.float32).astype(np.float64)
        assert (np.abs(c - nearest) < 1e-3 * ulp).any(), kind                          # (the agent position is float64: the centre is rebuilt from it)


def test_the_margin_is_what_its_derivation_says():
    assert ro.ULP_COORD == 2.0 ** -22 and ro.ULP_QUAD == 2.0 ** -21
    assert ro.CLEAR_POS == 64 * (2.0 ** -22 + 0.066 * 2.0 ** -21.19) and 1e-5 < ro.CLEAR_POS < 2e-5
    assert ro.CLEAR_ANG == 64 * 2.0 ** -21 * math.pi / 2 and 4e-5 < ro.CLEAR_ANG < 5e-5


@pytest.mark.parametrize("s", range(ro.N_STATES))
def test_a_border_state_is_on_its_border_and_a_clear_state_on_none(s):
    """The key in float32, round-to-nearest, at the state and at the neighbouring float32 inputs (REACH ulps of x, z and a; plain and
    with contracted multiply-adds): two bins or more for a border state, one for a clear state -- and that one is the float64 host key."""
    bins = ro.bins32(ro.X[s], ro.Z[s], ro.A[s])
    if ro.BORDER[s]:
        assert len(bins) >= (4 if ro.KIND[s] == "both" else 2), (s, ro.KIND[s], bins)
        assert not ro.is_clear(ro.X[s], ro.Z[s], ro.A[s])
    else:
        assert bins == {int(ro.host_key(ro.X[s], ro.Z[s], ro.A[s]))}, (s, ro.KIND[s], bins)
        assert ro.is_clear(ro.X[s], ro.Z[s], ro.A[s])
        for mid in (0, 1):                             # the map term moves every evaluation alike
            assert int(ro.key32(ro.X[s], ro.Z[s], ro.A[s], mid)) == int(ro.host_key(ro.X[s], ro.Z[s], ro.A[s], mid))


def test_a_clear_state_keeps_its_bin_anywhere_within_the_margin():
    """Moved by the whole margin in every direction (float64), a clear state keeps its host key: the margin is inside the bin."""
    c = ~ro.BORDER
    for dx, dz, da in ((ro.CLEAR_POS, 0, 0), (-ro.CLEAR_POS, 0, 0), (0, ro.CLEAR_POS, 0), (0, -ro.CLEAR_POS, 0), (0, 0, ro.CLEAR_ANG), (0, 0, -ro.CLEAR_ANG)):
        # (a turn of CLEAR_ANG also moves the camera centre, by 0.066 x CLEAR_ANG = 3e-6 m: inside CLEAR_POS)
        assert np.array_equal(ro.host_key(ro.X[c] + dx, ro.Z[c] + dz, ro.A[c] + da), ro.host_key(ro.X[c], ro.Z[c], ro.A[c]))


def test_state_0_changes_its_bin_under_1e7():
    assert ro.KIND[0] == "quad" and ro.moves_under_1e7(ro.X[0], ro.Z[0], ro.A[0])


def test_the_host_key_is_the_one_the_c3_test_restates():
    rng = np.random.default_rng(3)
    x, z, a = rng.uniform(-0.3, 3.3, 500), rng.uniform(-0.3, 3.3, 500), rng.uniform(-7, 7, 500)
    cx, cz = x + 0.066 * np.cos(a), z - 0.066 * np.sin(a)
    ti, tj = np.clip(np.floor(cx / 0.585), 0, 31).astype(int), np.clip(np.floor(cz / 0.585), 0, 31).astype(int)
    key = (((tj << 5) | ti) << 2) | (np.floor(a * (2.0 / np.pi) + 0.5).astype(int) & 3)
    assert np.array_equal(ro.host_key(x, z, a), key)
    assert np.array_equal(ro.host_key(x, z, a, 1), key ^ 1237) and np.array_equal(ro.host_key(x, z, a, 5), key ^ ((5 * 1237) & 4095))


# ---- the layout --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", ro.BATCH_SIZES)
def test_layout_reaches_the_recompute_path_and_the_last_chunks(N):
    """Every batch size of the GPU test is 1 (mod 64) or 8192, so the tail chunk -- and at 8193 the whole recompute path -- is ONE slot: a region
    of r slots cannot hold more than r states.  Held instead: each region holds the first min(r, K) states of the list, which starts with the border
    states (state 0 the sharpest of them); and where the room is there, every state on both sides of slot 8192 and every border state
    twice past it."""
    K = ro.N_STATES
    lay = ro.layout(N)
    assert lay.shape == (N,) and np.array_equal(lay, ro.layout(N, K, ro.SEED)) and not np.array_equal(lay, ro.layout(N, K, ro.SEED + 1))
    assert not np.array_equal(lay, np.arange(N) % K) and (lay == np.arange(N) % K).mean() < 0.05       # a permutation, not e % K
    count = np.bincount(lay, minlength=K)
    assert count.max() - count.min() <= 1 and len(count) == K
    tail, stride = ro.ENVS_PER_CHUNK * ((N - 1) // ro.ENVS_PER_CHUNK), 1024 * ((N - 1) // 1024)
    regions = {"tail chunk": tail, "last stride": stride}
    if N > ro.KEEP_ENVS:
        regions["past 8192"] = ro.KEEP_ENVS
    for name, lo in regions.items():
        assert set(lay[lo:]) == set(range(min(N - lo, K))), (name, N)
    assert set(lay[:min(N, ro.KEEP_ENVS)]) == set(range(min(N, K)))                     # every state below slot 8192
    past = N - ro.KEEP_ENVS
    if past > 0:
        assert lay[ro.KEEP_ENVS] == 0 or past > 1                                      # 8193: the one recomputed env is state 0
    if past >= K:
        assert set(lay[ro.KEEP_ENVS:]) == set(range(K))                                # both sides of slot 8192
    if past >= K + ro.N_BORDER:
        assert (np.bincount(lay[ro.KEEP_ENVS:], minlength=K)[:ro.N_BORDER] >= 2).all()


def test_the_batch_sizes_give_the_chunk_counts_they_are_chosen_for():
    assert [-(-n // ro.ENVS_PER_CHUNK) for n in ro.BATCH_SIZES] == [2, 10, 17, 128, 129, 145, 257]
    assert 9217 in ro.BATCH_SIZES and 16385 in ro.BATCH_SIZES and ro.KEEP_ENVS == 8192


# ---- the order check ---------------------------------------------------------------------------------------------------------------

def _order(N=300, seed=1):
    lay = ro.layout(N)
    key, clear = ro.host_key(ro.X[lay], ro.Z[lay], ro.A[lay]), ~ro.BORDER[lay]
    # a valid order: by the key, border envs anywhere
    rng = np.random.default_rng(seed)
    k = key.astype(np.float64)
    k[~clear] = rng.uniform(0, 4096, int((~clear).sum()))
    env_at = np.lexsort((rng.random(N), k))
    rpos = np.empty(N, np.int32)
    rpos[env_at] = np.arange(N)
    return rpos, key, clear


def test_order_check_accepts_a_valid_order():
    rpos, key, clear = _order()
    assert ro.order_is_sorted(rpos, key, clear) and ro.order_fault(rpos, key, clear) is None
    sel = np.arange(len(rpos)) % 3 == 0
    m = np.full(len(rpos), -1, np.int32)
    m[sel] = np.argsort(np.argsort(rpos[sel]))
    assert ro.order_is_sorted(m, key, clear, sel)
    assert ro.order_is_sorted(np.full(len(rpos), -1), key, clear, np.zeros(len(rpos), bool))          # the empty mask
    # border envs out of order are the device's choice
    b = np.flatnonzero(~clear)
    r2 = rpos.copy()
    r2[b[0]], r2[b[-1]] = rpos[b[-1]], rpos[b[0]]
    assert ro.order_is_sorted(r2, key, clear)


def test_order_check_rejects_a_duplicated_position():
    rpos, key, clear = _order()
    rpos[5] = rpos[9]
    assert not ro.order_is_sorted(rpos, key, clear) and "1 positions shared" in ro.order_fault(rpos, key, clear)


def test_order_check_rejects_a_missing_position():
    rpos, key, clear = _order()
    rpos[np.argmax(rpos)] = len(rpos)                  # the last position moves out: N - 1 is missing
    assert not ro.order_is_sorted(rpos, key, clear)
    rpos, key, clear = _order()
    sel = np.arange(len(rpos)) % 2 == 0
    m = np.full(len(rpos), -1, np.int32)
    m[sel] = np.argsort(np.argsort(rpos[sel])) + 1     # positions 1..live: 0 is missing
    assert not ro.order_is_sorted(m, key, clear, sel)


def test_order_check_rejects_a_selected_env_without_a_position():
    rpos, key, clear = _order()
    sel = np.arange(len(rpos)) % 2 == 0
    m = np.full(len(rpos), -1, np.int32)
    m[sel] = np.argsort(np.argsort(rpos[sel]))
    assert ro.order_is_sorted(m, key, clear, sel)
    m[4] = -1
    assert not ro.order_is_sorted(m, key, clear, sel) and "selected env 4" in ro.order_fault(m, key, clear, sel)


def test_order_check_rejects_an_unselected_env_at_a_position():
    rpos, key, clear = _order()
    sel = np.arange(len(rpos)) % 2 == 0
    m = np.full(len(rpos), -1, np.int32)
    m[sel] = np.argsort(np.argsort(rpos[sel]))
    m[3] = 0
    assert not ro.order_is_sorted(m, key, clear, sel) and "unselected env 3" in ro.order_fault(m, key, clear, sel)


def test_order_check_rejects_two_clear_envs_swapped_across_a_bin_boundary():
    rpos, key, clear = _order()
    env_at = np.argsort(rpos)
    ce = env_at[clear[env_at]]
    i = int(np.flatnonzero(np.diff(key[ce]) > 0)[0])   # neighbours among the clear envs, in different bins
    a, b = ce[i], ce[i + 1]
    rpos[a], rpos[b] = rpos[b], rpos[a]
    assert not ro.order_is_sorted(rpos, key, clear) and "comes before" in ro.order_fault(rpos, key, clear)
    # the same swap inside one bin is no fault
    rpos, key, clear = _order()
    ce = np.argsort(rpos)[clear[np.argsort(rpos)]]
    i = int(np.flatnonzero(np.diff(key[ce]) == 0)[0])
    rpos[ce[i]], rpos[ce[i + 1]] = rpos[ce[i + 1]], rpos[ce[i]]
    assert ro.order_is_sorted(rpos, key, clear)


# ---- the workgroup map -------------------------------------------------------------------------------------------------------------

CHUNK_COUNTS = tuple(range(1, 41)) + (63, 64, 65, 128, 129, 256, 257)


@pytest.mark.parametrize("n_tiles", (1, 6, 12, 75, 300))
def test_the_live_workgroups_take_every_tile_of_every_chunk_once(n_tiles):
    for n_chunks in CHUNK_COUNTS:
        grid = ro.raster_wg_grid(n_tiles, n_chunks)
        q_tg, cpx = ro.tile_group(n_tiles), -(-n_chunks // 8)
        assert grid == -(-n_tiles // q_tg) * q_tg * cpx * 8 and grid % 8 == 0 and grid >= n_tiles * n_chunks
        b = np.arange(grid)
        tile, chunk, live = ro.raster_wg(b, n_tiles, n_chunks)
        assert ((b >> 3) // (q_tg * cpx) < -(-n_tiles // q_tg)).all()                  # no workgroup of the launch is past the last tile group
        assert int(live.sum()) == n_tiles * n_chunks, (n_tiles, n_chunks)
        assert (tile[live] >= 0).all() and (tile[live] < n_tiles).all() and (chunk[live] < n_chunks).all()
        assert len(np.unique(chunk[live] * n_tiles + tile[live])) == n_tiles * n_chunks, (n_tiles, n_chunks)     # each once: none twice, none left
        assert ((chunk[live] // cpx) == (b[live] & 7)).all()                           # XCD x serves the x-th eighth of the chunks
        # the masked pass: the same launch, any number of live chunks
        for n_live in sorted({0, 1, n_chunks // 2, n_chunks - 1, n_chunks}):
            t, c, lv = ro.raster_wg(b, n_tiles, n_live, sub=True)
            assert int(lv.sum()) == n_tiles * n_live and len(np.unique(c[lv] * n_tiles + t[lv])) == n_tiles * n_live


def test_which_chunk_counts_leave_an_xcd_without_chunks():
    """The batch sizes of the GPU test by their chunk counts: which XCDs get no chunk at all, and how much of the launch is padding."""
    got = {n: ro.empty_slices(-(-n // 64)) for n in ro.BATCH_SIZES}
    assert got == {65: [2, 3, 4, 5, 6, 7], 577: [5, 6, 7], 1025: [6, 7], 8192: [], 8193: [], 9217: [], 16385: []}
    # 129 chunks, 17 per XCD: XCD 7 owns chunks 119..128 and seven dead ones; 6 tiles in groups of 3
    tile, chunk, live = ro.raster_wg(np.arange(ro.raster_wg_grid(6, 129)), 6, 129)
    x7 = (np.arange(len(live)) & 7) == 7
    assert set(chunk[x7 & live]) == set(range(119, 129)) and set(chunk[x7 & ~live]) == set(range(129, 136))
    assert ro.n_raster_tiles(W, H) == 6 and ro.n_raster_tiles(640, 480) == 300 and ro.n_raster_tiles(160, 120) == 30


# ---- the oracle's own headroom at the small frame -----------------------------------------------------------------------------------

@pytest.mark.parametrize("map_name,tol", [("small_loop", fp.ORACLE_PLANE), ("small_loop_only_duckies", fp.ORACLE_MESH)])
@pytest.mark.parametrize("mode", ["pixel", "pixel-dr"])
def test_the_oracle_moves_a_quarter_of_the_bounds_at_most_under_a_float32_nudge(mode, map_name, tol):
    """As tests/test_crowd_scenes_host.py, at the frame of the GPU test's oracle comparison (160 x 120) through the fisheye: the oracle rendered again from the pose a float32 holds, the
    position scaled by (1 + 2e-7), stays within a quarter of every bound of the row the GPU test compares at.  What is left is the device's.
    (With the byte-weight filter, "pixel", half of the 96 states keep that headroom at this size, and at 128 x 48 the worst state moves its mean by
    0.058, three times the row: the compared states are picked among those that keep it, render_order_scenes.ORACLE_STATES.)"""
    W, H = ro.ORACLE_SIZE
    sc, rmap = fp.scene(map_name), pdist.distortion_maps(W, H)
    objs = [dict(pos=o.pos, y_rot=o.y_rot, visible=True) for o in sc.m.objects] or None
    worst, n_obj_px = dict(gt1=0.0, gt2=0.0, mean=0.0), 0
    for s in ro.ORACLE_STATES:
        pos, ang = np.array([ro.X[s], 0.0, ro.Z[s]]), float(ro.A[s])
        ref = raster.render_obs(raster.Camera(pos, ang, width=W, height=H), sc, mode, rmap, obj_states=objs)
        if objs:
            hidden = [dict(o, visible=False) for o in objs]
            n_obj_px += fp.object_pixels(ref, raster.render_obs(raster.Camera(pos, ang, width=W, height=H), sc, mode, rmap, obj_states=hidden))
        npos, nang = pos.astype(np.float32).astype(np.float64) * (1 + 2e-7), float(np.float32(ang))
        again = raster.render_obs(raster.Camera(npos, nang, width=W, height=H), sc, mode, rmap, obj_states=objs)
        st = fp.stats(again, ref)
        fp.assert_within(st, fp.tighter(tol, 4), (mode, map_name, s, ro.KIND[s]))
        assert ref.std() > 5.0, (s, ro.KIND[s])         # a view, not one colour
        worst = {f: max(worst[f], st[f]) for f in worst}
    assert not objs or n_obj_px > 100, n_obj_px         # the duckies are in view of the compared states
    print(f"{mode} {map_name} {W} x {H}: nudged oracle against itself over {len(ro.ORACLE_STATES)} states: worst {worst}")
