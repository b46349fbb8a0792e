"""The map sets of tests/multimap_scenes.py on the host packer and the oracle alone: the sets sit on the side of every dispatch limit they
are meant to sit on and fit the packer's budgets; the layout is what tests/test_gpu_multimap_render.py relies on; the frames it holds to the
oracle reach the last column, the last row and the special tiles of the 24 x 16 map and the ground beyond it; and the oracle itself, moved by
a float32's worth, stays within a quarter of the row each compared state is held to.  Runs on a CPU."""
import math

import numpy as np
import pytest

import frame_parity as fp
import multimap_scenes as ms
from dtsim import assets, batched
from test_scene_tables_host import pk  # noqa: F401  (the packers of csrc/scene_tables.h, compiled for the host)

V3_TABLE = {(s, m): p for s in ms.V3_SETS for m, p in (("shared", "k_raster_v3"), ("dr", "k_raster_v3dr"), ("light", "k_raster_v3+light"))}
Q_TABLE = {(s, m): p for s in ("S5", "Lw", "Lh") for m, p in (("shared", "k_raster_q"), ("dr", "k_raster_env"), ("light", "k_raster_q+light"))}


def test_expected_pipeline_is_the_table():
    assert set(ms.V3_SETS) | {"S5", "Lw", "Lh"} == set(ms.SETS)
    for (s, m), want in {**V3_TABLE, **Q_TABLE}.items():
        assert ms.expected_pipeline(s, m == "dr", m == "light") == want, (s, m)
    for s in ms.V3_SETS:                                   # DTSIM_RASTER_OLD=1 keeps k_raster_q and the generic per-env raster
        assert [ms.expected_pipeline(s, m == "dr", m == "light", raster_old=True) for m in ms.MODES] == ["k_raster_q", "k_raster_env", "k_raster_q+light"]


@pytest.mark.parametrize("set_name", list(ms.SETS))
def test_set_tables(pk, set_name):  # noqa: F811
    names = ms.SETS[set_name]
    lib = assets.AssetLibrary(None)
    sc = batched.load_scene(lib, names, [ms.map_data(n) for n in names])
    tarr, marr, farr, keep = batched.scene_ffi(sc)
    assert pk.lib.st_assets(tarr, len(sc.textures), marr, len(sc.mesh_order)) == 0, pk.err()
    assert pk.lib.st_maps(farr, len(names), 1) == 0, pk.err()                  # DTSIM_OK: the k_step LDS staging budget and the raster records hold
    s, want = pk.scalars(), ms.set_tables(names)
    assert {k: int(s[k]) for k in ("qlog2", "n_qtiles", "grid_rows", "grid_cols", "n_maps")} == want
    assert s["tex_w"] == s["tex_h"] == 256 and s["n_qtiles"] <= 4096 and s["total_words"] * 8 <= 60000
    assert (s["max_tris"] > 0) == ms.has_objects(set_name)
    rm = pk.table("rmaps")
    assert [(int(r["grid_w"]), int(r["grid_h"])) for r in rm] == [ms.dims(n) for n in names]
    assert [np.float32(r["tile_size"]) for r in rm] == [np.float32(ms.map_data(n)["tile_size"]) for n in names]
    assert s["q_per_m"] == np.float32(256.0 / min(ms.map_data(n)["tile_size"] for n in names))
    limit = (ms.V3_MAX_ROWS, ms.V3_MAP_COLS)
    if set_name in ("L1", "L2", "L4"):
        assert (want["grid_rows"], want["grid_cols"]) == limit                 # exactly at the limit
    if set_name in ("Lw", "Lh"):
        assert (want["grid_rows"], want["grid_cols"]) == {"Lw": (limit[0], limit[1] + 1), "Lh": (limit[0] + 1, limit[1])}[set_name]   # one past it
    if set_name == "L4":                                   # the large map is the LAST of four: columns 96 .. 127 of the LDS row
        assert names[3] == "mm_Lo" and int(rm[3]["qt_pitch"]) == ms.V3_MAP_COLS and 3 * ms.V3_MAP_COLS + int(rm[3]["qt_pitch"]) == ms.V3_TAB_PITCH // 2
    del keep


def test_the_edge_maps_are_as_described():
    for name in ("mm_L", "mm_Lo", "mm_Lw", "mm_Lh"):
        md, (w, h) = ms.map_data(name), ms.dims(name)
        t = md["tiles"]
        kind = lambda i, j: t[j][i].split("/")[0]
        drivable = ("straight", "curve_left", "curve_right", "3way_left", "3way_right", "4way")
        assert all(kind(i, j) in drivable for i, j in ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)))
        ring = [(i, j) for j in range(h) for i in range(w) if i in (0, w - 1) or j in (0, h - 1)]
        special = [(i, j) for j in range(h) for i in range(w) if kind(i, j) == ms.SPECIAL]
        assert special == [(w - 1, h - 2), (w - 2, h - 1)]                        # one in the last column, one in the last row, nowhere else
        assert all(kind(i, j) in drivable or (i, j) in special for i, j in ring)
        inner = {kind(i, j) for j in range(1, h - 1) for i in range(1, w - 1)}
        assert inner == {"grass", "asphalt", "empty"} and sum(row.count("empty") for row in t) == 2
        objs = md["objects"]
        assert len(objs) == (4 if name in ("mm_Lo", "mm_Lh") else 0)
        assert all(o["static"] and w - 2 <= o["pos"][0] <= w and h - 2 <= o["pos"][1] <= h for o in objs)
    assert ms.dims("mm_L") == ms.dims("mm_Lo") == (24, 16) and ms.dims("mm_Lw") == (25, 16) and ms.dims("mm_Lh") == (24, 17)
    assert ms.map_data("mm_t47")["tiles"] == ms.map_data("small_loop")["tiles"] and ms.map_data("mm_t47")["tile_size"] == 0.47
    assert not any(ms.map_data(n)["objects"] for n in ms.SETS["P4"]) and len({str(ms.map_data(n)["tiles"]) for n in ms.SETS["P4"]}) == 4


@pytest.mark.parametrize("set_name", list(ms.SETS))
def test_layout(set_name):
    names, mid = ms.SETS[set_name], ms.map_ids(set_name)
    n = len(names)
    assert ms.N == 130 and np.array_equal(mid[:64], np.arange(64) % n) and (mid[64:] == n - 1).all()
    for mode, fisheye in (("shared", False), ("dr", False), ("light", False), ("shared", True)):
        p = ms.pose_of(mode, fisheye)
        assert np.array_equal(p[:65], p[65:]) and set(p.tolist()) == set(range(ms.N_POSES))
        assert p[63] == 5 and p[64] == (3 if mode == "dr" else 5 if fisheye else 6)
        picks = ms.picks(set_name, mode)
        assert len(picks) <= 6 and {63, 64, ms.N - 1} <= set(picks) and {int(mid[e]) for e in picks} == set(range(n))
        # the shared camera's oracle filter has no headroom on the tile-filled far views; the per-env filters have: one is compared
        far = [e for e in picks if p[e] in (2, 3, 4, 7)]
        assert bool(far) == (mode == "dr"), (mode, far)
        if mode == "dr" and set_name in ("L1", "L2", "L4", "Lw", "Lh"):      # ... of the large map, from its last tile
            assert any(names[mid[e]].startswith("mm_L") and p[e] in (3, 4) for e in picks), (set_name, picks)
    reps = ms.replicas(set_name)
    assert (64, 129) in reps and ((63, 128) in reps) == (63 % n == n - 1) and len(reps) >= 64 // n
    st = ms.init_states(set_name, "dr")
    for a, b in reps:
        assert bytes(st[a]) == bytes(st[b])
    assert len({bytes(st[e]) for e in range(ms.N)}) >= min(n, 2) * ms.N_POSES    # (not one state over and over)
    for name in names:
        (w, h), ts, ps = ms.dims(name), ms.map_data(name)["tile_size"], ms.poses(name)
        assert len(ps) == ms.N_POSES
        assert all(0.05 <= x <= w * ts - 0.05 and 0.05 <= z <= h * ts - 0.05 for x, z, _ in ps)
        off_axis = [abs(a - round(a / (math.pi / 2)) * (math.pi / 2)) for _, _, a in ps]
        assert sum(1 for d in off_axis if 0 < d <= 1e-4) == 2
        assert {(int(x // ts), int(z // ts)) for x, z, _ in ps} >= {(0, 0), (w - 1, h - 1), (w - 1, h - 2), (w - 2, h - 1), (w // 2, h // 2)}


@pytest.mark.parametrize("set_name", ["L1", "L2", "L4"])
def test_the_compared_frames_of_the_large_map_reach_its_far_entries(set_name):
    """Tile column 23, tile row 15 and the special kind: hit by at least 1 % of the samples of some frame the GPU test holds to the oracle."""
    names, mid = ms.SETS[set_name], ms.map_ids(set_name)
    col = row = special = 0.0
    for e in ms.picks(set_name):
        name = names[mid[e]]
        if name not in ("mm_L", "mm_Lo"):
            continue
        srf, ti, tj = ms.hits(name, int(ms.pose_of()[e]))
        sc = ms.scene(name)
        tile = srf == -1
        is_special = np.array([[k == ms.SPECIAL for k in r] for r in sc.kinds])
        col, row = max(col, float((tile & (ti == 23)).mean())), max(row, float((tile & (tj == 15)).mean()))
        special = max(special, float((tile & is_special[np.clip(tj, 0, 15), np.clip(ti, 0, 23)]).mean()))
    print(f"{set_name}: largest share of a compared frame's samples on tile column 23 {col:.3f}, on tile row 15 {row:.3f}, on the special kind {special:.3f}")
    assert col >= 0.01 and row >= 0.01 and special >= 0.01


@pytest.mark.parametrize("set_name", list(ms.SETS))
def test_outward_views_see_the_ground_and_every_map_owns_a_compared_frame(set_name):
    """On L4 -- the set the bound is set for -- every map id owns at least 5 % of some compared frame, and so does every map with objects in any
    set.  In the other sets (S3, S4, S5, P4, L1, L2, Lw, Lh, T2) an object-free map owns 3 % at least: its only compared shared-camera views may
    be the outward ones, and ORACLE_PLANE's quarter leaves room for no more at the far corner of the large map (multimap_scenes.OUT_MARGIN)."""
    names, mid = ms.SETS[set_name], ms.map_ids(set_name)
    own, outward = {}, []
    for e in ms.picks(set_name):
        k = int(ms.pose_of()[e])
        srf, ti, tj = ms.hits(names[mid[e]], k)
        own[int(mid[e])] = max(own.get(int(mid[e]), 0.0), float((srf == -1).mean()))
        if k in ms.OUTWARD:
            outward.append(float((srf == -2).mean()))          # the ground quad shows only where no tile covers it: beyond the grid (or an empty cell)
            assert outward[-1] >= 0.3 and 0 < float((srf == -1).mean()) < 0.2, (set_name, e, k, outward[-1])
    assert outward, set_name
    print(f"{set_name}: largest share of a compared frame that each map id's tiles own", {m: round(v, 3) for m, v in own.items()})
    assert all(own[m] >= (0.05 if set_name == "L4" or ms.map_data(names[m])["objects"] else 0.03) for m in range(len(names))), (set_name, own)


@pytest.mark.parametrize("set_name,name", [("L4", "mm_Lo"), ("Lh", "mm_Lh")])
def test_the_far_duckies_meet_the_oracle_under_domain_randomisation(set_name, name):
    """Some frame of the map with the far-corner duckies that the "dr" case holds to the oracle shows them: >= 1 % of its samples are an object's."""
    names, mid, p = ms.SETS[set_name], ms.map_ids(set_name), ms.pose_of("dr")
    share = max(float((ms.hits(name, int(p[e]), "dr")[0] >= 0).mean()) for e in ms.picks(set_name, "dr") if names[mid[e]] == name)
    print(f"{set_name}: largest object-owned share of a compared dr frame of {name}: {share:.4f}")
    assert share >= 0.01, share


def headroom_cases():
    out = [(s, m, False) for s in ms.SETS for m in ms.MODES]
    return out + [("L4", "shared", True)]


@pytest.mark.parametrize("set_name,mode,fisheye", headroom_cases())
def test_the_oracle_moves_a_quarter_of_the_row_at_most_under_a_float32_nudge(set_name, mode, fisheye):
    """Every state the GPU test holds to the oracle: the oracle rendered again from the pose a float32 holds, the position scaled by 1 + 2e-7, stays
    within frame_parity.tighter(row, 4) -- what is left of the row is the device's."""
    names, mid = ms.SETS[set_name], ms.map_ids(set_name)
    lighting = ms.oracle_mode_of(ms.expected_pipeline(set_name, mode == "dr", mode == "light"))
    tol, worst = fp.tighter(ms.tolerance(set_name), 4), dict(gt1=0.0, gt2=0.0, mean=0.0)
    for e in ms.picks(set_name, mode):
        name, k = names[mid[e]], int(ms.pose_of(mode, fisheye)[e])
        s = fp.stats(ms.oracle_frame(name, k, mode, lighting, fisheye), ms.oracle_frame(name, k, mode, lighting, fisheye, True))
        fp.assert_within(s, tol, (set_name, mode, e, name, k))
        worst = {f: max(worst[f], s[f]) for f in worst}
    print(f"{set_name} {mode} ({lighting}{', fisheye' if fisheye else ''}): nudged oracle against itself, worst", worst)
