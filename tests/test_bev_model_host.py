"""`not gpu`: the model of dtsim_bev (tests/bev_model.py) on this CPU -- against a plain double loop over the cells, its candidate sets on
hand-made cases (a cell centre on a footprint edge, on a tile seam, on the grid's border, under two overlapping rectangles), the condition on
the inputs of tests/test_gpu_bev.py (at least 80 % of every case's cells are sure; the shares: profiles/bev_parity.txt) --, the ctypes
binding, the place of ob_corners in the state blob, and the packer of the objects' corner table (csrc/scene_tables.h) in a program of its
own under AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import re
import subprocess

import numpy as np
import pytest

import bev_model as bm
import test_state_fields_host as sf
from dtsim import BatchedSimulator, _ffi, labels as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gym-duckietown_amd", "csrc")
TS = bm.TS
ONE = (1, 1, 0.02, 0)                   # one cell, 0.01 m ahead of the pose; with theta = 0 that is P = (x + 0.01, z)


def rect(x0, x1, z0, z1):
    return np.array([[x0, z0], [x1, z0], [x1, z1], [x0, z1]], np.float64)


def at(px, pz):
    return (px - 0.01, pz, 0.0)


def ids(e):
    return set(np.nonzero(e.cand_id[0, 0])[0].tolist())


def classes(e):
    return set(np.nonzero(e.cand_cls[0, 0])[0].tolist())


# ---- the model ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case,k,mi,shape", [("crowd", 8, 0, (9, 7, 0.05, 3)), ("two_maps", 1, 1, (6, 11, 0.11, 0))])
def test_the_model_equals_a_plain_loop_over_the_cells(case, k, mi, shape):
    c = bm.CASES[case]
    mm = bm.map_model(c.maps[mi])
    corners, drawn = bm.host_footprints(case)[mi]
    want = bm.expected(mm, c.poses[k], corners, drawn, shape)
    cls, inst = bm.loop_expected(mm, c.poses[k], corners, drawn, shape)
    assert np.array_equal(cls, want.cls) and np.array_equal(inst, want.inst)
    if case == "crowd":
        assert (inst > 0).sum() >= 3 and not set(np.unique(inst).tolist()) & {h + 1 for h in c.hidden}      # objects in view, no hidden one


def test_cell_points_follow_the_agents_frame():
    wx, wz = bm.cell_points((1.0, 2.0, 0.0), 4, 3, 0.1, 1)          # theta = 0: ahead is +x, right is +z
    assert np.allclose(wx[:, 0], [1.25, 1.15, 1.05, 0.95]) and np.allclose(wz[0], [1.9, 2.0, 2.1])
    wx, wz = bm.cell_points((1.0, 2.0, np.pi / 2), 4, 3, 0.1, 1)    # theta = pi / 2: ahead is -z, right is +x
    assert np.allclose(wz[:, 0], [1.75, 1.85, 1.95, 2.05]) and np.allclose(wx[0], [0.9, 1.0, 1.1])


def test_a_cell_centre_on_a_footprint_edge_is_not_sure():
    mm = bm.map_model("small_loop")
    mm = mm._replace(obj_cls=np.array([9], np.int64))
    r, drawn = rect(1.0, 1.1, 0.9, 1.0)[None], np.array([True])
    e = bm.expected(mm, at(1.0, 0.95), r, drawn, ONE)                # on the edge x = 1.0
    tile = int(bm.tile_class(mm, np.array([1.0]), np.array([0.95]))[0])
    assert ids(e) == {0, 1} and {9, tile} <= classes(e) and not e.sure_id[0, 0] and not e.sure_cls[0, 0]
    e = bm.expected(mm, at(1.0 - 0.5 * bm.M, 0.95), r, drawn, ONE)    # half a margin outside: the model says tile, the object stays possible
    assert e.inst[0, 0] == 0 and ids(e) == {0, 1}
    e = bm.expected(mm, at(1.0 + 2 * bm.M, 0.95), r, drawn, ONE)      # two margins inside: the object alone
    assert e.inst[0, 0] == 1 and e.cls[0, 0] == 9 and ids(e) == {1} and classes(e) == {9} and e.sure_id[0, 0] and e.sure_cls[0, 0]
    e = bm.expected(mm, at(1.0 - 2 * bm.M, 0.95), r, drawn, ONE)      # two margins outside: the tile alone
    assert ids(e) == {0} and 9 not in classes(e)
    e = bm.expected(mm, at(1.05, 0.95), r, np.array([False]), ONE)    # a hidden object: never a candidate
    assert ids(e) == {0} and 9 not in classes(e)


def test_a_cell_centre_on_a_tile_seam_or_the_grid_border_is_not_sure():
    mm = bm.map_model("small_loop")
    none, nobody = np.zeros((0, 4, 2)), np.zeros(0, bool)
    road = int(bm.tile_class(mm, np.array([2.5 * TS]), np.array([TS + 1e-3]))[0])
    e = bm.expected(mm, at(2.5 * TS, TS), none, nobody, ONE)          # the seam between the grass tile (2, 0) and the straight (2, 1)
    assert {L.FLOOR, road} <= classes(e) and road != L.FLOOR and not e.sure_cls[0, 0] and e.sure_id[0, 0]
    inner = int(bm.tile_class(mm, np.array([1e-3]), np.array([0.5 * TS]))[0])
    e = bm.expected(mm, at(0.0, 0.5 * TS), none, nobody, ONE)         # the grid's border x = 0
    assert {L.GROUND, inner} <= classes(e) and inner != L.GROUND and not e.sure_cls[0, 0]
    e = bm.expected(mm, at(-0.3, 0.5 * TS), none, nobody, ONE)        # well off the grid
    assert classes(e) == {L.GROUND} and e.cls[0, 0] == L.GROUND and e.sure_cls[0, 0]


def test_under_two_overlapping_rectangles_the_lowest_index_is_sure_only_off_both_edges():
    mm = bm.map_model("small_loop")._replace(obj_cls=np.array([9, 10], np.int64))
    r, drawn = np.stack([rect(1.0, 1.2, 0.9, 1.1), rect(1.1, 1.3, 0.9, 1.1)]), np.array([True, True])
    e = bm.expected(mm, at(1.15, 1.0), r, drawn, ONE)                # deep inside both
    assert e.inst[0, 0] == 1 and ids(e) == {1} and classes(e) == {9} and e.sure_id[0, 0]
    e = bm.expected(mm, at(1.1, 1.0), r, drawn, ONE)                 # deep inside the first, on the second's edge
    assert e.inst[0, 0] == 1 and ids(e) == {1, 2} and not e.sure_id[0, 0]
    e = bm.expected(mm, at(1.2, 1.0), r, drawn, ONE)                 # on the first's edge, deep inside the second: no tile alternative
    assert ids(e) == {1, 2} and classes(e) == {9, 10} and not e.sure_id[0, 0]
    e = bm.expected(mm, at(1.25, 1.0), r, drawn, ONE)                # the second alone
    assert e.inst[0, 0] == 2 and ids(e) == {2} and e.sure_id[0, 0]
    e = bm.expected(mm, at(1.15, 1.0), r, np.array([False, True]), ONE)   # the first hidden: the second shows
    assert e.inst[0, 0] == 2 and ids(e) == {2}


def test_the_margin_is_the_derived_one():
    assert bm.M == 1e-4 and 3 * 16 * 2.0 ** -19 <= bm.M
    for name in ("small_loop", "test_town", "mm_t47"):
        assert bm.map_model(name).texel > 10 * bm.M                    # the texel neighbourhood is wider than the margin


# ---- the condition on the device test's inputs -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(bm.CASES))
def test_at_least_four_fifths_of_every_case_are_sure(case):
    prof = open(os.path.join(ROOT, "profiles", "bev_parity.txt")).read()
    for shape in bm.SHAPES:
        a, b = bm.sure_shares(case, shape)
        print(f"{case} {shape}: sure class {a:.4f}, sure id {b:.4f}")
        assert a >= 0.8 and b >= 0.8, (case, shape, a, b)
        m = re.search(rf"^{case}\s+{shape[0]:3d} x {shape[1]:3d} cell {shape[2]:.3f} behind {shape[3]:3d} .*sure class (\S+)  sure id (\S+)", prof, re.M)
        assert m and abs(float(m.group(1)) - a) <= 5e-4 and abs(float(m.group(2)) - b) <= 5e-4, (case, shape, m and m.group(0))


def test_the_cases_reach_what_the_device_test_is_meant_to_see():
    big = bm.SHAPES[0]
    seen = {name: set() for name in bm.CASES}
    for name, c in bm.CASES.items():
        for k in range(len(c.poses)):
            for e in bm.host_expected(name, k, big):
                seen[name] |= {int(v) for v in np.unique(e.cls)} | {-int(v) for v in np.unique(e.inst) if v}
    marks = {L.MARK_WHITE, L.MARK_YELLOW}
    assert {L.GROUND, L.FLOOR, L.ROAD} | marks <= seen["small_loop"] and not any(v < 0 for v in seen["small_loop"])
    assert L.MARK_RED in seen["test_town"]                                         # the 4-way's stop line
    assert {L.CLASS_IDS[k] for k in ("cone", "sign", "tree", "duckiebot")} <= seen["test_town"]
    assert L.CLASS_IDS["duckie"] in seen["loop_pedestrians"] and L.CLASS_IDS["duckie"] in seen["two_maps"]
    crowd = {-v for v in seen["crowd"] if v < 0}
    assert len(crowd) >= 30 and not crowd & {h + 1 for h in bm.CASES["crowd"].hidden}
    # the walking duckies have walked: the footprints after the steps are not the map's
    moved, _ = bm.host_footprints("loop_pedestrians")[0]
    still, _ = bm.host_footprints("two_maps")[0]
    assert moved.shape == still.shape and np.abs(moved - still).max() > 0.01
    a, b = bm.map_model("loop_pedestrians"), bm.map_model("mm_t47")
    assert a.sc.m.tile_size != b.sc.m.tile_size and len(a.obj_cls) != len(b.obj_cls)  # two tile sizes, two object lists
    # the corner pose looks off the grid: most of its window is ground
    assert (bm.host_expected("small_loop", 2, big)[0].cls == L.GROUND).mean() > 0.5


# ---- the binding ----------------------------------------------------------------------------------------------------------------------

def test_the_entry_point_is_declared_mirrored_and_exported():
    src = open(os.path.join(ROOT, "include", "dtsim.h")).read()
    assert re.search(r"^int dtsim_bev\(dtsim_t\* h, uint8_t\* cls, uint8_t\* inst, int oh, int ow, double cell, int rows_behind, uint32_t flags, "
                     r"const uint8_t\* mask\);", src, re.M)
    m = re.search(r"#define DTSIM_BEV_MAX_SIDE (\d+)", src)
    assert m and int(m.group(1)) == _ffi.BEV_MAX_SIDE == 1024
    assert re.search(r"#define DTSIM_ABI_VERSION 12\b", src) and _ffi.ABI_VERSION == 12
    lib = _ffi.load()
    assert "dtsim_bev" in _ffi.EXPORTS and len(lib.dtsim_bev.argtypes) == 9
    assert lib.dtsim_bev(None, None, None, 1, 1, 0.02, 0, 0, None) == _ffi.E_INVALID     # a null handle, before anything touches a device


def test_ob_corners_lies_where_the_slab_has_it():
    for n in (1, 33, 130, 4096):
        off = 0
        for name, dt, planes in sf.ARRAYS:
            if name == "ob_corners":
                break
            off += (n * planes * np.dtype(dt).itemsize + 255) & ~255
        assert BatchedSimulator._state_array_offset("ob_corners", n) == off
    with pytest.raises(KeyError):
        BatchedSimulator._state_array_offset("ob_vel", 4)


PACKER_PROGRAM = r"""
#include "scene_tables.h"
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %d: %s (%s)\n", __LINE__, #c, err.c_str()); return 1; } } while (0)
struct Map1 {                                                // a 1 x 1 map of one empty tile with n objects
  uint8_t kind = DTSIM_TILE_EMPTY, angle = 0, cnt = 0;
  int16_t tex = -1, off = -1;
  std::vector<dtsim_object> objs;
  dtsim_map m{};
  Map1(int n, int first_dynamic, double base) : objs((size_t)n) {
    for (int o = 0; o < n; ++o) {
      dtsim_object& ob = objs[o];
      ob = dtsim_object{};
      ob.mesh_id = -1; ob.dynamic = o >= first_dynamic ? 1 : 0; ob.collidable = ob.dynamic ? 0 : 1; ob.scale = 1.0; ob.safety_radius = 0.1;
      for (int k = 0; k < 8; ++k) ob.corners[k] = base + o * 8 + k;
    }
    m.grid_w = m.grid_h = 1; m.tile_size = 0.5;
    m.tile_kind = &kind; m.tile_angle = &angle; m.tile_tex = &tex; m.tile_curve_off = &off; m.tile_curve_cnt = &cnt;
    m.n_objects = n; m.objects = n ? objs.data() : nullptr;     // exactly n objects: a read past the list is a heap overflow here
  }
};
int main() {
  std::string err;
  Map1 a(3, 2, 1000.0), b(0, 0, 0.0), c(DTSIM_MAX_OBJECTS, DTSIM_MAX_OBJECTS - DTSIM_MAX_DYNAMIC, 5000.0);
  const dtsim_map maps[3] = {a.m, b.m, c.m};
  std::vector<double> t{-1.0};
  CHECK(dt_pack_object_corners(t, err, maps, 3) == DTSIM_OK);
  CHECK(t.size() == (size_t)(3 + DTSIM_MAX_OBJECTS) * 8);
  for (int o = 0; o < 3; ++o) for (int k = 0; k < 8; ++k) CHECK(t[(size_t)o * 8 + k] == 1000.0 + o * 8 + k);
  for (int o = 0; o < DTSIM_MAX_OBJECTS; ++o) for (int k = 0; k < 8; ++k) CHECK(t[(size_t)(3 + o) * 8 + k] == 5000.0 + o * 8 + k);
  // every refusal leaves the output as it was
  const std::vector<double> t0 = t;
  CHECK(dt_pack_object_corners(t, err, nullptr, 3) == DTSIM_E_INVALID);
  CHECK(dt_pack_object_corners(t, err, maps, 0) == DTSIM_E_INVALID);
  dtsim_map bad = a.m; bad.objects = nullptr;
  CHECK(dt_pack_object_corners(t, err, &bad, 1) == DTSIM_E_INVALID);
  bad = a.m; bad.n_objects = DTSIM_MAX_OBJECTS + 1;
  CHECK(dt_pack_object_corners(t, err, &bad, 1) == DTSIM_E_INVALID);
  bad.n_objects = -1;
  CHECK(dt_pack_object_corners(t, err, &bad, 1) == DTSIM_E_INVALID);
  CHECK(t == t0);
  CHECK(dt_pack_object_corners(t, err, &b.m, 1) == DTSIM_OK && t.empty());     // no object anywhere: an empty table
  // dt_pack_maps keeps the table in the order of its object instances: object o of map m at RenderMapDev.obj_off + o
  AssetTables none;
  CHECK(dt_pack_assets(none, err, nullptr, 0, nullptr, 0) == DTSIM_OK);
  MapTables M;
  CHECK(dt_pack_maps(M, err, maps, 3, none, false) == DTSIM_OK);
  CHECK(M.ocorners.size() == M.robjs.size() * 8 && M.ocorners == t0);
  CHECK(M.rmaps[0].obj_off == 0 && M.rmaps[1].obj_off == 3 && M.rmaps[2].obj_off == 3 && M.rmaps[2].n_obj == DTSIM_MAX_OBJECTS);
  for (int o = 0; o < DTSIM_MAX_OBJECTS; ++o) {
    CHECK(M.ocorners[(size_t)(M.rmaps[2].obj_off + o) * 8] == 5000.0 + o * 8);
    CHECK(M.robjs[M.rmaps[2].obj_off + o].dyn_slot == (o < DTSIM_MAX_OBJECTS - DTSIM_MAX_DYNAMIC ? -1 : o - (DTSIM_MAX_OBJECTS - DTSIM_MAX_DYNAMIC)));
  }
  // a failed dt_pack_maps leaves its output, the table included
  const std::vector<double> kept = M.ocorners;
  CHECK(dt_pack_maps(M, err, maps, DTSIM_MAX_MAPS + 1, none, false) == DTSIM_E_LIMIT && M.ocorners == kept);
  return 0;
}
"""


def test_the_corner_table_packer_under_sanitizers(tmp_path):
    """dt_pack_object_corners and its use in dt_pack_maps (csrc/scene_tables.h: plain C++) in a program of its own, built with
    AddressSanitizer and UndefinedBehaviorSanitizer and run as a child process: the layout over three maps (one without objects, one at the
    object limit), every refusal, the empty case; it exits clean."""
    (tmp_path / "corner_table.cpp").write_text(PACKER_PROGRAM)
    exe = tmp_path / "corner_table"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                           str(tmp_path / "corner_table.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]


# ---- the vector env's arguments ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw,word", [
    (dict(bev_instances=True), "bev_shape"),
    (dict(bev_shape=64), "bev_shape"),
    (dict(bev_shape=(64, 64, 1)), "bev_shape"),
    (dict(bev_shape=(0, 64)), "1 .."),
    (dict(bev_shape=(64, 1025)), "1 .."),
    (dict(bev_shape=(64, 64), bev_cell=0.0), "bev_cell"),
    (dict(bev_shape=(64, 64), bev_cell=float("nan")), "bev_cell"),
    (dict(bev_shape=(64, 64), bev_cell=float("inf")), "bev_cell"),
    (dict(bev_shape=(64, 64), bev_rows_behind=65), "bev_rows_behind"),
    (dict(bev_shape=(64, 64), bev_rows_behind=-1), "bev_rows_behind"),
    (dict(bev_shape=(64, 64), bev_rows_behind=1.5), "bev_rows_behind"),
    (dict(bev_shape=(64, 64), render=False), "render"),
])
def test_the_vector_env_refuses_bad_arguments_before_it_touches_a_device(kw, word):
    from dtsim.vecenv import DuckietownVecEnv
    with pytest.raises(ValueError, match=word):
        DuckietownVecEnv("small_loop", 4, **kw)
