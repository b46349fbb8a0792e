"""`not gpu`: the label map's model (tests/label_model.py) and the host side of dtsim_labels, on the oracle alone: the nearest-sample rule on
hand-made buffers; the marking rule and the default tables of dtsim/labels.py on the fixtures and on tests/golden/assets; that the oracle
against its nudged self disagrees on at most a quarter of the cap on every case (and nowhere on the sure mask); that the cases reach what
the GPU test is meant to see; the C-ABI's declarations; the table packer of csrc/scene_tables.h in a program of its own under
AddressSanitizer and UndefinedBehaviorSanitizer; and that DuckietownVecEnv refuses bad label arguments before a device is touched."""
import os
import re
import subprocess

import numpy as np
import pytest

import depth_model as dm
import frame_parity as fp
import label_model as lm
from dtsim import DuckietownVecEnv, _ffi, assets, labels as L, maps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gym-duckietown_amd", "csrc")
ENVS = [(name, e) for name, c in lm.CASES.items() for e in range(len(c.states))]
INF = np.inf


# ---- the model on hand-made buffers ------------------------------------------------------------------------------------------------

def test_nearest_sample_ties_sky_and_a_hair():
    # one pixel per column: [4 samples][1][n]
    depths = np.array([[2.0, 2.0, INF, INF, 1.0, 3.0],
                       [2.0, 1.0, INF, 5.0, 1.0, 3.0],
                       [1.0, 1.0, INF, INF, np.nextafter(1.0, 0.0), 3.0],
                       [1.0, 2.0, INF, 4.0, 1.0, np.nextafter(3.0, 0.0)]])[:, None, :]
    #                  tie 2/3 -> 2; tie 1/2 -> 1; all sky -> 0; sky loses -> 3; a mesh sample nearer by one ulp -> 2; -> 3
    assert lm.nearest_sample(depths)[0].tolist() == [2, 1, 0, 3, 2, 3]
    cls = np.array([[L.ROAD] * 6, [L.MARK_WHITE] * 6, [9] * 6, [L.GROUND] * 6])[:, None, :]
    cls[0, 0, 2] = L.SKY
    assert lm.labels_of(depths, cls)[0].tolist() == [9, L.MARK_WHITE, L.SKY, L.GROUND, 9, L.GROUND]
    # all four equal: the lowest index
    assert lm.nearest_sample(np.full((4, 2, 2), 0.7)).tolist() == [[0, 0], [0, 0]]


def test_compare_holds_the_sure_pixels_exactly_and_caps_the_rest():
    want = np.full((10, 100), L.ROAD, np.uint8)
    want[0, :5] = 0
    sure = np.ones(want.shape, bool)
    sure[5, :10] = False
    got = want.copy()
    assert lm.compare(got, want, sure, 1e-3)["n_off"] == 0
    got[5, 3] = L.MARK_WHITE                                  # one unsure pixel of 1000: at the cap
    assert lm.compare(got, want, sure, 1e-3)["n_off"] == 1
    got[5, 4] = L.MARK_WHITE
    with pytest.raises(AssertionError):
        lm.compare(got, want, sure, 1e-3)                     # two: beyond it
    got = want.copy()
    got[7, 7] = L.MARK_WHITE
    with pytest.raises(AssertionError, match="sure pixels differ"):
        lm.compare(got, want, sure, 1.0)
    got = want.copy()
    got[0, 0] = L.ROAD
    with pytest.raises(AssertionError, match="border"):
        lm.compare(got, want, sure, 1.0)


# ---- dtsim/labels.py ---------------------------------------------------------------------------------------------------------------

def test_the_marking_rule_separates_the_fixture_paint():
    assert L.marking_class(np.array([(232, 232, 226), (238, 200, 36), (200, 40, 36)], np.uint8)).tolist() == [L.MARK_WHITE, L.MARK_YELLOW, L.MARK_RED]
    # with the fixtures' noise (+- 14 x 1.2 on every channel at most) the three still fall apart
    rng = np.random.default_rng(0)
    for rgb, want in (((232, 232, 226), L.MARK_WHITE), ((238, 200, 36), L.MARK_YELLOW), ((200, 40, 36), L.MARK_RED)):
        noisy = np.clip(np.array(rgb) + rng.integers(-17, 18, (500, 3)), 0, 255).astype(np.uint8)
        assert (L.marking_class(noisy) == want).all(), rgb
    assert (L.NONE, L.SKY, L.GROUND, L.FLOOR, L.ROAD, L.MARK_WHITE, L.MARK_YELLOW, L.MARK_RED, L.OBJECT_FIRST) == tuple(range(9))


def _paint_hue(tex, sel):
    """Median hue (degrees) and share of the selected texels, from the RGB bytes (independent of the rule under test)."""
    rgb = tex[..., :3][sel].astype(np.float64)
    mx, mn = rgb.max(axis=1), rgb.min(axis=1)
    d = np.maximum(mx - mn, 1e-9)
    r, g, b = rgb.T
    h = np.where(mx == r, (g - b) / d % 6, np.where(mx == g, (b - r) / d + 2, (r - g) / d + 4)) * 60
    sat = (mx - mn) / np.maximum(mx, 1)
    return h, sat


@pytest.mark.parametrize("tree", [False, True])
def test_default_texel_classes_of_every_tile_texture(tree):
    """Every drivable texture has ROAD and at least one marking class, every other one is constant FLOOR; and the marking classes are
    the paint's colours: red texels have a red hue, yellow ones a yellow hue, white ones are unsaturated or bright -- on the fixtures and
    on the photographed textures of tests/golden/assets."""
    tiles, _ = lm.host_tables("town" if tree else "pedestrians")
    sc = lm.scene_of("town" if tree else "pedestrians")
    if not tree:
        tiles = dict(tiles)
        for kd in ("curve_left", "curve_right", "3way_left", "4way", "floor", "asphalt", "grass"):     # every fixture kind
            tex = assets.get_texture(kd)
            tiles[kd] = L.texel_classes(tex, assets.segment_texture(tex, os.path.join("tiles-processed", "photos", kd, "texture.png")), kd)
    seen = set()
    for kd, t in tiles.items():
        tex = sc.textures[kd] if kd in sc.textures else assets.get_texture(kd)
        assert t.shape == tex.shape[:2] and t.dtype == np.uint8
        if kd not in maps.DRIVABLE:
            assert (t == L.FLOOR).all(), kd
            continue
        ids = set(np.unique(t).tolist())
        assert L.ROAD in ids and ids & {L.MARK_WHITE, L.MARK_YELLOW, L.MARK_RED} and ids <= {L.ROAD, L.MARK_WHITE, L.MARK_YELLOW, L.MARK_RED}, (kd, ids)
        assert (t == L.ROAD).mean() > 0.8, kd
        seen |= ids
        for cid, lo, hi in ((L.MARK_RED, -25.0, 25.0), (L.MARK_YELLOW, 30.0, 70.0)):
            sel = t == cid
            if sel.sum() >= 16:
                h, sat = _paint_hue(tex, sel)
                h = (h + 180) % 360 - 180
                assert lo <= np.median(h) <= hi and np.median(sat) > 0.4, (kd, cid, float(np.median(h)), float(np.median(sat)))
        sel = t == L.MARK_WHITE
        if sel.sum() >= 16:
            _, sat = _paint_hue(tex, sel)
            assert np.median(sat) < 0.35, (kd, float(np.median(sat)))
    assert {L.MARK_WHITE, L.MARK_YELLOW, L.MARK_RED} <= seen


def test_mesh_classes_are_stable_and_injective_on_the_default_kinds():
    kinds = ("duckiebot", "duckie", "cone", "sign_stop", "trafficlight", "building", "tree", "bus", "barrier", "*")
    ids = L.mesh_classes(kinds)
    assert ids.dtype == np.uint8 and ids.tolist() == list(range(8, 18))                 # from 8 up, in this order: the ids are part of the interface
    assert len(set(ids.tolist())) == len(kinds) and ids.min() >= L.OBJECT_FIRST
    assert L.mesh_class("house") == L.mesh_class("building") and L.mesh_class("truck") == L.mesh_class("bus")
    assert L.mesh_class("duckiebot:red") == L.CLASS_IDS["duckiebot"] and L.mesh_class("duckie") == L.CLASS_IDS["duckie"]
    assert L.mesh_class("sign_T_intersect") == L.CLASS_IDS["sign"] and L.mesh_class("checkerboard") == L.CLASS_IDS["object"]
    assert all(L.CLASS_IDS[n] == i for i, n in L.CLASS_NAMES.items()) and len(L.CLASS_NAMES) == 18
    assert L.mesh_classes(()).shape == (0,)
    _, obj = lm.host_tables("town")                          # cone, sign_stop, tree, duckiebot, duckie, cone, trafficlight
    assert [L.CLASS_NAMES[int(k)] for k in obj] == ["cone", "sign", "tree", "duckiebot", "duckie", "cone", "trafficlight"]


def test_texel_classes_refuses_mismatched_arrays():
    tex = assets.get_texture("straight")
    with pytest.raises(ValueError):
        L.texel_classes(tex, tex[:128], "straight")


# ---- the cap's condition -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,e", ENVS)
def test_the_nudged_oracle_stays_within_a_quarter_of_the_cap(name, e):
    """A disagreement with the oracle is allowed only off the sure mask, on at most Case.cap of the pixels; the oracle's own class flips
    under a perturbation of the size of float32 rounding must leave three quarters of that, and none of them may lie on the sure mask."""
    r = lm.nudge_share(name, e)
    c = lm.CASES[name]
    print(f"{name} env {e}: off {r['off']:.2e} ({r['n_off']} px), unsure {r['unsure']:.3f}, cap / 4 = {c.cap / 4:.2e}")
    assert r["off"] <= c.cap / 4, (name, e, r)
    assert r["sure_off"] == 0
    assert c.cap == (fp.ORACLE_MESH.gt1 if c.mesh else fp.ORACLE_PLANE.gt1)
    # the sure mask holds most of every frame, so exact equality means something (the close-ups of photographed paint have the most class
    # edges: a texel is seven pixels wide there, and a pixel within a texel of an edge is not sure)
    assert r["unsure"] < 0.5, (name, e, r)
    # the recorded shares (profiles/labels_parity.txt) state this run
    prof = open(os.path.join(ROOT, "profiles", "labels_parity.txt")).read()
    m = re.search(rf"^{name}\s+env {e}\s.*?off (\S+) \(\s*(\d+) px\)", prof, re.M)
    assert m and int(m.group(2)) == r["n_off"] and abs(float(m.group(1)) - r["off"]) <= 5e-3 * max(r["off"], 1e-9), (name, e, m and m.group(0))


def test_the_cases_reach_what_the_device_test_is_meant_to_see():
    assert set(dm.CASES) < set(lm.CASES) and len(lm.OWN) >= 2
    marks = {L.MARK_WHITE, L.MARK_YELLOW, L.MARK_RED}
    seen = {}
    for name, e in ENVS:
        lab, sure = lm.expected(name, e)
        ids, n = np.unique(lab, return_counts=True)
        for k, v in zip(ids.tolist(), n.tolist()):
            seen.setdefault(name, {}).setdefault(k, 0)
            seen[name][k] += v
        assert 0 not in ids                                   # no border without a source map
        if name in dm.CASES:
            assert L.SKY in ids and L.GROUND in ids, (name, e)
    # the marking cases: markings fill the view -- thousands of pixels, where a road pose has a few hundred
    assert seen["marks_straight"][L.MARK_WHITE] > 3000 and seen["marks_straight"][L.MARK_YELLOW] > 900, seen["marks_straight"]
    assert seen["marks_town"][L.MARK_RED] > 3000 and seen["marks_town"].get(L.MARK_YELLOW, 0) > 300 and L.MARK_WHITE in seen["marks_town"], seen["marks_town"]
    for e in range(3):
        assert max(int((lm.expected(n, e)[0] == k).sum()) for n in lm.OWN for k in marks) > 500
    # the objects of the town: five default classes in view
    assert {L.CLASS_IDS[k] for k in ("cone", "sign", "tree", "duckiebot", "duckie", "trafficlight")} <= set(seen["town"])
    assert L.CLASS_IDS["duckie"] in seen["pedestrians"]
    # through the rectify map there is a border, and it is sure
    lab, sure = lm.expected("planes", 0, "undistort")
    assert (lab == 0).sum() > 300 and sure[lab == 0].all()
    lab, _ = lm.expected("planes", 0, "fisheye")
    assert (lab == 0).sum() == 0


def test_a_tile_seam_is_never_sure_unless_both_tiles_agree():
    """The 3 x 3 neighbourhood is taken in the world: next to a grass tile (FLOOR) the road's edge texels (ROAD) are not sure."""
    name = "planes"
    sc = lm.scene_of(name)
    tiles, _ = lm.host_tables(name)
    ts = sc.m.tile_size
    z = np.array([1.0 * ts + 1e-4])                                            # just inside the straight at tile (2, 1)
    x = np.array([2.5 * ts])
    assert lm.tile_class_at(sc, tiles, x, z)[0] in (L.ROAD, L.MARK_WHITE, L.MARK_YELLOW)
    assert lm.tile_class_at(sc, tiles, x, z - ts / 256)[0] == L.FLOOR          # one texel further: the grass tile
    assert lm.tile_class_at(sc, tiles, np.array([-0.1]), np.array([0.3]))[0] == -1


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------------------

def test_entry_points_are_declared_mirrored_and_exported():
    src = open(os.path.join(ROOT, "include", "dtsim.h")).read()
    assert re.search(r"^int dtsim_set_label_assets\(dtsim_t\* h, const uint8_t\* const\* texel_class, int n_textures, const uint8_t\* mesh_class, int n_meshes\);", src, re.M)
    assert re.search(r"^int dtsim_labels\(dtsim_t\* h, uint8_t\* out, int oh, int ow, uint32_t flags\);", src, re.M)
    assert re.search(r"^int dtsim_labels_masked\(dtsim_t\* h, uint8_t\* out, int oh, int ow, uint32_t flags, const uint8_t\* mask\);", src, re.M)
    for name, value in (("NONE", 0), ("SKY", 1), ("GROUND", 2), ("FLOOR", 3), ("ROAD", 4), ("MARK_WHITE", 5), ("MARK_YELLOW", 6), ("MARK_RED", 7)):
        m = re.search(rf"DTSIM_LABEL_{name} = (\d+)", src)
        assert m and int(m.group(1)) == value == getattr(_ffi, "LABEL_" + name) == getattr(L, name), name
    assert re.search(r"#define DTSIM_ABI_VERSION 12\b", src) and _ffi.ABI_VERSION == 12
    lib = _ffi.load()
    for name in ("dtsim_set_label_assets", "dtsim_labels", "dtsim_labels_masked"):
        assert name in _ffi.EXPORTS and getattr(lib, name) is not None
    assert lib.dtsim_abi_version() == 12
    # a null handle is refused before anything touches a device
    assert lib.dtsim_labels(None, None, 1, 1, 0) == _ffi.E_INVALID
    assert lib.dtsim_labels_masked(None, None, 1, 1, 0, None) == _ffi.E_INVALID
    assert lib.dtsim_set_label_assets(None, None, 0, None, 0) == _ffi.E_INVALID


PACKER_PROGRAM = r"""
#include "scene_tables.h"
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %d: %s (%s)\n", __LINE__, #c, err.c_str()); return 1; } } while (0)
int main() {
  std::string err;
  AssetTables A, none;
  // three textures of different sizes (the last 1 x 1) and two meshes
  const int W[3] = {8, 4, 1}, H[3] = {4, 16, 1};
  std::vector<std::vector<uint8_t>> px, cls;
  std::vector<dtsim_texture> tx;
  for (int t = 0; t < 3; ++t) {
    px.emplace_back((size_t)W[t] * H[t] * 4, (uint8_t)t);
    cls.emplace_back((size_t)W[t] * H[t]);                   // exactly h x w bytes: a read past a table's end is a heap overflow here
    for (size_t i = 0; i < cls.back().size(); ++i) cls.back()[i] = (uint8_t)(3 + (i * 5 + t) % 250);
  }
  for (int t = 0; t < 3; ++t) tx.push_back({W[t], H[t], px[t].data()});
  std::vector<float> v(9, 0.25f);
  std::vector<dtsim_mesh> ms(2, dtsim_mesh{1, v.data(), v.data(), v.data(), nullptr, nullptr});
  CHECK(dt_pack_assets(A, err, tx.data(), 3, ms.data(), 2) == DTSIM_OK);
  const uint8_t* tc[3] = {cls[0].data(), cls[1].data(), cls[2].data()};
  const uint8_t mc[2] = {8, 201};
  std::vector<uint8_t> pool{1, 2, 3}, mesh{4};
  CHECK(dt_pack_label_tables(pool, mesh, err, tc, 3, mc, 2, A) == DTSIM_OK);
  CHECK(pool.size() == A.pool.size() && mesh.size() == 2 && mesh[0] == 8 && mesh[1] == 201);
  for (int t = 0; t < 3; ++t)                                // every texel where the texel pool has it, the padding wrapped as GL_REPEAT
    for (int y = 0; y <= H[t]; ++y)
      for (int x = 0; x <= W[t]; ++x)
        CHECK(pool[A.tex[t].off + (size_t)y * (W[t] + 1) + x] == cls[t][(size_t)(y % H[t]) * W[t] + x % W[t]]);
  // every refusal leaves the outputs as they were
  const std::vector<uint8_t> pool0 = pool, mesh0 = mesh;
  CHECK(dt_pack_label_tables(pool, mesh, err, tc, 2, mc, 2, A) == DTSIM_E_INVALID);
  CHECK(dt_pack_label_tables(pool, mesh, err, tc, 3, mc, 1, A) == DTSIM_E_INVALID);
  CHECK(dt_pack_label_tables(pool, mesh, err, tc, 4, mc, 2, A) == DTSIM_E_INVALID);
  CHECK(dt_pack_label_tables(pool, mesh, err, nullptr, 3, mc, 2, A) == DTSIM_E_INVALID);
  CHECK(dt_pack_label_tables(pool, mesh, err, tc, 3, nullptr, 2, A) == DTSIM_E_INVALID);
  const uint8_t* hole[3] = {cls[0].data(), nullptr, cls[2].data()};
  CHECK(dt_pack_label_tables(pool, mesh, err, hole, 3, mc, 2, A) == DTSIM_E_INVALID);
  CHECK(pool == pool0 && mesh == mesh0);
  // no textures and no meshes: empty pool, one (unused) mesh entry, null arrays accepted
  CHECK(dt_pack_assets(none, err, nullptr, 0, nullptr, 0) == DTSIM_OK);
  CHECK(dt_pack_label_tables(pool, mesh, err, nullptr, 0, nullptr, 0, none) == DTSIM_OK && pool.empty() && mesh.size() == 1 && mesh[0] == 0);
  // the limits of dtsim_set_assets
  px.assign(DTSIM_MAX_TEXTURES, std::vector<uint8_t>(2 * 2 * 4, 9));
  tx.clear();
  for (auto& p : px) tx.push_back({2, 2, p.data()});
  std::vector<dtsim_mesh> many(DTSIM_MAX_MESHES, ms[0]);
  CHECK(dt_pack_assets(A, err, tx.data(), DTSIM_MAX_TEXTURES, many.data(), DTSIM_MAX_MESHES) == DTSIM_OK);
  std::vector<std::vector<uint8_t>> c2(DTSIM_MAX_TEXTURES, std::vector<uint8_t>(4, 7));
  std::vector<const uint8_t*> p2;
  for (auto& c : c2) p2.push_back(c.data());
  std::vector<uint8_t> m2(DTSIM_MAX_MESHES, 255);
  CHECK(dt_pack_label_tables(pool, mesh, err, p2.data(), DTSIM_MAX_TEXTURES, m2.data(), DTSIM_MAX_MESHES, A) == DTSIM_OK);
  CHECK(pool.size() == (size_t)DTSIM_MAX_TEXTURES * 9 && mesh.size() == DTSIM_MAX_MESHES && mesh.back() == 255);
  for (uint8_t b : pool) CHECK(b == 7);
  return 0;
}
"""


def test_the_table_packer_under_sanitizers(tmp_path):
    """dt_pack_label_tables (csrc/scene_tables.h: plain C++) in a program of its own, built with AddressSanitizer and
    UndefinedBehaviorSanitizer and run as a child process: the layout, every refusal, the empty case and the limits; it exits clean."""
    (tmp_path / "label_tables.cpp").write_text(PACKER_PROGRAM)
    exe = tmp_path / "label_tables"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                           str(tmp_path / "label_tables.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]


# ---- the vector env ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw,word", [
    (dict(label_shape=(60, 80), motion_blur=True, action_mode="wheels"), "motion_blur"),
    (dict(label_shape=(60, 80), camera_rand=True, distortion=True), "camera_rand"),
    (dict(label_shape=(50, 80)), "divide"),                              # 120 % 50
    (dict(label_shape=(60, 81)), "divide"),
    (dict(label_shape=(0, 80)), "divide"),
    (dict(label_shape=(240, 320)), "divide"),                            # larger than the camera
    (dict(label_shape=60), "label_shape"),
    (dict(label_shape=(60, 80, 3)), "label_shape"),
    (dict(label_shape=("a", "b")), "label_shape"),
    (dict(label_shape=(60, 80), depth_shape=(50, 80)), "depth_shape"),   # both on: depth's own refusal still comes first
])
def test_vecenv_refuses_bad_label_arguments_before_a_device_is_touched(kw, word, monkeypatch):
    import torch

    def touched(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(torch.cuda, "set_device", touched)
    monkeypatch.setattr(torch.cuda, "Stream", touched)
    monkeypatch.setattr(_ffi, "load", touched)
    with pytest.raises(ValueError, match=word):
        DuckietownVecEnv("small_loop", 4, camera_width=160, camera_height=120, **kw)
