"""The scene tables of csrc/scene_tables.h, packed on this CPU: the packers behind dtsim_set_assets, dtsim_set_segment_assets,
dtsim_set_maps and dtsim_set_distortion_lut, compiled with g++ behind a test-only extern "C" wrapper and given the ctypes arrays
BatchedSimulator gives libdtsim (batched.load_scene / scene_ffi).  The tile orientation is held to an independent statement: the four
taps of a quad record, blended, against the TileLds affine map over the padded texel pool."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from dtsim import _ffi, assets, batched

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "gym-duckietown_amd", "csrc")
GOLDEN_ASSETS = os.path.join(HERE, "golden", "assets")
QRING, LDS_TILES, STATIC_WORDS, OBJ_WORDS, HDR_WORDS = 4, 1024, 15, 6, 8

WRAPPER = r"""
#include "scene_tables.h"
namespace {
AssetTables A;
MapTables M;
std::vector<uint32_t> seg;
std::vector<uint8_t> rgbx;
std::vector<float> lut;
std::string err;
}
extern "C" {
const char* st_err() { return err.c_str(); }
int st_assets(const dtsim_texture* t, int nt, const dtsim_mesh* m, int nm) { return dt_pack_assets(A, err, t, nt, m, nm); }
int st_segment(const dtsim_texture* t, int nt, const uint8_t* rgb, int nm) { return dt_pack_segment_texels(seg, rgbx, err, t, nt, rgb, nm, A); }
int st_maps(const dtsim_map* m, int n, int render) { return dt_pack_maps(M, err, m, n, A, render != 0); }
void st_lut(int W, int H, const float* rx, const float* ry) { dt_pack_lut(W, H, rx, ry, lut); }
size_t st_table(int id, const void** p) {
#define TABLE(i, v) case i: *p = v.data(); return v.size() * sizeof(v[0]);
  switch (id) {
    TABLE(0, A.pool) TABLE(1, A.tex) TABLE(2, A.meshes) TABLE(3, A.tris)
    TABLE(4, M.blobs) TABLE(5, M.dyn) TABLE(6, M.rmaps) TABLE(7, M.rtiles) TABLE(8, M.trecs) TABLE(9, M.robjs) TABLE(10, M.qblocks) TABLE(11, M.qtiles)
    TABLE(12, seg) TABLE(13, rgbx) TABLE(14, lut)
  }
  *p = nullptr;
  return 0;
}
size_t st_scalars(const void** p) { *p = static_cast<const MapScalars*>(&M); return sizeof(MapScalars); }
void st_tile_lds(int w, int h, int off, int ang, TileLds* out) { TexDev td{w, h, off, 0}; *out = TileLds{}; dt_tile_lds_map(*out, td, ang); }
void st_quad_block(const uint32_t* pool, int S, int ang, uint32_t* out) {
  std::vector<uint32_t> v;
  dt_pack_quad_block(v, pool, S, ang);
  memcpy(out, v.data(), v.size() * 4);
}
}
"""
TABLES = dict(pool=(0, "<u4"), tex=(1, [("w", "<i4"), ("h", "<i4"), ("off", "<i4"), ("pad", "<i4")]),
              meshes=(2, [("n_tris", "<i4"), ("off", "<i4"), ("mn", "<f4", 3), ("mx", "<f4", 3)]),
              tris=(3, [("v", "<f4", (3, 3)), ("n", "<f4", (3, 3)), ("c", "<f4", (3, 3)), ("uv", "<f4", (3, 2)), ("tex", "<i4"), ("pad", "<i4")]),
              blobs=(4, "<u8"),
              dyn=(5, [("cx", "<f8"), ("cz", "<f8"), ("corners", "<f8", 8), ("norm", "<f8", 4), ("heading", "<f8", 2), ("angle", "<f8"),
                       ("safety_radius", "<f8"), ("walk", "<f8", 4), ("obj_index", "<i4"), ("kind", "<i4")]),
              rmaps=(6, [("grid_w", "<i4"), ("grid_h", "<i4"), ("n_obj", "<i4"), ("n_tris", "<i4"), ("tile_size", "<f4"), ("inv_tile_size", "<f4"),
                         ("tile_off", "<i4"), ("obj_off", "<i4"), ("qt_off", "<i4"), ("qt_pitch", "<i4")]),
              rtiles=(7, "<u4"),
              trecs=(8, [("tex_off", "<u4"), ("flags", "<u4"), ("m", "<f4", 6)]),
              robjs=(9, [("xyz", "<f4", 3), ("scale", "<f4"), ("yrot_deg", "<f4"), ("mesh_id", "<i4"), ("dyn_slot", "<i4"), ("light_tris", "<i4"),
                         ("light_tex", "<i4", 2), ("pad", "<i4", 2)]),
              qblocks=(10, "<u4"), qtiles=(11, "<u4"), seg=(12, "<u4"), rgbx=(13, "u1"), lut=(14, "<f4"))
SCALARS = np.dtype([("n_maps", "<i4"), ("blob_off", "<i4", 32), ("total_words", "<i4"), ("blobs", "<u8"), ("dyn", "<u8"), ("grid_w", "<i4", 32),
                    ("grid_h", "<i4", 32), ("grid_rows", "<i4"), ("grid_cols", "<i4"), ("n_tilerecs", "<i4"), ("tex_w", "<i4"), ("tex_h", "<i4"),
                    ("n_qtiles", "<i4"), ("qlog2", "<i4"), ("q_per_m", "<f4"), ("max_tris", "<i4")], align=True)
HDR = np.dtype([(k, "<i4") for k in ("grid_w", "grid_h", "n_curves", "n_static", "n_dyn", "n_obj", "off_tiles", "off_curves", "off_heads", "off_static",
                                     "off_objs", "total_words", "n_lights", "pad_l")] + [("tile_size", "<f8")])
TILEREC = np.dtype([("kind", "u1"), ("angle", "u1"), ("drivable", "u1"), ("curve_cnt", "u1"), ("curve_off", "<i2"), ("tex", "<i2")])


class Packers:
    def __init__(self, so):
        self.lib = lib = C.CDLL(so)
        vpp = C.POINTER(C.c_void_p)
        lib.st_err.restype = C.c_char_p
        lib.st_assets.argtypes = [C.POINTER(_ffi.Texture), C.c_int, C.POINTER(_ffi.Mesh), C.c_int]
        lib.st_segment.argtypes = [C.POINTER(_ffi.Texture), C.c_int, C.POINTER(C.c_uint8), C.c_int]
        lib.st_maps.argtypes = [C.POINTER(_ffi.Map), C.c_int, C.c_int]
        lib.st_lut.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        lib.st_table.restype, lib.st_table.argtypes = C.c_size_t, [C.c_int, vpp]
        lib.st_scalars.restype, lib.st_scalars.argtypes = C.c_size_t, [vpp]
        lib.st_tile_lds.argtypes = [C.c_int] * 4 + [C.c_void_p]
        lib.st_quad_block.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]

    def err(self):
        return self.lib.st_err().decode()

    def table(self, name):
        tid, dt = TABLES[name]
        p = C.c_void_p()
        n = self.lib.st_table(tid, C.byref(p))
        return np.frombuffer(C.string_at(p, n) if n else b"", dtype=np.dtype(dt)).copy()

    def scalars(self):
        p = C.c_void_p()
        n = self.lib.st_scalars(C.byref(p))
        assert n == SCALARS.itemsize
        s = np.frombuffer(C.string_at(p, n), dtype=SCALARS)[0].copy()
        s["blobs"] = s["dyn"] = 0
        return s

    def snapshot(self):
        return [self.table(k).tobytes() for k in TABLES] + [self.scalars().tobytes()]

    def assets(self, textures, meshes=(), n_textures=None, n_meshes=None):
        tarr, marr = tex_array(textures), mesh_array(meshes)
        return self.lib.st_assets(tarr, len(textures) if n_textures is None else n_textures, marr, len(meshes) if n_meshes is None else n_meshes)

    def maps(self, ms, n=None, render=True):
        arr = (_ffi.Map * max(len(ms), 1))(*ms)
        return self.lib.st_maps(arr, len(ms) if n is None else n, int(render))

    def quad_block(self, pool, S, ang):
        out = np.zeros(S * S * 4, np.uint32)
        self.lib.st_quad_block(np.ascontiguousarray(pool, np.uint32).ctypes.data, S, ang, out.ctypes.data)
        return out

    def tile_lds(self, w, h, off, ang):
        out = np.zeros(1, TABLES["trecs"][1])
        self.lib.st_tile_lds(w, h, off, ang, out.ctypes.data)
        return out[0]


@pytest.fixture(scope="module")
def pk(tmp_path_factory):
    d = tmp_path_factory.mktemp("scene_tables")
    (d / "wrap.cpp").write_text(WRAPPER)
    so = d / "libscene_tables_test.so"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O1", "-shared", "-fPIC", "-I", CSRC, str(d / "wrap.cpp"), "-o", str(so)])
    return Packers(str(so))


def tex_array(textures):
    arr = (_ffi.Texture * max(len(textures), 1))()
    for i, t in enumerate(textures):
        if t is None:
            continue
        arr[i].width, arr[i].height = t.shape[1], t.shape[0]
        arr[i].rgba = t.ctypes.data_as(C.POINTER(C.c_uint8))
    return arr


def mesh_array(meshes):
    arr = (_ffi.Mesh * max(len(meshes), 1))()
    for i, m in enumerate(meshes):
        arr[i].n_tris = m["n_tris"]
        for k in ("verts", "normals", "colors", "uvs"):
            if m.get(k) is not None:
                setattr(arr[i], k, m[k].ctypes.data_as(C.POINTER(C.c_float)))
        if m.get("tri_tex") is not None:
            arr[i].tri_tex = m["tri_tex"].ctypes.data_as(C.POINTER(C.c_int32))
    return arr


def tri_mesh(n_tris=1, tex=None):
    m = dict(n_tris=n_tris, verts=np.arange(n_tris * 9, dtype=np.float32), normals=np.ones(n_tris * 9, np.float32), colors=np.full(n_tris * 9, .5, np.float32))
    if tex is not None:
        m.update(uvs=np.zeros(n_tris * 6, np.float32), tri_tex=np.full(n_tris, tex, np.int32))
    return m


def distinct_texture(w, h=None, seed=0):
    """every texel another (R, G) pair; B, A from a seeded draw"""
    h = h or w
    v = np.arange(w * h).reshape(h, w)
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.stack([v & 255, v >> 8, rng.integers(0, 256, (h, w)), rng.integers(0, 256, (h, w))], axis=-1).astype(np.uint8))


KEEP = []


def make_map(w, h, kind=7, tex=0, angle=0, objects=(), n_curves=0, tile_size=0.585, **over):
    """a synthetic dtsim_map: w x h tiles of one kind (7 asphalt: not drivable) unless arrays are given in `over`"""
    n = max(w * h, 1)
    a = dict(tile_kind=np.full(n, kind, np.uint8), tile_angle=np.full(n, angle, np.uint8), tile_tex=np.full(n, tex, np.int16),
             tile_curve_off=np.full(n, -1, np.int16), tile_curve_cnt=np.zeros(n, np.uint8),
             curves=np.arange(max(n_curves, 1) * 8, dtype=np.float64), curve_heads=np.ones(max(n_curves, 1) * 2))
    a.update({k: v for k, v in over.items() if k in a})
    m = _ffi.Map()
    m.grid_w, m.grid_h, m.tile_size, m.n_curves = w, h, tile_size, n_curves
    ct = dict(tile_kind=C.c_uint8, tile_angle=C.c_uint8, tile_tex=C.c_int16, tile_curve_off=C.c_int16, tile_curve_cnt=C.c_uint8,
              curves=C.c_double, curve_heads=C.c_double)
    for k, v in a.items():
        if v is not None:
            setattr(m, k, np.ascontiguousarray(v).ctypes.data_as(C.POINTER(ct[k])))
    objs = (_ffi.Object * max(len(objects), 1))()
    for i, o in enumerate(objects):
        objs[i].mesh_id, objs[i].scale = -1, 1.0
        for k, v in o.items():
            setattr(objs[i], k, v)
    m.n_objects, m.objects = over.get("n_objects", len(objects)), C.cast(objs, C.POINTER(_ffi.Object))
    if over.get("null_objects"):
        m.objects = None
    KEEP.append((a, objs))
    return m


# ---- orientation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [4, 8, 256])
def test_quad_records_and_tile_map_agree(pk, S):
    """For every angle, every cell (x0, z0) and the four points (x0 +- .25, z0 +- .25) / S of the tile frame: the bilinear blend of the
    record's four taps equals the GL_LINEAR blend (floor, GL_REPEAT wrap, +1 taps in the padding) of the padded pool through the TileLds
    affine map -- exactly (integer texels, float64 weights: every product and sum is exact).  The two are built from one
    dt_tile_orient; this restates neither."""
    t = distinct_texture(S, seed=S)
    assert pk.assets([t]) == 0
    pool = pk.table("pool").reshape(S + 1, S + 1)
    chan = np.stack([(pool >> (8 * c)) & 255 for c in range(3)], axis=-1).astype(np.float64)
    assert len({(int(r), int(g)) for r, g in chan[:S, :S, :2].reshape(-1, 2)}) == S * S
    z0, x0 = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    rec = ((x0 >> 2) << 10) | (z0 << 2) | (x0 & 3) if S == 256 else z0 * S + x0
    assert np.array_equal(np.sort(rec.ravel()), np.arange(S * S))
    for ang in range(4):
        blk = pk.quad_block(pool.ravel(), S, ang).reshape(S * S, 4)
        q = blk[rec]                                                     # [z0][x0][4]
        assert np.array_equal(q[..., 3], np.minimum(np.minimum(x0, S - x0), np.minimum(z0, S - z0)))
        taps = np.stack([[(q[..., c] >> (8 * k)) & 255 for k in range(4)] for c in range(3)], axis=-1).astype(np.float64)   # [tap][z0][x0][c]
        lds = pk.tile_lds(S, S, 0, ang)
        assert lds["flags"] == 2 and lds["tex_off"] == 0
        mxx, mxz, ox, myx, myz, oy = (float(v) for v in lds["m"])
        for a in (-.25, .25):
            for b in (-.25, .25):
                fx, fz = a + .5, b + .5                                  # the point inside quad cell (x0, z0): taps x0 - 1, x0
                rec_blend = (taps[0] * ((1 - fx) * (1 - fz)) + taps[1] * (fx * (1 - fz)) + taps[2] * ((1 - fx) * fz) + taps[3] * (fx * fz))
                px, pz = (x0 + a) / S, (z0 + b) / S
                x, y = mxx * px + mxz * pz + ox, myx * px + myz * pz + oy
                u, v = [1 - px, pz, px, 1 - pz][ang], [pz, px, 1 - pz, 1 - px][ang]      # glRotatef(angle * 90 + 180), uv = (pu, 1 - pv)
                assert np.array_equal(x, u * S - .5) and np.array_equal(y, v * S - .5), (S, ang)
                i0, j0 = np.floor(x), np.floor(y)
                wx, wy = (x - i0)[..., None], (y - j0)[..., None]
                i, j = i0.astype(np.int64) % S, j0.astype(np.int64) % S
                pool_blend = (chan[j, i] * ((1 - wx) * (1 - wy)) + chan[j, i + 1] * (wx * (1 - wy)) + chan[j + 1, i] * ((1 - wx) * wy)
                              + chan[j + 1, i + 1] * (wx * wy))
                assert np.array_equal(rec_blend, pool_blend), (S, ang, a, b)


# ---- the product's maps --------------------------------------------------------------------------------------------------------
PRODUCT_MAPS = [(n, None) for n in sorted(assets.MAPS)] + [("test_town", GOLDEN_ASSETS)]


def expected_quad_tiles(sc, S):
    """[n_qtiles][2] and the (texture, angle) pair of each block, blocks numbered as first met over the maps' padded grids, row by row"""
    block, out = {}, []
    for mt in sc.maps:
        for j in range(-QRING, mt.grid_h + QRING):
            for i in range(-QRING, mt.grid_w + QRING):
                off, sel = 0, 0
                if 0 <= i < mt.grid_w and 0 <= j < mt.grid_h and mt.tile_kind[j * mt.grid_w + i] != 0:
                    t = j * mt.grid_w + i
                    if mt.tile_tex[t] < 0:
                        off = 16
                    else:
                        b = block.setdefault((int(mt.tile_tex[t]), int(mt.tile_angle[t]) & 3), len(block))
                        off, sel = ((b + 1) << 20, 0xFFFFF) if S == 256 else (32 + b * S * S * 16, S * S - 1)
                out.append((off, sel))
    return np.array(out, np.uint32), block


@pytest.mark.parametrize("name,root", PRODUCT_MAPS, ids=[n for n, _ in PRODUCT_MAPS])
def test_tables_of_a_product_map(pk, name, root):
    lib = assets.AssetLibrary(root)
    sc = batched.load_scene(lib, [name], [lib.map_data(name)])
    tarr, marr, farr, keep = batched.scene_ffi(sc)
    assert pk.lib.st_assets(tarr, len(sc.textures), marr, len(sc.mesh_order)) == 0, pk.err()
    assert pk.lib.st_maps(farr, 1, 1) == 0, pk.err()
    mt, f, s = sc.maps[0], farr[0], pk.scalars()
    if name == "test_town":
        assert sc.textures[0].shape[0] == 128 and any(sc.meshes[k].textures for k in sc.mesh_order)
    # assets: the pool is each texture padded by its first row / column; meshes in order
    tex, pool, off = pk.table("tex"), pk.table("pool"), 0
    for t, d in zip(sc.textures, tex):
        h, w = t.shape[:2]
        assert (d["w"], d["h"], d["off"]) == (w, h, off)
        want = np.pad(t, ((0, 1), (0, 1), (0, 0)), mode="wrap").view("<u4")[..., 0]
        assert np.array_equal(pool[off:off + (w + 1) * (h + 1)].reshape(h + 1, w + 1), want)
        off += (w + 1) * (h + 1)
    assert off == pool.size
    meshes, tris = pk.table("meshes"), pk.table("tris")
    assert [int(m["n_tris"]) for m in meshes] == [sc.meshes[k].n_tris for k in sc.mesh_order] and tris.size == sum(m["n_tris"] for m in meshes)
    for k, d in zip(sc.mesh_order, meshes):
        m, tr = sc.meshes[k], tris[d["off"]:d["off"] + d["n_tris"]]
        assert np.array_equal(tr["v"].reshape(-1), m.verts.reshape(-1)) and np.array_equal(d["mn"], m.verts.reshape(-1, 3).min(axis=0))
        assert np.array_equal(tr["tex"], np.where(m.tri_tex >= 0, m.tri_tex + sc.mesh_tex_base[k], -1) if m.textures else np.full(m.n_tris, -1))
    # blob: header offsets, tiles, curves, static records, object words
    nt, nc, objs = mt.grid_w * mt.grid_h, f.n_curves, [f.objects[o] for o in range(f.n_objects)]
    stat = [o for o in objs if not o.dynamic and o.collidable]
    dyn = [(i, o) for i, o in enumerate(objs) if o.dynamic]
    blob = pk.table("blobs")
    hd = blob[:HDR_WORDS].view(HDR)[0]
    offs = np.cumsum([HDR_WORDS, nt, 8 * nc, 2 * nc, STATIC_WORDS * len(stat), OBJ_WORDS * len(objs)])
    assert [hd[k] for k in ("off_tiles", "off_curves", "off_heads", "off_static", "off_objs", "total_words")] == list(offs)
    assert s["n_maps"] == 1 and s["total_words"] == offs[-1] == blob.size and s["blob_off"][0] == 0
    assert (hd["grid_w"], hd["grid_h"], hd["n_curves"], hd["n_static"], hd["n_dyn"], hd["n_obj"], hd["tile_size"]) == \
        (mt.grid_w, mt.grid_h, nc, len(stat), len(dyn), len(objs), mt.tile_size)
    assert hd["n_lights"] == sum(o.light_freq > 0 for o in objs)
    tr = blob[offs[0]:offs[1]].view(TILEREC)
    for k, src in (("kind", mt.tile_kind), ("angle", mt.tile_angle), ("curve_cnt", mt.tile_curve_cnt), ("curve_off", mt.tile_curve_off), ("tex", mt.tile_tex)):
        assert np.array_equal(tr[k], src), k
    assert np.array_equal(tr["drivable"], (mt.tile_kind >= 1) & (mt.tile_kind <= 6))
    assert np.array_equal(blob[offs[1]:offs[2]].view("<f8"), np.asarray(mt.curves, np.float64).ravel())
    assert np.array_equal(blob[offs[2]:offs[3]].view("<f8"), np.asarray(mt.curve_heads, np.float64).ravel())
    st = blob[offs[3]:offs[4]].view("<f8").reshape(-1, STATIC_WORDS)
    for r, o in zip(st, stat):
        assert list(r) == list(o.corners) + list(o.norm) + [o.pos[0], o.pos[2], o.safety_radius]
    ow = blob[offs[4]:offs[5]].view("<f8").reshape(-1, OBJ_WORDS)
    slots = {i: k for k, (i, _) in enumerate(dyn)}
    for i, (r, o) in enumerate(zip(ow, objs)):
        assert list(r) == [o.pos[0], o.pos[2], o.spawn_clear, slots.get(i, -2 if o.optional else -1), o.light_freq, o.light_pattern & 1]
    di = pk.table("dyn")
    assert di.size == _ffi.MAX_DYNAMIC and not di[len(dyn):].tobytes().strip(b"\0")
    for d, (i, o) in zip(di, dyn):
        assert (d["cx"], d["cz"], d["angle"], d["safety_radius"], d["obj_index"], d["kind"]) == (o.pos[0], o.pos[2], o.angle, o.safety_radius, i, o.dynamic)
        assert list(d["corners"]) == list(o.corners) and list(d["norm"]) == list(o.norm)
        assert list(d["heading"]) == [math.cos(o.angle), -math.sin(o.angle)] and list(d["walk"]) == [o.walk_distance, o.vel, o.wait_time, o.wiggle]
    # raster view
    rm, ro = pk.table("rmaps")[0], pk.table("robjs")
    n_tris = sum(sc.meshes[sc.mesh_order[o.mesh_id]].n_tris for o in objs if o.mesh_id >= 0)
    assert rm["n_tris"] == n_tris == s["max_tris"] and (rm["grid_w"], rm["grid_h"], rm["n_obj"], rm["tile_off"], rm["obj_off"]) == (mt.grid_w, mt.grid_h, len(objs), 0, 0)
    assert rm["tile_size"] == np.float32(mt.tile_size) and rm["inv_tile_size"] == np.float32(1.0 / mt.tile_size)
    assert [int(v) for v in ro["mesh_id"]] == [o.mesh_id for o in objs] and [int(v) for v in ro["dyn_slot"]] == [slots.get(i, -1) for i in range(len(objs))]
    present, textured = mt.tile_kind != 0, mt.tile_tex >= 0
    want = np.where(textured, mt.tile_tex, 0xFF).astype(np.uint32) | ((mt.tile_angle & 3).astype(np.uint32) << 8) | (present.astype(np.uint32) << 15) | \
        (textured.astype(np.uint32) << 14)
    assert np.array_equal(pk.table("rtiles"), want)
    trecs = pk.table("trecs")
    assert s["n_tilerecs"] == nt == trecs.size and np.array_equal(trecs["flags"], present + 2 * (present & textured))
    for t in np.flatnonzero(present & textured):
        d = tex[mt.tile_tex[t]]
        want_rec = pk.tile_lds(int(d["w"]), int(d["h"]), int(d["off"]), int(mt.tile_angle[t]))
        assert trecs[t]["tex_off"] == want_rec["tex_off"] == d["off"] and np.array_equal(trecs[t]["m"], want_rec["m"])
    # quad tables
    S = sc.textures[0].shape[0]
    assert (s["tex_w"], s["tex_h"], s["qlog2"]) == (S, S, int(math.log2(S))) and s["q_per_m"] == np.float32(S / mt.tile_size)
    assert (s["grid_rows"], s["grid_cols"], s["grid_w"][0], s["grid_h"][0]) == (mt.grid_h + 2 * QRING, mt.grid_w + 2 * QRING, mt.grid_w, mt.grid_h)
    want, block = expected_quad_tiles(sc, S)
    qt, qb = pk.table("qtiles").reshape(-1, 2), pk.table("qblocks")
    assert s["n_qtiles"] == len(want) and np.array_equal(qt, want) and (rm["qt_off"], rm["qt_pitch"]) == (0, mt.grid_w + 2 * QRING)
    assert list(qb[:8]) == [0, 0, 0, 1 << 16, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0]
    for (tx, ang), b in block.items():
        first = ((b + 1) << 20 if S == 256 else 32 + b * S * S * 16) // 4
        d = tex[tx]
        assert np.array_equal(qb[first:first + S * S * 4], pk.quad_block(pool[d["off"]:], S, ang)), (tx, ang)
    assert qb.size == ((len(block) + 1) << 20 if S == 256 else 32 + len(block) * S * S * 16) // 4


def test_untextured_and_empty_tiles_and_the_ring(pk):
    """present but untextured tiles name record 1, empty tiles and the ring record 0; two maps share the blocks and follow each other in
    the tables"""
    assert pk.assets([distinct_texture(8), distinct_texture(8, seed=1)]) == 0
    kinds, texs = np.array([7, 0, 7, 7, 7, 7], np.uint8), np.array([0, 0, -1, 1, 0, 1], np.int16)
    angs = np.array([0, 0, 0, 3, 0, 7], np.uint8)
    assert pk.maps([make_map(3, 2, tile_kind=kinds, tile_tex=texs, tile_angle=angs), make_map(1, 1, tex=1, angle=3, tile_size=0.5)]) == 0, pk.err()
    s, rm = pk.scalars(), pk.table("rmaps")
    qt = pk.table("qtiles").reshape(-1, 2)
    g0 = qt[:11 * 10].reshape(10, 11, 2)
    blk = lambda b: [32 + b * 64 * 16, 63]
    assert g0[QRING:QRING + 2, QRING:QRING + 3].tolist() == [[blk(0), [0, 0], [16, 0]], [blk(1), blk(0), blk(1)]]
    ring = np.ones((10, 11), bool)
    ring[QRING:QRING + 2, QRING:QRING + 3] = False
    assert not g0[ring].any()
    g1 = qt[110:].reshape(9, 9, 2)
    assert g1[QRING, QRING].tolist() == blk(1) and np.count_nonzero(g1) == 2
    assert [tuple(r) for r in rm[["qt_off", "qt_pitch", "tile_off"]].tolist()] == [(0, 11, 0), (110, 9, 6)]
    assert (s["n_qtiles"], s["qlog2"], s["grid_rows"], s["grid_cols"], s["n_tilerecs"]) == (191, 3, 10, 11, 7) and s["q_per_m"] == np.float32(8 / 0.5)
    assert pk.table("qblocks").size == (32 + 2 * 64 * 16) // 4 and list(s["blob_off"][:2]) == [0, HDR_WORDS + 6]
    # without DTSIM_F_RENDER, or with tile textures that are not square: no quad records, so the generic raster
    assert pk.maps([make_map(3, 2)], render=False) == 0
    assert (pk.scalars()["qlog2"], pk.scalars()["n_qtiles"], pk.table("qblocks").size, pk.scalars()["tex_w"]) == (0, 0, 0, 8)
    assert pk.assets([distinct_texture(8, 4)]) == 0 and pk.maps([make_map(3, 2)]) == 0
    s = pk.scalars()
    assert (s["qlog2"], s["n_qtiles"], s["q_per_m"], s["tex_w"], s["tex_h"], pk.table("qtiles").size) == (0, 0, 0, 8, 4, 0)


# ---- camera table --------------------------------------------------------------------------------------------------------------
def test_lut_rounds_half_to_even_and_blacks_the_border(pk):
    W, H = 8, 6
    rng = np.random.default_rng(3)
    rx, ry = rng.uniform(-2, W + 2, (H, W)).astype(np.float32), rng.uniform(-2, H + 2, (H, W)).astype(np.float32)
    rx[0, :6] = [0.5, 1.5, 2.5, -0.5, 6.5, 7.5]                            # -> 0, 2, 2, -0 (inside), 6, 8 (outside)
    ry[0, :6] = 0
    ry[1, :5] = [0.5, 1.5, 4.5, 5.5, -0.5000001]                           # -> 0, 2, 4, 6 (outside), -1 (outside)
    rx[1, :5] = 3
    rx[2, :3], ry[2, :3] = [-1, W, 1e6], [1, 1, 1]
    pk.lib.st_lut(W, H, rx.ctypes.data_as(C.POINTER(C.c_float)), ry.ctypes.data_as(C.POINTER(C.c_float)))
    lut = pk.table("lut").reshape(H, W, 4)
    sx, sy = np.rint(rx.astype(np.float64)), np.rint(ry.astype(np.float64))
    ok = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
    assert ok[0, :6].tolist() == [True] * 5 + [False] and ok[1, :5].tolist() == [True, True, True, False, False] and not ok[2, :3].any()
    want = np.zeros((H, W, 4), np.float32)
    want[..., 0] = np.where(ok, (2.0 * (sx + 0.5)) / W - 1.0, 0)
    want[..., 1] = np.where(ok, 1.0 - (2.0 * (sy + 0.5)) / H, 0)
    want[..., 2] = ok
    assert np.array_equal(lut, want)
    pk.lib.st_lut(W, H, None, None)
    c, r = np.meshgrid(np.arange(W), np.arange(H))
    ident = np.stack([(2.0 * (c + 0.5)) / W - 1.0, 1.0 - (2.0 * (r + 0.5)) / H, np.ones((H, W)), np.zeros((H, W))], axis=-1).astype(np.float32)
    assert np.array_equal(pk.table("lut").reshape(H, W, 4), ident)


# ---- rejections ----------------------------------------------------------------------------------------------------------------
def _installed(pk):
    """a valid scene in the packers' outputs: three 8 x 8 textures + one 4 x 4, two meshes, one map with an object, segment tables"""
    texs = [distinct_texture(8, seed=i) for i in range(3)] + [distinct_texture(4)]
    assert pk.assets(texs, [tri_mesh(2, tex=1), tri_mesh(1)]) == 0
    assert pk.lib.st_segment(tex_array(texs), 4, np.arange(6, dtype=np.uint8).ctypes.data_as(C.POINTER(C.c_uint8)), 2) == 0
    assert pk.maps([make_map(2, 2, objects=[dict(mesh_id=1, collidable=1)])]) == 0
    return texs


def _rejected(pk, rc, code, msg):
    assert (rc, pk.err()) == (code, msg)


E_INVALID, E_LIMIT = _ffi.E_INVALID, _ffi.E_LIMIT


def test_every_rejection_of_the_asset_packers(pk):
    texs = _installed(pk)
    before = pk.snapshot()
    t8 = texs[0]
    cases = [
        (lambda: pk.assets([], n_textures=97), E_LIMIT, "n_textures 97 > 96"),
        (lambda: pk.assets([], n_textures=-1), E_LIMIT, "n_textures -1 > 96"),
        (lambda: pk.assets([], n_meshes=65), E_LIMIT, "n_meshes 65 > 64"),
        (lambda: pk.assets([t8, np.zeros((8, 12, 4), np.uint8)]), E_INVALID, "texture 1: size must be a power of two"),
        (lambda: pk.assets([None]), E_INVALID, "texture 0: size must be a power of two"),
        (lambda: pk.assets([t8], [tri_mesh(1), dict(n_tris=1, verts=t8.view(np.float32), normals=None, colors=None)]), E_INVALID, "mesh 1: null arrays"),
        (lambda: pk.assets([t8], [dict(n_tris=-1)]), E_INVALID, "mesh 0: null arrays"),
        (lambda: pk.assets([t8], [tri_mesh(3, tex=1)]), E_INVALID, "mesh 0 triangle 0: texture 1 not loaded"),
    ]
    rgb = np.zeros(6, np.uint8).ctypes.data_as(C.POINTER(C.c_uint8))
    seg = lambda ts, nt=4, mrgb=rgb, nm=2: pk.lib.st_segment(tex_array(ts) if ts is not None else None, nt, mrgb, nm)
    null_rgba = tex_array(texs)
    null_rgba[2].rgba = None
    cases += [
        (lambda: seg(texs[:3], 3), E_INVALID, "segment assets must mirror dtsim_set_assets (4 textures, 2 meshes), got 3 / 2"),
        (lambda: seg(texs, nm=1), E_INVALID, "segment assets must mirror dtsim_set_assets (4 textures, 2 meshes), got 4 / 1"),
        (lambda: seg(None), E_INVALID, "null argument"),
        (lambda: seg(texs, mrgb=None), E_INVALID, "null argument"),
        (lambda: seg(texs[:3] + [texs[0]]), E_INVALID, "segmented texture 3 is 8x8, the texture it replaces is 4x4"),
        (lambda: pk.lib.st_segment(null_rgba, 4, rgb, 2), E_INVALID, "texture 2: size must be a power of two"),
    ]
    for call, code, msg in cases:
        _rejected(pk, call(), code, msg)
        assert pk.snapshot() == before, msg


def test_every_rejection_of_the_map_packer(pk):
    _installed(pk)
    before = pk.snapshot()
    ok = make_map(2, 2)
    stat, dyn = dict(collidable=1), dict(dynamic=1)
    drv = dict(tile_kind=np.array([1, 7, 7, 7], np.uint8), tile_curve_off=np.array([0, -1, -1, -1], np.int16))
    one_of = lambda a, b: np.array([a, b, a, a], np.int16)
    cases = [
        (lambda: pk.lib.st_maps(None, 1, 1), E_INVALID, "null argument"),
        (lambda: pk.maps([ok], n=0), E_LIMIT, "n_maps 0 outside [1,32]"),
        (lambda: pk.maps([ok] * 33), E_LIMIT, "n_maps 33 outside [1,32]"),
        (lambda: pk.maps([ok, make_map(33, 32)]), E_LIMIT, "map 1: 1056 tiles > 1024"),
        (lambda: pk.maps([make_map(0, 4)]), E_LIMIT, "map 0: 0 tiles > 1024"),
        (lambda: pk.maps([make_map(2, 2, n_curves=1025)]), E_LIMIT, "map 0: n_curves 1025"),
        (lambda: pk.maps([make_map(2, 2, n_curves=-1)]), E_LIMIT, "map 0: n_curves -1"),
        (lambda: pk.maps([make_map(2, 2, objects=[stat] * 65)]), E_LIMIT, "map 0: n_objects 65 > 64"),
        (lambda: pk.maps([make_map(2, 2, tile_tex=None)]), E_INVALID, "map 0: null tile arrays / tile_size"),
        (lambda: pk.maps([make_map(2, 2, tile_size=0.0)]), E_INVALID, "map 0: null tile arrays / tile_size"),
        (lambda: pk.maps([make_map(2, 2, n_curves=2, curve_heads=None)]), E_INVALID, "map 0: null curves"),
        (lambda: pk.maps([make_map(2, 2, n_objects=1, null_objects=True)]), E_INVALID, "map 0: null objects"),
        (lambda: pk.maps([make_map(2, 2, objects=[stat] * 57)]), E_LIMIT, "map 0: 57 static collidables > 56"),
        (lambda: pk.maps([make_map(2, 2, objects=[dyn] * 9)]), E_LIMIT, "map 0: 9 dynamic objects > 8"),
        (lambda: pk.maps([make_map(2, 2, n_curves=1, **drv)]), E_INVALID, "map 0 tile 0: drivable tile without curves"),
        (lambda: pk.maps([make_map(2, 2, n_curves=1, tile_curve_cnt=np.array([2, 0, 0, 0], np.uint8), **drv)]), E_INVALID,
         "map 0 tile 0: drivable tile without curves"),
        (lambda: pk.maps([make_map(2, 2, tile_tex=one_of(0, 4))]), E_INVALID, "map 0 tile 1: texture 4 not loaded"),
        (lambda: pk.maps([ok, make_map(2, 2, tile_tex=one_of(1, 3))]), E_LIMIT, "map 1 tile 1: all tile textures must share one size (4x4 vs 8x8)"),
        (lambda: pk.maps([make_map(2, 2, objects=[stat, dict(mesh_id=2)])]), E_INVALID, "map 0 object 1: mesh 2 not loaded"),
        (lambda: pk.maps([make_map(2, 2, objects=[dict(light_freq=-3)])]), E_INVALID, "map 0 object 0: light_freq -3"),
        (lambda: pk.maps([make_map(2, 2, objects=[dict(mesh_id=0, light_freq=2, light_tris=1, light_tex=(C.c_int32 * 2)(0, 4))])]), E_INVALID,
         "map 0 object 0: light texture not loaded"),
        (lambda: pk.maps([make_map(32, 32)] * 8), E_LIMIT, "map tables 66048 B exceed the 60 KB LDS staging budget"),
        (lambda: pk.maps([make_map(32, 32), ok]), E_LIMIT, "1028 tiles over all maps exceed the 1024 LDS raster records"),
    ]
    for call, code, msg in cases:
        _rejected(pk, call(), code, msg)
        assert pk.snapshot() == before, msg


# ---- limits, under a sanitizer ---------------------------------------------------------------------------------------------------
LIMITS_PROGRAM = r"""
#include "scene_tables.h"
#include <cstdlib>
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %d: %s (%s)\n", __LINE__, #c, err.c_str()); return 1; } } while (0)
struct Map {
  std::vector<uint8_t> kind, angle, cnt;
  std::vector<int16_t> tex, coff;
  std::vector<double> curves, heads;
  std::vector<dtsim_object> objs;
  dtsim_map m{};
  Map(int w, int h, int tx = 0, int n_static = 0, int n_dyn = 0, int n_plain = 0, int n_curves = 0)
      : kind(w * h, 7), angle(w * h), cnt(w * h, 0), tex(w * h, (int16_t)tx), coff(w * h, -1), curves(8 * n_curves + 1, 0.5), heads(2 * n_curves + 1, 1.0) {
    for (int t = 0; t < w * h; ++t) angle[t] = (uint8_t)(t % 2 ? 3 : 0);
    dtsim_object o{};
    o.mesh_id = -1;
    for (int i = 0; i < n_static; ++i) { o.collidable = 1; o.dynamic = 0; objs.push_back(o); }
    for (int i = 0; i < n_dyn; ++i) { o.collidable = 1; o.dynamic = 1 + i % 3; objs.push_back(o); }
    for (int i = 0; i < n_plain; ++i) { o.collidable = 0; o.dynamic = 0; objs.push_back(o); }
    m.grid_w = w; m.grid_h = h; m.tile_size = 0.585;
    m.tile_kind = kind.data(); m.tile_angle = angle.data(); m.tile_tex = tex.data(); m.tile_curve_off = coff.data(); m.tile_curve_cnt = cnt.data();
    m.n_curves = n_curves; m.curves = curves.data(); m.curve_heads = heads.data();
    m.n_objects = (int)objs.size(); m.objects = objs.data();
  }
};
int main() {
  std::string err;
  AssetTables A, none;
  MapTables M;
  std::vector<std::vector<uint8_t>> px;
  std::vector<dtsim_texture> tx;
  auto add = [&](int w, int h) { px.emplace_back((size_t)w * h * 4); for (size_t i = 0; i < px.back().size(); ++i) px.back()[i] = (uint8_t)(i * 7 + w); tx.push_back({w, h, nullptr}); };
  auto fix = [&] { for (size_t i = 0; i < tx.size(); ++i) tx[i].rgba = px[i].data(); };
  // zero textures, zero meshes, zero objects
  CHECK(dt_pack_assets(none, err, nullptr, 0, nullptr, 0) == DTSIM_OK && none.pool.empty() && none.tris.empty());
  { Map a(3, 2, -1); CHECK(dt_pack_maps(M, err, &a.m, 1, none, true) == DTSIM_OK && M.qlog2 == 0 && M.qblocks.empty() && M.robjs.empty() && M.tex_w == 1 && M.trecs.size() == 6); }
  // DTSIM_MAX_TEXTURES textures of S = 2 and DTSIM_MAX_MESHES meshes; one more of either is refused
  for (int i = 0; i < DTSIM_MAX_TEXTURES + 1; ++i) add(2, 2);
  fix();
  std::vector<float> v(9 * 4, 0.25f);
  std::vector<int32_t> tt(4, DTSIM_MAX_TEXTURES - 1);
  std::vector<dtsim_mesh> ms(DTSIM_MAX_MESHES + 1, dtsim_mesh{4, v.data(), v.data(), v.data(), v.data(), tt.data()});
  ms[1].n_tris = 0;
  CHECK(dt_pack_assets(A, err, tx.data(), DTSIM_MAX_TEXTURES, ms.data(), DTSIM_MAX_MESHES) == DTSIM_OK && A.tex.size() == DTSIM_MAX_TEXTURES && A.tris.size() == 4 * (DTSIM_MAX_MESHES - 1));
  CHECK(dt_pack_assets(A, err, tx.data(), DTSIM_MAX_TEXTURES + 1, ms.data(), 1) == DTSIM_E_LIMIT);
  CHECK(dt_pack_assets(A, err, tx.data(), 1, ms.data(), DTSIM_MAX_MESHES + 1) == DTSIM_E_LIMIT);
  CHECK(A.tex.size() == DTSIM_MAX_TEXTURES);
  {  // S = 2; DTSIM_MAX_MAPS maps; the full object set; DTSIM_MAX_CURVES curves
    std::vector<Map> maps;
    std::vector<dtsim_map> mm;
    maps.reserve(DTSIM_MAX_MAPS + 1);
    maps.emplace_back(2, 1, DTSIM_MAX_TEXTURES - 1, DTSIM_MAX_STATIC, DTSIM_MAX_DYNAMIC);
    for (auto& o : maps[0].objs) o.mesh_id = DTSIM_MAX_MESHES - 1;
    maps.emplace_back(1, 1, 0, 0, 0, 0, 200);
    for (int i = 2; i < DTSIM_MAX_MAPS + 1; ++i) maps.emplace_back(1, 2, i);
    for (auto& a : maps) mm.push_back(a.m);
    CHECK(dt_pack_maps(M, err, mm.data(), DTSIM_MAX_MAPS, A, true) == DTSIM_OK);
    CHECK(M.qlog2 == 1 && M.M.n_maps == DTSIM_MAX_MAPS && M.robjs.size() == DTSIM_MAX_OBJECTS && M.max_tris == 4 * DTSIM_MAX_OBJECTS && M.grid_rows == 2 + 2 * DT_QRING);
    CHECK(M.qblocks.size() == 8 + (size_t)(2 + 1 + 2 * (DTSIM_MAX_MAPS - 2)) * 4 * 4);
    CHECK(dt_pack_maps(M, err, mm.data(), DTSIM_MAX_MAPS + 1, A, true) == DTSIM_E_LIMIT && M.M.n_maps == DTSIM_MAX_MAPS);
    Map s57(1, 1, 0, DTSIM_MAX_STATIC + 1), d9(1, 1, 0, 0, DTSIM_MAX_DYNAMIC + 1), o65(1, 1, 0, 0, 0, DTSIM_MAX_OBJECTS + 1), o64(1, 1, 0, 0, 0, DTSIM_MAX_OBJECTS);
    CHECK(dt_pack_maps(M, err, &s57.m, 1, A, true) == DTSIM_E_LIMIT && dt_pack_maps(M, err, &d9.m, 1, A, true) == DTSIM_E_LIMIT);
    CHECK(dt_pack_maps(M, err, &o65.m, 1, A, true) == DTSIM_E_LIMIT && M.M.n_maps == DTSIM_MAX_MAPS);
    CHECK(dt_pack_maps(M, err, &o64.m, 1, A, true) == DTSIM_OK && M.robjs.size() == DTSIM_MAX_OBJECTS);
    Map c(1, 1, 0, 0, 0, 0, DTSIM_MAX_CURVES), c1(1, 1, 0, 0, 0, 0, DTSIM_MAX_CURVES + 1);
    CHECK(dt_pack_maps(M, err, &c1.m, 1, A, true) == DTSIM_E_LIMIT);
    CHECK(dt_pack_maps(M, err, &c.m, 1, A, true) == DTSIM_E_LIMIT);     // 10 * 1024 words: over the 60 KB staging budget
    Map c2(1, 1, 0, 0, 0, 0, 700);
    CHECK(dt_pack_maps(M, err, &c2.m, 1, A, true) == DTSIM_OK && M.M.total_words == (int)MAPHDR_WORDS + 1 + 7000);
  }
  {  // a 32 x 32 grid (DTSIM_MAX_TILES tiles = DTSIM_LDS_TILES records); one row or one map more is refused
    Map g(32, 32), g1(32, 33), one(1, 1);
    CHECK(dt_pack_maps(M, err, &g.m, 1, A, true) == DTSIM_OK && M.trecs.size() == DTSIM_LDS_TILES && M.n_qtiles == 40 * 40 && M.grid_cols == 40);
    CHECK(dt_pack_maps(M, err, &g1.m, 1, A, true) == DTSIM_E_LIMIT);
    dtsim_map two[2] = {g.m, one.m};
    CHECK(dt_pack_maps(M, err, two, 2, A, true) == DTSIM_E_LIMIT && M.trecs.size() == DTSIM_LDS_TILES);
  }
  // tile textures that are not square: no quad records; mixed sizes over the maps are refused
  px.clear(); tx.clear();
  add(4, 8); add(8, 4); add(256, 256); add(256, 256);
  fix();
  CHECK(dt_pack_assets(A, err, tx.data(), 4, nullptr, 0) == DTSIM_OK);
  { Map a(3, 3, 0); CHECK(dt_pack_maps(M, err, &a.m, 1, A, true) == DTSIM_OK && M.qlog2 == 0 && M.tex_w == 4 && M.tex_h == 8 && M.qtiles.empty()); }
  { Map a(3, 3, 0), b(2, 2, 1); dtsim_map two[2] = {a.m, b.m}; CHECK(dt_pack_maps(M, err, two, 2, A, true) == DTSIM_E_LIMIT && M.tex_h == 8); }
  {  // S = 256: two (texture, angle) pairs per texture here -- 1 MB blocks behind the block of the two special records
    Map a(2, 1, 2), b(1, 2, 3);
    dtsim_map two[2] = {a.m, b.m};
    CHECK(dt_pack_maps(M, err, two, 2, A, true) == DTSIM_OK && M.qlog2 == 8 && M.qblocks.size() == (size_t)5 << 18);
    CHECK(M.qtiles[2 * (4 * 10 + 4)] == 1u << 20 && M.qtiles[2 * (4 * 10 + 5)] == 2u << 20 && M.qtiles[2 * (4 * 10 + 4) + 1] == 0xFFFFFu);
    CHECK(dt_pack_maps(M, err, &a.m, 1, A, true) == DTSIM_OK && M.qblocks.size() == (size_t)3 << 18);
  }
  std::vector<float> lut;
  dt_pack_lut(7, 5, nullptr, nullptr, lut);
  CHECK(lut.size() == 7 * 5 * 4);
  return 0;
}
"""


def test_limits_under_sanitizers(tmp_path):
    """every limit of the packers and each limit plus one, in a program of its own built with AddressSanitizer and
    UndefinedBehaviorSanitizer: it exits clean"""
    (tmp_path / "limits.cpp").write_text(LIMITS_PROGRAM)
    exe = tmp_path / "limits"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                           str(tmp_path / "limits.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
