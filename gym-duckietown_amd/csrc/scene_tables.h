// scene_tables.h -- the scene tables of a handle, packed on the host: the layouts the kernels read (map blobs, raster maps, tile
// records, object instances, quad-record blocks, the texel pool, meshes) and the packers behind dtsim_set_assets,
// dtsim_set_segment_assets, dtsim_set_maps and dtsim_set_distortion_lut.  Plain C++17 without a HIP header, so a host program can
// include it (tests/test_scene_tables_host.py drives the packers with g++).  A packer returns the error code and fills `err`; on an
// error its output object is left as it was.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dtsim.h"

// ---- packed map blob --------------------------------------------------------
struct MapHdr {            // 8-byte words; offsets are in words from the blob start
  int32_t grid_w, grid_h;
  int32_t n_curves, n_static;
  int32_t n_dyn, n_obj;
  int32_t off_tiles, off_curves;   // tiles: 1 word each; curves: 8 words each (P0x,P0z..P3x,P3z)
  int32_t off_heads, off_static;   // heads: 2 words per curve; static: 15 words each
  int32_t off_objs, total_words;   // objs: OBJ_WORDS words each
  int32_t n_lights, pad_l;         // traffic lights among the objects (0: k_step skips the light clock)
  double tile_size;
};
static_assert(sizeof(MapHdr) % 8 == 0, "MapHdr must be whole words");
#define MAPHDR_WORDS (sizeof(MapHdr) / 8)

struct TileRec {           // one 8-byte word
  uint8_t kind, angle, drivable, curve_cnt;
  int16_t curve_off, tex;
};
static_assert(sizeof(TileRec) == 8, "TileRec is one word");

// static collidable record: corners[8] norms[4] center[2] radius[1]
#define STATIC_WORDS 15
#define OBJ_WORDS 6      // x, z, spawn_clear, dyn_slot (-1 static, -2 optional static), light_freq, light_pattern0

struct DynInit {           // per map, per dynamic slot: initial DuckieObj state
  double cx, cz, corners[8], norm[4], heading_x, heading_z, angle, safety_radius;
  double walk_distance, vel, wait_time, wiggle;   // DuckieObj; DuckiebotObj: follow_dist, velocity, gain, trim
  int32_t obj_index, kind;                        // kind: 1 DuckieObj, 2 DuckiebotObj, 3 CheckerboardObj
};

// All maps, device side
struct MapSet {
  int32_t n_maps;
  int32_t blob_off[DTSIM_MAX_MAPS];   // word offset of each map blob inside `blobs`
  int32_t total_words;
  const uint64_t* blobs;
  const DynInit* dyn;                 // [n_maps][DTSIM_MAX_DYNAMIC]
};

// ---- raster -----------------------------------------------------------------
struct TexDev { int32_t w, h, off, pad; };   // off: texel offset into the texel pool; storage is (h+1) x (w+1), padded for REPEAT
struct MeshDev { int32_t n_tris, off; float mn[3], mx[3]; };   // off: triangle offset into the pool; model-space AABB
struct TriDev { float v[3][3]; float n[3][3]; float c[3][3]; float uv[3][2]; int32_t tex, pad; };   // tex: texture index or -1

struct RenderMapDev {       // per map, raster view of the grid + objects
  int32_t grid_w, grid_h, n_obj, n_tris;   // n_tris: total mesh triangles of the map's objects
  float tile_size, inv_tile_size;
  int32_t tile_off;         // offset into tile table (uint32 per tile: tex | angle<<8 | present<<15)
  int32_t obj_off;          // offset into object-instance table
  int32_t qt_off, qt_pitch; // quad-texture tile table of the map: first entry, row pitch (grid_w + 2*DT_QRING)
};

struct ObjInstDev {         // static render instance (dynamic ones are patched per env)
  float x, y, z, scale, yrot_deg;
  int32_t mesh_id, dyn_slot;
  int32_t light_tris, light_tex0, light_tex1;   // traffic light: first `light_tris` triangles take texture 0 / 1 by pattern
  int32_t pad[2];
};
static_assert(sizeof(ObjInstDev) == 48, "ObjInstDev is 48 bytes");

// LDS-staged raster tile record: texel base of the (padded) texture, flags (bit0 present,
// bit1 textured), and the affine map tile-fraction (fx, fz) -> texel coordinates
// x = mxx*fx + mxz*fz + ox, y = myx*fx + myz*fz + oy encoding glRotatef(angle*90+180)
// about y, uv = (pu, 1-pv) (simulator.py:394-401,1872-1873) and the GL_LINEAR half-texel shift.
struct alignas(16) TileLds { uint32_t tex_off, flags; float mxx, mxz, ox, myx, myz, oy; };
static_assert(sizeof(TileLds) == 32, "TileLds is 32 bytes");
#define DTSIM_LDS_TILES 1024   // raster tile records of all maps together (32 KB of LDS)

// Quad-layout tile textures for the one-ray fast path (render.hip k_raster_q): per (texture, tile angle) pair one
// block of S x S records of 16 bytes, record (x0, z0) = the four GL_LINEAR taps of the pre-rotated tile texture around
// quad cell (x0, z0) as channel-planar bytes {R00 R10 R01 R11}, {G..}, {B..} + a meta dword (see DT_QMETA_*).
#define DT_QRING 4                           // ring of off-grid cells around each map's tile table, in tiles
// The pool starts with two single records every cell of a non-textured tile maps to: record 0 = off the grid (ground
// quad / sky), record 1 = present but untextured tile (exact path).
// DT_QMETA -- meta dword: low 16 bits = cells to the nearest tile boundary if the cell belongs to a textured tile (else 0),
// high 16 bits = 1 if the cell is off the grid (else 0); 0 / 0 = always the exact path.

inline int dt_scene_fail(std::string& err, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  err = buf;
  return code;
}

// ---- assets -------------------------------------------------------------------------------------------------------------------
struct AssetTables {
  std::vector<uint32_t> pool;     // the RGBA8 texel pool (dt_pack_maps builds the quad blocks from it)
  std::vector<TexDev> tex;
  std::vector<MeshDev> meshes;
  std::vector<TriDev> tris;       // every mesh's triangles, MeshDev.off apart
};

// textures appended to one RGBA8 pool: padded (h+1) x (w+1) storage so that GL_REPEAT bilinear fetches never wrap
inline int dt_pack_texels(std::vector<uint32_t>& pool, std::vector<TexDev>* descs, std::string& err, const dtsim_texture* textures, int n_textures) {
  for (int t = 0; t < n_textures; ++t) {
    const dtsim_texture& tx = textures[t];
    if (tx.width <= 0 || tx.height <= 0 || (tx.width & (tx.width - 1)) || (tx.height & (tx.height - 1)) || !tx.rgba)
      return dt_scene_fail(err, DTSIM_E_INVALID, "texture %d: size must be a power of two", t);
    TexDev d{tx.width, tx.height, (int32_t)pool.size(), 0};
    const int pw = tx.width + 1;
    pool.resize(pool.size() + (size_t)pw * (tx.height + 1));
    uint32_t* dst = pool.data() + d.off;
    for (int y = 0; y <= tx.height; ++y)
      for (int x = 0; x <= tx.width; ++x) {
        const uint8_t* s = tx.rgba + ((size_t)(y % tx.height) * tx.width + (x % tx.width)) * 4;
        dst[(size_t)y * pw + x] = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)s[3] << 24);
      }
    if (descs) descs->push_back(d);
  }
  return DTSIM_OK;
}

inline int dt_pack_assets(AssetTables& out, std::string& err, const dtsim_texture* textures, int n_textures, const dtsim_mesh* meshes, int n_meshes) {
  if (n_textures < 0 || n_textures > DTSIM_MAX_TEXTURES) return dt_scene_fail(err, DTSIM_E_LIMIT, "n_textures %d > %d", n_textures, DTSIM_MAX_TEXTURES);
  if (n_meshes < 0 || n_meshes > DTSIM_MAX_MESHES) return dt_scene_fail(err, DTSIM_E_LIMIT, "n_meshes %d > %d", n_meshes, DTSIM_MAX_MESHES);
  AssetTables T;
  if (int rc = dt_pack_texels(T.pool, &T.tex, err, textures, n_textures)) return rc;
  for (int m = 0; m < n_meshes; ++m) {
    const dtsim_mesh& ms = meshes[m];
    if (ms.n_tris < 0 || (ms.n_tris > 0 && (!ms.verts || !ms.normals || !ms.colors)))
      return dt_scene_fail(err, DTSIM_E_INVALID, "mesh %d: null arrays", m);
    MeshDev d{};
    d.n_tris = ms.n_tris; d.off = (int32_t)T.tris.size();
    for (int k = 0; k < 3; ++k) { d.mn[k] = 1e30f; d.mx[k] = -1e30f; }
    for (int t = 0; t < ms.n_tris * 3; ++t)
      for (int k = 0; k < 3; ++k) { d.mn[k] = std::min(d.mn[k], ms.verts[t * 3 + k]); d.mx[k] = std::max(d.mx[k], ms.verts[t * 3 + k]); }
    for (int t = 0; t < ms.n_tris; ++t) {
      TriDev td;
      memcpy(td.v, ms.verts + (size_t)t * 9, 36);
      memcpy(td.n, ms.normals + (size_t)t * 9, 36);
      memcpy(td.c, ms.colors + (size_t)t * 9, 36);
      if (ms.uvs) memcpy(td.uv, ms.uvs + (size_t)t * 6, 24); else memset(td.uv, 0, 24);
      td.tex = (ms.uvs && ms.tri_tex) ? ms.tri_tex[t] : -1; td.pad = 0;
      if (td.tex >= n_textures) return dt_scene_fail(err, DTSIM_E_INVALID, "mesh %d triangle %d: texture %d not loaded", m, t, td.tex);
      if (td.tex < 0) td.tex = -1;
      T.tris.push_back(td);
    }
    T.meshes.push_back(d);
  }
  out = std::move(T);
  return DTSIM_OK;
}

// dtsim_set_segment_assets: the segmented versions of A's textures in A.pool's layout, and [max(n_meshes, 1)][4] flat mesh colours
inline int dt_pack_segment_texels(std::vector<uint32_t>& pool, std::vector<uint8_t>& mesh_rgbx, std::string& err, const dtsim_texture* textures,
                                  int n_textures, const uint8_t* mesh_rgb, int n_meshes, const AssetTables& A) {
  const int n_tex = (int)A.tex.size(), n_mesh = (int)A.meshes.size();
  if (n_textures != n_tex || n_meshes != n_mesh)
    return dt_scene_fail(err, DTSIM_E_INVALID, "segment assets must mirror dtsim_set_assets (%d textures, %d meshes), got %d / %d", n_tex, n_mesh,
                         n_textures, n_meshes);
  if ((n_textures > 0 && !textures) || (n_meshes > 0 && !mesh_rgb)) return dt_scene_fail(err, DTSIM_E_INVALID, "null argument");
  for (int t = 0; t < n_textures; ++t)
    if (textures[t].width != A.tex[t].w || textures[t].height != A.tex[t].h)
      return dt_scene_fail(err, DTSIM_E_INVALID, "segmented texture %d is %dx%d, the texture it replaces is %dx%d", t, textures[t].width,
                           textures[t].height, A.tex[t].w, A.tex[t].h);
  std::vector<uint32_t> p;
  if (int rc = dt_pack_texels(p, nullptr, err, textures, n_textures)) return rc;
  std::vector<uint8_t> rgbx((size_t)std::max(n_meshes, 1) * 4, 0);
  for (int m = 0; m < n_meshes; ++m) { rgbx[m * 4] = mesh_rgb[m * 3]; rgbx[m * 4 + 1] = mesh_rgb[m * 3 + 1]; rgbx[m * 4 + 2] = mesh_rgb[m * 3 + 2]; }
  pool = std::move(p); mesh_rgbx = std::move(rgbx);
  return DTSIM_OK;
}

// dtsim_set_label_assets: the class of every texel in A.pool's layout, one byte per texel (texture t at A.tex[t].off, padded to
// (h+1) x (w+1) by GL_REPEAT as the texels are, so that a tile record's tex_off addresses both pools), and [max(n_meshes, 1)] mesh classes.
// texel_class[t]: [h][w] bytes of texture t, in its row order.
inline int dt_pack_label_tables(std::vector<uint8_t>& pool, std::vector<uint8_t>& mesh_tab, std::string& err, const uint8_t* const* texel_class,
                                int n_textures, const uint8_t* mesh_class, int n_meshes, const AssetTables& A) {
  const int n_tex = (int)A.tex.size(), n_mesh = (int)A.meshes.size();
  if (n_textures != n_tex || n_meshes != n_mesh)
    return dt_scene_fail(err, DTSIM_E_INVALID, "label assets must mirror dtsim_set_assets (%d textures, %d meshes), got %d / %d", n_tex, n_mesh,
                         n_textures, n_meshes);
  if ((n_textures > 0 && !texel_class) || (n_meshes > 0 && !mesh_class)) return dt_scene_fail(err, DTSIM_E_INVALID, "null argument");
  for (int t = 0; t < n_textures; ++t)
    if (!texel_class[t]) return dt_scene_fail(err, DTSIM_E_INVALID, "texel classes of texture %d: null", t);
  std::vector<uint8_t> p(A.pool.size(), 0);
  for (int t = 0; t < n_textures; ++t) {
    const TexDev& d = A.tex[t];
    const size_t pw = (size_t)d.w + 1;
    if ((size_t)d.off + pw * ((size_t)d.h + 1) > p.size()) return dt_scene_fail(err, DTSIM_E_INVALID, "texture %d lies outside the texel pool", t);
    uint8_t* dst = p.data() + d.off;
    for (int y = 0; y <= d.h; ++y)
      for (int x = 0; x <= d.w; ++x) dst[(size_t)y * pw + x] = texel_class[t][(size_t)(y % d.h) * d.w + (x % d.w)];
  }
  std::vector<uint8_t> mt((size_t)std::max(n_meshes, 1), 0);
  for (int m = 0; m < n_meshes; ++m) mt[m] = mesh_class[m];
  pool = std::move(p); mesh_tab = std::move(mt);
  return DTSIM_OK;
}

// ---- maps ---------------------------------------------------------------------------------------------------------------------
// How a tile's texture lies in the tile frame: glRotatef(angle*90+180) about y with uv = (pu, 1-pv) (simulator.py:394-401,1872-1873)
// gives, at tile fraction (fx, fz), u = {1-fx, fz, fx, 1-fz}[angle] and v = {fz, fx, 1-fz, 1-fx}[angle] -- u takes fz instead of fx
// (and v fx instead of fz) when swp, and runs backwards when flip_u (v: flip_v).  TileLds and the quad blocks both derive from this.
struct TileOrient { bool swp, flip_u, flip_v; };
inline TileOrient dt_tile_orient(int ang) {
  ang &= 3;
  return {(ang & 1) != 0, ang == 0 || ang == 3, ang == 2 || ang == 3};
}

// the tile record of a present, textured tile: x = u*TW - 0.5, y = v*TH - 0.5 (the GL_LINEAR half-texel shift)
inline void dt_tile_lds_map(TileLds& tr, const TexDev& td, int ang) {
  const TileOrient o = dt_tile_orient(ang);
  const float TW = (float)td.w, TH = (float)td.h;
  tr.tex_off = (uint32_t)td.off;
  tr.flags |= 2u;
  const float mu = o.flip_u ? -TW : TW, mv = o.flip_v ? -TH : TH;
  tr.mxx = o.swp ? 0.f : mu; tr.mxz = o.swp ? mu : 0.f; tr.ox = o.flip_u ? TW - 0.5f : -0.5f;
  tr.myx = o.swp ? mv : 0.f; tr.myz = o.swp ? 0.f : mv; tr.oy = o.flip_v ? TH - 0.5f : -0.5f;
}

// One quad block (S x S records of 16 B) of a tile texture pre-rotated by the tile angle (render.hip k_raster_q), appended to `out`.
// Cell (x0, z0) covers the padded-quad coordinates [x0, x0+1) x [z0, z0+1) of the tile, i.e. the GL_LINEAR taps
// P[z0-1][x0-1], P[z0-1][x0], P[z0][x0-1], P[z0][x0] (GL_REPEAT wrap) of the tile-frame image P with
// P[zz][xx] = T[y][x], (x, y) the texel the tile-local point ((xx+.5)/S, (zz+.5)/S) maps to under dt_tile_orient(ang).
// `pool` holds T padded to (S+1) x (S+1).  Meta dword: cells to the nearest tile boundary (DT_QMETA).
inline void dt_pack_quad_block(std::vector<uint32_t>& out, const uint32_t* pool, int S, int ang) {
  const size_t base = out.size();
  out.resize(base + (size_t)S * S * 4);
  const TileOrient o = dt_tile_orient(ang);
  auto texel = [&](int xx, int zz) -> uint32_t {
    xx &= S - 1; zz &= S - 1;
    const int a = o.swp ? zz : xx, b = o.swp ? xx : zz;
    const int x = o.flip_u ? S - 1 - a : a, y = o.flip_v ? S - 1 - b : b;
    return pool[(size_t)y * (S + 1) + x];
  };
  for (int z0 = 0; z0 < S; ++z0)
    for (int x0 = 0; x0 < S; ++x0) {
      const uint32_t t00 = texel(x0 - 1, z0 - 1), t10 = texel(x0, z0 - 1), t01 = texel(x0 - 1, z0), t11 = texel(x0, z0);
      // S = 256: 4 x 2 cells per 128-byte line -- record number (x0 >> 2) << 10 | z0 << 2 | (x0 & 3) (raster_common.h, q8_rec256: a 32 x 2 pixel slot of the
      // raster touches ~ 15 % fewer lines than with the rows of the texture laid end to end); other sizes: row-major
      const size_t rec = (S == 256) ? ((size_t)(x0 >> 2) << 10) | ((size_t)z0 << 2) | (size_t)(x0 & 3) : (size_t)z0 * S + x0;
      uint32_t* q = &out[base + rec * 4];
      for (int c = 0; c < 3; ++c)
        q[c] = ((t00 >> (8 * c)) & 255u) | (((t10 >> (8 * c)) & 255u) << 8) | (((t01 >> (8 * c)) & 255u) << 16) | (((t11 >> (8 * c)) & 255u) << 24);
      q[3] = (uint32_t)std::min(std::min(std::min(x0, S - x0), std::min(z0, S - z0)), 0xFFFF);
    }
}

// The collision rectangles of the maps' objects as the host packed them (dtsim_object.corners: four (x, z) corners in order, float64), maps
// concatenated in the order of MapTables.robjs -- object o of map m at [RenderMapDev.obj_off + o][8] -- for dtsim_bev (render_views.hip k_bev),
// which draws a static object's footprint from here and a dynamic one's (ObjInstDev.dyn_slot >= 0) from the env's SimArrays::ob_corners.
// The maps are dt_pack_maps' arguments, already checked by it (object counts within DTSIM_MAX_OBJECTS, non-null lists).
inline int dt_pack_object_corners(std::vector<double>& out, std::string& err, const dtsim_map* maps, int n_maps) {
  if (!maps || n_maps <= 0) return dt_scene_fail(err, DTSIM_E_INVALID, "null argument");
  std::vector<double> t;
  for (int mi = 0; mi < n_maps; ++mi) {
    const dtsim_map& mp = maps[mi];
    if (mp.n_objects < 0 || mp.n_objects > DTSIM_MAX_OBJECTS || (mp.n_objects > 0 && !mp.objects))
      return dt_scene_fail(err, DTSIM_E_INVALID, "map %d: object list", mi);
    for (int o = 0; o < mp.n_objects; ++o) t.insert(t.end(), mp.objects[o].corners, mp.objects[o].corners + 8);
  }
  out = std::move(t);
  return DTSIM_OK;
}

// what a handle keeps of the packed maps besides the tables themselves
struct MapScalars {
  MapSet M{};                                  // blob offsets; blobs / dyn are the owner's device copies (null in MapTables)
  int grid_w[DTSIM_MAX_MAPS] = {0}, grid_h[DTSIM_MAX_MAPS] = {0};
  int grid_rows = 0, grid_cols = 0;            // the largest padded tile grid of the maps (DT_QRING ring included)
  int n_tilerecs = 0, tex_w = 1, tex_h = 1;    // the one size of all tile textures (1 x 1: no textured tile)
  int n_qtiles = 0, qlog2 = 0;                 // qlog2 = 0: no quad records, so the generic raster
  float q_per_m = 0.f;
  int max_tris = 0;                            // most mesh triangles of any map's objects
};

struct MapTables : MapScalars {
  std::vector<uint64_t> blobs;                 // MapHdr | tiles | curves | heads | static | objs per map (M.blob_off)
  std::vector<DynInit> dyn;                    // [n_maps][DTSIM_MAX_DYNAMIC]
  std::vector<RenderMapDev> rmaps;
  std::vector<uint32_t> rtiles;                // tex | angle << 8 | textured << 14 | present << 15 per tile
  std::vector<TileLds> trecs;
  std::vector<ObjInstDev> robjs;
  std::vector<uint32_t> qblocks, qtiles;       // quad records (4 dwords each); [n_qtiles][2] block offset, record mask
  std::vector<double> ocorners;                // dt_pack_object_corners: [robjs.size()][8]
};

// render: the handle's DTSIM_F_RENDER, without which no quad tables are built
inline int dt_pack_maps(MapTables& out, std::string& err, const dtsim_map* maps, int n_maps, const AssetTables& A, bool render) {
  if (!maps) return dt_scene_fail(err, DTSIM_E_INVALID, "null argument");
  if (n_maps <= 0 || n_maps > DTSIM_MAX_MAPS) return dt_scene_fail(err, DTSIM_E_LIMIT, "n_maps %d outside [1,%d]", n_maps, DTSIM_MAX_MAPS);
  const int n_tex = (int)A.tex.size(), n_meshes = (int)A.meshes.size();
  MapTables T;
  T.dyn.resize((size_t)n_maps * DTSIM_MAX_DYNAMIC);
  memset(T.dyn.data(), 0, T.dyn.size() * sizeof(DynInit));
  T.rmaps.resize(n_maps);
  int tex_w = 0, tex_h = 0;
  T.M.n_maps = n_maps;
  for (int mi = 0; mi < n_maps; ++mi) {
    const dtsim_map& mp = maps[mi];
    const int nt = mp.grid_w * mp.grid_h;
    if (mp.grid_w <= 0 || mp.grid_h <= 0 || nt > DTSIM_MAX_TILES) return dt_scene_fail(err, DTSIM_E_LIMIT, "map %d: %d tiles > %d", mi, nt, DTSIM_MAX_TILES);
    if (mp.n_curves < 0 || mp.n_curves > DTSIM_MAX_CURVES) return dt_scene_fail(err, DTSIM_E_LIMIT, "map %d: n_curves %d", mi, mp.n_curves);
    if (mp.n_objects < 0 || mp.n_objects > DTSIM_MAX_OBJECTS) return dt_scene_fail(err, DTSIM_E_LIMIT, "map %d: n_objects %d > %d", mi, mp.n_objects, DTSIM_MAX_OBJECTS);
    if (!mp.tile_kind || !mp.tile_angle || !mp.tile_tex || !mp.tile_curve_off || !mp.tile_curve_cnt || !(mp.tile_size > 0))
      return dt_scene_fail(err, DTSIM_E_INVALID, "map %d: null tile arrays / tile_size", mi);
    if (mp.n_curves > 0 && (!mp.curves || !mp.curve_heads)) return dt_scene_fail(err, DTSIM_E_INVALID, "map %d: null curves", mi);
    if (mp.n_objects > 0 && !mp.objects) return dt_scene_fail(err, DTSIM_E_INVALID, "map %d: null objects", mi);
    int n_static = 0, n_dyn = 0;
    for (int o = 0; o < mp.n_objects; ++o) {
      if (mp.objects[o].dynamic) ++n_dyn;
      else if (mp.objects[o].collidable) ++n_static;
    }
    if (n_static > DTSIM_MAX_STATIC) return dt_scene_fail(err, DTSIM_E_LIMIT, "map %d: %d static collidables > %d", mi, n_static, DTSIM_MAX_STATIC);
    if (n_dyn > DTSIM_MAX_DYNAMIC) return dt_scene_fail(err, DTSIM_E_LIMIT, "map %d: %d dynamic objects > %d", mi, n_dyn, DTSIM_MAX_DYNAMIC);
    MapHdr hd{};
    hd.grid_w = mp.grid_w; hd.grid_h = mp.grid_h; hd.n_curves = mp.n_curves; hd.n_static = n_static;
    hd.n_lights = 0;
    for (int o = 0; o < mp.n_objects; ++o) hd.n_lights += mp.objects[o].light_freq > 0 ? 1 : 0;
    hd.n_dyn = n_dyn; hd.n_obj = mp.n_objects; hd.tile_size = mp.tile_size;
    int w = MAPHDR_WORDS;
    hd.off_tiles = w; w += nt;
    hd.off_curves = w; w += 8 * mp.n_curves;
    hd.off_heads = w; w += 2 * mp.n_curves;
    hd.off_static = w; w += STATIC_WORDS * n_static;
    hd.off_objs = w; w += OBJ_WORDS * mp.n_objects;
    hd.total_words = w;
    const size_t base = T.blobs.size();
    T.M.blob_off[mi] = (int32_t)base;
    T.blobs.resize(base + w);
    uint64_t* b = T.blobs.data() + base;
    memcpy(b, &hd, sizeof hd);
    for (int t = 0; t < nt; ++t) {
      TileRec tr{};
      tr.kind = mp.tile_kind[t]; tr.angle = mp.tile_angle[t];
      tr.drivable = (tr.kind >= DTSIM_TILE_STRAIGHT && tr.kind <= DTSIM_TILE_4WAY) ? 1 : 0;
      tr.curve_cnt = mp.tile_curve_cnt[t]; tr.curve_off = mp.tile_curve_off[t]; tr.tex = mp.tile_tex[t];
      if (tr.drivable && (tr.curve_off < 0 || tr.curve_off + tr.curve_cnt > mp.n_curves || tr.curve_cnt == 0))
        return dt_scene_fail(err, DTSIM_E_INVALID, "map %d tile %d: drivable tile without curves", mi, t);
      if (tr.tex >= n_tex) return dt_scene_fail(err, DTSIM_E_INVALID, "map %d tile %d: texture %d not loaded", mi, t, tr.tex);
      memcpy(&b[hd.off_tiles + t], &tr, 8);
    }
    if (mp.n_curves) {
      memcpy(&b[hd.off_curves], mp.curves, sizeof(double) * 8 * mp.n_curves);
      memcpy(&b[hd.off_heads], mp.curve_heads, sizeof(double) * 2 * mp.n_curves);
    }
    double* st = reinterpret_cast<double*>(&b[hd.off_static]);
    double* ob = reinterpret_cast<double*>(&b[hd.off_objs]);
    int si = 0, di = 0;
    T.grid_w[mi] = mp.grid_w; T.grid_h[mi] = mp.grid_h;
    T.grid_rows = std::max(T.grid_rows, mp.grid_h + 2 * DT_QRING); T.grid_cols = std::max(T.grid_cols, mp.grid_w + 2 * DT_QRING);
    RenderMapDev& rm = T.rmaps[mi];
    rm.grid_w = mp.grid_w; rm.grid_h = mp.grid_h; rm.n_obj = mp.n_objects; rm.n_tris = 0;
    for (int o = 0; o < mp.n_objects; ++o)
      if (mp.objects[o].mesh_id >= 0 && mp.objects[o].mesh_id < n_meshes) rm.n_tris += A.meshes[mp.objects[o].mesh_id].n_tris;
    rm.tile_size = (float)mp.tile_size; rm.inv_tile_size = (float)(1.0 / mp.tile_size);
    rm.tile_off = (int32_t)T.rtiles.size(); rm.obj_off = (int32_t)T.robjs.size();
    for (int t = 0; t < nt; ++t) {
      const bool present = mp.tile_kind[t] != DTSIM_TILE_EMPTY;
      const int tex = mp.tile_tex[t] < 0 ? 0xFF : mp.tile_tex[t];
      T.rtiles.push_back((uint32_t)tex | ((uint32_t)(mp.tile_angle[t] & 3) << 8) | ((present ? 1u : 0u) << 15) |
                         ((mp.tile_tex[t] >= 0 ? 1u : 0u) << 14));
      TileLds tr{};
      tr.flags = present ? 1u : 0u;
      if (present && mp.tile_tex[t] >= 0 && mp.tile_tex[t] < n_tex) {
        const TexDev& td = A.tex[mp.tile_tex[t]];
        if (tex_w == 0) { tex_w = td.w; tex_h = td.h; }
        if (td.w != tex_w || td.h != tex_h)
          return dt_scene_fail(err, DTSIM_E_LIMIT, "map %d tile %d: all tile textures must share one size (%dx%d vs %dx%d)", mi, t, td.w, td.h, tex_w, tex_h);
        dt_tile_lds_map(tr, td, mp.tile_angle[t]);
      }
      T.trecs.push_back(tr);
    }
    for (int o = 0; o < mp.n_objects; ++o) {
      const dtsim_object& ob_ = mp.objects[o];
      if (ob_.mesh_id >= n_meshes) return dt_scene_fail(err, DTSIM_E_INVALID, "map %d object %d: mesh %d not loaded", mi, o, ob_.mesh_id);
      int slot = -1;
      if (ob_.dynamic) {
        slot = di++;
        DynInit& d = T.dyn[(size_t)mi * DTSIM_MAX_DYNAMIC + slot];
        d.cx = ob_.pos[0]; d.cz = ob_.pos[2];
        memcpy(d.corners, ob_.corners, sizeof d.corners);
        memcpy(d.norm, ob_.norm, sizeof d.norm);
        d.heading_x = std::cos(ob_.angle); d.heading_z = -std::sin(ob_.angle);  // collision.py:223-230
        d.angle = ob_.angle; d.safety_radius = ob_.safety_radius;
        d.walk_distance = ob_.walk_distance; d.vel = ob_.vel; d.wait_time = ob_.wait_time; d.wiggle = ob_.wiggle;
        d.obj_index = o; d.kind = ob_.dynamic;
      } else if (ob_.collidable) {
        double* r = st + STATIC_WORDS * si++;
        memcpy(r, ob_.corners, 8 * sizeof(double));
        memcpy(r + 8, ob_.norm, 4 * sizeof(double));
        r[12] = ob_.pos[0]; r[13] = ob_.pos[2]; r[14] = ob_.safety_radius;
      }
      ob[o * OBJ_WORDS + 0] = ob_.pos[0]; ob[o * OBJ_WORDS + 1] = ob_.pos[2];
      ob[o * OBJ_WORDS + 2] = ob_.spawn_clear;
      ob[o * OBJ_WORDS + 3] = (double)(slot >= 0 ? slot : (ob_.optional ? -2 : -1));   // -2: optional static object
      ob[o * OBJ_WORDS + 4] = (double)ob_.light_freq; ob[o * OBJ_WORDS + 5] = (double)(ob_.light_pattern & 1);
      if (ob_.light_freq < 0) return dt_scene_fail(err, DTSIM_E_INVALID, "map %d object %d: light_freq %d", mi, o, ob_.light_freq);
      ObjInstDev oi{};
      oi.x = (float)ob_.pos[0]; oi.y = (float)ob_.pos[1]; oi.z = (float)ob_.pos[2];
      oi.scale = (float)ob_.scale; oi.yrot_deg = (float)(ob_.angle * (180.0 / 3.141592653589793));
      oi.mesh_id = ob_.mesh_id; oi.dyn_slot = slot;
      oi.light_tris = ob_.light_freq > 0 ? ob_.light_tris : 0; oi.light_tex0 = ob_.light_tex[0]; oi.light_tex1 = ob_.light_tex[1];
      if (oi.light_tris > 0 && (oi.light_tex0 >= n_tex || oi.light_tex1 >= n_tex))
        return dt_scene_fail(err, DTSIM_E_INVALID, "map %d object %d: light texture not loaded", mi, o);
      T.robjs.push_back(oi);
    }
  }
  T.M.total_words = (int32_t)T.blobs.size();
  if (int rc = dt_pack_object_corners(T.ocorners, err, maps, n_maps)) return rc;
  if ((size_t)T.M.total_words * 8 > 60000)
    return dt_scene_fail(err, DTSIM_E_LIMIT, "map tables %zu B exceed the 60 KB LDS staging budget", (size_t)T.M.total_words * 8);
  if (T.trecs.size() > DTSIM_LDS_TILES)
    return dt_scene_fail(err, DTSIM_E_LIMIT, "%zu tiles over all maps exceed the %d LDS raster records", T.trecs.size(), DTSIM_LDS_TILES);
  // ---- quad-layout fast path tables: possible when every tile texture is one square power-of-two size
  std::vector<uint32_t>& qblocks = T.qblocks;
  std::vector<uint32_t>& qtiles = T.qtiles;
  int qlog2 = -1;
  float q_per_m = 0.f;
  if (render && tex_w == tex_h && tex_w >= 2) {
    const int S = tex_w;
    qlog2 = 0; while ((1 << qlog2) < S) ++qlog2;
    std::vector<int> block_of((size_t)std::max(n_tex, 1) * 4, -1);
    // the two one-record blocks: off-grid (meta high half 1) and untextured (meta 0); then the S x S blocks
    const uint32_t special[8] = {0u, 0u, 0u, 1u << 16, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u};   // untextured: white vertex colour
    qblocks.assign(special, special + 8);
    const size_t block_bytes = (size_t)S * S * 16;
    // second dword of a table entry: the mask of the record's byte offset inside its block (S = 256, q8_rec256) / of the cell number (other sizes): 0 for the
    // two one-record blocks.  S = 256: the blocks start at multiples of 1 MB (the offset is OR-ed in), the first one holds the two special records only.
    const uint32_t cell_sel = (qlog2 == 8) ? 0xFFFFFu : (uint32_t)(S * S - 1);
    const uint32_t zero_sel = 0u;
    if (qlog2 == 8) qblocks.resize(block_bytes / 4, 0u);
    int n_blocks = 0;
    for (int mi = 0; mi < n_maps; ++mi) {
      const dtsim_map& mp = maps[mi];
      RenderMapDev& rm = T.rmaps[mi];
      rm.qt_off = (int32_t)(qtiles.size() / 2); rm.qt_pitch = mp.grid_w + 2 * DT_QRING;
      q_per_m = std::max(q_per_m, (float)((double)S / mp.tile_size));
      for (int j = -DT_QRING; j < mp.grid_h + DT_QRING; ++j)
        for (int i = -DT_QRING; i < mp.grid_w + DT_QRING; ++i) {
          uint32_t off = 0u, sel = zero_sel;        // record 0: off-grid
          if (i >= 0 && j >= 0 && i < mp.grid_w && j < mp.grid_h) {
            const int t = j * mp.grid_w + i;
            if (mp.tile_kind[t] != DTSIM_TILE_EMPTY) {
              const int tx = mp.tile_tex[t];
              if (tx < 0 || tx >= n_tex) off = 16u;   // record 1: present but untextured
              else {
                int& b = block_of[(size_t)tx * 4 + (mp.tile_angle[t] & 3)];
                if (b < 0) { b = n_blocks++; dt_pack_quad_block(qblocks, A.pool.data() + A.tex[tx].off, S, mp.tile_angle[t]); }
                off = (qlog2 == 8) ? (uint32_t)((size_t)(b + 1) << 20) : (uint32_t)(32 + (size_t)b * block_bytes); sel = cell_sel;
              }
            }
          }
          qtiles.push_back(off); qtiles.push_back(sel);
        }
    }
    if (32 + (size_t)(n_blocks + 1) * block_bytes >= ((size_t)1 << 32)) qlog2 = -1;   // 32-bit block offsets
    if ((size_t)(std::max(T.grid_rows, T.grid_cols)) * S >= 32768) qlog2 = -1;          // quad coordinates below 32768 (raster_common.h, Q8_SNAP): else the generic raster
  }
  if (qlog2 <= 0 || qtiles.empty()) { qblocks.clear(); qtiles.clear(); qlog2 = 0; q_per_m = 0.f; }   // no quad records: the generic raster
  for (auto& rm : T.rmaps) T.max_tris = std::max(T.max_tris, rm.n_tris);
  T.n_tilerecs = (int)T.trecs.size();
  T.tex_w = tex_w ? tex_w : 1; T.tex_h = tex_h ? tex_h : 1;
  T.n_qtiles = (int)qtiles.size() / 2; T.qlog2 = qlog2; T.q_per_m = q_per_m;
  out = std::move(T);
  return DTSIM_OK;
}

// ---- camera table -------------------------------------------------------------------------------------------------------------
// [H*W][4] per output pixel: NDC x, y of the centre of its rectilinear source pixel, valid flag, pad.  Null maps: the identity.
inline void dt_pack_lut(int W, int H, const float* rmapx, const float* rmapy, std::vector<float>& lut) {
  lut.assign((size_t)W * H * 4, 0.f);
  for (int r = 0; r < H; ++r)
    for (int c = 0; c < W; ++c) {
      long sx = c, sy = r;
      if (rmapx) {
        // cv2.remap(INTER_NEAREST): cvRound = round-half-to-even of the float map
        // (distortion.py:118-124); outside the source image => BORDER_CONSTANT 0.
        sx = std::lrint((double)rmapx[(size_t)r * W + c]);
        sy = std::lrint((double)rmapy[(size_t)r * W + c]);
      }
      float* o = &lut[((size_t)r * W + c) * 4];
      const bool ok = sx >= 0 && sx < W && sy >= 0 && sy < H;
      // NDC of the centre of rectilinear pixel (sy, sx); row 0 = image top (simulator.py:1949)
      o[0] = ok ? (float)((2.0 * (sx + 0.5)) / W - 1.0) : 0.f;
      o[1] = ok ? (float)(1.0 - (2.0 * (sy + 0.5)) / H) : 0.f;
      o[2] = ok ? 1.f : 0.f;
      o[3] = 0.f;
    }
}
