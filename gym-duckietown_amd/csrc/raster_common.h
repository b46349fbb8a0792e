// raster_common.h -- the device helpers that two or more units of the render pass use (render_setup.hip, render.hip, render_v3.hip,
// render_exact.hip): the work decomposition's constants, the ground quad's shading rule, the queue-entry layout and the work lists, the
// scaffolding the rasters and the exact paths must agree on, the per-pixel invariants of the shared camera (pix_inv), GL's integer filter
// (gl_linear_rgb) and the byte-weight ("dtsim8") filter, and the launch size of the persistent kernels.  A helper that one unit alone uses stays in that unit.
// A device header with internal linkage, like render_scene.h: each unit compiles its own copy with the pass's flags (build.py).
#ifndef DTSIM_RASTER_COMMON_H
#define DTSIM_RASTER_COMMON_H
#include "dtsim_dev.h"
#include "raster_map.h"
#include "render_scene.h"
#include <hip/hip_fp16.h>
#include <type_traits>
#include <algorithm>
#include <map>
#include <mutex>
#include <tuple>

#define RB 256            // threads per workgroup (4 wavefronts)
#define PPT DT_PPT         // pixels per thread
#define WAVE_W DT_WAVE_W  // pixel columns per wavefront block (dtsim_dev.h)
// pixel slot k of lane l is pixel number k*64 + l of the block, row-major: adjacent lanes = adjacent pixels
#define SLOT_X(k, l) (((k) * 64 + (l)) % WAVE_W)
#define SLOT_Y(k, l) (((k) * 64 + (l)) / WAVE_W)
#define WAVE_PIX (64 * PPT)
#define ENVS_PER_BLOCK DT_ENVS_PER_BLOCK
#ifndef DT_Q_PRIO
#define DT_Q_PRIO 3                                  // k_raster_q, k_raster_v3: s_setprio level while a wavefront issues its quad loads (0: off)
#endif

namespace {

// ---- ground quad (simulator.py:1806-1812): N.L is lit at the four corners (EnvCam.gndl) and interpolated bilinearly at (a, b) in [0, 1]^2; a channel is
// gnd * min(base + dif * N.L, 1) -- ground_lit, and still written out in shade_msaa and the env loops of k_raster, k_raster_q and k_raster_v3dr.
__device__ inline float ground_corner_ndl(const float a, const float b, const float g0, const float g1, const float g2, const float g3) {
  const float n0 = g0 + a * (g1 - g0), n1 = g2 + a * (g3 - g2);
  return n0 + b * (n1 - n0);
}
__device__ inline float ground_lit(const float gnd, const float base, const float dif, const float ndl) { return gnd * fminf(base + dif * ndl, 1.f); }
__device__ inline float ground_ndl(const EnvCam& c, float wx, float wz) {      // at a world position
  const float a = fminf(fmaxf((wx + GROUND_HALF) * (0.5f / GROUND_HALF), 0.f), 1.f);
  const float b = fminf(fmaxf((wz + GROUND_HALF) * (0.5f / GROUND_HALF), 0.f), 1.f);
  return ground_corner_ndl(a, b, c.gndl[0], c.gndl[1], c.gndl[2], c.gndl[3]);
}

// max(|a|, |b|) in one instruction (source modifiers; no NaN canonicalisation needed: inputs are finite)
__device__ inline float absmax(float a, float b) { float r; asm("v_max_f32 %0, |%1|, |%2|" : "=v"(r) : "v"(a), "v"(b)); return r; }
// floor(x) as int in one instruction
__device__ inline int flr_i32(float x) { int r; asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(r) : "v"(x)); return r; }

__device__ inline uint32_t pack_rgb(const float col[3]) {  // glReadPixels float -> unorm8: round(255 c)
  const uint32_t r = (uint32_t)(fminf(fmaxf(col[0], 0.f), 255.f) + 0.5f);
  const uint32_t g = (uint32_t)(fminf(fmaxf(col[1], 0.f), 255.f) + 0.5f);
  const uint32_t b = (uint32_t)(fminf(fmaxf(col[2], 0.f), 255.f) + 0.5f);
  return r | (g << 8) | (b << 16);
}

// Edge-pixel queue: one fixed region per (workgroup, wavefront) of the raster launch, worst-case
// sized (every pixel of every env of the chunk), so appends need no atomics; entry =
// (env-in-chunk << 8) | (row-slot k << 6 | lane).  k_resolve drains the regions 64 entries at a time.
#define QREGION (WAVE_PIX * ENVS_PER_BLOCK)
// Queue entry: pixel of the wavefront block (bits 0..7) | env position in the chunk << 8 (bits 8..13).  Object-box entries
// (far end of the region, k_resolve_obj's) carry bit 15 when the pixel is ALSO a plane edge, i.e. when what the raster
// stored for it is not final: k_resolve_obj leaves a pixel alone when no mesh triangle covers any of its samples and the
// bit is clear (the raster's one-ray colour is the pixel).  The quad-record rasters tell; the generic raster always sets it (its filter is the exact path's).
#define QE_PLANE_EDGE 0x8000u
__device__ inline int qe_pixel(const uint32_t ent) { return (int)(ent & 255u); }            // row-major pixel number in the wavefront block
__device__ inline int qe_envpos(const uint32_t ent) { return (int)((ent >> 8) & 63u); }     // env position in the chunk (k_resolve reads ent >> 8: front entries carry no flags, the mask costs it 13 instructions)
__device__ inline bool qe_plane_edge(const uint32_t ent) { return (ent & QE_PLANE_EDGE) != 0u; }
static_assert(ENVS_PER_BLOCK <= 64, "the env position of a queue entry has six bits");
#define ITEM_B DT_ITEM_B   // 64-entry batches per k_resolve work item
#define ITEMS_PER_WG DT_ITEMS_PER_WG
#define GRAB_MAX 16       // work items per cursor atomic, at most
#ifndef DT_RES_ENVS
#define DT_RES_ENVS 1             // round 4: 8 -> 1 (one env per item: the launch ended on its longest octet; C5 - 8 %, profiles/r04_wave_spans.txt)
#endif
#define RES_ENVS DT_RES_ENVS  // env positions of a chunk per k_resolve_obj work item
static_assert(ENVS_PER_BLOCK % RES_ENVS == 0 && ENVS_PER_BLOCK / RES_ENVS <= ITEMS_PER_WG, "octet items");

// The live count of a masked pass (positions [0, live) of the render order), written by k_env_sort<true> after the pass's work-list clear.
__device__ inline int dt_sub_live(const RenderParams& R) { return __builtin_amdgcn_readfirstlane(R.work[DT_WORK_LIVE]); }
// Work items of k_resolve_obj (its own list: the DT_WORK_OBJ_* slots of R.work; R.items2): one per RES_ENVS
// env positions of a raster workgroup that queued object-box pixels.
// groups: bit g = env group g of the chunk (RES_ENVS positions) has object-box entries in some region of the workgroup; the
// quad-record rasters pass what they queued (round 4: 60 % of the items used to be empty), the others every group.
// Round 4: the list has two ends.  Items of env groups that queued a lot (heavy: bit g, a subset of groups) go to the front in push
// order, the others to the back (from the last slot down); k_resolve_obj walks front to back, so the units of close-up objects -- up to
// 1 024 pixels against every triangle of the object, 100 - 250 us of one wavefront -- start first instead of wherever their raster
// workgroup happened to finish (the launch used to end on a third of the wavefronts, profiles/r04_wave_spans.txt).
// DT_WORK_OBJ_FRONT / DT_WORK_OBJ_BACK count the two ends, DT_WORK_OBJ_CURSOR is the cursor; capacity = one slot per (raster workgroup, env group).
__device__ inline size_t obj_items_cap(const RenderParams& R) {
  const int n_tiles = ((R.W + DT_TILE_W - 1) / DT_TILE_W) * ((R.H + DT_TILE_H - 1) / DT_TILE_H);
  return (size_t)((R.N + ENVS_PER_BLOCK - 1) / ENVS_PER_BLOCK) * n_tiles * (ENVS_PER_BLOCK / RES_ENVS);
}
typedef unsigned long long envmask_t;                 // one bit per env group of a chunk (ENVS_PER_BLOCK / RES_ENVS <= 64)
__device__ inline void push_obj_items(const RenderParams& R, uint32_t rwg, envmask_t groups = ~0ull, envmask_t heavy = 0ull) {
  const int ng = ENVS_PER_BLOCK / RES_ENVS;
  if (ng < 64) groups &= (1ull << ng) - 1ull;
  heavy &= groups;
  const envmask_t light = groups & ~heavy;
  const int nh = __popcll(heavy), nl = __popcll(light);
  if (nh) {
    int pos = atomicAdd(R.work + DT_WORK_OBJ_FRONT, nh);
    for (int i = 0; i < ng; ++i) if ((heavy >> i) & 1ull) R.items2[pos++] = rwg * ITEMS_PER_WG + (uint32_t)i;
  }
  if (nl) {
    size_t pos = obj_items_cap(R) - 1 - (size_t)atomicAdd(R.work + DT_WORK_OBJ_BACK, nl);
    for (int i = 0; i < ng; ++i) if ((light >> i) & 1ull) R.items2[pos--] = rwg * ITEMS_PER_WG + (uint32_t)i;
  }
}
#ifndef DT_RO_HEAVY
#define DT_RO_HEAVY 128            // entries of one env in one 256-pixel wavefront region from which its unit counts as heavy
#endif
// which env groups of the chunk have entries in THIS wavefront's region: qend_v = the region's fill after each env (lane = position)
__device__ inline envmask_t obj_groups_of(int qend_v, int lane, envmask_t* heavy = nullptr) {
  static_assert(ENVS_PER_BLOCK / RES_ENVS <= 64, "one bit per env group");
  const int up = __shfl_up(qend_v, 1);
  const int cnt = lane < ENVS_PER_BLOCK ? qend_v - (lane == 0 ? 0 : up) : 0;
  const unsigned long long m = __ballot(cnt != 0), mh = __ballot(cnt >= DT_RO_HEAVY);
  envmask_t g = 0ull, gh = 0ull;
#pragma unroll
  for (int i = 0; i < ENVS_PER_BLOCK / RES_ENVS; ++i) {
    g |= ((m >> (i * RES_ENVS)) & ((1ull << RES_ENVS) - 1ull)) ? (1ull << i) : 0ull;
    gh |= ((mh >> (i * RES_ENVS)) & ((1ull << RES_ENVS) - 1ull)) ? (1ull << i) : 0ull;
  }
  if (heavy) *heavy = gh;
  return g;
}

// ==== scaffolding shared by the rasters ===================================================================================================
// What every raster must agree on with the host and the exact-path kernels, stated once: the workgroup map and its launch size, the v3 LDS
// tile table, the chunk's object masks and the packed source-pixel centres; further down the exact paths' rules (below; ground_lit at ground_ndl,
// qe_* at the entry layout, store_rgb after the byte-weight filter).  A helper stays only where the compiled kernel is unchanged (tools/isa_compare.py,
// profiles/exact_path_identity.txt).  Still written out per kernel, because as helpers they changed the generated code: the queue appends, push_obj,
// the transposes and the hand-over epilogues (the env loops); the item -> workgroup / part / tile / chunk decode and the four regions' batch lookup of
// k_resolve / k_resolve_dr / k_resolve_obj (a struct, a struct with lazy members, free functions over rn[] / rb[]: 35 - 65 instructions more); k_raster's
// tile-record fill; ground_lit in k_raster_v3dr's env loop; k_resolve's unmasked env position.  What a kernel does differently is an argument at its call site.

// ---- XCD-affine workgroup map of the quad-record rasters (k_raster_q, k_raster_v3, k_raster_v3dr): raster_map.h states the lists, the launch
// size and the prefix / suffix split; here is what a workgroup does with them.
// NL: envs of the pass; live: false for a workgroup of the grid's padding (the whole workgroup leaves, before anything else is derived);
// rwg: the logical workgroup index (queue regions, counts, work items) -- of the ITEM, whichever workgroup runs it; [e0, e1): the chunk's
// positions in the render order.  claims (TICKET only): the workgroup draws its item (raster_claim_*) instead of decoding it; thief: its slot
// lies past the lists.
struct RasterWg {
  int NL, tile, chunk; bool live, claims, thief;
  __device__ int rwg(const int n_tiles) const { return chunk * n_tiles + tile; }
  __device__ int e0() const { return chunk * ENVS_PER_BLOCK; }
  __device__ int e1() const { return min(e0() + ENVS_PER_BLOCK, NL); }
};
// SUB: the masked pass -- positions [0, live) of k_env_sort<true>'s order, few live chunks: workgroup b takes tile b % n_tiles of chunk
// b / n_tiles, so that every chunk's tiles spread over all eight XCDs.
// SCALAR: tile and chunk through readfirstlane -- the divisions run on the vector ALU, and without it the env loop's counter and the per-env
// address arithmetic of k_raster_v3 / k_raster_v3dr stay vector instructions; k_raster_q was tuned without it and keeps its form.
// TICKET (k_raster_v3's full pass): the list's last DT_RASTER_TICKET_UNITS units are claimed, not decoded, and the launch carries raster_thieves() more slots
// per XCD -- with the static map the XCDs ended up to 4 % of the launch apart (sorted render order: the scenes of the slices differ); an XCD whose list is
// dry now takes what is left of a late one's suffix, and they end within 0.6 % (C3 - 1.5 %, C5 - 1.8 %: profiles/raster_ticket_map.txt).
template <bool SUB, bool SCALAR, bool TICKET = false>
__device__ inline RasterWg raster_wg(const RenderParams& R, const int n_tiles, const unsigned bx) {
  static_assert(!(SUB && TICKET), "the masked pass keeps its linear map");
  RasterWg w;
  w.NL = SUB ? dt_sub_live(R) : R.N;                 // (SUB: the live chunks)
  const int n_chunks = (w.NL + ENVS_PER_BLOCK - 1) / ENVS_PER_BLOCK;
  const int xcd = bx & 7, bi = bx >> 3;
  const bool thief = TICKET && bi >= raster_list_slots(n_tiles, n_chunks);   // a slot past the lists (raster_ticket_grid): nothing to decode
  const RasterItem it = raster_item(n_tiles, n_chunks, xcd, thief ? 0 : bi);
  const int tile = SUB ? (int)bx % n_tiles : it.tile;
  w.tile = SCALAR ? __builtin_amdgcn_readfirstlane(tile) : tile;
  const int chunk = SUB ? (int)bx / n_tiles : it.chunk;
  w.chunk = SCALAR ? __builtin_amdgcn_readfirstlane(chunk) : chunk;
  w.live = SUB ? w.chunk < n_chunks : (it.live && !thief);
  w.claims = TICKET && __builtin_amdgcn_readfirstlane((int)(thief || !raster_slot_static(n_tiles, n_chunks, xcd, thief ? 0 : bi, DT_RASTER_TICKET_UNITS))) != 0;
  w.thief = thief;
  return w;
}
// The claim of a workgroup with w.claims, in two halves so that work which does not depend on the item (the LDS tile table) hides the
// round trip: raster_claim_issue draws the first ticket (thread 0, the own XCD's counter; a device-scope atomic like the cursors of
// k_resolve_*; a thief starts when its XCD's own slots have all started and draws none), raster_claim_finish turns it into the item -- with
// the own list dry it reads the other seven counters at once and draws from those that are not dry, in rotation from xcd + 1 -- and hands the
// item to the workgroup through LDS (one barrier, claimers only).  At most DT_RASTER_XCDS atomic adds, no waiting on another workgroup.
static_assert(DT_WORK_TICKETS >= DT_TICKET_STRIDE && DT_WORK_TICKETS + DT_RASTER_XCDS * DT_TICKET_STRIDE <= DT_WORK_INTS, "the ticket counters lie inside R.work (zeroed before every pass)");
__device__ inline int raster_claim_issue(const RenderParams& R, const unsigned bx, const int tid, const RasterWg& w) {
  if (w.thief) return 0x7fffffff;
  return tid == 0 ? atomicAdd(R.work + DT_WORK_TICKETS + (int)(bx & 7) * DT_TICKET_STRIDE, 1) : 0;
}
__device__ inline void raster_claim_finish(const RenderParams& R, const int n_tiles, const unsigned bx, const int first, int* s_claim, const int tid, RasterWg& w) {
  const int n_chunks = (w.NL + ENVS_PER_BLOCK - 1) / ENVS_PER_BLOCK;
  if (tid == 0) {
    RasterItem it = raster_ticket_item(n_tiles, n_chunks, (int)(bx & 7), first, DT_RASTER_TICKET_UNITS);
    if (!it.live) {
      int seen[DT_RASTER_XCDS];
#pragma unroll
      for (int a = 1; a < DT_RASTER_XCDS; ++a)
        seen[a] = __hip_atomic_load(R.work + DT_WORK_TICKETS + raster_claim_xcd((int)(bx & 7), a) * DT_TICKET_STRIDE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
      for (int a = 1; a < DT_RASTER_XCDS; ++a) {
        const int x = raster_claim_xcd((int)(bx & 7), a);
        if (it.live || seen[a] >= raster_ticket_len(n_tiles, n_chunks, x, DT_RASTER_TICKET_UNITS)) continue;   // a counter only grows: dry stays dry
        it = raster_ticket_item(n_tiles, n_chunks, x, atomicAdd(R.work + DT_WORK_TICKETS + x * DT_TICKET_STRIDE, 1), DT_RASTER_TICKET_UNITS);
      }
    }
    s_claim[0] = it.live ? it.tile : -1; s_claim[1] = it.chunk;
  }
  __syncthreads();
  w.tile = __builtin_amdgcn_readfirstlane(s_claim[0]); w.chunk = __builtin_amdgcn_readfirstlane(s_claim[1]);
  w.live = w.tile >= 0;
}

// ---- LDS tile table of k_raster_v3 / k_raster_v3dr / k_resolve_dr: the tile tables of all maps in rows of V3_TAB_PITCH entries, block byte
// offsets in the first half of a row, record-offset masks in the second (defaults of the unused columns: record 0 = off the grid, mask 0).
// The caller's barrier follows.  (V3_TAB_PITCH, V3_MAP_COLS: render_records.h.)
#define V3_MAX_ROWS 24                                // padded grid height <= 24 (24 KB of LDS)
__device__ inline void v3_fill_tile_table(const RenderParams& R, const uint32_t* __restrict__ qtiles, uint32_t* s_qt, const int tid) {
  for (int i = tid; i < R.q3_rows * V3_TAB_PITCH; i += RB) s_qt[i] = 0u;
  __syncthreads();
  for (int mi = 0; mi < R.n_maps; ++mi) {
    const int pitch = R.maps[mi].qt_pitch, off = R.maps[mi].qt_off, n = pitch * (R.maps[mi].grid_h + 2 * DT_QRING);
    for (int i = tid; i < n; i += RB) {
      const int r = i / pitch, c = i - r * pitch;
      const uint2 te = reinterpret_cast<const uint2*>(qtiles)[off + i];
      s_qt[r * V3_TAB_PITCH + mi * V3_MAP_COLS + c] = te.x;
      s_qt[r * V3_TAB_PITCH + V3_TAB_PITCH / 2 + mi * V3_MAP_COLS + c] = te.y;
    }
  }
}

// ---- per-pixel quantities that do not depend on the env when the camera is shared: k_raster<false, OBJ> keeps them in registers, k_pix_setup
// (render_setup.hip) turns them into the quad-record rasters' PixTab ------
struct PixInv {
  float lr, lf;     // tile-plane hit in the yaw-local frame (right, forward), metres
  float ndl;        // max(0, N.L) of the tile plane at the hit
  float mrg;        // conservative world-space footprint radius of the 4 MSAA samples
  uint32_t flags;   // PF_*
};
#define PF_VALID 1u       // inside the source image (else BORDER_CONSTANT 0)
#define PF_SKY 2u         // all 4 samples certainly miss every plane
#define PF_ALWAYS_EDGE 4u // horizon band / near-far limits: always take the exact path
#define PF_TILE_OK 8u     // tile-plane hit within [near, far]
#define PF_GROUND_OK 16u  // ground-plane hit within [near, far]

__device__ inline PixInv pix_inv(float nx, float ny, bool valid, float tx, float ty, float sth, float cth,
                                 float Cy, const float L[4], float ex_n, float ey_n) {
  PixInv p;
  p.flags = valid ? PF_VALID : 0u;
  p.lr = p.lf = p.ndl = p.mrg = 0.f;
  const Ray r = make_ray(nx, ny, tx, ty, sth, cth);
  const float ex = ex_n * tx, ey = ey_n * ty;
  const float dy = ey * fabsf(cth);
  if (!(r.yla < 0.f)) {
    p.flags |= (r.yla - dy >= 0.f) ? PF_SKY : PF_ALWAYS_EDGE;
    return p;
  }
  const float inv = frcp(-r.yla);
  const float t = Cy * inv;
  p.lr = t * r.xe; p.lf = t * r.fwd;
  p.ndl = plane_ndl(L, sth, cth, r, t);
  const float rho = dy * inv;
  // World-space reach of the MSAA samples around the pixel-centre hit.  A sample offset
  // (dx, dy) px moves the hit by  t*ex*dx  along `right` and, through the change of the ray
  // parameter (kappa = rho/(1-rho) per full y-offset), by (lr, lf)*kappa*dy + t*ey*|sth|*dy along
  // (right, forward).  The rotated-grid samples sit at (+-0.375, +-0.125) and (+-0.125, +-0.375):
  // take the larger of the two reaches (ex/ey already carry the 0.375 and a 1% pad), +5%.
  {
    const float kappa = rho * frcp(fmaxf(1.f - rho, 0.25f));
    const float ax_ = t * ex, ry_ = fabsf(p.lr) * kappa, fy_ = fabsf(p.lf) * kappa + t * ey * fabsf(sth);
    const float third = 1.f / 3.f;
    const float r1x = ax_ + third * ry_, r1f = third * fy_;          // (0.375, 0.125)
    const float r2x = third * ax_ + ry_, r2f = fy_;                  // (0.125, 0.375)
    p.mrg = 1.05f * fsqrt_(fmaxf(r1x * r1x + r1f * r1f, r2x * r2x + r2f * r2f));
  }
  const float tg = (Cy - GROUND_Y) * inv;
  if (t >= NEAR_Z && t <= FAR_Z) p.flags |= PF_TILE_OK;
  if (tg >= NEAR_Z && tg <= FAR_Z) p.flags |= PF_GROUND_OK;
  if (rho > 0.25f || tg * (1.f + 2.f * rho) > FAR_Z * 0.98f || t * (1.f - 2.f * rho) < NEAR_Z * 1.02f)
    p.flags |= PF_ALWAYS_EDGE;
  return p;
}

// ==== scaffolding shared by the exact paths: what resolve_region_q / _v3, k_resolve, k_resolve_dr and k_resolve_obj must agree on, stated once ====
// ---- the tile that OWNS an MSAA sample at padded quad coordinates (Xs, Zs), on the v3 LDS tile table (qtb; tab: byte offset of the env's map
// columns): tile boundaries sit at k * 256 + 0.5 (GL_LINEAR's half-texel shift), so ownership goes by (X - 0.5, Z - 0.5), clamped into the padded
// grid.  tb: the tile's block byte offset (0: none), sel: its record-offset mask; returns s_in: inside the grid.  (resolve_region_q: tile_entry.)
__device__ inline float med3f(float x, float lo, float hi) { return __builtin_amdgcn_fmed3f(x, lo, hi); }
__device__ inline bool v3_sample_owner(const float Xs, const float Zs, const float lo, const float Xhi, const float Zhi, const char* qtb,
                                       const uint32_t tab, uint32_t& tb, uint32_t& sel) {
  const float Xo = Xs - 0.5f, Zo = Zs - 0.5f;
  const float Xc = med3f(Xo, lo, Xhi), Zc = med3f(Zo, lo, Zhi);
  const uint32_t ta = (__builtin_amdgcn_perm((uint32_t)flr_i32(Zc), (uint32_t)flr_i32(Xc), 0x0c0c0501u) << 2) + tab;
  const uint32_t* tp = reinterpret_cast<const uint32_t*>(qtb + ta);
  tb = tp[0]; sel = tp[V3_TAB_PITCH / 2];
  return (Xc == Xo) & (Zc == Zo);
}
// ---- ground-quad hit in padded quad coordinates, per axis: camera + kg * (tile-plane hit - camera); inside +-50 m (goff: world 0, ghalf: 50 m)
__device__ inline float ground_quad_at(const float kg, const float X, const float C) { return fmaf(kg, X - C, C); }
__device__ inline bool ground_quad_in(const float G, const float goff, const float ghalf) { return fabsf(G - goff) <= ghalf; }

// ---- work lists of the persistent kernels (k_resolve, k_resolve_dr, k_resolve_obj).  One atomic buys `grab` items, taken with stride n_grabs through
// the list: same-address atomics are serialised by the L2 (~0.2 ms per 100 k), and the stride keeps the consecutive items of one hot raster
// workgroup on different wavefronts.  Granularity: ~4 grabs per resident wavefront, <= GRAB_MAX items.
__device__ inline int work_n_grabs(const int n_items) {
  const int grab = max(1, min(GRAB_MAX, n_items / (int)(gridDim.x * (RB / 64) * 4)));
  return (n_items + grab - 1) / grab;
}
// A wavefront's first grab is its own index (round 4: the launch holds exactly the resident workgroups; 5 000 wavefronts starting on one cursor atomic
// waited 30 - 60 us each, profiles/r04_wave_spans.txt); this is every later one, from the list's cursor slot (g: the previous grab, kept by lanes > 0).
__device__ inline int work_next_grab(const RenderParams& R, const int cursor, int g, const int lane) {
  if (lane == 0) g = (int)gridDim.x * (RB / 64) + atomicAdd(R.work + cursor, 1);
  return __builtin_amdgcn_readfirstlane(g);
}

// ---- object masks (k_obj_setup: bit o = object o's screen box meets the block) of the chunk's envs for one wavefront block.  One vector
// load up front: lane l holds the mask of position e0 + l (a scalar load per env would sit in the same counter as the LDS reads of the env
// loop and stall them: measured +0.4 ms); per env two v_readlane.
template <bool OBJ>
struct ChunkObjMasks {
  static_assert(ENVS_PER_BLOCK <= 64, "one lane per env of the chunk");
  uint32_t lo, hi;
  int e0;
  __device__ void load(const RenderParams& R, const int e0_, const int e1, const int n_blk, const int blk, const int lane) {
    uint32_t om_lo = 0u, om_hi = 0u;
    if (OBJ && lane < e1 - e0_) {
      const unsigned long long v = R.objmask[(size_t)(e0_ + lane) * n_blk + blk];
      om_lo = (uint32_t)v; om_hi = (uint32_t)(v >> 32);
    }
    lo = om_lo; hi = om_hi; e0 = e0_;
  }
  __device__ unsigned long long of(const int e) const {
    if (!OBJ) return 0ull;
    return ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)hi, e - e0) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)lo, e - e0);
  }
};

// ---- spxy: the source-pixel centre of a pixel (from its LUT entry) as two fp16 in one register (x | y << 16): 0.25 px rounding below
// 1024, which the object-box margin covers.  The unpack sits behind a register barrier: it is redone per env, not hoisted ahead of the env
// loop (8 registers).
__device__ inline uint32_t spxy_pack(const float4& l, const int W, const int H) {
  float sx, sy;
  src_px(l.x, l.y, W, H, sx, sy);
  return (uint32_t)__half_as_ushort(__float2half(sx)) | ((uint32_t)__half_as_ushort(__float2half(sy)) << 16);
}
__device__ inline void spxy_unpack(uint32_t t, float& sx, float& sy) {
  asm volatile("" : "+v"(t));
  sx = __half2float(__ushort_as_half((unsigned short)(t & 0xFFFFu)));
  sy = __half2float(__ushort_as_half((unsigned short)(t >> 16)));
}

struct alignas(4) U3 { uint32_t a, b, c; };           // 4 pixels x RGB: a lane's 12 bytes of a frame row

// ---- GL_LINEAR as the reference's renderer computes it -------------------------------------------------------------------
// GL leaves the filter's precision to the implementation.  The reference's CI renderer -- Mesa llvmpipe, the one the GL goldens
// come from (tests/golden/ref_gl_*.npz) -- filters RGBA8 textures in integers (measured bit-exact, profiles/r06_gl_filter_precision.txt):
// texel coordinate * 256, rounded, minus half a texel; the low 8 bits are the weight; lerp(w, p, q) = p + ((w (q - p) + 128) >> 8),
// along s for both rows, then along t on the 8-bit results.  gl_fix: coordinate already shifted by the half texel -> fixed point.
// The generic k_raster (render.hip) and the exact-path shaders (tile_color, mesh_texel: render_exact.hip) filter with it.
__device__ inline int gl_lerp8(int w, int p, int q) { return p + ((w * (q - p) + 128) >> 8); }
__device__ inline int gl_fix(float x) { return (int)floorf(fmaf(x, 256.f, 0.5f)); }
__device__ inline void gl_linear_rgb(uint32_t t00, uint32_t t10, uint32_t t01, uint32_t t11, int wx, int wy, int out[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int c00 = (int)((t00 >> (8 * k)) & 255u), c10 = (int)((t10 >> (8 * k)) & 255u);
    const int c01 = (int)((t01 >> (8 * k)) & 255u), c11 = (int)((t11 >> (8 * k)) & 255u);
    out[k] = gl_lerp8(wy, gl_lerp8(wx, c00, c10), gl_lerp8(wx, c01, c11));
  }
}

// ---- the quad-record filter ("dtsim8") -------------------------------------------------------------------
// GL's own filter (llvmpipe: gl_linear_rgb, above) works with 8-bit weights and 8-bit intermediates, so nothing is gained by filtering
// finer than that; the quad pipeline filters in ONE v_dot4_u32_u8 per channel: the four bilinear weights, times the lit factor
// where it is the same for the three channels (shared camera), times 256, rounded to bytes (v_cvt_pk_u8_f32); colour =
// (sum(texel * weight) + 128) >> 8.  Measured against the GL goldens it differs from llvmpipe by +-1/255 on about a quarter of the
// textured pixels -- what the 16-bit filter it replaces did too (tests/test_gl_golden.py::test_quad_filter_distance_to_gl).
// The texture coordinate itself is snapped to 256ths of a texel first -- llvmpipe rounds its coordinates to 8 fractional bits before it
// splits them into texel index and weight (gl_linear_rgb) -- by ONE float add: X + 32768 (X in quad cells, 0 <= X < 32768; the host
// checks the padded grid against it) rounds X to a multiple of 1/256 and leaves it in the sum's bit pattern: byte 0 = the fraction in
// 256ths, bits 8..22 = the cell number (S = 256: byte 1 = the cell inside the tile, byte 2 = the tile).  A fraction that rounds up to 1
// carries into the cell number, as in GL.  The hot loops take everything from these bits -- no v_cvt_flr, no v_fract.
#define Q8_SNAP 32768.f
#define Q8_LIT (1.f / 256.f)                         // the weights' light argument is lit / 256 (the fractions come as 0..255)
__device__ inline uint32_t q8_bits(float X) { return __float_as_uint(X + Q8_SNAP); }
__device__ inline uint32_t q8_cell(uint32_t b) { return (b >> 8) & 0x7FFFu; }      // the cell number (one v_bfe_u32)
__device__ inline float q8_frac(uint32_t b) { return (float)(b & 255u); }          // the fraction x 256 (one v_cvt_f32_ubyte0)
// Byte offset of the record of the cell of snapped coordinates (xb, zb) inside a 256 x 256 block, masked by the tile's table entry (0 for the
// one-record blocks): the records lie 4 x 2 cells to a 128-byte line -- offset = (cx >> 2) << 14 | cz << 6 | (cx & 3) << 4 -- because the texture
// unit charges a gather per distinct line, and the footprint of a 32 x 2 pixel slot is a slanted strip: 12.0 lines per gather instead of 14.0 with
// the texture's rows laid end to end (tools/gather_lines_model.py; profiles/r06_variants_ab.txt block H).  cx * 0x1010 puts cx at bits 12.. and
// 4..; cz (byte 1 of zb, shifted to bits 6..13) goes over the middle: 3 instructions + the v_and_or that masks and adds the block's offset.
__device__ inline uint32_t q8_rec256(uint32_t xb, uint32_t zb, uint32_t m) {
  uint32_t P, Zs;                                    // (the byte selects written out: the compiler's SDWA peephole finds them for some of the four pixels only)
  asm("v_mul_u32_u24_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_1 src1_sel:DWORD" : "=v"(P) : "v"(xb), "s"(0x1010u));
  asm("v_lshlrev_b32_sdwa %0, 6, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1" : "=v"(Zs) : "v"(zb));
  return ((P & 0xFC030u) | Zs) & m;
}
// a8, b8: the fractions x 256 (0..255); l = lit / 256 (1 / 256 for an unlit filter).  Byte order = the record's texel order:
// (x0,z0) (x1,z0) (x0,z1) (x1,z1).  (The packed forms in the env loops of k_raster_q / k_raster_v3 are these operations, two pixels each.)
typedef float f2_t __attribute__((ext_vector_type(2)));
__device__ inline f2_t fma2(f2_t a, f2_t b, f2_t c) { return __builtin_elementwise_fma(a, b, c); }   // one v_pk_fma_f32, whatever the contraction mode
__device__ inline uint32_t quad_weights8(float a8, float b8, float l) {
#pragma clang fp contract(off)                       // which products are fused is part of the definition (the oracle restates it): u and the w*1 are rounded products
  const float u = a8 * l, v = fmaf(l, 256.f, -u);
  const float w11 = u * b8, w01 = v * b8, w10 = fmaf(u, 256.f, -w11), w00 = fmaf(v, 256.f, -w01);
  uint32_t W = __builtin_amdgcn_cvt_pk_u8_f32(w00, 0, 0u);
  W = __builtin_amdgcn_cvt_pk_u8_f32(w10, 1, W);
  W = __builtin_amdgcn_cvt_pk_u8_f32(w01, 2, W);
  return __builtin_amdgcn_cvt_pk_u8_f32(w11, 3, W);
}
// The tile plane's lit factor / 256 of one pixel (yaw-local centre hit lr, lf) under an env's own light (EnvL): the raster's env loops and the
// exact paths all go through these operations, so that a one-ray pixel gets the same bytes from either (the packed form in the env loops is
// these operations, two pixels each).  base8 = the shared ambient term / 256; the clamp at 1 / 256 is exact (a power of two).
__device__ inline float env_lit8(const EnvL& l, float lr, float lf, float base8) {
#pragma clang fp contract(off)
  const float dx = l.Lr - lr, dz = l.Lf - lf;
  return fminf(fmaf(l.kd8, frsq(fmaf(dx, dx, fmaf(dz, dz, l.h2))), base8), Q8_LIT);
}
__device__ inline float env_base8() { return default_cam(1.f).base * Q8_LIT; }
__device__ inline f2_t env_lit8_2(const EnvL& l, const f2_t lr, const f2_t lf) {   // env_lit8 of two pixels
#pragma clang fp contract(off)
  const f2_t dx = f2_t{l.Lr, l.Lr} - lr, dz = f2_t{l.Lf, l.Lf} - lf;
  const f2_t d2 = fma2(dx, dx, fma2(dz, dz, f2_t{l.h2, l.h2}));
  const float b8 = env_base8();
  const f2_t t = fma2(f2_t{l.kd8, l.kd8}, f2_t{frsq(d2.x), frsq(d2.y)}, f2_t{b8, b8});
  return f2_t{fminf(t.x, Q8_LIT), fminf(t.y, Q8_LIT)};
}
// one-ray colour 0x00BBGGRR of a record (a8, b8 as above; I = lit factor, 0..1)
__device__ inline uint32_t quad_filter(const uint4& q, float a8, float b8, float I) {
  const uint32_t W = quad_weights8(a8, b8, I * Q8_LIT);
  const uint32_t vr = __builtin_amdgcn_udot4(q.x, W, 128u, false), vg = __builtin_amdgcn_udot4(q.y, W, 128u, false),
                 vb = __builtin_amdgcn_udot4(q.z, W, 128u, false);                 // the channel is byte 1 of each sum
  const uint32_t rg = __builtin_amdgcn_perm(vg, vr, 0x0c0c0501u);
  return __builtin_amdgcn_perm(vb, rg, 0x0c050100u);
}
__device__ inline void quad_filter3(const uint4& q, float a8, float b8, float I, float out[3]) {   // 0..255 floats, unrounded
  const uint32_t W = quad_weights8(a8, b8, I * Q8_LIT);
  out[0] = (float)__builtin_amdgcn_udot4(q.x, W, 0u, false) * (1.f / 256.f);
  out[1] = (float)__builtin_amdgcn_udot4(q.y, W, 0u, false) * (1.f / 256.f);
  out[2] = (float)__builtin_amdgcn_udot4(q.z, W, 0u, false) * (1.f / 256.f);
}

#define RQ_LIST 256                                  // MSAA entries compacted per round (the wavefront's 1 KB of LDS)
// one pixel's colour 0x00BBGGRR into frame e of the exact paths' byte patches: two stores, a 2-byte aligned half + one byte,
// whichever way the pixel's 3 bytes fall
__device__ inline void store_rgb(uint8_t* frames, const int npix, const int e, const int pix, const uint32_t rgb) {
  uint8_t* dst = frames + ((size_t)e * npix + pix) * 3;
  const bool odd = (reinterpret_cast<uintptr_t>(dst) & 1u) != 0u;
  uint8_t* p8 = odd ? dst : dst + 2;
  uint16_t* p16 = reinterpret_cast<uint16_t*>(odd ? dst + 1 : dst);
  *p8 = (uint8_t)(odd ? rgb : rgb >> 16);
  *p16 = (uint16_t)(odd ? rgb >> 8 : rgb);
}

}  // namespace

// Workgroups of `kernel` (RB threads, lds bytes of dynamic LDS) the device holds at once: the launch size of the persistent exact-path kernels.
template <class K> static size_t resident_blocks(K kernel, size_t lds) {
  static std::mutex mu;
  static std::map<std::tuple<int, size_t, const void*>, size_t> cache;   // (the template is instantiated per function-pointer TYPE: two kernels of one signature share it)
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> lk(mu);
  const auto key = std::make_tuple(dev, lds, reinterpret_cast<const void*>(kernel));
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  int per_cu = 0, n_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, RB, lds) != hipSuccess || per_cu < 1) per_cu = 3;
  if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n_cu < 1) n_cu = 256;
  return cache[key] = (size_t)per_cu * (size_t)n_cu;
}

#endif
