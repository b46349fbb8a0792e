// render_exact.hip -- the kernels of a render pass that patch pixels after its raster, stream-ordered behind it so that the byte patches land
// after the raster's stores, and dt_launch_render_exact, which sizes and launches them.  (The quad-record rasters resolve their own plane-edge
// pixels inside the raster: resolve_region_q in render.hip, resolve_region_v3 / k_resolve_dr in render_v3.hip.)
//   k_resolve:    exact 4-sample resolve of the plane-edge pixels the generic k_raster queued (front of the queue regions): persistent
//                 wavefronts pull work items (8 queue batches of one raster workgroup), 64 entries at a time -- coverage per sample, shading
//                 once per distinct primitive at the pixel centre (shade_msaa) -- and patch the 3 bytes of each pixel.
//   k_resolve_obj: the pixels inside mesh-object screen boxes (far end of the queue regions, any raster), one unit per (raster tile, env):
//                 triangles streamed and staged in LDS once per unit, z-buffered per sample in 1/depth space (zbuffer_chunk), then the same shading.
// The filter is llvmpipe's integer GL_LINEAR (gl_linear_rgb, raster_common.h: the generic raster's too) on tiles (tile_color) and mesh textures
// (mesh_texel).  The work lists, the queue-entry layout and the ground quad's rule are raster_common.h's; classify() and test_tri render_scene.h's.
#include "raster_common.h"

#ifndef DT_TRI_CAP
#define DT_TRI_CAP 96              // round 3: 128 -> 96 (with 256 pair slots: 40 KB of LDS per workgroup, 4 workgroups per CU; block M)
#endif
#define TRI_CAP DT_TRI_CAP  // LDS triangle slots per wavefront in k_resolve_obj (streamed chunks)

// The staged triangle: the coverage-only half of a ScreenTri, kept in LDS by k_resolve_obj (loaded as the record's first 64 bytes); the
// winner's colours are fetched from global memory.
struct alignas(16) TriCov { float bx0, bx1, by0, by1; float sx[3], sy[3], iw[3]; float inv_area; int32_t index; int32_t pad; };   // == first half of ScreenTri
static_assert(sizeof(TriCov) == 64, "TriCov is 64 bytes");

namespace {

// ---- the raster tile records of every map -> LDS (k_resolve, k_resolve_obj: [n_tile_recs] TileLds at the start of the workgroup's
// dynamic LDS).  The caller's barrier follows.  (k_raster keeps the same loop written out: the call moved an instruction of its prologue.)
__device__ inline void fill_tile_recs(const RenderParams& R, uint32_t* s_mem, const int tid) {
  const uint32_t* src = reinterpret_cast<const uint32_t*>(R.tile_recs);
  for (int i = tid; i < R.n_tile_recs * (int)(sizeof(TileLds) / 4); i += RB) s_mem[i] = src[i];
}

// GL_LINEAR/GL_REPEAT fetch from the padded texture (the exact paths and the generic raster: llvmpipe's arithmetic), times the lit
// vertex colour I.
__device__ inline void tile_color(const RenderParams& R, const TileLds& tr, float fx, float fz, const float I[3],
                                  float out[3]) {
  if (!(tr.flags & 2u)) {  // untextured tile: white vertex colour
    out[0] = 255.f * I[0]; out[1] = 255.f * I[1]; out[2] = 255.f * I[2];
    return;
  }
  float x, y;
  tile_texel_xy(tr, fx, fz, x, y);
  const int xf = gl_fix(x), yf = gl_fix(y);
  const int x0 = (xf >> 8) & (R.tex_w - 1), y0 = (yf >> 8) & (R.tex_h - 1);
  const uint32_t* pt = R.texels + tr.tex_off + y0 * (R.tex_w + 1) + x0;
  uint2 top2, bot2;               // two 8-byte loads: (x0,y0),(x0+1,y0) and the row above
  __builtin_memcpy(&top2, pt, 8);
  __builtin_memcpy(&bot2, pt + (R.tex_w + 1), 8);
  int T[3];
  gl_linear_rgb(top2.x, top2.y, bot2.x, bot2.y, xf & 255, yf & 255, T);
#pragma unroll
  for (int k = 0; k < 3; ++k) out[k] = (float)T[k] * I[k];
}

// GL_LINEAR / GL_REPEAT fetch of a mesh texture at (u, v) in texture coordinates; out in 0..1 (the sampler's 8-bit result / 255).
// Any power-of-two size; storage is the padded (h+1) x (w+1) layout of the texel pool.
__device__ inline void mesh_texel(const RenderParams& R, int tex, float u, float v, float out[3]) {
  const TexDev td = R.tex[tex];
  const int xf = gl_fix(u * (float)td.w) - 128, yf = gl_fix(v * (float)td.h) - 128;
  const int x0 = (xf >> 8) & (td.w - 1), y0 = (yf >> 8) & (td.h - 1);
  const uint32_t* pt = R.texels + td.off + y0 * (td.w + 1) + x0;
  int T[3];
  gl_linear_rgb(pt[0], pt[1], pt[td.w + 1], pt[td.w + 2], xf & 255, yf & 255, T);
#pragma unroll
  for (int k = 0; k < 3; ++k) out[k] = (float)T[k] * (1.f / 255.f);
}

// z-buffer the `fill` staged triangles of the wavefront-local LDS chunk against the pixels of the
// lanes with `mine` set.  Two schedules, picked per call from a cost estimate (wave-uniform):
//   pixel-parallel    every `mine` lane collects the staged triangles whose box holds its pixel, then walks its own
//                     list (dense blocks: many pixels);
//   triangle-parallel for each `mine` pixel in turn, the 64 lanes test 64 staged triangles at once and
//                     the per-sample winners are reduced across the wavefront (a handful of pixels of a
//                     small / distant object, where the pixel-parallel loop would idle most lanes).
// Depth func LESS with the draw-order tie break, identical in both schedules.
#ifndef RO_PAIR_CAP
#define RO_PAIR_CAP 256                                  // pair slots per wavefront (16-bit entries)
#endif
#define RO_SCR_BYTES (64 * 4 * 8 + RO_PAIR_CAP * 2)       // per wavefront: sample keys + the pair list
__device__ inline void zbuffer_chunk(const TriCov* w_tris, uint32_t* w_scr, int fill, bool mine, int lane, float pcx, float pcy,
                                     float wbest[4], int tbest[4]) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const unsigned long long mm = __ballot(mine);
  const int n_mine = __popcll(mm);
  const int n_chunks = (fill + 63) >> 6;
  const bool tri_parallel = n_mine * (n_chunks * 110 + 110) < fill * 8 + 400;
  if (tri_parallel) {
    unsigned long long todo = mm;
    while (todo) {                                   // wave-uniform
      const int src = __builtin_ctzll(todo);
      todo &= todo - 1ull;
      const float qx = __shfl(pcx, src), qy = __shfl(pcy, src);
      float wb[4] = {0.f, 0.f, 0.f, 0.f};
      int tb[4] = {0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff};
      for (int k = lane; k < fill; k += 64) test_tri(w_tris[k], qx, qy, wb, tb);   // tb starts at "no triangle" = +inf: ties keep the lower index
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        float wmax = wb[s];
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) wmax = fmaxf(wmax, __shfl_xor(wmax, d));
        int tmin = (wb[s] == wmax && wmax > 0.f) ? tb[s] : 0x7fffffff;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) tmin = min(tmin, __shfl_xor(tmin, d));
        if (lane == src && tmin != 0x7fffffff && (wmax > wbest[s] || (wmax == wbest[s] && tmin < tbest[s]))) {
          wbest[s] = wmax; tbest[s] = tmin;
        }
      }
    }
  } else {
    // Pixel-parallel in two steps.  (1) Every lane tests its pixel against the screen boxes of all staged triangles
    // (one broadcast 16-byte LDS read + four compares each) and keeps the hits as a bit mask.  (2) Each lane walks
    // its own mask: the wavefront runs max-over-lanes(candidates) passes of the 4-sample test, with a different
    // triangle per lane.
    static_assert(TRI_CAP <= 128 && TRI_CAP % 32 == 0, "up to four 32-bit candidate masks");
    // Round 3: balanced.  Walking per-lane candidate masks costs max-over-lanes passes of the 4-sample test -- measured
    // 18 passes per call where the (pixel, triangle) pairs would fill 5.8 (profiles/r03_variants_ab.txt block G): the
    // pixels of a batch straddle the dense middle of an object and the empty corners of its box.  Instead (1) the box
    // test of each staged triangle appends its hits to a wavefront-local pair list (ballot + mbcnt: one 16-bit LDS
    // write per hit), (2) the list is drained 64 pairs at a time, every lane testing ITS pair, and the per-sample
    // winners meet in LDS as 64-bit keys (w bits : reversed triangle index) under ds_max_u64 -- LESS depth test with
    // the draw-order tie break, the same order relation as the register compare; (3) each pixel's lane reads its four
    // keys back.
    unsigned long long* zb = reinterpret_cast<unsigned long long*>(w_scr);                   // [64 pixels][4 samples]
    uint16_t* plist = reinterpret_cast<uint16_t*>(w_scr + 64 * 4 * 2);
#pragma unroll
    for (int q = 0; q < 4; ++q) zb[lane * 4 + q] = 0ull;
    int base = 0;
    auto drain = [&]() {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      for (int q0 = 0; q0 < base; q0 += 64) {          // wave-uniform
        const bool act = q0 + lane < base;
        const uint32_t pr = act ? plist[q0 + lane] : 0u;
        const int src = pr & 63;
        const float qx = __shfl(pcx, src), qy = __shfl(pcy, src);
        if (act) {
          const TriCov& st = w_tris[pr >> 6];
          const auto &ox = MSAA_POS.x, &oy = MSAA_POS.y;
          const float ia = st.inv_area;
          const float e0x = st.sx[0] - qx, e0y = st.sy[0] - qy, e1x = st.sx[1] - qx, e1y = st.sy[1] - qy, e2x = st.sx[2] - qx, e2y = st.sy[2] - qy;
          const float b0c = (e1x * e2y - e2x * e1y) * ia, b1c = (e2x * e0y - e0x * e2y) * ia;
          const float g0x = (e1y - e2y) * ia, g0y = (e2x - e1x) * ia, g1x = (e2y - e0y) * ia, g1y = (e0x - e2x) * ia;
          const float d0 = st.iw[0] - st.iw[2], d1 = st.iw[1] - st.iw[2];
          const float wc = fmaf(b1c, d1, fmaf(b0c, d0, st.iw[2]));
          const float gwx = fmaf(g1x, d1, g0x * d0), gwy = fmaf(g1y, d1, g0y * d0);
          const uint32_t rix = 0x7fffffffu - (uint32_t)st.index;
#pragma unroll
          for (int q = 0; q < 4; ++q) {                  // the arithmetic of test_tri_inside, term for term
            const float b0 = fmaf(g0y, oy[q], fmaf(g0x, ox[q], b0c));
            const float b1 = fmaf(g1y, oy[q], fmaf(g1x, ox[q], b1c));
            const float b2 = 1.f - b0 - b1;
            const float w = fmaf(gwy, oy[q], fmaf(gwx, ox[q], wc));
            const bool in = fminf(fminf(b0, b1), b2) >= 0.f && w <= 1.f / NEAR_Z && w >= 1.f / FAR_Z;
            if (in) atomicMax(zb + src * 4 + q, ((unsigned long long)__float_as_uint(w) << 32) | rix);
          }
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    for (int jj = 0; jj < fill; ++jj) {                // wave-uniform
      const int j = jj;
      const float4 bb = *reinterpret_cast<const float4*>(&w_tris[j]);              // bx0, bx1, by0, by1
      // four compares straight into scalar masks, ANDed on the scalar unit (as one bool expression the compiler builds the
      // conjunction out of 0 / 1 integers: 17 vector instructions instead of 4)
      const unsigned long long m = mm & __ballot(pcx >= bb.x) & __ballot(pcx <= bb.y) & __ballot(pcy >= bb.z) & __ballot(pcy <= bb.w);
      if (!m) continue;
      if (__builtin_amdgcn_inverse_ballot_w64(m))
        plist[base + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = (uint16_t)((j << 6) | lane);
      base += __popcll(m);
      if (base > RO_PAIR_CAP - 64) { drain(); base = 0; }
    }
    if (base) drain();
    if (mine) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const unsigned long long k = zb[lane * 4 + q];
        const float w = __uint_as_float((uint32_t)(k >> 32));
        const int ix = (int)(0x7fffffffu - (uint32_t)k);
        if (k != 0ull && (w > wbest[q] || (w == wbest[q] && ix < tbest[q]))) { wbest[q] = w; tbest[q] = ix; }
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// exact 4-sample resolve of one pixel (centre NDC nx, ny): coverage and depth per sample,
// shading once per primitive at the pixel centre; zbest/tbest = 1 / depth and index of the nearest mesh triangle per
// sample (from the mesh pass; tbest < 0: none), z-buffered against the planes here.
template <bool OBJ>
__device__ inline uint32_t shade_msaa(const EnvCam& c, const MapU& m, const RenderParams& R,
                                      const TileLds* tiles, float nx, float ny, const ScreenTri* tris,
                                      const float zbest[4], const int tbest[4]) {
  const auto &ox = MSAA_POS.x, &oy = MSAA_POS.y;
  const float sxn = 2.f / (float)R.W, syn = 2.f / (float)R.H;
  const Ray rc = make_ray(nx, ny, c.tx, c.ty, c.sth, c.cth);
  // 1. coverage: which primitive owns each sample.  key: 0 sky, 1 ground, 2|tj<<2|ti<<14 tile,
  //    3|tri<<2 mesh triangle (depth func LESS against the plane hit).
  uint32_t key[4];
  int n_sky = 0, n_gnd = 0;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const Ray rs = make_ray(nx + ox[s] * sxn, ny - oy[s] * syn, c.tx, c.ty, c.sth, c.cth);
    const Hit hs = classify(c, m, tiles, rs);
    const float zplane = hs.cls == CLS_SKY ? 3.0e38f : hs.t;
    if (OBJ && tbest[s] >= 0 && 1.f / zbest[s] < zplane) key[s] = 3u | ((uint32_t)tbest[s] << 2);   // zbest holds w = 1 / depth
    else if (hs.cls == CLS_TILE) key[s] = 2u | ((uint32_t)hs.tj << 2) | ((uint32_t)hs.ti << 14);
    else { key[s] = (uint32_t)hs.cls; n_sky += hs.cls == CLS_SKY; n_gnd += hs.cls == CLS_GROUND; }
  }
  // 2. shading: once per primitive, at the pixel centre, weighted by its sample count.  Sky and the
  //    ground quad are single primitives; tiles / triangles are walked as a list of distinct keys so
  //    that a wavefront runs max-over-lanes(distinct) passes of the expensive code, not one per sample.
  float acc[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) acc[k] = (float)n_sky * c.hor[k];
  if (n_gnd > 0) {
    float t = 0.f, wx = 0.f, wz = 0.f;
    plane_hit(c, rc, c.Cy - GROUND_Y, t, wx, wz);    // centre ray extrapolates when it misses (yla >= 0: t < 0)
    if (!(rc.yla < 0.f)) {                           // oracle: keep the sample's own hit in that case
#pragma unroll
      for (int s = 3; s >= 0; --s)
        if (key[s] == 1u) {
          const Ray rs = make_ray(nx + ox[s] * sxn, ny - oy[s] * syn, c.tx, c.ty, c.sth, c.cth);
          plane_hit(c, rs, c.Cy - GROUND_Y, t, wx, wz);
        }
    }
    const float ndl = ground_ndl(c, wx, wz);
#pragma unroll
    for (int k = 0; k < 3; ++k) acc[k] += (float)n_gnd * (c.gnd[k] * fminf(c.base[k] + c.dif[k] * ndl, 1.f));
  }
  uint32_t todo = 0;
#pragma unroll
  for (int s = 0; s < 4; ++s) todo |= (key[s] & 3u) >= 2u ? (1u << s) : 0u;
  float tI[3] = {0.f, 0.f, 0.f}, twx = 0.f, twz = 0.f;
  bool have_tile_lit = false;
  while (todo) {
    const int s0 = __builtin_ctz(todo);
    const uint32_t k0 = s0 == 0 ? key[0] : s0 == 1 ? key[1] : s0 == 2 ? key[2] : key[3];
    int cnt = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) { const bool same = ((todo >> s) & 1u) && key[s] == k0; cnt += same; todo &= same ? ~(1u << s) : ~0u; }
    float col[3];
    if ((k0 & 3u) == 2u) {
      if (!have_tile_lit) {                          // tile-plane hit and light of the centre ray: shared by all tiles
        float t = 0.f;
        if (rc.yla < 0.f) plane_hit(c, rc, c.Cy, t, twx, twz);
        else {                                       // centre ray misses the plane: the sample's own hit (first tile sample)
          const int sf = s0;
          const Ray rs = make_ray(nx + ox[sf] * sxn, ny - oy[sf] * syn, c.tx, c.ty, c.sth, c.cth);
          plane_hit(c, rs, c.Cy, t, twx, twz);
        }
        const float ndl = plane_ndl(c.L, c.sth, c.cth, rc, t);
#pragma unroll
        for (int k = 0; k < 3; ++k) tI[k] = fminf(c.base[k] + c.dif[k] * ndl, 1.f);
        have_tile_lit = true;
      }
      const int tj = (int)((k0 >> 2) & 4095u), ti = (int)(k0 >> 14);
      const float fx = twx * m.its - (float)ti, fz = twz * m.its - (float)tj;
      tile_color(R, tiles[m.tile_off + tj * m.gw + ti], fx, fz, tI, col);
    } else if (OBJ) {
      const ScreenTri& st = tris[k0 >> 2];
      float pcx, pcy;                                     // pixel centre, px
      src_px(nx, ny, R.W, R.H, pcx, pcy);
      const float b0 = ((st.sx[1] - pcx) * (st.sy[2] - pcy) - (st.sx[2] - pcx) * (st.sy[1] - pcy)) * st.inv_area;
      const float b1 = ((st.sx[2] - pcx) * (st.sy[0] - pcy) - (st.sx[0] - pcx) * (st.sy[2] - pcy)) * st.inv_area;
      const float b2 = 1.f - b0 - b1;
      const float inv = 1.f / (b0 * st.iw[0] + b1 * st.iw[1] + b2 * st.iw[2]);
      float tx[3] = {1.f, 1.f, 1.f};                   // GL_MODULATE with the chunk's texture (objmesh.py:360-375)
      if (st.tex >= 0) {
        const float u = (b0 * st.uw[0] + b1 * st.uw[1] + b2 * st.uw[2]) * inv;
        const float v = (b0 * st.vw[0] + b1 * st.vw[1] + b2 * st.vw[2]) * inv;
        mesh_texel(R, st.tex, u == u ? u : 0.f, v == v ? v : 0.f, tx);
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float v = (b0 * st.cw[0][k] + b1 * st.cw[1][k] + b2 * st.cw[2][k]) * inv;
        col[k] = fminf(fmaxf(v == v ? v : 0.f, 0.f), 255.f) * tx[k];
      }
    } else { col[0] = col[1] = col[2] = 0.f; }
#pragma unroll
    for (int k = 0; k < 3; ++k) acc[k] += (float)cnt * col[k];
  }
  const float o[3] = {0.25f * acc[0], 0.25f * acc[1], 0.25f * acc[2]};
  return pack_rgb(o);
}

// Exact 4-sample resolve of the queued edge pixels, stream-ordered after k_raster so the byte patches
// land after the fast-path stores.  Persistent wavefronts pull work items (ITEM_B consecutive 64-entry
// batches of one raster workgroup's four queue regions) from the global list k_raster appended to.
#ifndef DT_RES_WAVES
#define DT_RES_WAVES 5             // wavefronts per SIMD k_resolve is compiled for (90 VGPRs)
#endif
__global__ __launch_bounds__(RB) __attribute__((amdgpu_waves_per_eu(DT_RES_WAVES, DT_RES_WAVES))) void k_resolve(RenderParams R, const EnvCam* __restrict__ cams,
                                                const uint16_t* __restrict__ queue, const int32_t* __restrict__ qcount) {
  extern __shared__ uint32_t s_mem[];
  TileLds* s_tiles = reinterpret_cast<TileLds*>(s_mem);
  const int tid = threadIdx.x;
  const int npix = R.W * R.H;
  const int tiles_x = (R.W + DT_TILE_W - 1) / DT_TILE_W, n_tiles = tiles_x * ((R.H + DT_TILE_H - 1) / DT_TILE_H);
  const int wave = tid >> 6, lane = tid & 63;
  fill_tile_recs(R, s_mem, tid);
  __syncthreads();
  uint32_t* s_wave = s_mem + R.n_tile_recs * (sizeof(TileLds) / 4);
  EnvCam* w_cams = reinterpret_cast<EnvCam*>(s_wave) + wave * ENVS_PER_BLOCK;                    // wavefront-local
  const int n_items = R.work[DT_WORK_ITEMS];         // written by the raster launch
  const int n_grabs = work_n_grabs(n_items);
  bool first_grab = true;
  while (true) {
    int g = wave * (int)gridDim.x + (int)blockIdx.x;
    if (!first_grab) g = work_next_grab(R, DT_WORK_CURSOR, g, lane);
    first_grab = false;
    if (g >= n_grabs) break;
    for (int it = g; it < n_items; it += n_grabs) {  // wave-uniform
      const uint32_t item = R.items[it];
      const int rwg = (int)(item / ITEMS_PER_WG), part = (int)(item % ITEMS_PER_WG);
      const int tile = rwg % n_tiles, chunk = rwg / n_tiles;
      const int e0 = chunk * ENVS_PER_BLOCK;
      {  // the chunk's EnvCams -> wavefront-private LDS (64 bytes per lane; DS ops of one wavefront are ordered)
        static_assert((ENVS_PER_BLOCK * sizeof(EnvCam)) % (64 * 64) == 0, "whole 64-byte slices per lane");
        constexpr int SL = (int)(ENVS_PER_BLOCK * sizeof(EnvCam) / (64 * 64));   // 64-byte slices per lane
        const int ne = min(ENVS_PER_BLOCK, R.N - e0);
#pragma unroll
        for (int sl = 0; sl < SL; ++sl) {
          const int o = (sl * 64 + lane) * 4;          // uint4 index of the slice
          const uint4* src = reinterpret_cast<const uint4*>(cams + e0) + o;
          uint4* dst = reinterpret_cast<uint4*>(w_cams) + o;
          if (o * 16 < ne * (int)sizeof(EnvCam)) { dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2]; dst[3] = src[3]; }
        }
      }
      const int tile_x0 = (tile % tiles_x) * DT_TILE_W, tile_y0 = (tile / tiles_x) * DT_TILE_H;
      static_assert(RB / 64 == 4, "region lookup assumes 4 wavefronts");
      int rn[4], rb[5];
      rb[0] = 0;
#pragma unroll
      for (int r = 0; r < 4; ++r) { rn[r] = qcount[rwg * 4 + r]; rb[r + 1] = rb[r] + ((rn[r] + 63) >> 6); }
      const int b_end = min(rb[4], (part + 1) * ITEM_B);
      for (int b = part * ITEM_B; b < b_end; ++b) {  // wave-uniform
        const int reg = (b >= rb[1]) + (b >= rb[2]) + (b >= rb[3]);
        const int q0 = (b - (reg == 0 ? rb[0] : reg == 1 ? rb[1] : reg == 2 ? rb[2] : rb[3])) * 64;
        const int n = reg == 0 ? rn[0] : reg == 1 ? rn[1] : reg == 2 ? rn[2] : rn[3];
        const uint16_t* w_queue = queue + ((size_t)rwg * 4 + reg) * QREGION;
        const int wave_y0 = tile_y0 + reg * (WAVE_PIX / WAVE_W);
        const bool have = q0 + lane < n;
        const uint32_t ent = have ? w_queue[q0 + lane] : 0u;
        const int el = have ? (int)(ent >> 8) : -1, lp = qe_pixel(ent);
        const int pix = (wave_y0 + lp / WAVE_W) * R.W + tile_x0 + lp % WAVE_W;      // entries only exist for in-image pixels
        const float4 l = reinterpret_cast<const float4*>(R.lut)[pix];
        if (have) {
          const float wb[4] = {0.f, 0.f, 0.f, 0.f};
          const int tb[4] = {-1, -1, -1, -1};
          const EnvCam c = w_cams[el];
          const MapU m = map_u(R.maps[c.map_id]);
          const uint32_t v = shade_msaa<false>(c, m, R, s_tiles, l.x, l.y, nullptr, wb, tb);
          // three byte stores, here and in k_resolve_obj: another memory pattern than store_rgb (the quad-record exact paths'), kept as tuned
          uint8_t* dst = R.frames + ((size_t)(e0 + el) * npix + pix) * 3;
          dst[0] = (uint8_t)v; dst[1] = (uint8_t)(v >> 8); dst[2] = (uint8_t)(v >> 16);
        }
      }
    }
  }
}

// Exact path of the pixels inside mesh-object screen boxes (the entries every raster appends from the far end of its queue regions).
// Work unit = (raster tile, env): the entries one env left in the four wavefront regions of a raster workgroup are taken
// together, up to NB 64-entry batches at a time, so that the env's triangles are streamed, culled and staged ONCE for
// the 128 x 8 pixels of the tile instead of once per 128 x 2 block (the round-1 kernel: one pass per
// (batch, env) pair, ~45 pairs per env and frame).  The raster records the queue fill of every region after every env
// (qend), so a unit's entries are four contiguous ranges; a work item covers RES_ENVS consecutive env positions of a chunk.
#ifndef DT_RES_NB
#define DT_RES_NB 2
#endif
#ifndef DT_RO_WAVES
#define DT_RO_WAVES 4              // wavefronts per SIMD the kernel is compiled for (142 VGPRs at 3; 4 caps it at 128)
#endif
template <int NB>
__global__ __launch_bounds__(RB) __attribute__((amdgpu_waves_per_eu(DT_RO_WAVES, DT_RO_WAVES))) void k_resolve_obj(RenderParams R, const EnvCam* __restrict__ cams, const uint16_t* __restrict__ queue,
                                                    const EnvQ* __restrict__ envq) {
  extern __shared__ uint32_t s_mem[];
  TileLds* s_tiles = reinterpret_cast<TileLds*>(s_mem);
  const int tid = threadIdx.x;
  const int npix = R.W * R.H;
  const int tiles_x = (R.W + DT_TILE_W - 1) / DT_TILE_W, n_tiles = tiles_x * ((R.H + DT_TILE_H - 1) / DT_TILE_H);
  const int wave = tid >> 6, lane = tid & 63;
  fill_tile_recs(R, s_mem, tid);
  __syncthreads();
  uint32_t* s_wave = s_mem + R.n_tile_recs * (sizeof(TileLds) / 4);
  static_assert(RES_ENVS == 1, "a work item is ONE (raster tile, env) unit: everything about it is wave-uniform");
  TriCov* w_tris = reinterpret_cast<TriCov*>(s_wave) + wave * TRI_CAP;                             // wavefront-local
  uint32_t* w_scr = reinterpret_cast<uint32_t*>(reinterpret_cast<TriCov*>(s_wave) + (RB / 64) * TRI_CAP) + wave * (RO_SCR_BYTES / 4);   // z-buffer scratch of the pair schedule
  const int n_front = R.work[DT_WORK_OBJ_FRONT], n_items = n_front + R.work[DT_WORK_OBJ_BACK];   // written by the raster launch (push_obj_items): heavy items first
  const size_t items_cap = obj_items_cap(R);
  auto item_at = [&](int i) -> uint32_t { return R.items2[i < n_front ? (size_t)i : items_cap - 1 - (size_t)(i - n_front)]; };
  const int n_grabs = work_n_grabs(n_items);
  bool first_grab = true;
  while (true) {
    int g = wave * (int)gridDim.x + (int)blockIdx.x;
    if (!first_grab) g = work_next_grab(R, DT_WORK_OBJ_CURSOR, g, lane);
    first_grab = false;
    if (g >= n_grabs) break;
    // The item loop is software-pipelined: everything a unit needs before it can touch its entries -- the id of the item after next, and for
    // the NEXT item its four entry ranges (the fills of the regions after env p and after env p - 1: eight 16-bit loads on eight lanes), the
    // frame index of its position and the object masks of its four blocks -- is loaded while the current unit is processed.  Round 5: a
    // unit is one env, so all of this is wave-uniform; the per-item staging of 32 envs' fills, 32 envs' masks and the EnvCam copy through
    // LDS (with its barrier) are gone: that chain of dependent round trips was ~ 280 of the kernel's 600 us (profiles/r05_variants_ab.txt, block H).
    static_assert(RB / 64 == 4, "four regions per raster workgroup");
    auto prefetch = [&](const uint32_t item_, uint32_t& qv, int& ev, unsigned long long& hv) {
      const int rwg_ = (int)(item_ / ITEMS_PER_WG), p_ = (int)(item_ % ITEMS_PER_WG);
      const int tile_ = rwg_ % n_tiles, pos_ = min((rwg_ / n_tiles) * ENVS_PER_BLOCK + p_, R.N - 1);
      qv = 0u;                                          // lane 2r: fill of region r after env p, lane 2r + 1: after env p - 1 (= where p's entries start)
      if (lane < 8) { const int pp = p_ - (lane & 1); if (pp >= 0) qv = R.qend[((size_t)rwg_ * 4 + (lane >> 1)) * ENVS_PER_BLOCK + pp]; }
      ev = envq ? (int)envq[pos_].env : pos_;           // position in the render order -> env (one address for the wavefront)
      hv = 0ull;
      if (lane < 4) hv = R.objmask[((size_t)pos_ * n_tiles + tile_) * 4 + lane];
    };
    uint32_t item_cur = item_at(g), item_nxt = g + n_grabs < n_items ? item_at(g + n_grabs) : 0u;
    uint32_t qv_nxt; int ev_nxt; unsigned long long hv_nxt;
    prefetch(item_cur, qv_nxt, ev_nxt, hv_nxt);
    for (int it = g; it < n_items; it += n_grabs) {  // wave-uniform
      const uint32_t item = item_cur;
      const uint32_t qv = qv_nxt;
      const int ev = ev_nxt;
      const unsigned long long hv = hv_nxt;
      item_cur = item_nxt;
      if (it + n_grabs < n_items) prefetch(item_cur, qv_nxt, ev_nxt, hv_nxt);
      item_nxt = it + 2 * n_grabs < n_items ? item_at(it + 2 * n_grabs) : 0u;
      const int rwg = (int)(item / ITEMS_PER_WG), p0 = (int)(item % ITEMS_PER_WG);
      const int tile = rwg % n_tiles, chunk = rwg / n_tiles;
      const int e0 = chunk * ENVS_PER_BLOCK;
      const int ne = min(ENVS_PER_BLOCK, R.N - e0);
      if (p0 >= ne) continue;
      const int tile_x0 = (tile % tiles_x) * DT_TILE_W, tile_y0 = (tile / tiles_x) * DT_TILE_H;
      {                                                // the (tile, env) unit
        const int p = p0;
        int c_[4], s_[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) { s_[r] = __builtin_amdgcn_readlane((int)qv, 2 * r + 1); c_[r] = __builtin_amdgcn_readlane((int)qv, 2 * r) - s_[r]; }
        const int t1 = c_[0], t2 = t1 + c_[1], t3 = t2 + c_[2], n_p = t3 + c_[3];
        if (n_p == 0) continue;
        unsigned long long hm0 = 0ull;                 // OR of the four blocks' masks: the unit spans the whole raster tile
#pragma unroll
        for (int r = 0; r < 4; ++r)
          hm0 |= ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(hv >> 32), r) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)hv, r);
        const int env_p = __builtin_amdgcn_readfirstlane(ev);
        const EnvCam& c = cams[env_p];                 // wave-uniform address: scalar loads where the fields are used
        (void)p;
        const MapU m = map_u(R.maps[c.map_id]);
        const ScreenTri* base = R.stris + (size_t)env_p * R.max_tris;
        const uint2* rng = R.objrange + (size_t)__builtin_amdgcn_readfirstlane(c.map_id) * DTSIM_MAX_OBJECTS;
        for (int g0 = 0; g0 < n_p; g0 += 64 * NB) {   // wave-uniform: up to NB batches of the unit at a time
          bool have[NB], pedge[NB];
          int pix[NB];
          float nxv[NB], nyv[NB];
          float zbest[NB][4];
          int tbest[NB][4];
          float x0 = 1e30f, x1 = -1e30f, y0 = 1e30f, y1 = -1e30f;
#pragma unroll
          for (int j = 0; j < NB; ++j) {
            const int idx = g0 + j * 64 + lane;
            have[j] = idx < n_p;
            const int r = (idx >= t1) + (idx >= t2) + (idx >= t3);
            const int li = idx - (r == 0 ? 0 : r == 1 ? t1 : r == 2 ? t2 : t3) + (r == 0 ? s_[0] : r == 1 ? s_[1] : r == 2 ? s_[2] : s_[3]);
            const uint16_t* w_queue = queue + ((size_t)rwg * 4 + r) * QREGION;
            const uint32_t ent = have[j] ? w_queue[QREGION - 1 - li] : 0u;   // appended from the far end of the region
            pedge[j] = qe_plane_edge(ent);
            const int lp = qe_pixel(ent);
            pix[j] = (tile_y0 + r * (WAVE_PIX / WAVE_W) + lp / WAVE_W) * R.W + tile_x0 + lp % WAVE_W;   // entries only exist for in-image pixels
            if (!have[j]) pix[j] = 0;
            const float4 l = reinterpret_cast<const float4*>(R.lut)[pix[j]];
            nxv[j] = l.x; nyv[j] = l.y;
            float pcx, pcy;
            src_px(l.x, l.y, R.W, R.H, pcx, pcy);
            if (have[j]) { x0 = fminf(x0, pcx); x1 = fmaxf(x1, pcx); y0 = fminf(y0, pcy); y1 = fmaxf(y1, pcy); }
#pragma unroll
            for (int q = 0; q < 4; ++q) { zbest[j][q] = 0.f; tbest[j][q] = -1; }   // w = 1 / depth: 0 = nothing yet
          }
          unsigned long long hm = hm0;
          if (hm) {
            // ---- mesh pass: stream the triangles of the objects whose screen box meets the tile, 64 at a time (one per
            // lane, coverage half only), keep those whose box meets the bounding box of the unit's pixels, compact them
            // into the wavefront-local LDS chunk and z-buffer the chunk against every batch of the group.
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) {
              x0 = fminf(x0, __shfl_xor(x0, d)); x1 = fmaxf(x1, __shfl_xor(x1, d));
              y0 = fminf(y0, __shfl_xor(y0, d)); y1 = fmaxf(y1, __shfl_xor(y1, d));
            }
            int first = 0, count = 0, t0 = 0;
            auto advance = [&]() -> bool {             // wave-uniform: next (object, t0); false when exhausted
              t0 += 64;
              while (t0 >= count) {
                if (!hm) return false;
                const uint2 fc = rng[__builtin_ctzll(hm)];
                hm &= hm - 1ull;
                first = (int)fc.x; count = (int)fc.y; t0 = 0;
              }
              return true;
            };
            // Round 3: the cull reads the triangles' screen boxes from their own contiguous array (16 B per triangle, written by
            // k_obj_setup) and only the survivors load their 64-byte coverage record: the stream used to touch one 128-byte
            // line per triangle for every (tile, env) unit an object's box meets.
            const float4* boxes = R.tribox + (size_t)env_p * R.max_tris;
            auto fetch = [&](float4& bb, int& idx) -> bool {     // this lane's triangle of the current chunk: box + index
              const bool in = t0 + lane < count;
              idx = first + t0 + lane;
              if (in) bb = boxes[idx];
              return in;
            };
            int fill = 0;
            float4 cur = make_float4(0.f, 0.f, 0.f, 0.f), nxt = cur;
            int cur_idx = 0, nxt_idx = 0;
            bool more = advance();
            bool cur_in = more ? fetch(cur, cur_idx) : false;
            while (more) {
              const bool has_next = advance();
              const bool nxt_in = has_next ? fetch(nxt, nxt_idx) : false;
              const bool pass = cur_in && !(cur.x > x1 || cur.y < x0 || cur.z > y1 || cur.w < y0);
              const unsigned long long pm = __ballot(pass);
              if (pass) w_tris[fill + __popcll(pm & ((1ull << lane) - 1ull))] = *reinterpret_cast<const TriCov*>(base + cur_idx);
              fill += __popcll(pm);
              if (fill > TRI_CAP - 64 || (!has_next && fill > 0)) {   // chunk full, or the last one: z-buffer it
#pragma unroll
                for (int j = 0; j < NB; ++j) {
                  if (j > 0 && g0 + j * 64 >= n_p) break;            // wave-uniform
                  float pcx, pcy;
                  src_px(nxv[j], nyv[j], R.W, R.H, pcx, pcy);
                  zbuffer_chunk(w_tris, w_scr, fill, have[j], lane, pcx, pcy, zbest[j], tbest[j]);
                }
                fill = 0;
              }
              cur = nxt; cur_idx = nxt_idx; cur_in = nxt_in; more = has_next;
            }
          }
#pragma unroll
          for (int j = 0; j < NB; ++j) {
            if (j > 0 && g0 + j * 64 >= n_p) break;                  // wave-uniform
            // a pixel no mesh triangle covers, and that is no plane edge either, already holds its colour (the raster's)
            have[j] = have[j] && (pedge[j] || (tbest[j][0] & tbest[j][1] & tbest[j][2] & tbest[j][3]) >= 0);   // all four < 0  <=>  the AND is negative
            if (!__ballot(have[j])) continue;                        // wave-uniform: nothing of this batch needs shading
            if (have[j]) {
              const uint32_t v = shade_msaa<true>(c, m, R, s_tiles, nxv[j], nyv[j], base, zbest[j], tbest[j]);
              uint8_t* dst = R.frames + ((size_t)env_p * npix + pix[j]) * 3;
              dst[0] = (uint8_t)v; dst[1] = (uint8_t)(v >> 8); dst[2] = (uint8_t)(v >> 16);
            }
          }
        }
      }
    }
  }
}

}  // namespace

// The exact-path kernels after raster `pipe`, on stream s.  Quad pipelines: the plane-edge pixels were resolved inside the raster
// (resolve_region_q, resolve_region_v3); generic raster: k_resolve drains them (front of the queue regions).  Pixels inside mesh-object
// screen boxes (far end of the regions) are k_resolve_obj's, after any raster; has_pos: the pass ran in k_env_sort's order (its positions
// become envs through EnvQ.env).
void dt_launch_render_exact(hipStream_t s, const RenderParams& R, const EnvRecs& x, int pipe, bool has_pos) {
  const bool obj = R.max_tris > 0, quad = pipe == DTSIM_PIPE_V3 || pipe == DTSIM_PIPE_Q;
  const size_t lds = (size_t)R.n_tile_recs * sizeof(TileLds);               // the tile records (fill_tile_recs)
  const size_t lds2 = lds + (size_t)(RB / 64) * ENVS_PER_BLOCK * sizeof(EnvCam);   // + the wavefronts' EnvCam chunks
  const dim3 grid((unsigned)(dt_raster_tiles(R.W, R.H) * ((R.N + ENVS_PER_BLOCK - 1) / ENVS_PER_BLOCK)));   // the raster's workgroups: never more than these
  // persistent wavefronts pulling work items: enough workgroups to fill every CU at the kernel's occupancy
  // (round 4: EXACTLY the resident workgroups -- every wavefront's first grab is static, a workgroup that waits for a slot would sit on its items)
  if (!quad && pipe != DTSIM_PIPE_V3DR) {            // (k_raster_v3dr's plane-edge pixels: k_resolve_dr, launched with it)
    const dim3 rgrid((unsigned)std::min<size_t>(grid.x, resident_blocks(k_resolve, lds2)));
    hipLaunchKernelGGL(k_resolve, rgrid, dim3(RB), lds2, s, R, x.cams, R.queue, R.qcount);
  }
  if (obj) {
    const size_t lds4 = lds + (size_t)(RB / 64) * TRI_CAP * sizeof(TriCov) + (size_t)(RB / 64) * RO_SCR_BYTES;
    const dim3 rgrid((unsigned)std::min<size_t>(grid.x, resident_blocks(k_resolve_obj<DT_RES_NB>, lds4)));
    hipLaunchKernelGGL(k_resolve_obj<DT_RES_NB>, rgrid, dim3(RB), lds4, s, R, x.cams, R.queue, has_pos ? x.envq : (const EnvQ*)nullptr);
  }
}
