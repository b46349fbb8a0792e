// render.hip -- Simulator.render_obs as a forward per-pixel raster for gfx950.
//
// Replaces simulator.py:1707-1951 (_render_img: fixed-function GL into a 4xMSAA FBO,
// glReadPixels, flip) and distortion.py:85-125 (cv2.remap INTER_NEAREST through the
// inverted rectify map).  Render spec: SURVEY.md Appendix B / DESIGN.md "Render spec";
// the CPU statement of the same spec is oracle/raster.py.
//
// Structure
//   k_raster<DR,OBJ>: workgroup = 4 independent wavefronts owning a DT_TILE_W x DT_TILE_H = 128 x 8 pixel
//                 tile of the frame (wavefront w: rows 2w, 2w+1; lane l: columns l and l+64 of each row), looping over
//                 ENVS_PER_BLOCK envs.  Adjacent lanes are adjacent pixels, so one texel-load
//                 instruction touches neighbouring texture lines (TA coalescing) and the tile's
//                 2-D texture footprint stays in L1.  Everything that does not depend on the env
//                 -- the LUT entry of each pixel (NDC of the rectilinear source pixel: the
//                 fisheye remap is folded into the ray set-up, there is no second pass) and, for
//                 the shared camera (DR=false), the whole ray / tile-plane intersection in the
//                 yaw-local frame, the light term and the MSAA edge margin -- is computed once
//                 and kept in REGISTERS across the env loop; per env only the 64-B EnvFast
//                 changes (one wave-uniform scalar load) and a pixel costs one 2-D rotation +
//                 tile lookup (LDS) + one bilinear fetch (two 8-byte loads from the L2-resident
//                 padded texture, llvmpipe's integer GL_LINEAR: gl_linear_rgb), times the lit factor.
//                 MSAA: pixels whose 4 samples may see different primitives (horizon, map
//                 border, tile seams, mesh boxes; conservative test) are appended (ballot +
//                 mbcnt, no atomics) to a per-wavefront global queue region.
//                 Output: px -> wavefront-private LDS transpose -> 12 B (4 px) per lane, three
//                 dword stores, 384 contiguous bytes per tile row.
//   k_raster_q<OBJ,S256> (shared camera, square power-of-two tile textures): quad-record one-ray path +
//                 the exact path of plane-edge pixels inside the same wavefronts (resolve_region_q).
//   Host side: dt_render_layout lays out the render scratch (per-env records, per-pixel tables, queues, work lists); dt_raster_pipe picks the
//                 raster; dt_launch_render runs a pass: the setup kernels, the pipe's raster, the exact-path kernels, on one stream.
//   The pass's other units:
//     render_setup.hip  what a raster reads: k_env_sort (render order), k_cam_setup (EnvCam .. EnvD), k_blk_setup / k_obj_setup (mesh objects),
//                       k_pix_setup (PixTab, SampTab); dt_launch_render_setup.
//     render_v3.hip     k_raster_v3<OBJ> (256 x 256 tile textures, the BASELINE configurations): k_raster_q on an instruction diet, the headline
//                       kernel; k_raster_v3dr<OBJ>: domain randomisation on the same records, with its exact path k_resolve_dr.
//     render_exact.hip  what patches pixels after a raster: k_resolve (the plane-edge pixels the generic k_raster queued), k_resolve_obj (the
//                       pixels inside mesh-object screen boxes, after any raster); dt_launch_render_exact.
//     render_views.hip  every kernel that reads what a pass leaves behind (overlays, depth, labels / instances, bird's-eye map, ground projection).
//   Headers: raster_common.h -- what two or more of these units use (work decomposition, queue entries and work lists, the rasters' and the exact
//                 paths' scaffolding, pix_inv, both filters); render_records.h -- every record one stage writes and another reads, typed;
//                 render_scene.h -- the planes and classify(), test_tri, MSAA_POS, src_px: shared with render_views.hip.
//
// Roofline: algorithmic bytes per env-step = W*H*3 (921 600 B at 640x480), written once (+ the ~1.3 % edge
// pixels a second time); LUT / textures / tables are shared by all envs and stay in registers / LDS / L2.
// Measured (profiles/): the pass is co-limited by vector issue and the texture path's cache-line rate -- 31.1 vector instructions per
// pixel (round 1: 64.8; round 5: 36.9), 12 lines per record gather, vector ALUs 82 % and texture unit 73 % busy -- at 31.5 - 32.3 % of the HBM roofline; float32 geometry, byte-weight
// filter at the precision GL's own GL_LINEAR has on the reference's renderer, uint8 output.
// Parity: every pipeline is held to frames the unmodified reference rendered on Mesa llvmpipe (tests/test_gpu_gl_golden.py).
#include "raster_common.h"

namespace {

// Per-env camera (domain randomisation): the same quantities per (pixel, env), with everything that only depends on
// the env folded into DrCam once per env, and the MSAA reach as a cheaper upper bound -- kappa = rho / (1 - rho) <=
// rho + (4/3) rho^2 for rho <= 1/4 (beyond that the pixel takes the exact path anyway), and both sample-offset terms of
// pix_inv are bounded by (ax + ry)^2 + fy^2.  A larger reach only sends more pixels to the exact path.
struct DrCam { float tx, ty, a1, a2, sth, cth, Cy, dy, cex, eys, kgc, ndl_dir; bool directional; };

__device__ inline DrCam dr_cam(const EnvCam& c, float ex_n, float ey_n) {
  DrCam d;
  d.tx = c.tx; d.ty = c.ty; d.a1 = c.ty * c.cth; d.a2 = c.ty * c.sth; d.sth = c.sth; d.cth = c.cth; d.Cy = c.Cy;
  const float ey = ey_n * c.ty;
  d.dy = ey * fabsf(c.cth); d.cex = ex_n * c.tx; d.eys = ey * fabsf(c.sth);
  d.kgc = (c.Cy - GROUND_Y) / c.Cy;
  d.directional = c.L[3] == 0.f;
  d.ndl_dir = fmaxf(c.cth * c.L[1] + c.sth * c.L[2], 0.f);
  return d;
}

__device__ inline PixInv pix_inv_dr(float nx, float ny, bool valid, const DrCam& d, const float L[4]) {
  PixInv p;
  p.flags = valid ? PF_VALID : 0u;
  p.lr = p.lf = p.ndl = p.mrg = 0.f;
  const float xe = nx * d.tx, yla = fmaf(ny, d.a1, -d.sth), fwd = fmaf(ny, d.a2, d.cth);
  if (!(yla < 0.f)) {
    p.flags |= (yla - d.dy >= 0.f) ? PF_SKY : PF_ALWAYS_EDGE;
    return p;
  }
  const float inv = frcp(-yla);
  const float t = d.Cy * inv;
  p.lr = t * xe; p.lf = t * fwd;
  if (d.directional) p.ndl = d.ndl_dir;             // wave-uniform: the DR light is a direction (simulator.py:565-584)
  else { Ray r; r.xe = xe; r.ye = ny * d.ty; r.yla = yla; r.fwd = fwd; p.ndl = plane_ndl(L, d.sth, d.cth, r, t); }
  const float rho = d.dy * inv;
  const float kappa = fmaf(rho * 1.3334f, rho, rho);
  const float sx = fmaf(fabsf(p.lr), kappa, t * d.cex), fy = fmaf(fabsf(p.lf), kappa, t * d.eys);
  p.mrg = 1.05f * fsqrt_(fmaf(sx, sx, fy * fy));
  const float tg = t * d.kgc;
  if (t >= NEAR_Z && t <= FAR_Z) p.flags |= PF_TILE_OK;
  if (tg >= NEAR_Z && tg <= FAR_Z) p.flags |= PF_GROUND_OK;
  if (rho > 0.25f || tg * (1.f + 2.f * rho) > FAR_Z * 0.98f || t * (1.f - 2.f * rho) < NEAR_Z * 1.02f)
    p.flags |= PF_ALWAYS_EDGE;
  return p;
}

template <bool DR, bool OBJ>
__global__ __launch_bounds__(RB) void k_raster(RenderParams R, const EnvCam* __restrict__ cams,
                                               const EnvFast* __restrict__ fasts, uint8_t* __restrict__ frames, const uint32_t* __restrict__ texels,
                                               const float4* __restrict__ lut, const RenderMapDev* __restrict__ maps,
                                               const TileLds* __restrict__ tile_recs, uint16_t* __restrict__ queue,
                                               int32_t* __restrict__ qcount) {
  extern __shared__ uint32_t s_mem[];
  TileLds* s_tiles = reinterpret_cast<TileLds*>(s_mem);                                   // [n_tile_recs]

  const int tid = threadIdx.x;
  const int npix = R.W * R.H;
  const int tiles_x = (R.W + DT_TILE_W - 1) / DT_TILE_W, n_tiles = tiles_x * ((R.H + DT_TILE_H - 1) / DT_TILE_H);
  const int tile = blockIdx.x % n_tiles;
  const int chunk = blockIdx.x / n_tiles;
  const int e0 = chunk * ENVS_PER_BLOCK;
  const int e1 = min(e0 + ENVS_PER_BLOCK, R.N);
  {  // stage the raster tile records of every map once per workgroup
    const uint32_t* src = reinterpret_cast<const uint32_t*>(tile_recs);
    for (int i = tid; i < R.n_tile_recs * (int)(sizeof(TileLds) / 4); i += RB) s_mem[i] = src[i];
  }
  __syncthreads();

  // Pixel ownership: the workgroup owns a WAVE_W x DT_TILE_H (128 x 8) pixel tile, wavefront w its rows 2w, 2w+1, lane l
  // pixel (k*64 + l) of the wavefront's row-major block (slot k).  Adjacent lanes are adjacent pixels, so the texel
  // addresses of one load instruction are neighbours in the texture, and the 2D footprint of the tile
  // keeps its texture lines in L1.
  const int wave = tid >> 6, lane = tid & 63;
  const int blk = tile * 4 + __builtin_amdgcn_readfirstlane(wave);   // raster wavefront block (objmask / blockbox index)
  const int tile_x0 = (tile % tiles_x) * DT_TILE_W;
  const int wave_y0 = (tile / tiles_x) * DT_TILE_H + wave * (WAVE_PIX / WAVE_W);
  const float aspect = (float)R.W / (float)R.H;
  const float ex_n = 0.375f * 2.f / (float)R.W * 1.01f, ey_n = 0.375f * 2.f / (float)R.H * 1.01f;

  // per-pixel LUT -> registers (shared by all envs)
  float nx[PPT], ny[PPT];
  bool ok[PPT];
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    if (tile_x0 + SLOT_X(k, lane) < R.W && wave_y0 + SLOT_Y(k, lane) < R.H) {
      const float4 l = lut[(wave_y0 + SLOT_Y(k, lane)) * R.W + tile_x0 + SLOT_X(k, lane)];
      nx[k] = l.x; ny[k] = l.y; ok[k] = l.z != 0.f;
    } else { nx[k] = ny[k] = 0.f; ok[k] = false; }
  }
  PixInv pv[PPT];
  if (!DR) {
    const CamShared cs = default_cam(aspect);
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      pv[k] = pix_inv(nx[k], ny[k], ok[k], cs.tx, cs.ty, cs.sth, cs.cth, cs.Cy, cs.L, ex_n, ey_n);
      pv[k].ndl = fminf(fmaf(cs.dif, pv[k].ndl, cs.base), 1.f);   // lit factor, env-invariant
    }
  }

  // source-pixel bounding box of this wavefront's pixels (for the mesh-object test)
  float spx[PPT], spy[PPT];
  float wbx0 = 1e30f, wbx1 = -1e30f, wby0 = 1e30f, wby1 = -1e30f;
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    src_px(nx[k], ny[k], R.W, R.H, spx[k], spy[k]);
    if (ok[k]) { wbx0 = fminf(wbx0, spx[k]); wbx1 = fmaxf(wbx1, spx[k]); wby0 = fminf(wby0, spy[k]); wby1 = fmaxf(wby1, spy[k]); }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    wbx0 = fminf(wbx0, __shfl_xor(wbx0, d)); wbx1 = fmaxf(wbx1, __shfl_xor(wbx1, d));
    wby0 = fminf(wby0, __shfl_xor(wby0, d)); wby1 = fmaxf(wby1, __shfl_xor(wby1, d));
  }

  uint16_t* w_queue = queue + ((size_t)blockIdx.x * (RB / 64) + wave) * QREGION;
  int qn = 0, qo = 0;                                   // wave-uniform queue fill: plane edges (front), object-box pixels (back)
  int qend_v = 0;
  // Frame stores go through a wavefront-private LDS transpose: lane l then owns the 12 bytes of the
  // 4 consecutive pixels 4l..4l+3 (row-major in the wavefront's block) -> three dword stores per lane,
  // 3*WAVE_W contiguous bytes per block row.
  uint32_t* s_px = s_mem + R.n_tile_recs * (sizeof(TileLds) / 4) + wave * WAVE_PIX;
  const int st_x = tile_x0 + (lane * 4) % WAVE_W, st_y = wave_y0 + (lane * 4) / WAVE_W;
  const bool aligned_rows = (R.W & 3) == 0;
  const bool st_ok = aligned_rows && lane * 4 < WAVE_PIX && st_x < R.W && st_y < R.H;
  const size_t st_off = ((size_t)st_y * R.W + st_x) * 3;
  const int tw1 = R.tex_w + 1, xmask = R.tex_w - 1, ymask = R.tex_h - 1;

  // object masks of the chunk's envs for this block: one vector load, lane l <-> env e0 + l.  (Written out, not ChunkObjMasks: with the struct
  // the compiler assigns the registers of this kernel's env loop differently.)
  uint32_t om_lo = 0u, om_hi = 0u;
  if (OBJ && lane < e1 - e0) {
    const unsigned long long v = R.objmask[(size_t)(e0 + lane) * (n_tiles * 4) + blk];
    om_lo = (uint32_t)v; om_hi = (uint32_t)(v >> 32);
  }
  for (int e = e0; e < e1; ++e) {
    const EnvFast f = fasts[e];                      // wave-uniform: one 64-byte scalar load
    float base0 = 0.f, base1 = 0.f, base2 = 0.f, dif0 = 0.f, dif1 = 0.f, dif2 = 0.f;
    if (DR) {
      const EnvCam c = cams[e];
      base0 = c.base[0]; base1 = c.base[1]; base2 = c.base[2]; dif0 = c.dif[0]; dif1 = c.dif[1]; dif2 = c.dif[2];
      const DrCam dc = dr_cam(c, ex_n, ey_n);
#pragma unroll
      for (int k = 0; k < PPT; ++k)
        pv[k] = pix_inv_dr(nx[k], ny[k], ok[k], dc, c.L);
    }
    const uint32_t hor_rgb = f.hor_rgb;
    const float A = f.A, B = f.B, Cxi = f.Cxi, Czi = f.Czi;

    // ---- fast path: one ray per pixel, straight-line (predicated) code so that the LDS
    // tile-record reads and the 8 texel loads of the 4 pixels are all in flight together.
    // Per-pixel predicates are kept as bools (lane masks in SGPR pairs), not as VGPR bit fields.
    uint32_t px[PPT];
    bool edge[PPT], oedge[PPT];                        // oedge: inside a mesh object's screen box (k_resolve_obj's pixels)
#pragma unroll
    for (int k = 0; k < PPT; ++k) oedge[k] = false;
    bool any_work = false;
#pragma unroll
    for (int k = 0; k < PPT; ++k) any_work |= (pv[k].flags & (PF_VALID | PF_SKY)) == PF_VALID;
    if (!__ballot(any_work)) {                       // wave-uniform: all sky / border
#pragma unroll
      for (int k = 0; k < PPT; ++k) { px[k] = (pv[k].flags & PF_VALID) ? hor_rgb : 0u; edge[k] = false; }
    } else {
      float fx[PPT], fz[PPT], gxs[PPT], gzs[PPT];
      bool cand[PPT], is_tile[PPT], fast[PPT];
      bool need_ground = false;
      TileLds tr[PPT];
#pragma unroll
      for (int k = 0; k < PPT; ++k) {
        const PixInv& p = pv[k];
        const float gx = fmaf(p.lf, B, fmaf(p.lr, A, Cxi));
        const float gz = fmaf(p.lf, -A, fmaf(p.lr, B, Czi));
        gxs[k] = gx; gzs[k] = gz;
        fx[k] = __builtin_amdgcn_fractf(gx); fz[k] = __builtin_amdgcn_fractf(gz);
        const int ti = flr_i32(gx), tj = flr_i32(gz);
        cand[k] = (p.flags & (PF_VALID | PF_SKY | PF_ALWAYS_EDGE)) == PF_VALID;
        const bool ingrid = cand[k] & ((p.flags & PF_TILE_OK) != 0) & ((unsigned)ti < (unsigned)f.gw) & ((unsigned)tj < (unsigned)f.gh);
        const int idx = ingrid ? f.tile_off + (int)__umul24(tj, f.gw) + ti : f.tile_off;
        tr[k] = s_tiles[idx];
        // flags: 0 absent, 1 present (untextured: exact path), 3 present + textured
        is_tile[k] = ingrid & (tr[k].flags != 0u);
        // interior test: every MSAA sample stays inside the tile  <=>  max(|fx-.5|, |fz-.5|) < .5 - mrg/tile_size
        const float dmax = absmax(fx[k] - 0.5f, fz[k] - 0.5f);
        const bool inside = dmax < fmaf(-p.mrg, f.its, 0.5f);
        fast[k] = ingrid & (tr[k].flags == 3u) & inside;       // plain textured tile interior: the one-ray result is exact
        need_ground |= cand[k] & !is_tile[k];
        edge[k] = ((p.flags & (PF_VALID | PF_ALWAYS_EDGE)) == (PF_VALID | PF_ALWAYS_EDGE)) | (is_tile[k] & !fast[k]);
      }
      bool any_fast = false;
#pragma unroll
      for (int k = 0; k < PPT; ++k) any_fast |= fast[k];
      if (!__ballot(any_fast)) {                     // wave-uniform: nothing here takes the textured one-ray result
#pragma unroll                                       // (ground beyond the map, horizon band): no texel loads, no filter
        for (int k = 0; k < PPT; ++k) px[k] = (pv[k].flags & PF_VALID) ? hor_rgb : 0u;
      } else {
      uint2 top2[PPT], bot2[PPT];
      int wxi[PPT], wyi[PPT];                        // 8-bit filter weights (gl_fix)
      const uint8_t* tex_bytes = reinterpret_cast<const uint8_t*>(texels);
      const uint32_t row_bytes = (uint32_t)tw1 * 4u;
#pragma unroll
      for (int k = 0; k < PPT; ++k) {
        const float x = fmaf(tr[k].mxz, fz[k], fmaf(tr[k].mxx, fx[k], tr[k].ox));
        const float y = fmaf(tr[k].myz, fz[k], fmaf(tr[k].myx, fx[k], tr[k].oy));
        const int xf = gl_fix(x), yf = gl_fix(y);
        wxi[k] = xf & 255; wyi[k] = yf & 255;
        const uint32_t x0 = (uint32_t)((xf >> 8) & xmask), y0 = (uint32_t)((yf >> 8) & ymask);
        // 32-bit byte offset from the (uniform) pool base -> saddr-form loads; always in bounds
        const uint32_t off = (__umul24(y0, (uint32_t)tw1) + x0 + tr[k].tex_off) << 2;
        __builtin_memcpy(&top2[k], tex_bytes + off, 8);
        __builtin_memcpy(&bot2[k], tex_bytes + (off + row_bytes), 8);
      }
#pragma unroll
      for (int k = 0; k < PPT; ++k) {
        const PixInv& p = pv[k];
        // llvmpipe's integer GL_LINEAR (gl_linear_rgb), then the lit factor: pv.ndl holds min(base + dif*ndl, 1) for the shared
        // camera (all channels equal), max(0, N.L) under domain randomisation (per-channel base / dif)
        int T[3];
        gl_linear_rgb(top2[k].x, top2[k].y, bot2[k].x, bot2[k].y, wxi[k], wyi[k], T);
        float v0 = (float)T[0], v1 = (float)T[1], v2 = (float)T[2];
        if (DR) {
          v0 *= fminf(fmaf(dif0, p.ndl, base0), 1.f);
          v1 *= fminf(fmaf(dif1, p.ndl, base1), 1.f);
          v2 *= fminf(fmaf(dif2, p.ndl, base2), 1.f);
        } else { v0 *= p.ndl; v1 *= p.ndl; v2 *= p.ndl; }
        uint32_t rgb = 0;
        rgb = __builtin_amdgcn_cvt_pk_u8_f32(v0, 0, rgb);
        rgb = __builtin_amdgcn_cvt_pk_u8_f32(v1, 1, rgb);
        rgb = __builtin_amdgcn_cvt_pk_u8_f32(v2, 2, rgb);
        px[k] = fast[k] ? rgb : ((p.flags & PF_VALID) ? hor_rgb : 0u);
      }
      }
      if (__ballot(need_ground)) {                   // wave-uniform: ground quad beyond the map
        const EnvCam c = cams[e];                    // colours / ground-corner light: only needed here
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
          const PixInv& p = pv[k];
          const bool gcand = cand[k] & !is_tile[k];
          // every sample's tile-plane hit must stay clear of the grid, ground hit inside the quad
          const float wx = gxs[k] * f.ts, wz = gzs[k] * f.ts;
          const float wxg = fmaf(f.kg, wx - f.Cx, f.Cx), wzg = fmaf(f.kg, wz - f.Cz, f.Cz);
          const bool clear = (wx < -p.mrg) | (wx > f.gw_m + p.mrg) | (wz < -p.mrg) | (wz > f.gh_m + p.mrg);
          const bool inq = (fabsf(wxg) + 2.f * p.mrg < GROUND_HALF) & (fabsf(wzg) + 2.f * p.mrg < GROUND_HALF);
          const bool gfast = gcand & clear & inq & ((p.flags & PF_GROUND_OK) != 0);
          const float ndl = ground_ndl(c, wxg, wzg);
          uint32_t rgb = 0;
          rgb = __builtin_amdgcn_cvt_pk_u8_f32(c.gnd[0] * fminf(c.base[0] + c.dif[0] * ndl, 1.f), 0, rgb);
          rgb = __builtin_amdgcn_cvt_pk_u8_f32(c.gnd[1] * fminf(c.base[1] + c.dif[1] * ndl, 1.f), 1, rgb);
          rgb = __builtin_amdgcn_cvt_pk_u8_f32(c.gnd[2] * fminf(c.base[2] + c.dif[2] * ndl, 1.f), 2, rgb);
          px[k] = gfast ? rgb : px[k];
          edge[k] = edge[k] | (gcand & !gfast);
        }
      }
    }

    // ---- mesh objects: every pixel inside the union box of the env's projected triangles
    // takes the exact path (which z-buffers the triangles per sample)
    if (OBJ) {
      unsigned long long om = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)om_hi, e - e0) << 32) |
                              (uint32_t)__builtin_amdgcn_readlane((int)om_lo, e - e0);   // objects whose box meets this block
      const ObjBox* boxes = R.objbox + (size_t)e * DTSIM_MAX_OBJECTS;
      while (om) {
        const ObjBox ob = boxes[__builtin_ctzll(om)];  // wave-uniform
        om &= om - 1ull;
#pragma unroll
        for (int k = 0; k < PPT; ++k)
          if (ok[k] && spx[k] >= ob.bx0 && spx[k] <= ob.bx1 && spy[k] >= ob.by0 && spy[k] <= ob.by1) oedge[k] = true;
      }
    }

    if (aligned_rows) {
#pragma unroll
      for (int k = 0; k < PPT; ++k) s_px[k * 64 + lane] = px[k];
      const uint4 q = *reinterpret_cast<const uint4*>(s_px + (lane * 4) % WAVE_PIX);   // same wavefront: DS ops are ordered
      if (st_ok) {
        uint32_t* d32 = reinterpret_cast<uint32_t*>(frames + (size_t)e * npix * 3 + st_off);   // 12-byte aligned
        // non-temporal: the frame is written once and not read back by this pass (keeps the texels in L2)
        __builtin_nontemporal_store(q.x | (q.y << 24), d32);
        __builtin_nontemporal_store((q.y >> 8) | (q.z << 16), d32 + 1);
        __builtin_nontemporal_store((q.z >> 16) | (q.w << 8), d32 + 2);
      }
    } else {                                           // odd widths: bytes, straight from the owning lane
#pragma unroll
      for (int k = 0; k < PPT; ++k)
        if (tile_x0 + SLOT_X(k, lane) < R.W && wave_y0 + SLOT_Y(k, lane) < R.H) {
          uint8_t* dst = frames + ((size_t)e * npix + (size_t)(wave_y0 + SLOT_Y(k, lane)) * R.W + tile_x0 + SLOT_X(k, lane)) * 3;
          dst[0] = (uint8_t)px[k]; dst[1] = (uint8_t)(px[k] >> 8); dst[2] = (uint8_t)(px[k] >> 16);
        }
    }

    // ---- edge pixels: exact 4-sample resolve, deferred to k_resolve (own launch, own
    // register budget): append them to this wavefront's queue region.
    bool any_edge = false, any_oedge = false;
#pragma unroll
    for (int k = 0; k < PPT; ++k) { any_oedge |= oedge[k]; edge[k] &= !oedge[k]; any_edge |= edge[k]; }
    const uint32_t etag = (uint32_t)(e - e0) << 8;
    if (OBJ && __ballot(any_oedge)) {    // wave-uniform: object-box pixels fill the region from its far end
#pragma unroll
      for (int k = 0; k < PPT; ++k) {
        const bool ek = oedge[k];
        const unsigned long long mk = __ballot(ek);
        if (ek) {
          const int rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u));
          w_queue[QREGION - 1 - (qo + rank)] = (uint16_t)(etag | QE_PLANE_EDGE | (uint32_t)(k * 64 + lane));   // (this raster does not tell: always "plane edge")
        }
        qo += __popcll(mk);
      }
    }
    if (__ballot(any_edge)) {    // wave-uniform
#pragma unroll
      for (int k = 0; k < PPT; ++k) {                // per pixel slot: ballot -> rank -> masked store
        const bool ek = edge[k];
        const unsigned long long mk = __ballot(ek);
        if (ek) {
          const int rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u));
          w_queue[qn + rank] = (uint16_t)(etag | (uint32_t)(k * 64 + lane));
        }
        qn += __popcll(mk);
      }
    }
    if (OBJ) qend_v = lane >= e - e0 ? qo : qend_v;   // lane l: object-entry fill after env e0 + l (k_resolve_obj's per-env ranges)
  }
  if (lane == 0) qcount[blockIdx.x * (RB / 64) + wave] = qn;
  if (OBJ && lane < ENVS_PER_BLOCK) R.qend[((size_t)blockIdx.x * (RB / 64) + wave) * ENVS_PER_BLOCK + lane] = (uint16_t)qend_v;
  // Work items for k_resolve: the workgroup's 64-entry batches (four regions, flattened), ITEM_B at a
  // time, appended to a global list so that the resolve launch can spread hot tiles (close-up meshes,
  // horizon band) over the whole chip.  The append order is arbitrary; items touch disjoint pixels.
  __shared__ int s_nb[RB / 64], s_no[RB / 64];
  if (lane == 0) { s_nb[wave] = (qn + 63) >> 6; s_no[wave] = qo; }
  __syncthreads();
  if (tid == 0) {
    int nb = 0, no = 0;
#pragma unroll
    for (int r = 0; r < RB / 64; ++r) { nb += s_nb[r]; no += s_no[r]; }
    if (nb > 0) {                                    // k_resolve: ITEM_B batches of plane-edge entries per item
      const int ni = (nb + ITEM_B - 1) / ITEM_B;
      const int pos = atomicAdd(R.work + DT_WORK_ITEMS, ni);
      for (int i = 0; i < ni; ++i) R.items[pos + i] = (uint32_t)blockIdx.x * ITEMS_PER_WG + (uint32_t)i;
    }
    if (OBJ && no > 0) push_obj_items(R, (uint32_t)blockIdx.x);
  }
}

// ---- resolve_region_q: exact path of k_raster_q (shared camera, no mesh objects) ------------------------------------
// Called by every wavefront of k_raster_q at the end of its env loop on ITS OWN queue region (the entries it appended):
// no second launch, no work list, no atomics -- and the gather-bound resolve of one wavefront overlaps the VALU-bound
// env loops of the other wavefronts on the CU.  Per entry (one pixel of one env):
//   1. the pixel's centre hit -> padded quad coordinates -> its tile's table entry and quad record, as in k_raster_q;
//   2. exact interior test (distance of the hit to the tile boundary, in cells, against the MSAA reach): the
//      cell-granular test of k_raster_q is conservative by up to a cell and sends every pixel of the seam cell here;
//      most entries pass and get the one-ray colour from the same integer filter (bit-identical to k_raster_q);
//   3. otherwise the four samples: their tile-plane hits in the yaw-local frame are env-invariant (SampTab, built by
//      k_pix_setup), so a sample costs one 2x2 transform and one table lookup.  Coverage per sample (tile if the
//      tile plane is hit within [near, far] on a present tile; else the ground quad if hit within range and inside
//      +-50 m; else the clear colour), shading once per distinct primitive at the pixel centre (GL semantics:
//      simulator.py:1932-1934, graphics.py:172-251): a tile is shaded with ITS texture at the centre hit -- outside the
//      tile the coordinate wraps (GL_REPEAT), which the quad records encode -- times the centre's lit factor.
// k_raster_v3 drains its regions with its own exact path, resolve_region_v3 (render_v3.hip): no interior test, no list.
// LIGHT: the shared camera with per-env lights (EnvL in render order, envl): the lit factor of the tile plane is env_lit8's, per entry.
template <bool S256, bool LIGHT = false>
__device__ inline void resolve_region_q(const RenderParams& R, const EnvCam* __restrict__ cams, const EnvQ* __restrict__ envq,
                                        const PixTab* __restrict__ pixtab, const SampTab* __restrict__ samptab,
                                        const uint8_t* __restrict__ qtex, const uint32_t* s_qt, uint32_t* w_list,
                                        const uint16_t* w_queue, const int n, const int e0, const int tile_x0, const int wave_y0,
                                        const int lane, const EnvL* __restrict__ envl) {
  const int npix = R.W * R.H;
  const int LS = R.qlog2;
  const uint32_t SM = (1u << LS) - 1u;
  const float Sf = (float)(1 << LS), lo = 0.5f * Sf;
  const char* qtb = reinterpret_cast<const char*>(s_qt);
  const uint32_t tex_min = 32u;                        // block offsets from here on are textured tiles

  // (k_raster_q's table layout, any power-of-two tile size: not v3_sample_owner's.)
  // Table entry (block byte offset, record-offset mask) of the tile that OWNS padded quad coordinates (X, Z): tile
  // boundaries sit at k*S + 0.5 (the GL_LINEAR half-texel shift folded into the coordinates), so ownership is decided
  // on (X - 0.5, Z - 0.5) -- unlike the record lookup, which goes by whole cells.  (ox, oz): the tile's origin.
  auto tile_entry = [&](float X, float Z, const float Xhi, const float Zhi, const uint32_t tab_b, const uint32_t pitch4, uint32_t& ta,
                        float& ox, float& oz) -> uint2 {
    const float Xc = med3f(X - 0.5f, lo, Xhi), Zc = med3f(Z - 0.5f, lo, Zhi);
    const uint32_t ti = (uint32_t)flr_i32(Xc) >> LS, tj = (uint32_t)flr_i32(Zc) >> LS;
    ox = (float)(ti << LS) + 0.5f; oz = (float)(tj << LS) + 0.5f;
    ta = (ti << 3) + __umul24(tj, pitch4) + tab_b;
    return *reinterpret_cast<const uint2*>(qtb + ta);
  };
  // quad record of block entry `te` at the cell of the snapped (unclamped) coordinates xb, zb (q8_bits), wrapped into the tile
  auto tile_quad = [&](const uint2 te, const uint32_t xb, const uint32_t zb) -> uint4 {
    if (S256) return *reinterpret_cast<const uint4*>(qtex + (te.x | q8_rec256(xb, zb, te.y)));
    const uint32_t local = (((q8_cell(zb) & SM) << LS) | (q8_cell(xb) & SM)) & te.y;
    return *reinterpret_cast<const uint4*>(qtex + (te.x + (local << 4)));
  };

  // ---- phase 1: per entry, the exact interior test; interior entries get the one-ray colour, the others are
  // compacted into the wavefront's list for phase 2.
  // The (up to four) 64-entry batches of a round go through every stage together, so that each dependent memory round
  // trip (entry -> tables -> tile entry -> quad record -> store) is paid once per round: the phase is latency bound.
  // Instantiated for 1, 2 and 4 batches: most regions hold one seam's worth of entries, not 256.
  auto phase1 = [&](auto utag, const int r0) __attribute__((always_inline)) -> int {
    constexpr int U = decltype(utag)::value;
    int n_list = 0;                                  // wave-uniform
    bool have[U], interior[U], skip[U];
    int pix[U], el[U], env[U];
    PixTab pt[U];
    float Xu[U], Zu[U];
    uint2 te_c[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      have[u] = r0 + u * 64 + lane < n;
      const int qoff = r0 + u * 64 + lane;
      // the entries were written by this wavefront (workgroup) a moment ago: bypass the (possibly stale) L1 line
      const uint32_t ent = have[u] ? (uint32_t)__builtin_nontemporal_load(w_queue + qoff) : 0u;
      el[u] = qe_envpos(ent);
      skip[u] = !__ballot(have[u]);                  // wave-uniform: a batch past the region's fill
      const int lp = qe_pixel(ent);
      pix[u] = (wave_y0 + lp / WAVE_W) * R.W + tile_x0 + lp % WAVE_W;
    }
    float4 qa[U];
    uint4 qb[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      qa[u] = make_float4(0.f, 0.f, 0.f, 0.f); qb[u] = make_uint4(0u, 0u, 0u, 0u); env[u] = 0;
      pt[u] = PixTab{0.f, 0.f, 0.f, 0xFFFFu};
      if (skip[u]) continue;                         // wave-uniform
      pt[u] = pixtab[pix[u]];
      const EnvQ* fq = envq + min(e0 + el[u], R.N - 1);   // position in the render order -> constants, frame index
      qa[u] = *reinterpret_cast<const float4*>(&fq->A);     // A, B, Cx, Cz
      qb[u] = *reinterpret_cast<const uint4*>(&fq->Xhi);    // Xhi, Zhi, tab_b, pitch4
      const uint4 qd = *reinterpret_cast<const uint4*>(&fq->reach);   // reach, env, tab3, qpm_bits (one 16-byte piece: the path is bound by its vector-memory instruction count)
      env[u] = (int)qd.y;
      if constexpr (LIGHT) { const EnvL l = envl[min(e0 + el[u], R.N - 1)]; pt[u].lit = pt[u].lit > 0.f ? 256.f * env_lit8(l, pt[u].lr, pt[u].lf, env_base8()) : pt[u].lit; }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      interior[u] = false; Xu[u] = Zu[u] = 0.f; te_c[u] = make_uint2(0u, 0u);
      if (skip[u]) continue;                         // wave-uniform
      const float A = qa[u].x, B = qa[u].y, Cx = qa[u].z, Cz = qa[u].w;
      const float Xhi = __uint_as_float(qb[u].x), Zhi = __uint_as_float(qb[u].y);
      Xu[u] = fmaf(pt[u].lf, B, fmaf(pt[u].lr, A, Cx)); Zu[u] = fmaf(pt[u].lf, -A, fmaf(pt[u].lr, B, Cz));
      uint32_t ta_c;
      float ox, oz;
      te_c[u] = tile_entry(Xu[u], Zu[u], Xhi, Zhi, qb[u].z, qb[u].w, ta_c, ox, oz);
      // distance of the hit to the boundary of the tile that owns it, in cells, against the MSAA reach
      const float mrg = __half2float(__ushort_as_half((unsigned short)(pt[u].mi >> 16)));   // metres, rounded up
      const float ux = Xu[u] - ox, uz = Zu[u] - oz;        // in [0, S) inside the owner tile
      const float d = fminf(fminf(ux, Sf - ux), fminf(uz, Sf - uz));
      const bool in_range = Xu[u] - 0.5f >= lo && Xu[u] - 0.5f <= Xhi && Zu[u] - 0.5f >= lo && Zu[u] - 0.5f <= Zhi;
      interior[u] = have[u] && in_range && te_c[u].x >= tex_min && pt[u].lit > 0.f && (pt[u].mi & 0xFFFFu) < 0xFFF0u && d > mrg * R.q_per_m;
    }
    uint4 qc[U];
#pragma unroll
    // only the INTERIOR entries (~ 30 %) use the record: the gather runs under their lanes -- its cost on the texture path is per distinct line
    for (int u = 0; u < U; ++u) { qc[u] = make_uint4(0u, 0u, 0u, 0u); if (!skip[u] && interior[u]) qc[u] = tile_quad(te_c[u], q8_bits(Xu[u]), q8_bits(Zu[u])); }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (!skip[u]) {                                // wave-uniform
        const uint32_t rgb = quad_filter(qc[u], q8_frac(q8_bits(Xu[u])), q8_frac(q8_bits(Zu[u])), pt[u].lit);
        if (interior[u]) store_rgb(R.frames, npix, env[u], pix[u], rgb);
      }
      const bool msaa = have[u] && !interior[u];
      const unsigned long long mm = __ballot(msaa);
      if (msaa) w_list[n_list + __builtin_amdgcn_mbcnt_hi((uint32_t)(mm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mm, 0u))] = (uint32_t)pix[u] | ((uint32_t)el[u] << 24);
      n_list += __popcll(mm);
    }
    return n_list;
  };
  for (int r0 = 0; r0 < n; r0 += RQ_LIST) {          // wave-uniform: rounds of up to RQ_LIST entries
    const int rem = n - r0;
    const int n_list = rem > 128 ? phase1(std::integral_constant<int, 4>{}, r0)
                     : rem > 64 ? phase1(std::integral_constant<int, 2>{}, r0) : phase1(std::integral_constant<int, 1>{}, r0);
    // ---- phase 2: the four samples of the listed pixels, on dense lanes
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int l0 = 0; l0 < n_list; l0 += 64) {          // wave-uniform
      const bool have = l0 + lane < n_list;
      const uint32_t le = have ? w_list[l0 + lane] : 0u;
      const int pix = (int)(le & 0xFFFFFFu), el = (int)(le >> 24);
      const SampTab sp = samptab[pix];
      const PixTab pt = pixtab[pix];
      const EnvQ* fq = envq + min(e0 + el, R.N - 1);
      const float A = fq->A, B = fq->B, Cx = fq->Cx, Cz = fq->Cz, Xhi = fq->Xhi, Zhi = fq->Zhi;
      const uint32_t tab_b = fq->tab_b, pitch4 = fq->pitch4;
      const int e = (int)fq->env;
      const EnvCam* c = cams + e;
      const float wCx = c->Cx, wCy = c->Cy, wCz = c->Cz, sa = c->sa, ca = c->ca;
      const float kg = (wCy - GROUND_Y) / wCy;
      const float Xu = fmaf(pt.lf, B, fmaf(pt.lr, A, Cx)), Zu = fmaf(pt.lf, -A, fmaf(pt.lr, B, Cz));
      const uint32_t xub = q8_bits(Xu), zub = q8_bits(Zu);
      const float ax = q8_frac(xub), az = q8_frac(zub);
      float lit = pt.lit > 0.f ? pt.lit : 0.55f;
      if constexpr (LIGHT) { if (pt.lit > 0.f) lit = 256.f * env_lit8(envl[min(e0 + el, R.N - 1)], pt.lr, pt.lf, env_base8()); }
      // coverage: per sample tile (tile plane hit within [near, far] on a present tile), else ground quad, else clear colour
      uint32_t key[4];                                 // 0 sky, 1 ground, else 2 + table address of the tile
      uint2 te[4];
      int n_sky = 0, n_gnd = 0;
      float gwx = 0.f, gwz = 0.f;                      // ground hit used for shading: the lowest-index ground sample's
#pragma unroll
      for (int s = 3; s >= 0; --s) {
        const uint32_t hr = sp.dlr[s >> 1], hf = sp.dlf[s >> 1];
        const float slr = pt.lr + __half2float(__ushort_as_half((unsigned short)((s & 1) ? hr >> 16 : hr)));
        const float slf = pt.lf + __half2float(__ushort_as_half((unsigned short)((s & 1) ? hf >> 16 : hf)));
        const float Xs = fmaf(slf, B, fmaf(slr, A, Cx)), Zs = fmaf(slf, -A, fmaf(slr, B, Cz));
        uint32_t ta;
        float sox, soz;
        te[s] = tile_entry(Xs, Zs, Xhi, Zhi, tab_b, pitch4, ta, sox, soz);
        const bool s_in = Xs - 0.5f >= lo && Xs - 0.5f <= Xhi && Zs - 0.5f >= lo && Zs - 0.5f <= Zhi;
        const bool is_tile = ((sp.flags >> s) & 1u) && s_in && te[s].x != 0u;
        // ground-quad hit of the sample (world): camera + kg * (tile-plane hit - camera)
        const float wx = kg * (slr * sa + slf * ca) + wCx, wz = kg * (slr * ca - slf * sa) + wCz;
        const bool is_gnd = !is_tile && ((sp.flags >> (4 + s)) & 1u) && fabsf(wx) <= GROUND_HALF && fabsf(wz) <= GROUND_HALF;
        key[s] = !have ? 0u : is_tile ? 2u + ta : is_gnd ? 1u : 0u;
        n_sky += key[s] == 0u; n_gnd += key[s] == 1u;
        if (is_gnd) { gwx = wx; gwz = wz; }
      }
      // shading, once per primitive at the pixel centre
      float acc[3];
      acc[0] = (float)n_sky * c->hor[0]; acc[1] = (float)n_sky * c->hor[1]; acc[2] = (float)n_sky * c->hor[2];
      if (__ballot(have && n_gnd > 0)) {               // wave-uniform
        if (pt.lit > 0.f && (pt.lr != 0.f || pt.lf != 0.f)) {   // the centre ray hits the planes: shade at its ground hit
          gwx = kg * (pt.lr * sa + pt.lf * ca) + wCx; gwz = kg * (pt.lr * ca - pt.lf * sa) + wCz;
        }
        const float a_ = fminf(fmaxf((gwx + GROUND_HALF) * (0.5f / GROUND_HALF), 0.f), 1.f);
        const float b_ = fminf(fmaxf((gwz + GROUND_HALF) * (0.5f / GROUND_HALF), 0.f), 1.f);
        const float ndl = ground_corner_ndl(a_, b_, c->gndl[0], c->gndl[1], c->gndl[2], c->gndl[3]);
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[k] += (float)n_gnd * ground_lit(c->gnd[k], c->base[k], c->dif[k], ndl);
      }
      uint32_t todo = 0u;
#pragma unroll
      for (int s = 0; s < 4; ++s) todo |= key[s] >= 2u ? (1u << s) : 0u;
      while (__ballot(todo != 0u)) {                   // wave-uniform: one pass per distinct tile over the lanes
        const int s0 = todo ? __builtin_ctz(todo) : 0;
        const uint32_t k0 = s0 == 0 ? key[0] : s0 == 1 ? key[1] : s0 == 2 ? key[2] : key[3];
        uint2 t0;
        t0.x = s0 == 0 ? te[0].x : s0 == 1 ? te[1].x : s0 == 2 ? te[2].x : te[3].x;
        t0.y = s0 == 0 ? te[0].y : s0 == 1 ? te[1].y : s0 == 2 ? te[2].y : te[3].y;
        int cnt = 0;
#pragma unroll
        for (int s = 0; s < 4; ++s) { const bool same = ((todo >> s) & 1u) && key[s] == k0; cnt += same; todo &= same ? ~(1u << s) : ~0u; }
        const uint4 qt = tile_quad(t0, xub, zub);
        float col[3];
        quad_filter3(qt, ax, az, lit, col);
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[k] += (float)cnt * col[k];
      }
      const float o[3] = {0.25f * acc[0], 0.25f * acc[1], 0.25f * acc[2]};
      if (have) store_rgb(R.frames, npix, e, pix, pack_rgb(o));
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

// ---- quad-layout fast path -------------------------------------------------------------------------------------
// k_raster_q<OBJ>: same work decomposition, queue protocol and store path as k_raster<false, OBJ> (shared camera), with
// the per-pixel cost cut to what the VALU issue rate of gfx950 allows (profiles/r02_ubench_valu_rates.txt: every
// vector opcode costs one ~4-cycle issue slot per wavefront, only v_pk_*_f32 does two results per slot):
//   * the tile lookup and the per-tile affine texture map are gone: tile textures are stored pre-rotated, per
//     (texture, angle), as S x S "quad" records of 16 B -- the four GL_LINEAR taps around one cell, channel-planar,
//     plus a meta dword -- and the hit goes from the yaw-local frame straight to padded quad coordinates (EnvQ);
//     the only table read is the block offset of the cell's tile (LDS, 4 B per tile incl. an off-grid ring);
//   * the bilinear filter is integer, at the precision GL's own filter has (round 6: the byte-weight filter of quad_weights8 /
//     quad_filter -- one v_dot4_u32_u8 per channel against the planar taps, light folded into the weights);
//   * interior / edge classification is one compare: meta.lo = cells to the nearest tile boundary (0 for anything
//     that is not a textured tile) against the pixel's MSAA reach in cells, computed once per pixel (Mi).  Cell 0 of
//     each axis straddles the seam (half of it belongs to the neighbour tile) and is always an edge;
//   * all-sky wavefront blocks (env-invariant with the shared camera) take a three-store loop.
// Anything that is not a fast tile pixel falls into a wave-uniform slow branch that decides ground-fast vs edge and
// appends edge pixels to the wavefront's queue region; the exact path (resolve_region_q) drains it at the end of the env loop.
// With mesh objects (OBJ) the pixels inside object screen boxes are appended from the far end of the region instead and
// left to k_resolve_obj.

#ifndef DT_Q_WAVES
#define DT_Q_WAVES 5                                 // wavefronts per SIMD the register allocation is held to (96 VGPRs)
#endif
// LIGHT: per-env lights (EnvL in render order), as k_raster_v3<OBJ, true> (render_v3.hip)
// SUB: the masked pass -- positions [0, live) of k_env_sort<true>'s order, live = R.work[DT_WORK_LIVE] (dt_sub_live); the grid is sized for
// R.N and the workgroups past the live chunks leave at once.
template <bool OBJ, bool S256, bool LIGHT = false, bool SUB = false>
__global__ __launch_bounds__(RB) __attribute__((amdgpu_waves_per_eu(OBJ ? DT_Q_WAVES - 1 : DT_Q_WAVES, OBJ ? DT_Q_WAVES - 1 : DT_Q_WAVES))) void k_raster_q(RenderParams R, const EnvCam* __restrict__ cams, const EnvFast* __restrict__ fasts,
                                                 const EnvQ* __restrict__ envq, uint8_t* __restrict__ frames,
                                                 const uint8_t* __restrict__ qtex, const float4* __restrict__ lut, const PixTab* __restrict__ pixtab, const SampTab* __restrict__ samptab,
                                                 const uint32_t* __restrict__ qtiles, uint16_t* __restrict__ queue,
                                                 int32_t* __restrict__ qcount, const EnvL* __restrict__ envl) {
  extern __shared__ uint32_t s_mem[];
  uint32_t* s_qt = s_mem;                                                                   // [n_qtiles]
  const int tid = threadIdx.x;
  const int npix = R.W * R.H;
  const int tiles_x = (R.W + DT_TILE_W - 1) / DT_TILE_W, n_tiles = tiles_x * ((R.H + DT_TILE_H - 1) / DT_TILE_H);
  const RasterWg wg = raster_wg<SUB, /*SCALAR=*/false>(R, n_tiles, blockIdx.x);   // (tile and chunk stay as computed: this kernel was tuned so)
  if (!wg.live) return;
  const int tile = wg.tile, rwg = wg.rwg(n_tiles), e0 = wg.e0(), e1 = wg.e1();
  for (int i = tid; i < R.n_qtiles * 2; i += RB) s_qt[i] = qtiles[i];
  __syncthreads();

  const int wave = tid >> 6, lane = tid & 63;
  const int tile_x0 = (tile % tiles_x) * DT_TILE_W;
  const int wave_y0 = (tile / tiles_x) * DT_TILE_H + wave * (WAVE_PIX / WAVE_W);
  const int LS = R.qlog2;
  const uint32_t SM = (1u << LS) - 1u;
  const float lo = 0.5f * (float)(1 << LS);

  // per-pixel invariants (shared camera) from the PixTab: hit in the yaw-local frame, lit factor, MSAA reach, flags
  float lr[PPT], lf[PPT], lit[PPT];
  uint32_t Mi[PPT];
  bool cand[PPT], gok[PPT], valid[PPT];
  uint32_t spxy[PPT];                                 // OBJ: source-pixel coordinates of the slot as two halves (x | y << 16)
  bool any_cand = false;
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    PixTab t{0.f, 0.f, -1.f, 0xFFFFu};
    const bool inimg = tile_x0 + SLOT_X(k, lane) < R.W && wave_y0 + SLOT_Y(k, lane) < R.H;
    const int pix = (wave_y0 + SLOT_Y(k, lane)) * R.W + tile_x0 + SLOT_X(k, lane);
    if (inimg) t = pixtab[pix];
    lr[k] = t.lr; lf[k] = t.lf; lit[k] = fmaxf(t.lit, 0.f); Mi[k] = t.mi;
    valid[k] = t.lit >= 0.f; cand[k] = t.lit > 0.f; gok[k] = (t.mi & 0xFFFFu) != 0xFFFFu;
    any_cand |= cand[k];
    spxy[k] = 0u;
    if (OBJ && inimg) spxy[k] = spxy_pack(lut[pix], R.W, R.H);
  }

  uint16_t* w_queue = queue + ((size_t)rwg * (RB / 64) + wave) * QREGION;
  int qn = 0, qo = 0;                                  // plane-edge entries (front of the region), object-box entries (back)
  int qend_v = 0;                                      // lane l: object-entry fill after the env at position e0 + l
  uint32_t* s_px = s_mem + R.n_qtiles * 2 + wave * WAVE_PIX;
  const int st_x = tile_x0 + (lane * 4) % WAVE_W, st_y = wave_y0 + (lane * 4) / WAVE_W;
  // frame rows are dword aligned (W % 4 == 0: launch precondition; other widths take the generic k_raster)
  const bool st_ok = lane * 4 < WAVE_PIX && st_x < R.W && st_y < R.H;
  const size_t st_off = ((size_t)st_y * R.W + st_x) * 3;

  // object masks (OBJ) are indexed by position in the render order (k_obj_setup)
  ChunkObjMasks<OBJ> objmasks;
  objmasks.load(R, e0, e1, n_tiles * 4, tile * 4 + __builtin_amdgcn_readfirstlane(wave), lane);
  // pixels of this block inside the screen boxes of the objects in `om` -> appended from the far end of the region
  // pedge: the pixel is a plane edge too (what this raster stores for it is not final).  A box pixel that is none keeps the stored one-ray colour --
  // the byte-weight filter's, as every pixel outside the boxes -- unless a mesh triangle covers a sample of it (k_resolve_obj, QE_PLANE_EDGE).
  auto push_obj = [&](const int e, const uint32_t env, unsigned long long om, bool oedge[PPT], const bool pedge[PPT]) __attribute__((always_inline)) {
    const ObjBox* boxes = R.objbox + (size_t)env * DTSIM_MAX_OBJECTS;
    // The coordinates are kept as halves (registers); their rounding (<= 0.25 px below 1024) is covered by widening the
    // box: a pixel just outside a box may take the exact path for nothing, one inside always does.
    float sx[PPT], sy[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) spxy_unpack(spxy[k], sx[k], sy[k]);
    while (om) {                                     // wave-uniform
      const ObjBox ob = boxes[__builtin_ctzll(om)];
      om &= om - 1ull;
#pragma unroll
      for (int k = 0; k < PPT; ++k)
        if (valid[k] && sx[k] >= ob.bx0 - 0.3f && sx[k] <= ob.bx1 + 0.3f && sy[k] >= ob.by0 - 0.3f && sy[k] <= ob.by1 + 0.3f) oedge[k] = true;
    }
    bool any_oedge = false;
#pragma unroll
    for (int k = 0; k < PPT; ++k) any_oedge |= oedge[k];
    if (__ballot(any_oedge)) {                       // wave-uniform (a pixel is in one list or the other: the region never overflows)
      const uint32_t etag = (uint32_t)(e - e0) << 8;
#pragma unroll
      for (int k = 0; k < PPT; ++k) {
        const bool ek = oedge[k];
        const unsigned long long mk = __ballot(ek);
        if (ek) {
          const int rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u));
          w_queue[QREGION - 1 - (qo + rank)] = (uint16_t)(etag | (pedge[k] ? QE_PLANE_EDGE : 0u) | (uint32_t)(k * 64 + lane));
        }
        qo += __popcll(mk);
      }
    }
  };
  const bool wave_sky = !__ballot(any_cand);
  if (wave_sky) {
    // ---- all sky / border for every env: the lane's 12 bytes are the horizon colour pattern, masked where the
    // source pixel lies outside the rectilinear image.
#pragma unroll
    for (int k = 0; k < PPT; ++k) s_px[k * 64 + lane] = valid[k] ? 0xFFFFFFFFu : 0u;
    const uint4 vm = *reinterpret_cast<const uint4*>(s_px + (lane * 4) % WAVE_PIX);
    const uint32_t m0 = (vm.x & 0x00FFFFFFu) | (vm.y << 24), m1 = ((vm.y >> 8) & 0xFFFFu) | (vm.z << 16), m2 = ((vm.z >> 16) & 0xFFu) | (vm.w << 8);
    for (int e = e0; e < e1; ++e) {
      const EnvQ f = envq[e];
      const unsigned long long om = objmasks.of(e);
      if (st_ok) {
        uint32_t* d32 = reinterpret_cast<uint32_t*>(frames + (size_t)f.env * npix * 3 + st_off);
        d32[0] = f.sky[0] & m0; d32[1] = f.sky[1] & m1; d32[2] = f.sky[2] & m2;
      }
      if (OBJ && om) {                               // mesh objects in front of the sky
        bool oedge[PPT], pedge[PPT];                 // (no plane edge in an all-sky block: the stored horizon colour is final)
#pragma unroll
        for (int k = 0; k < PPT; ++k) oedge[k] = pedge[k] = false;
        push_obj(e, f.env, om, oedge, pedge);
      }
      if (OBJ) qend_v = lane >= e - e0 ? qo : qend_v;
    }
    if (lane == 0) qcount[rwg * (RB / 64) + wave] = OBJ ? qo : 0;
  } else {
  typedef float f2 __attribute__((ext_vector_type(2)));
  static_assert(PPT % 2 == 0, "pixel slots are processed in pairs (packed fp32)");
  f2 lr2[PPT / 2], lf2[PPT / 2], lit2[PPT / 2];
#pragma unroll
  for (int j = 0; j < PPT / 2; ++j) {
    lr2[j] = f2{lr[2 * j], lr[2 * j + 1]}; lf2[j] = f2{lf[2 * j], lf[2 * j + 1]}; lit2[j] = f2{lit[2 * j], lit[2 * j + 1]};
  }
  const char* s_qtb = reinterpret_cast<const char*>(s_qt);
  unsigned long long candm[PPT], validm[PPT], plainm[PPT];
#pragma unroll
  for (int k = 0; k < PPT; ++k) { candm[k] = __ballot(cand[k]); validm[k] = __ballot(valid[k]); plainm[k] = __ballot(gok[k]); }
  uint32_t blk_reach;                                // farthest tile-plane hit of the wavefront's pixels from the camera, cells
  {
    float r2 = 0.f;
#pragma unroll
    for (int k = 0; k < PPT; ++k) r2 = fmaxf(r2, lr[k] * lr[k] + lf[k] * lf[k]);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) r2 = fmaxf(r2, __shfl_xor(r2, d));
    const float r = fsqrt_(r2) * R.q_per_m * 1.0001f + 1.f;
    blk_reach = (uint32_t)__builtin_amdgcn_readfirstlane((int)(r < 1.0e9f ? (uint32_t)r : 0x7FFFFFFFu));
  }
  bool any_invalid = false;                          // wave-uniform
#pragma unroll
  for (int k = 0; k < PPT; ++k) any_invalid |= validm[k] != ~0ull;
  // The env loop is software-pipelined two deep: the quad loads of env e+1 are issued BEFORE the frame stores of env e.
  // gfx950 retires vector memory operations of a wavefront in issue order (one vmcnt for loads and stores), so a
  // load issued after a store cannot be waited for without also waiting for that store's write acknowledge; with the
  // loads of the next env ahead of the stores, a wavefront only ever waits for stores that are two envs old.
  struct QStage { uint4 q[PPT]; f2 ax2[PPT / 2], az2[PPT / 2]; };
  auto issue_t = [&](const EnvQ& f, QStage& st, auto clamp_tag) __attribute__((always_inline)) {
    constexpr bool CLAMP = decltype(clamp_tag)::value;
    const f2 vA = f2{f.A, f.A}, vB = f2{f.B, f.B}, vCx = f2{f.Cx, f.Cx}, vCz = f2{f.Cz, f.Cz}, vK = f2{Q8_SNAP, Q8_SNAP};
#pragma unroll
    for (int j = 0; j < PPT / 2; ++j) {
      // two pixels per packed op: X = Cx + lr*A + lf*B, Z = Cz + lr*B - lf*A
      // (+ Q8_SNAP as a third, separate add: ONE rounding to 256ths of a texel; the sum's bits are the fixed-point coordinate, see quad_weights8)
      const f2 X2 = fma2(lf2[j], vB, fma2(lr2[j], vA, vCx)) + vK;       // (explicit fused multiply-adds in resolve_region_q's order: the snap makes the last bit visible)
      const f2 Z2 = fma2(lf2[j], -vA, fma2(lr2[j], vB, vCz)) + vK;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int k = 2 * j + h;
        float X = h ? X2.y : X2.x, Z = h ? Z2.y : Z2.x;
        if (CLAMP) { X = med3f(X, lo + Q8_SNAP, f.Xhi + Q8_SNAP); Z = med3f(Z, lo + Q8_SNAP, f.Zhi + Q8_SNAP); }
        const uint32_t xb = __float_as_uint(X), zb = __float_as_uint(Z);
        if (h) { st.ax2[j].y = q8_frac(xb); st.az2[j].y = q8_frac(zb); }
        else { st.ax2[j].x = q8_frac(xb); st.az2[j].x = q8_frac(zb); }
        // block offset of the cell's tile: LDS table, byte address = tab_b + (zi >> LS) * pitch4 + ((xi >> LS) << 2)
        // The table entry is 8 bytes: the block's byte offset and how the cell index is formed -- for the two
        // one-record blocks (off-grid, untextured) every cell maps to record 0, so they do not occupy cache lines.
        uint32_t ta, local;
        if (S256) {   // S = 256 and a padded grid under 128 tiles: tile = byte 2, cell = byte 1 of the snapped coordinate
          uint32_t t1, t2;
          asm("v_mul_u32_u24_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_2 src1_sel:DWORD" : "=v"(t1) : "v"(zb), "s"(f.pitch4));
          asm("v_lshlrev_b32_sdwa %0, 3, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_2" : "=v"(t2) : "v"(xb));
          ta = t1 + t2 + f.tab_b;
        } else ta = ((q8_cell(xb) >> LS) << 3) + (__umul24(q8_cell(zb) >> LS, f.pitch4) + f.tab_b);
        const uint2 te = *reinterpret_cast<const uint2*>(s_qtb + ta);
        const uint32_t tb = te.x;
        if (S256) local = q8_rec256(xb, zb, te.y) >> 4;                        // te.y: mask of the record's byte offset (4 x 2 cells per line), or 0
        else local = (((q8_cell(zb) & SM) << LS) | (q8_cell(xb) & SM)) & te.y; // te.y: cell mask
        st.q[k] = *reinterpret_cast<const uint4*>(qtex + (tb + (local << 4)));
      }
    }
  };
  // The lane's 12 bytes of frame e.  The store is unconditional (no branch around it, so that the wait counts the
  // compiler derives for the texel loads do not have to cover it): lanes without pixels write to a dump slot.
  uint8_t* const st_base = st_ok ? frames + st_off : reinterpret_cast<uint8_t*>(R.dump) + lane * 16;
  const uint32_t st_stride = st_ok ? (uint32_t)npix * 3u : 0u;
  auto store = [&](const uint32_t env, const U3& o) __attribute__((always_inline)) {   // env: frame index
    uint32_t* d = reinterpret_cast<uint32_t*>(st_base + (size_t)env * st_stride);
    // non-temporal: the frame is written once and not read back by this pass; keep the taps in L2
    __builtin_nontemporal_store(o.a, d); __builtin_nontemporal_store(o.b, d + 1); __builtin_nontemporal_store(o.c, d + 2);
  };
  // Clamping the coordinates into the padded grid (two v_med3 per pixel) is only needed when a hit of this block can
  // leave it: the block's farthest hit (cells, env-invariant) against the camera's distance to the border (per env).
  auto issue = [&](const EnvQ& f, QStage& st) __attribute__((always_inline)) {
#if DT_Q_PRIO
    __builtin_amdgcn_s_setprio(DT_Q_PRIO);           // a wavefront about to issue its quad loads goes first
#endif
    if (f.reach > blk_reach) issue_t(f, st, std::false_type{});       // wave-uniform, scalar compare
    else issue_t(f, st, std::true_type{});
#if DT_Q_PRIO
    __builtin_amdgcn_s_setprio(0);
#endif
  };
  auto finish = [&](const int e, const uint32_t env, const uint32_t hor_rgb, const QStage& st, unsigned long long om) __attribute__((always_inline)) -> U3 {   // e: position, env: frame, om: object mask of the block (OBJ)
    U3 out{0u, 0u, 0u};
    uint32_t px[PPT];
    bool edge[PPT], oedge[PPT];                      // oedge: inside a mesh object's screen box (OBJ)
    unsigned long long fastm[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) oedge[k] = false;
    const uint4* q = st.q;
    const f2* ax2 = st.ax2; const f2* az2 = st.az2;
    unsigned long long slow = 0ull;                  // lane masks live in SGPR pairs: predicate logic on the scalar unit
    const uint32_t hor_v = hor_rgb;
#pragma unroll
    for (int j = 0; j < PPT / 2; ++j) {
      if (j) __builtin_amdgcn_sched_barrier(0);      // one pixel pair at a time: fewer live temporaries
      // bilinear weights with the lit factor folded in (quad_weights8's operations: fractions in 256ths, lit / 256), two pixels per packed op
      f2 w00, w10, w01, w11;
      {
#pragma clang fp contract(off)
        f2 I2 = lit2[j] * Q8_LIT;
        if constexpr (LIGHT) I2 = env_lit8_2(envl[e], lr2[j], lf2[j]);
        const f2 c256 = f2{256.f, 256.f};
        const f2 u = ax2[j] * I2, v = fma2(I2, c256, -u);
        w11 = u * az2[j]; w01 = v * az2[j];
        w10 = fma2(u, c256, -w11); w00 = fma2(v, c256, -w01);
      }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int k = 2 * j + h;
        const unsigned long long fm = __ballot((q[k].w & 0xFFFFu) > (Mi[k] & 0xFFFFu));
        fastm[k] = fm;
        slow |= candm[k] & ~fm;
        edge[k] = false;
        uint32_t W = __builtin_amdgcn_cvt_pk_u8_f32(h ? w00.y : w00.x, 0, 0u);
        W = __builtin_amdgcn_cvt_pk_u8_f32(h ? w10.y : w10.x, 1, W);
        W = __builtin_amdgcn_cvt_pk_u8_f32(h ? w01.y : w01.x, 2, W);
        W = __builtin_amdgcn_cvt_pk_u8_f32(h ? w11.y : w11.x, 3, W);
        const uint32_t vr = __builtin_amdgcn_udot4(q[k].x, W, 128u, false), vg = __builtin_amdgcn_udot4(q[k].y, W, 128u, false),
                       vb = __builtin_amdgcn_udot4(q[k].z, W, 128u, false);          // the channel is byte 1 of each sum (quad_filter)
        const uint32_t rg = __builtin_amdgcn_perm(vg, vr, 0x0c0c0501u);
        const uint32_t rgb = __builtin_amdgcn_perm(vb, rg, 0x0c050100u);
        asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(px[k]) : "v"(hor_v), "v"(rgb), "s"(fm));   // not a one-ray tile pixel: clear colour
      }
    }
    if (slow) {                                      // wave-uniform: some pixel is not a certain tile interior
      // Per pixel slot, and only for the slots that have such lanes (scalar tests on lane masks):
      //   off-grid cell: ground quad, if every sample stays off the grid and inside the quad;
      //   anything else: queued for k_resolve -- the seam cell (half of it belongs to the neighbour tile, whose taps
      //     the record does not hold), untextured tiles, the horizon band, and the textured cells the cell-granular
      //     test rejected (conservative by up to a cell; k_resolve redoes it exactly on compacted lanes, which is
      //     cheaper than refining here at a few live lanes per wavefront).
#pragma unroll
      for (int k = 0; k < PPT; ++k) {
        const unsigned long long sk = candm[k] & ~fastm[k];
        if (!sk) continue;                           // wave-uniform
        const bool sl = (sk >> lane) & 1ull;
        const unsigned long long gm = sk & __ballot((q[k].w >> 16) != 0u) & plainm[k];
        edge[k] = sl;
        if (gm) {
          const float lrk = (k & 1) ? lr2[k / 2].y : lr2[k / 2].x, lfk = (k & 1) ? lf2[k / 2].y : lf2[k / 2].x;
          const float mrgk = __half2float(__ushort_as_half((unsigned short)(Mi[k] >> 16)));
          const EnvFast g = fasts[env];              // scalar loads, only on this (ground beyond the map) path: a load at the
          const EnvCam c = cams[env];                // top of the slow branch would be waited for by every LDS access after it
          const float wx = c.Cx + lrk * c.sa + lfk * c.ca, wz = c.Cz + lrk * c.ca - lfk * c.sa;          // tile-plane hit, world
          const float wxg = fmaf(g.kg, wx - c.Cx, c.Cx), wzg = fmaf(g.kg, wz - c.Cz, c.Cz);              // ground-quad hit
          // every sample's tile-plane hit stays clear of the grid rectangle (an absent tile inside the grid goes to
          // the exact path)
          const bool clear = (wx < -mrgk) | (wx > g.gw_m + mrgk) | (wz < -mrgk) | (wz > g.gh_m + mrgk);
          const bool inq = (fabsf(wxg) + 2.f * mrgk < GROUND_HALF) & (fabsf(wzg) + 2.f * mrgk < GROUND_HALF);
          const bool gfast = ((gm >> lane) & 1ull) & clear & inq;
          const float ndl = ground_ndl(c, wxg, wzg);
          uint32_t rgb = 0;
          rgb = __builtin_amdgcn_cvt_pk_u8_f32(c.gnd[0] * fminf(c.base[0] + c.dif[0] * ndl, 1.f), 0, rgb);
          rgb = __builtin_amdgcn_cvt_pk_u8_f32(c.gnd[1] * fminf(c.base[1] + c.dif[1] * ndl, 1.f), 1, rgb);
          rgb = __builtin_amdgcn_cvt_pk_u8_f32(c.gnd[2] * fminf(c.base[2] + c.dif[2] * ndl, 1.f), 2, rgb);
          px[k] = gfast ? rgb : px[k];
          edge[k] = sl & !gfast;
        }
      }
    }

    if (OBJ && om) push_obj(e, env, om, oedge, edge);   // wave-uniform: some object's screen box meets this block

    if (any_invalid) {                               // wave-uniform, rare: source pixels outside the rectilinear image are 0
#pragma unroll
      for (int k = 0; k < PPT; ++k) px[k] = ((validm[k] >> lane) & 1ull) ? px[k] : 0u;
    }
#pragma unroll
    for (int k = 0; k < PPT; ++k) s_px[k * 64 + lane] = px[k];
    const uint4 o = *reinterpret_cast<const uint4*>(s_px + (lane * 4) % WAVE_PIX);
    // 4 pixels 0x00BBGGRR -> 12 bytes: three byte permutes
    out = U3{__builtin_amdgcn_perm(o.y, o.x, 0x04020100u), __builtin_amdgcn_perm(o.z, o.y, 0x05040201u), __builtin_amdgcn_perm(o.w, o.z, 0x06050402u)};

    bool any_edge = false;
#pragma unroll
    for (int k = 0; k < PPT; ++k) { edge[k] &= !oedge[k]; any_edge |= edge[k]; }
    const uint32_t etag = (uint32_t)(e - e0) << 8;
    if (__ballot(any_edge)) {                          // wave-uniform
#pragma unroll
      for (int k = 0; k < PPT; ++k) {
        const bool ek = edge[k];
        const unsigned long long mk = __ballot(ek);
        if (ek) {
          const int rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u));
          w_queue[qn + rank] = (uint16_t)(etag | (uint32_t)(k * 64 + lane));
        }
        qn += __popcll(mk);
      }
    }
    return out;
  };
  {  // one stage, deferred store: the 12 bytes of env e-1 are held in registers and stored right after the loads of
     // env e have been issued, so that waiting for those loads never waits for a store of the same iteration.
     // No branch between the loads and the store (first env peeled).
    QStage sa;
    EnvQ f = envq[e0];
    issue(f, sa);
    uint32_t hor = f.hor_rgb, env = f.env, env_prev;
    f = envq[min(e0 + 1, e1 - 1)];
    U3 held = finish(e0, env, hor, sa, objmasks.of(e0));
    if (OBJ) qend_v = qo;
    for (int e = e0 + 1; e < e1; ++e) {
      env_prev = env; hor = f.hor_rgb; env = f.env;
      issue(f, sa);
      store(env_prev, held);
      f = envq[min(e + 1, e1 - 1)];                  // next env's constants: the scalar load has the whole filter to land
      held = finish(e, env, hor, sa, objmasks.of(e));
      if (OBJ) qend_v = lane >= e - e0 ? qo : qend_v;
    }
    store(env, held);
  }
  if (lane == 0) qcount[rwg * (RB / 64) + wave] = OBJ ? qo : qn;
  if (qn > 0) {
    // exact path for this wavefront's own edge pixels, right here (the frame stores of the env loop are ordered
    // before the byte patches: same wavefront, same addresses)
    __builtin_amdgcn_s_waitcnt(0);                 // queue stores have left the wavefront
    resolve_region_q<S256, LIGHT>(R, cams, envq, pixtab, samptab, qtex, s_qt, s_px, w_queue, qn, e0, tile_x0, wave_y0, lane, envl);
  }
  }
  if (OBJ) {   // mesh objects: k_resolve_obj drains the object-box entries (back of the regions) -- work items for it, every env group
    if (lane < ENVS_PER_BLOCK) R.qend[((size_t)rwg * (RB / 64) + wave) * ENVS_PER_BLOCK + lane] = (uint16_t)qend_v;
    __shared__ int s_nb[RB / 64];
    if (lane == 0) s_nb[wave] = qo;
    __syncthreads();
    if (tid == 0) {
      int nb = 0;
#pragma unroll
      for (int r = 0; r < RB / 64; ++r) nb += s_nb[r];
      if (nb > 0) push_obj_items(R, (uint32_t)rwg);
    }
  }
}

}  // namespace


// ---- the render scratch: every array of the slabs (dtsim_dev.h RenderSlab), each from a 64-byte boundary ----------------------------------
#define DT_SCRATCH_ALIGN 64
static_assert(DT_SCRATCH_ALIGN % 64 == 0 && DT_SCRATCH_ALIGN % alignof(EnvD) == 0 && DT_SCRATCH_ALIGN % alignof(float4) == 0,
              "EnvQ, EnvV and EnvD records are 64-byte aligned (one scalar load each), tribox 16-byte aligned (float4)");
struct Slab {                                         // the arrays of one allocation, one after the other (base null: sizes only)
  char* base; size_t bytes = 0;
  template <class T> T* take(size_t n) {
    const size_t off = (bytes + DT_SCRATCH_ALIGN - 1) / DT_SCRATCH_ALIGN * DT_SCRATCH_ALIGN;
    bytes = off + n * sizeof(T); return base ? reinterpret_cast<T*>(base + off) : nullptr;
  }
};
EnvRecs dt_render_layout(int N, int W, int H, int max_tris, size_t* bytes, void* const* base, RenderParams* R_out) {
  RenderParams tmp{}; RenderParams& R = R_out ? *R_out : tmp;
  const size_t n = (size_t)N, n_pix = (size_t)W * H, n_tiles = dt_raster_tiles(W, H), n_wg = dt_raster_groups(N, W, H);
  Slab sl[DT_SLABS];                                  // (null bases: sizes only)
  for (int i = 0; i < DT_SLABS; ++i) sl[i].base = base ? static_cast<char*>(base[i]) : nullptr;
  Slab &env = sl[DT_SLAB_ENV], &pix = sl[DT_SLAB_PIX], &qc = sl[DT_SLAB_QCOUNT], &it = sl[DT_SLAB_ITEMS], &ob = sl[DT_SLAB_OBJMASK];
  EnvRecs x;                                          // EnvV and EnvL: one record more (the env loops prefetch one past their chunk)
  R.envcam = x.cams = env.take<EnvCam>(n); x.fasts = env.take<EnvFast>(n); x.envq = env.take<EnvQ>(n); R.envpos = env.take<int32_t>(n);
  R.envv = x.envv = env.take<EnvV>(n + 1); R.envd = x.envd = env.take<EnvD>(n); x.envl = env.take<EnvL>(n + 1);
  R.pixtab = x.pixtab = pix.take<PixTab>(n_pix); x.samptab = pix.take<SampTab>(n_pix); R.dump = pix.take<RenderDump>(1);
  R.queue = sl[DT_SLAB_QUEUE].take<uint16_t>(n_wg * (RB / 64) * QREGION);
  R.qcount = qc.take<int32_t>(n_wg * (RB / 64)); R.work = qc.take<int32_t>(DT_WORK_INTS);
  R.items = it.take<uint32_t>(n_wg * ITEMS_PER_WG); R.items2 = it.take<uint32_t>(n_wg * ENVS_PER_BLOCK);   // items2: k_resolve_obj's, at most one per env of a workgroup
  R.qend = sl[DT_SLAB_QEND].take<uint16_t>(n_wg * (RB / 64) * ENVS_PER_BLOCK);
  if (max_tris > 0) {
    R.stris = sl[DT_SLAB_STRIS].take<ScreenTri>(n * max_tris); R.tribox = sl[DT_SLAB_STRIS].take<float4>(n * max_tris);
    R.objbox = sl[DT_SLAB_OBJBOX].take<ObjBox>(n * DTSIM_MAX_OBJECTS);
    R.blockbox = reinterpret_cast<float*>(ob.take<float4>(n_tiles * 4)); R.objrange = ob.take<uint2>((size_t)DTSIM_MAX_MAPS * DTSIM_MAX_OBJECTS);
    R.objmask = ob.take<unsigned long long>(n * n_tiles * 4);
  }
  if (bytes) for (int i = 0; i < DT_SLABS; ++i) bytes[i] = sl[i].bytes;
  return x;
}

int dt_raster_pipe(RenderParams& R, int grid_rows, int grid_cols, bool raster_old) {
  // k_raster_v3 / k_raster_v3dr: 256 x 256 tile textures; the maps' padded grids side by side in one LDS tile table
  const bool v3 = R.qlog2 == 8 && grid_rows <= V3_MAX_ROWS && grid_cols <= V3_MAP_COLS && R.n_maps * V3_MAP_COLS <= V3_TAB_PITCH / 2 && !raster_old;
  R.q3_rows = v3 ? grid_rows : 0;
  const bool records = R.qtex && !R.segment && (R.W & 3) == 0;   // the quad records (none with gl_filter)
  // shared camera: square power-of-two tile textures (S = 256 tables carry the record-offset mask of the S256 kernels -- q8_rec256 --,
  // which need a padded grid under 128 tiles: Q8_SNAP)
  if (records && !R.domain_rand && (size_t)R.n_qtiles * 8 <= 32768 && !(R.qlog2 == 8 && R.qmax_tiles >= 256)) return v3 ? DTSIM_PIPE_V3 : DTSIM_PIPE_Q;
  if (records && R.domain_rand && v3) return DTSIM_PIPE_V3DR;   // domain randomisation on the quad records
  return (R.domain_rand || R.segment || R.light) ? DTSIM_PIPE_GENERIC_ENV : DTSIM_PIPE_GENERIC;   // the generic k_raster
}

// The batch through raster `pipe`, on stream s (after dt_launch_render_setup, before dt_launch_render_exact).
// SUB: the masked pass -- the quad-record rasters' SUB instantiations over positions [0, live) (never the generic raster).
template <bool SUB>
static void launch_raster(hipStream_t s, const RenderParams& R, const EnvRecs& x, int pipe) {
  const bool obj = R.max_tris > 0;
  const int n_chunks = (R.N + ENVS_PER_BLOCK - 1) / ENVS_PER_BLOCK;
  const size_t lds1 = (size_t)R.n_tile_recs * sizeof(TileLds) + (size_t)RB * PPT * sizeof(uint32_t);   // the tile records + store transpose
  const dim3 grid((unsigned)(dt_raster_tiles(R.W, R.H) * n_chunks));
  const dim3 gridq((unsigned)raster_wg_grid(dt_raster_tiles(R.W, R.H), n_chunks));   // the quad-record rasters' XCD-affine map (raster_wg)
  const size_t ldsq = (size_t)R.n_qtiles * 8 + (size_t)RB * PPT * sizeof(uint32_t);
  const bool s256 = R.qlog2 == 8 && R.qmax_tiles < 256;
#define LAUNCH_RASTER(DR_, OBJ_)                                                                              \
  hipLaunchKernelGGL((k_raster<DR_, OBJ_>), grid, dim3(RB), lds1, s, R, x.cams, x.fasts, R.frames, R.texels,                  \
                     reinterpret_cast<const float4*>(R.lut), R.maps, R.tile_recs, R.queue, R.qcount)
#define LAUNCH_Q(OBJ_, S256_) do { if (R.light) hipLaunchKernelGGL((k_raster_q<OBJ_, S256_, true, SUB>), gridq, dim3(RB), ldsq, s, R, x.cams, x.fasts, x.envq, R.frames, \
                                           R.qtex, reinterpret_cast<const float4*>(R.lut), x.pixtab, x.samptab, R.qtiles, R.queue, R.qcount, x.envl); \
                                else hipLaunchKernelGGL((k_raster_q<OBJ_, S256_, false, SUB>), gridq, dim3(RB), ldsq, s, R, x.cams, x.fasts, x.envq, R.frames, R.qtex, \
                                           reinterpret_cast<const float4*>(R.lut), x.pixtab, x.samptab, R.qtiles, R.queue, R.qcount, nullptr); } while (0)
  switch (pipe) {
    case DTSIM_PIPE_V3: dt_launch_raster_v3(s, R, x, SUB); break;                     // render_v3.hip
    case DTSIM_PIPE_Q: if (obj) { if (s256) LAUNCH_Q(true, true); else LAUNCH_Q(true, false); } else if (s256) LAUNCH_Q(false, true); else LAUNCH_Q(false, false); break;
    case DTSIM_PIPE_V3DR: dt_launch_raster_v3dr(s, R, x, SUB); break;                 // render_v3.hip: k_raster_v3dr, then k_resolve_dr on its plane-edge pixels
    case DTSIM_PIPE_GENERIC_ENV: if (obj) LAUNCH_RASTER(true, true); else LAUNCH_RASTER(true, false); break;   // per-env EnvCam (light: the shared camera's, with the env's light)
    default: if (obj) LAUNCH_RASTER(false, true); else LAUNCH_RASTER(false, false);
  }
#undef LAUNCH_Q
#undef LAUNCH_RASTER
}

int dt_launch_render(hipStream_t s, const SimArrays& A, const RenderParams& R, const EnvRecs& x, int pipe, int tables, const uint8_t* mask) {
  const RenderSetup st = dt_launch_render_setup(s, A, R, x, pipe, tables, mask);   // render_setup.hip
  if (st.sub) launch_raster<true>(s, R, x, pipe); else launch_raster<false>(s, R, x, pipe);
  dt_launch_render_exact(s, R, x, pipe, st.has_pos);                                // render_exact.hip
  return st.tables;
}
