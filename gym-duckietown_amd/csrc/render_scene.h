// render_scene.h -- the scene as one camera ray sees it: what the render pass (render_setup.hip, the rasters, render_exact.hip) and the kernels that read what a pass leaves
// behind (render_views.hip) both use, so that an overlay, a depth or a label is decided by the frame's own code.  On the per-env camera record (EnvCam, render_records.h):
// the planes and their ownership test (classify), the z-buffer test of one projected mesh triangle (test_tri), and the two GL rules every
// per-sample path must agree on: the MSAA sample positions (MSAA_POS) and the source-pixel centre of an NDC point (src_px).
// A device header with internal linkage: each unit compiles its own copy with its own flags (all with render.hip's, build.py).
#ifndef DTSIM_RENDER_SCENE_H
#define DTSIM_RENDER_SCENE_H
#include "dtsim_dev.h"

#define CLS_SKY 0
#define CLS_GROUND 1
#define CLS_TILE 2

#define NEAR_Z 0.04f
#define FAR_Z 100.0f
#define GROUND_Y (-0.008f)   // ground quad: y=-0.8 scaled by 0.01 (simulator.py:510-526,1810)
#define GROUND_HALF 50.0f

namespace {

// Camera intrinsics / light shared by all envs when DTSIM_F_DOMAIN_RAND is off
// (simulator.py:119-131 CAMERA_ANGLE / CAMERA_FOV_Y / CAMERA_FLOOR_DIST, :570-576).
struct CamShared { float sth, cth, tx, ty, Cy, base, dif; float L[4]; };

__device__ inline CamShared default_cam(float aspect) {
  CamShared s;
  const float th = 19.15f * 0.017453292519943295f;
  s.sth = sinf(th); s.cth = cosf(th);
  s.ty = tanf(0.5f * 75.0f * 0.017453292519943295f); s.tx = s.ty * aspect;
  s.Cy = 0.108f; s.base = 0.3f + 0.25f; s.dif = 0.35f;
  s.L[0] = 0.f; s.L[1] = 3.f; s.L[2] = 0.f; s.L[3] = 1.f;
  return s;
}

// ---- per-map constants the raster needs (wave-uniform) -------------------------------
struct MapU { float its, ts, gwf, ghf; int gw, gh, tile_off; };

__device__ inline MapU map_u(const RenderMapDev& m) {
  MapU u;
  u.its = m.inv_tile_size; u.ts = m.tile_size; u.gw = m.grid_w; u.gh = m.grid_h;
  u.gwf = (float)m.grid_w; u.ghf = (float)m.grid_h; u.tile_off = m.tile_off;
  return u;
}

// 1-ulp hardware reciprocal / rsqrt / sqrt: a relative error of 1e-7 moves a ground hit by < 1e-3 texel
__device__ inline float frcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ inline float frsq(float x) { return __builtin_amdgcn_rsqf(x); }
__device__ inline float fsqrt_(float x) { return __builtin_amdgcn_sqrtf(x); }

struct Ray { float xe, ye, yla, fwd; };

__device__ inline Ray make_ray(float nx, float ny, float tx, float ty, float sth, float cth) {
  Ray r;
  r.xe = nx * tx; r.ye = ny * ty;
  r.yla = r.ye * cth - sth;      // world-up component of the ray
  r.fwd = r.ye * sth + cth;      // component along dir
  return r;
}

// positional / directional light on a surface with eye-space normal (0, cth, sth) at the
// eye-space point t*(xe, ye, -1): max(0, N.L)   (tiles; simulator.py:565-591)
__device__ inline float plane_ndl(const float L[4], float sth, float cth, const Ray& r, float t) {
  float ndl;
  if (L[3] == 0.f) ndl = cth * L[1] + sth * L[2];
  else {
    const float lx = L[0] - t * r.xe, ly = L[1] - t * r.ye, lz = L[2] + t;
    ndl = (cth * ly + sth * lz) * frsq(lx * lx + ly * ly + lz * lz);
  }
  return fmaxf(ndl, 0.f);
}

// The texel coordinates of a textured tile at tile fraction (fx, fz): the record's affine map (tile angle, uv = (pu, 1 - pv), the GL_LINEAR
// half-texel shift: x = u TW - 0.5, y = v TH - 0.5).  tile_color filters there; k_labels takes the nearest texel.
__device__ inline void tile_texel_xy(const TileLds& tr, const float fx, const float fz, float& x, float& y) {
  x = fmaf(tr.mxz, fz, fmaf(tr.mxx, fx, tr.ox)); y = fmaf(tr.myz, fz, fmaf(tr.myx, fx, tr.oy));
}

struct Hit { int cls; int ti, tj; float t, wx, wz; };

__device__ inline void plane_hit(const EnvCam& c, const Ray& r, float h, float& t, float& wx, float& wz) {
  t = h * frcp(-r.yla);
  const float rr = t * r.xe, ff = t * r.fwd;
  wx = c.Cx + rr * c.sa + ff * c.ca;
  wz = c.Cz + rr * c.ca - ff * c.sa;
}

__device__ inline Hit classify(const EnvCam& c, const MapU& m, const TileLds* tiles, const Ray& r) {
  Hit h;
  h.cls = CLS_SKY; h.ti = h.tj = 0; h.t = 0.f; h.wx = h.wz = 0.f;
  if (!(r.yla < 0.f)) return h;
  float t, wx, wz;
  plane_hit(c, r, c.Cy, t, wx, wz);                 // tile plane y = 0
  if (t >= NEAR_Z && t <= FAR_Z) {
    const float fi = floorf(wx * m.its), fj = floorf(wz * m.its);
    if (fi >= 0.f && fj >= 0.f && fi < m.gwf && fj < m.ghf) {
      const int i = (int)fi, j = (int)fj;
      if (tiles[m.tile_off + j * m.gw + i].flags & 1u) {
        h.cls = CLS_TILE; h.ti = i; h.tj = j; h.t = t; h.wx = wx; h.wz = wz;
        return h;
      }
    }
  }
  plane_hit(c, r, c.Cy - GROUND_Y, t, wx, wz);      // ground quad y = -0.008
  if (t >= NEAR_Z && t <= FAR_Z && fabsf(wx) <= GROUND_HALF && fabsf(wz) <= GROUND_HALF) {
    h.cls = CLS_GROUND; h.t = t; h.wx = wx; h.wz = wz;
  }
  return h;
}

// The two GL rules every per-sample path agrees on, stated here and nowhere else.  The 4 MSAA samples of a pixel, as offsets from its centre in
// pixels: GL_SAMPLE_POSITION of Mesa llvmpipe, rows flipped (+y down the image); the sites bind the arrays by reference and index them unrolled.
struct MsaaPos { float x[4], y[4]; };
constexpr MsaaPos MSAA_POS = {{-0.125f, 0.375f, -0.375f, 0.125f}, {0.375f, 0.125f, -0.125f, -0.375f}};

// The centre (sx, sy), in pixels of the W x H rectilinear source image (+y down), of the NDC point (nx, ny): of a LUT entry l, (l.x, l.y).
__device__ inline void src_px(const float nx, const float ny, const int W, const int H, float& sx, float& sy) {
  sx = (nx + 1.f) * 0.5f * (float)W; sy = (1.f - ny) * 0.5f * (float)H;
}

// z-buffer one mesh triangle against the 4 samples of the pixel centred at (pcx, pcy) px.  Depth is kept as
// w = 1 / depth (larger = nearer; 0 = nothing yet): barycentrics and w are affine in the sample position, so a triangle
// costs one set-up at the pixel centre + two fused multiply-adds per quantity and sample, and no division.
template <typename Tri>
__device__ inline void test_tri_inside(const Tri& st, float pcx, float pcy, float wbest[4], int tbest[4]);
template <typename Tri>
__device__ inline void test_tri(const Tri& st, float pcx, float pcy, float wbest[4], int tbest[4]) {
  if (pcx < st.bx0 || pcx > st.bx1 || pcy < st.by0 || pcy > st.by1) return;
  test_tri_inside(st, pcx, pcy, wbest, tbest);
}
// ... the pixel centre is already known to lie in the triangle's (padded) screen box
template <typename Tri>
__device__ inline void test_tri_inside(const Tri& st, float pcx, float pcy, float wbest[4], int tbest[4]) {
  const auto &ox = MSAA_POS.x, &oy = MSAA_POS.y;
  // b0(q) = ((x1-qx)(y2-qy) - (x2-qx)(y1-qy)) / area: d/dqx = (y1-y2)/area, d/dqy = (x2-x1)/area; b1 likewise;
  // w(q) = iw2 + b0 (iw0 - iw2) + b1 (iw1 - iw2)
  const float ia = st.inv_area;
  const float e0x = st.sx[0] - pcx, e0y = st.sy[0] - pcy, e1x = st.sx[1] - pcx, e1y = st.sy[1] - pcy, e2x = st.sx[2] - pcx, e2y = st.sy[2] - pcy;
  const float b0c = (e1x * e2y - e2x * e1y) * ia, b1c = (e2x * e0y - e0x * e2y) * ia;
  const float g0x = (e1y - e2y) * ia, g0y = (e2x - e1x) * ia, g1x = (e2y - e0y) * ia, g1y = (e0x - e2x) * ia;
  const float d0 = st.iw[0] - st.iw[2], d1 = st.iw[1] - st.iw[2];
  const float wc = fmaf(b1c, d1, fmaf(b0c, d0, st.iw[2]));
  const float gwx = fmaf(g1x, d1, g0x * d0), gwy = fmaf(g1y, d1, g0y * d0);
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const float b0 = fmaf(g0y, oy[s], fmaf(g0x, ox[s], b0c));
    const float b1 = fmaf(g1y, oy[s], fmaf(g1x, ox[s], b1c));
    const float b2 = 1.f - b0 - b1;
    const float w = fmaf(gwy, oy[s], fmaf(gwx, ox[s], wc));
    // depth func LESS within [near, far]; equal depth: the earlier triangle in draw order keeps the sample
    const bool in = fminf(fminf(b0, b1), b2) >= 0.f && w <= 1.f / NEAR_Z && w >= 1.f / FAR_Z;
    if (in && (w > wbest[s] || (w == wbest[s] && st.index < tbest[s]))) { wbest[s] = w; tbest[s] = st.index; }
  }
}

}  // namespace
#endif
