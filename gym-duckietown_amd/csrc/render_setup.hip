// render_setup.hip -- everything of a render pass that runs before its raster: the kernels that write what the rasters (render.hip,
// render_v3.hip) and the exact paths (render_exact.hip) read, and dt_launch_render_setup, which runs them in order on the pass's stream.
//   k_env_sort:   render order of the envs for the quad-record paths (tile under the camera, heading quadrant): an XCD's L2 serves one
//                 region of the map; DTSIM_FIELD_RENDER_POS reads the order back.
//   k_cam_setup:  one thread per env -> EnvCam (camera centre, yaw, colours, ground-corner lighting; with DR also pitch / frustum / light),
//                 128 B per env, and what each raster takes per env from it: EnvFast, EnvQ, EnvV, EnvL, EnvD (render_records.h).
//   k_blk_setup / k_obj_setup (maps with objects): source-pixel boxes of the raster wavefront blocks (env-invariant); one workgroup per env
//                 projects the env's mesh triangles to screen space (per-vertex lighting, texture index, traffic-light card by pattern,
//                 segmentation colour), reduces per-object screen boxes and writes, per (env, block), the mask of the objects whose box meets the block.
//   k_pix_setup:  the per-pixel tables of the shared camera (PixTab, SampTab; env-invariant) from pix_inv, the generic raster's own per-pixel rule.
//   Segmentation render (dtsim_render_ex): same kernels on the segmented texel pool, k_cam_setup forces the unlit state and the magenta
//                 clear / ground colour, k_obj_setup folds the mesh's flat colour into Kd.
#include "raster_common.h"

#ifndef DT_TRI_PAD
#define DT_TRI_PAD 0.5f        // round 3: was 1 px; a quarter fewer box candidates per pixel in k_resolve_obj's z-buffer, same frames
#endif

namespace {

// EnvD (render_records.h) of one env from its EnvCam and EnvQ: the per-env homography and the one-ray bounds of k_raster_v3dr (derived in
// render_v3.hip, at the kernel), and the same env packed for k_resolve_dr's gathers.  Here, ahead of k_cam_setup, its writer.
__device__ inline void fill_envd(EnvD& D, const EnvCam& c, const EnvQ& q, const RenderMapDev& m, float q_cells, int H, int W) {
  const float S = q_cells;                           // cells per tile (256)
  const float a1 = c.ty * c.cth, a2 = c.ty * c.sth;
  const float ey = (0.375f * 2.f / (float)H * 1.01f) * c.ty, cex = (0.375f * 2.f / (float)W * 1.01f) * c.tx;
  const float dy = ey * fabsf(c.cth), eys = ey * fabsf(c.sth);
  const float qpm = m.inv_tile_size * S;
  EnvDG& g = D.g; EnvDR& d = D.r;
  g.hx0 = c.Cy * c.tx * q.A; g.hx1 = c.Cy * a2 * q.B; g.hx2 = c.Cy * c.cth * q.B;
  g.hz0 = c.Cy * c.tx * q.B; g.hz1 = -c.Cy * a2 * q.A; g.hz2 = -c.Cy * c.cth * q.A;
  g.Cx = q.Cx; g.Cz = q.Cz;
  g.na1 = -a1; g.sth = c.sth;
  g.Xhi = q.Xhi; g.Zhi = q.Zhi; g.tab3 = q.tab3; g.env = q.env; g.pad[0] = g.pad[1] = 0u;
  d.dy = dy; d.a2 = a2; d.cth = c.cth; d.cE = cex + eys; d.Kr = 1.05f * c.Cy * qpm;
  d.tx = c.tx; d.ndy = -dy;
  const float kgc = (c.Cy - GROUND_Y) / c.Cy;
  // one-ray range of inv = 1 / den (t = Cy inv, rho = dy inv): rho <= 1/4, tg (1 + 2 rho) <= 0.98 far (with rho <= 1/4:
  // 1.5 tg), t (1 - 2 rho) >= 1.02 near (with rho <= 1/4: t / 2) -- pix_inv_dr's PF_ALWAYS_EDGE / PF_TILE_OK / PF_GROUND_OK,
  // conservatively
  d.inv_lo = 2.04f * NEAR_Z / c.Cy;
  d.inv_hi = fminf(0.25f / dy, 0.98f * FAR_Z / (1.5f * kgc * c.Cy));
  const float ndl = fmaxf(c.cth * c.L[1] + c.sth * c.L[2], 0.f);   // directional light on the tile plane (eye-space normal (0, cth, sth))
  if (c.L[3] != 0.f) d.inv_hi = -1.f;                // positional light: per-pixel light term -> everything to the exact path
  for (int k = 0; k < 3; ++k) d.kc[k] = fminf(c.base[k] + c.dif[k] * ndl, 1.f) * (1.f / 256.f);
  d.hor_rgb = q.hor_rgb;
  d.kg = kgc; d.gx1 = (float)m.grid_w * S; d.gz1 = (float)m.grid_h * S; d.qpm = qpm;
  for (int k = 0; k < 3; ++k) d.kcc[k] = -8388608.f * d.kc[k];
  EnvDX& x = D.x;
  x.hx0 = g.hx0; x.hx1 = g.hx1; x.hx2 = g.hx2; x.hz0 = g.hz0; x.hz1 = g.hz1; x.hz2 = g.hz2; x.Cx = q.Cx; x.Cz = q.Cz;
  x.na1 = -a1; x.sth = c.sth; x.Xhi = q.Xhi; x.Zhi = q.Zhi; x.tab3 = g.tab3; x.env = g.env; x.kg = kgc; x.qpm = qpm;
  x.Cy = c.Cy; x.positional = c.L[3] != 0.f ? -1.f : 1.f;
  for (int k = 0; k < 3; ++k) { x.kc[k] = d.kc[k]; x.hor[k] = c.hor[k]; x.gnd[k] = c.gnd[k]; x.base[k] = c.base[k]; }
  x.gndl0 = c.gndl[0]; x.gndl1 = c.gndl[1]; x.gndl2 = c.gndl[2]; x.gndl3 = c.gndl[3]; x.dif0 = c.dif[0]; x.dif1 = c.dif[1]; x.dif2 = c.dif[2];
  x.pad0 = x.pad1 = x.pad2 = 0.f;
  for (int k = 0; k < 16; ++k) D.pad_[k] = 0;
}

__device__ inline void fill_envd_at(EnvD* arr, int idx, const EnvCam& c, const EnvQ& q, const RenderMapDev& m, float q_cells, int H, int W) {
  EnvD d;
  fill_envd(d, c, q, m, q_cells, H, W);
  arr[idx] = d;
}

// Render order of the envs for the quad-layout path: envs standing on the same tile (and facing the same way) are
// made neighbours, so that the 64 envs a raster workgroup loops over -- and, with the XCD-affine workgroup map of
// k_raster_q, all the envs one XCD's L2 serves -- look at the same few texture blocks.  A counting sort by
// (tile under the camera, heading quadrant) in one workgroup; the order inside a bin is arbitrary (frames are
// independent, so the order never changes a result).  pos[e] = position of env e.
// MASKED (dtsim_render_masked): only the envs with mask[e] != 0 are binned; they take positions [0, live), the others pos = -1, and the
// live count goes to *live (the SUB rasters read it at entry).
// Past KEEP * 1024 envs bin_of runs twice per env, and nothing here makes the two evaluations round alike: that they agree, on envs within a float32
// ulp of a tile or quadrant border too, is what tests/test_gpu_render_order.py holds (a permutation at N = 8193 ... 16385, every frame written once).
#define SORT_BINS 4096
template <bool MASKED = false>
__global__ __launch_bounds__(1024) void k_env_sort(SimArrays A, const RenderMapDev* __restrict__ maps, int32_t* __restrict__ pos,
                                                   const uint8_t* __restrict__ mask, int32_t* __restrict__ live) {
  __shared__ int s_hist[SORT_BINS];
  __shared__ int s_part[1024];
  const int tid = threadIdx.x;
  for (int i = tid; i < SORT_BINS; i += 1024) s_hist[i] = 0;
  __syncthreads();
  // (any order is a valid render order: the bin only needs to be the same in both passes -- single-precision trigonometry,
  // computed once per env and kept in registers between the histogram and the scatter; N <= 8 * 1024 envs per launch keep
  // theirs, larger batches recompute)
  auto bin_of = [&](int e) -> int {
    const int mid = A.map_id[e] < 0 ? 0 : A.map_id[e];
    const float its = maps[mid].inv_tile_size;
    const float ang = (float)A.angle[e];
    float sa, ca;
    __sincosf(ang, &sa, &ca);
    const float px = (float)A.pos_x[e] + (float)DT_CAMERA_FORWARD_DIST * ca, pz = (float)A.pos_z[e] - (float)DT_CAMERA_FORWARD_DIST * sa;
    const int ti = min(max((int)floorf(px * its), 0), 31), tj = min(max((int)floorf(pz * its), 0), 31);
    const int quad = ((int)floorf(ang * (float)(2.0 / 3.141592653589793) + 0.5f)) & 3;
    return ((((tj << 5) | ti) << 2) | quad) ^ ((mid * 1237) & (SORT_BINS - 1));
  };
  constexpr int KEEP = 8;
  int bins[KEEP];
#pragma unroll
  for (int k = 0; k < KEEP; ++k) {
    const int e = tid + k * 1024;
    bins[k] = e < A.N && (!MASKED || mask[e]) ? bin_of(e) : -1;
    if (bins[k] >= 0) atomicAdd(&s_hist[bins[k]], 1);
  }
  for (int e = tid + KEEP * 1024; e < A.N; e += 1024) if (!MASKED || mask[e]) atomicAdd(&s_hist[bin_of(e)], 1);
  __syncthreads();
  // exclusive scan of the bins: each thread owns SORT_BINS / 1024 consecutive bins
  int loc[SORT_BINS / 1024], sum = 0;
#pragma unroll
  for (int k = 0; k < SORT_BINS / 1024; ++k) { loc[k] = sum; sum += s_hist[tid * (SORT_BINS / 1024) + k]; }
  // block-wide exclusive scan of the 1024 partial sums: within a wavefront by DPP-style shuffles, across the 16 wavefronts through LDS
  int incl = sum;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const int v = __shfl_up(incl, d); if ((tid & 63) >= d) incl += v; }
  if ((tid & 63) == 63) s_part[tid >> 6] = incl;
  __syncthreads();
  if (tid < 16) {
    int w = s_part[tid];
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) { const int v = __shfl_up(w, d, 16); if (tid >= d) w += v; }
    s_part[16 + tid] = w;                             // inclusive over the wavefronts
    if (MASKED && tid == 15) *live = w;               // selected envs in all
  }
  __syncthreads();
  const int base = incl - sum + ((tid >> 6) ? s_part[16 + (tid >> 6) - 1] : 0);
#pragma unroll
  for (int k = 0; k < SORT_BINS / 1024; ++k) s_hist[tid * (SORT_BINS / 1024) + k] = base + loc[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < KEEP; ++k)
    if (bins[k] >= 0) pos[tid + k * 1024] = atomicAdd(&s_hist[bins[k]], 1);
    else if (MASKED && tid + k * 1024 < A.N) pos[tid + k * 1024] = -1;
  for (int e = tid + KEEP * 1024; e < A.N; e += 1024) pos[e] = !MASKED || mask[e] ? atomicAdd(&s_hist[bin_of(e)], 1) : -1;
}

// light: DTSIM_F_LIGHT_CAPTURE with the shared camera -- the env's own eye-space light (colors[12..15]) instead of default_cam()'s, also as the
// rotated per-position constants of the quad kernels' LIGHT instantiations (envl, [N + 1], when given).
// MASKED: the masked pass (k_env_sort<true>'s order) -- envs at position -1 are not rendered and get no records.
template <bool MASKED = false>
__global__ void k_cam_setup(SimArrays A, int domain_rand, int segment, float aspect, EnvCam* out, EnvFast* fast,
                            const RenderMapDev* __restrict__ maps, EnvQ* envq, int qlog2, const int32_t* __restrict__ pos, EnvV* envv,
                            EnvD* envd, int W, int H, int light, EnvL* envl) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const size_t N = A.N;
  if (e >= A.N) return;
  if (MASKED && pos[e] < 0) return;
  EnvCam c;
  const double ang = A.angle[e];
  const double sa = sin(ang), ca = cos(ang);
  double px = A.pos_x[e], py = 0.0, pz = A.pos_z[e];
  float base[3], dif[3], L[4];
  if (domain_rand) {  // per-env camera / light (simulator.py:565-614, 1768-1769)
    px += (double)A.cam[3 * N + e]; py += (double)A.cam[4 * N + e]; pz += (double)A.cam[5 * N + e];
    py += (double)A.cam[0 * N + e];
    const float th = A.cam[1 * N + e], fov = A.cam[2 * N + e];
    for (int k = 0; k < 3; ++k) { base[k] = 0.3f + A.colors[(6 + k) * N + e]; dif[k] = A.colors[(9 + k) * N + e]; }
    for (int k = 0; k < 4; ++k) L[k] = A.colors[(12 + k) * N + e];
    c.sth = sinf(th); c.cth = cosf(th);
    const float tanh_ = tanf(0.5f * fov);
    c.tx = tanh_ * aspect; c.ty = tanh_;
    c.Cy = (float)py;
  } else {
    const CamShared s = default_cam(aspect);
    c.sth = s.sth; c.cth = s.cth; c.tx = s.tx; c.ty = s.ty; c.Cy = s.Cy;
    for (int k = 0; k < 3; ++k) { base[k] = s.base; dif[k] = s.dif; }
    for (int k = 0; k < 4; ++k) L[k] = light ? A.colors[(12 + k) * N + e] : s.L[k];
  }
  // glTranslatef(0,0,CAMERA_FORWARD_DIST) before gluLookAt (simulator.py:1784,1803): the
  // camera centre sits 6.6 cm ahead of the axle along dir = (cos a, 0, -sin a).
  c.Cx = (float)(px + DT_CAMERA_FORWARD_DIST * ca);
  c.Cz = (float)(pz - DT_CAMERA_FORWARD_DIST * sa);
  c.sa = (float)sa; c.ca = (float)ca;
  for (int k = 0; k < 3; ++k) {
    c.hor[k] = 255.f * A.colors[(0 + k) * N + e];
    c.gnd[k] = 255.f * A.colors[(3 + k) * N + e];
    c.base[k] = base[k];     // GL_LIGHT_MODEL_AMBIENT 0.3 (simulator.py:1741) + light ambient
    c.dif[k] = dif[k];
  }
  if (segment) {             // simulator.py:1730-1733 lighting off; :1753 clear and :1808 ground quad magenta
    for (int k = 0; k < 3; ++k) { c.base[k] = 1.f; c.dif[k] = 0.f; c.hor[k] = c.gnd[k] = (k == 1) ? 0.f : 255.f; }
  }
  if (L[3] == 0.f) {  // directional: normalise once
    const float inv = rsqrtf(L[0] * L[0] + L[1] * L[1] + L[2] * L[2]);
    L[0] *= inv; L[1] *= inv; L[2] *= inv;
  }
  for (int k = 0; k < 4; ++k) c.L[k] = L[k];
  if (envl) {                // (shared camera: c.sth, c.cth, c.Cy and dif are default_cam()'s)
    EnvL l;
    const float Lu = L[1] * c.cth + L[2] * c.sth;
    if (L[3] == 0.f) {
      l.Lr = l.Lf = 0.f; l.h2 = 0x1p120f; l.kd8 = dif[0] * fmaxf(Lu, 0.f) * (0x1p60f / 256.f);   // (/ 256: Q8_LIT)
    } else {
      const float h = Lu + c.Cy;
      l.Lr = L[0]; l.Lf = L[1] * c.sth - L[2] * c.cth; l.h2 = h > 0.f ? h * h : 1.f; l.kd8 = dif[0] * fmaxf(h, 0.f) * (1.f / 256.f);
    }
    envl[pos ? pos[e] : e] = l;
    if (e == A.N - 1) envl[A.N] = l;                 // the entry past the end (prefetched, never used)
  }
  // ground quad corners: per-vertex lighting (Gouraud over the 100 m quad)
  for (int k = 0; k < 4; ++k) {
    const float X = (k & 1) ? GROUND_HALF : -GROUND_HALF, Z = (k & 2) ? GROUND_HALF : -GROUND_HALF;
    const float rx = X - c.Cx, ry = GROUND_Y - c.Cy, rz = Z - c.Cz;
    const float xla = rx * c.sa + rz * c.ca;          // . right = (sin a, 0, cos a)
    const float zla = -(rx * c.ca - rz * c.sa);       // -(. dir)
    const float ye = ry * c.cth - zla * c.sth, ze = ry * c.sth + zla * c.cth, xe = xla;
    // The ground vertex list has no normals (simulator.py:526): GL lights it with the CURRENT normal -- (0, 0, 1), GL's initial value;
    // nothing on the reference's default path calls glNormal -- taken through the inverse transpose of glScalef(50, 0.01, 50) (:1810)
    // and the view rotation, NOT renormalised (GL_NORMALIZE is off): length 1/50.  Pinned on Mesa llvmpipe (tests/test_gpu_gl_golden.py).
    const float gnx = c.ca * (1.f / GROUND_HALF), gny = -c.sa * c.sth * (1.f / GROUND_HALF), gnz = c.sa * c.cth * (1.f / GROUND_HALF);
    float ndl;
    if (L[3] == 0.f) ndl = gnx * L[0] + gny * L[1] + gnz * L[2];
    else {
      const float lx = L[0] - xe, ly = L[1] - ye, lz = L[2] - ze;
      ndl = (gnx * lx + gny * ly + gnz * lz) * rsqrtf(lx * lx + ly * ly + lz * lz);
    }
    c.gndl[k] = fmaxf(ndl, 0.f);
  }
  c.map_id = A.map_id[e];
  c.pad[0] = c.pad[1] = 0.f;
  out[e] = c;
  const RenderMapDev m = maps[c.map_id];
  EnvFast f{};                                       // (the pad is written as zero: the scratch bytes stay deterministic)
  f.its = m.inv_tile_size; f.ts = m.tile_size;
  f.A = c.sa * f.its; f.B = c.ca * f.its; f.Cxi = c.Cx * f.its; f.Czi = c.Cz * f.its;
  f.kg = (c.Cy - GROUND_Y) / c.Cy; f.Cx = c.Cx; f.Cz = c.Cz;
  f.gw_m = (float)m.grid_w * m.tile_size; f.gh_m = (float)m.grid_h * m.tile_size;
  {
    const uint32_t r = (uint32_t)(fminf(fmaxf(c.hor[0], 0.f), 255.f) + 0.5f), g = (uint32_t)(fminf(fmaxf(c.hor[1], 0.f), 255.f) + 0.5f);
    const uint32_t b = (uint32_t)(fminf(fmaxf(c.hor[2], 0.f), 255.f) + 0.5f);
    f.hor_rgb = r | (g << 8) | (b << 16);
  }
  f.gw = m.grid_w; f.gh = m.grid_h; f.tile_off = m.tile_off;
  fast[e] = f;
  if (envq) {
    const float S = (float)(1 << qlog2);
    EnvQ q;
    q.A = f.A * S; q.B = f.B * S;
    q.Cx = f.Cxi * S + 0.5f + (float)DT_QRING * S; q.Cz = f.Czi * S + 0.5f + (float)DT_QRING * S;
    q.Xhi = ((float)(m.grid_w + 2 * DT_QRING) - 0.5f) * S; q.Zhi = ((float)(m.grid_h + 2 * DT_QRING) - 0.5f) * S;
    q.tab_b = (uint32_t)m.qt_off * 8u; q.pitch4 = (uint32_t)m.qt_pitch * 8u;   // 8-byte table entries
    q.hor_rgb = f.hor_rgb;
    const uint32_t r = f.hor_rgb & 255u, g = (f.hor_rgb >> 8) & 255u, b = (f.hor_rgb >> 16) & 255u;
    q.sky[0] = r | (g << 8) | (b << 16) | (r << 24);
    q.sky[1] = g | (b << 8) | (r << 16) | (g << 24);
    q.sky[2] = b | (r << 8) | (g << 16) | (b << 24);
    {
      const float xmax = (float)(m.grid_w + 2 * DT_QRING) * S, zmax = (float)(m.grid_h + 2 * DT_QRING) * S;
      const float r = fminf(fminf(q.Cx, xmax - q.Cx), fminf(q.Cz, zmax - q.Cz)) - 2.f;
      q.reach = r > 0.f ? (uint32_t)fminf(r, 1.0e9f) : 0u;      // NaN / outside the padded grid -> 0: always clamp
    }
    q.env = (uint32_t)e; q.qpm_bits = __float_as_uint(m.inv_tile_size * S);   // quad cells per metre of the env's map (the exact path's ground-quad test)
    q.tab3 = (uint32_t)c.map_id * (V3_MAP_COLS * 4);     // k_raster_v3: byte offset of the map's columns inside an LDS table row (V3_MAP_COLS entries)
    envq[pos ? pos[e] : e] = q;
    if (envv) {
      EnvV v;
      v.A2[0] = v.A2[1] = q.A; v.B2[0] = v.B2[1] = q.B; v.Cx2[0] = v.Cx2[1] = q.Cx; v.Cz2[0] = v.Cz2[1] = q.Cz;
      v.Xhi = q.Xhi; v.Zhi = q.Zhi; v.tab3 = q.tab3; v.hor_rgb = q.hor_rgb; v.reach = q.reach; v.env = q.env; v.pad[0] = v.pad[1] = 0u;
      envv[pos ? pos[e] : e] = v;
      if (e == A.N - 1) envv[A.N] = v;               // the entry past the end (prefetched, never used)
    }
    if (envd) fill_envd_at(envd, pos ? pos[e] : e, c, q, m, S, H, W);   // domain randomisation on the quad records (index = position in the render order)
  }
}

// order-preserving float <-> int map (for integer atomics on floats)
__device__ inline int f2ord(float f) { const int i = __float_as_int(f); return i >= 0 ? i : i ^ 0x7fffffff; }
__device__ inline float ord2f(int i) { return __int_as_float(i >= 0 ? i : i ^ 0x7fffffff); }

// Source-pixel bounding box of every raster wavefront block (tile * 4 + wavefront): env-invariant, one workgroup per
// raster tile.  Empty blocks (no pixel inside the rectilinear image) get an inverted box.
__global__ __launch_bounds__(RB) void k_blk_setup(RenderParams R, const float4* __restrict__ lut, float4* __restrict__ blockbox) {
  const int tiles_x = (R.W + DT_TILE_W - 1) / DT_TILE_W;
  const int tile = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int tile_x0 = (tile % tiles_x) * DT_TILE_W;
  const int wave_y0 = (tile / tiles_x) * DT_TILE_H + wave * (WAVE_PIX / WAVE_W);
  float x0 = 1e30f, x1 = -1e30f, y0 = 1e30f, y1 = -1e30f;
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    const int x = tile_x0 + SLOT_X(k, lane), y = wave_y0 + SLOT_Y(k, lane);
    if (x < R.W && y < R.H) {
      const float4 l = lut[y * R.W + x];
      if (l.z != 0.f) {
        float sx, sy;
        src_px(l.x, l.y, R.W, R.H, sx, sy);
        x0 = fminf(x0, sx); x1 = fmaxf(x1, sx); y0 = fminf(y0, sy); y1 = fmaxf(y1, sy);
      }
    }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    x0 = fminf(x0, __shfl_xor(x0, d)); x1 = fmaxf(x1, __shfl_xor(x1, d));
    y0 = fminf(y0, __shfl_xor(y0, d)); y1 = fmaxf(y1, __shfl_xor(y1, d));
  }
  if (lane == 0) blockbox[tile * 4 + wave] = make_float4(x0, x1, y0, y1);
  if (blockIdx.x == 0) {   // triangle range of every object in its map's triangle order (static; k_resolve_obj streams by it)
    for (int i = threadIdx.x; i < R.n_maps * DTSIM_MAX_OBJECTS; i += RB) {
      const int mi = i / DTSIM_MAX_OBJECTS, o = i % DTSIM_MAX_OBJECTS;
      const RenderMapDev m = R.maps[mi];
      uint2 fc = make_uint2(0u, 0u);
      if (o < m.n_obj) {
        for (int k = 0; k < o; ++k) { const int mid = R.objs[m.obj_off + k].mesh_id; fc.x += mid >= 0 ? (uint32_t)R.meshes[mid].n_tris : 0u; }
        const int mid = R.objs[m.obj_off + o].mesh_id;
        fc.y = mid >= 0 ? (uint32_t)R.meshes[mid].n_tris : 0u;
      }
      R.objrange[i] = fc;
    }
  }
}

// ---- mesh objects -> per-env screen-space triangles ------------------------------------
// One workgroup per env.  WorldObj.render (objects.py:123-148): T(pos) S(scale) Ry(y_rot), mesh
// chunks with per-vertex Kd colour (objmesh.py:241-293), GL per-vertex lighting (normals through the inverse transpose of the
// model-view, NOT renormalised: divided by the scale -- DESIGN.md "Render spec"), projected to rectilinear pixel coordinates.
#ifndef DT_OBJSETUP_T
#define DT_OBJSETUP_T 256           // threads of a k_obj_setup workgroup (one workgroup per env)
#endif
template <bool MASKED = false>   // MASKED: the masked pass -- envs at position -1 (not rendered) are skipped
__global__ __launch_bounds__(DT_OBJSETUP_T) void k_obj_setup(SimArrays A, RenderParams R, const EnvCam* __restrict__ cams, const int32_t* __restrict__ pos) {
  const int e = blockIdx.x;
  if (MASKED && pos[e] < 0) return;
  const int tid = threadIdx.x;
  const size_t N = A.N;
  const EnvCam c = cams[e];
  const RenderMapDev m = R.maps[c.map_id];
  ScreenTri* out = R.stris + (size_t)e * R.max_tris;
  // per-object screen boxes: LDS min / max through the order-preserving float -> int map
  __shared__ int s_obox[DTSIM_MAX_OBJECTS][4];
  __shared__ float s_oboxf[DTSIM_MAX_OBJECTS][4];
  if (tid < DTSIM_MAX_OBJECTS) {
    s_obox[tid][0] = s_obox[tid][2] = 0x7fffffff;    // min slots
    s_obox[tid][1] = s_obox[tid][3] = (int)0x80000000;   // max slots
  }
  // Round 5: object-level frustum cull first.  An env sees ~ 1 of its map's objects (profiles/r04_variants_ab.txt block G: 0.8 live objects per
  // env); an object whose model-space box, taken through the instance and the camera, lies wholly outside one frustum plane (or is invisible)
  // contributes no triangle: its triangles are neither loaded nor transformed nor written -- nothing reads them, the object's screen box
  // stays empty and so it appears in no block mask (k_resolve_obj streams the triangles of masked objects only).
  __shared__ uint8_t s_objlive[DTSIM_MAX_OBJECTS];
  __shared__ int s_nt[DTSIM_MAX_OBJECTS], s_first[DTSIM_MAX_OBJECTS + 1];   // triangles of each object, and before it (the walks below read LDS, not dependent global loads)
  if (tid < DTSIM_MAX_OBJECTS) {
    bool livef = false;
    s_nt[tid] = 0;
    if (tid < m.n_obj) {
      const ObjInstDev oi = R.objs[m.obj_off + tid];
      s_nt[tid] = oi.mesh_id >= 0 ? R.meshes[oi.mesh_id].n_tris : 0;
      if (oi.mesh_id >= 0 && A.ob_visible[(size_t)tid * N + e] != 0) {
        const MeshDev md = R.meshes[oi.mesh_id];
        float px = oi.x, py = oi.y, pz = oi.z, yrot = oi.yrot_deg;
        if (oi.dyn_slot >= 0) {
          px = (float)A.ob_cx[(size_t)oi.dyn_slot * N + e]; pz = (float)A.ob_cz[(size_t)oi.dyn_slot * N + e];
          py += (float)A.ob_cy[(size_t)oi.dyn_slot * N + e];
          yrot = (float)A.ob_yrot[(size_t)oi.dyn_slot * N + e];
        }
        const float ang = yrot * 0.017453292519943295f;
        const float co = cosf(ang), so = sinf(ang);
        uint32_t all_out = 0x1Fu;                       // bit set while every corner so far is outside that plane: near, left, right, bottom, top
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float mx = ((k & 1) ? md.mx[0] : md.mn[0]) * oi.scale, my = ((k & 2) ? md.mx[1] : md.mn[1]) * oi.scale, mz = ((k & 4) ? md.mx[2] : md.mn[2]) * oi.scale;
          const float rx = (mx * co + mz * so + px) - c.Cx, ry = (my + py) - c.Cy, rz = (-mx * so + mz * co + pz) - c.Cz;
          const float xla = rx * c.sa + rz * c.ca, zla = -(rx * c.ca - rz * c.sa);
          const float xe = xla, ye = ry * c.cth - zla * c.sth, w = -(ry * c.sth + zla * c.cth);
          // the four side planes pass through the eye: xe + w tx >= 0 ... are half-spaces for any sign of w; two pixels of slack (the
          // triangle boxes are padded by DT_TRI_PAD)
          const float lx = w * c.tx, ly = w * c.ty, sx_ = fabsf(w) * c.tx * (4.f / (float)R.W), sy_ = fabsf(w) * c.ty * (4.f / (float)R.H);
          uint32_t o = 0u;
          if (w <= NEAR_Z) o |= 1u;
          if (xe < -lx - sx_) o |= 2u;
          if (xe > lx + sx_) o |= 4u;
          if (ye < -ly - sy_) o |= 8u;
          if (ye > ly + sy_) o |= 16u;
          all_out &= o;
        }
        livef = all_out == 0u;
      }
    }
    s_objlive[tid] = livef ? 1 : 0;
  }
  __syncthreads();
  if (tid == 0) {
    int acc = 0;
    for (int o = 0; o < m.n_obj; ++o) { s_first[o] = acc; acc += s_nt[o]; }
    s_first[m.n_obj] = acc;
  }
  __syncthreads();
  int obj = 0;                             // walk the object list as t grows (t is monotone per thread)
  for (int t = tid; t < m.n_tris; t += DT_OBJSETUP_T) {
    while (obj + 1 < m.n_obj && t >= s_first[obj + 1]) ++obj;
    if (!s_objlive[obj]) continue;        // the whole object is out of view (or invisible)
    const int obj_first = s_first[obj];
    const ObjInstDev oi = R.objs[m.obj_off + obj];
    const TriDev td = R.tris[R.meshes[oi.mesh_id].off + (t - obj_first)];
    float px = oi.x, py = oi.y, pz = oi.z, yrot = oi.yrot_deg;
    if (oi.dyn_slot >= 0) {               // DuckieObj: pos = center, y_rot wiggles (objects.py:408-410)
      px = (float)A.ob_cx[(size_t)oi.dyn_slot * N + e]; pz = (float)A.ob_cz[(size_t)oi.dyn_slot * N + e];
      py += (float)A.ob_cy[(size_t)oi.dyn_slot * N + e];
      yrot = (float)A.ob_yrot[(size_t)oi.dyn_slot * N + e];
    }
    const bool visible = A.ob_visible[(size_t)obj * N + e] != 0;
    const float ang = yrot * 0.017453292519943295f;
    const float co = cosf(ang), so = sinf(ang);
    ScreenTri st;
    bool ok = visible;
    float w[3];
#pragma unroll
    for (int v = 0; v < 3; ++v) {
      const float mx = td.v[v][0] * oi.scale, my = td.v[v][1] * oi.scale, mz = td.v[v][2] * oi.scale;
      const float rx = (mx * co + mz * so + px) - c.Cx, ry = (my + py) - c.Cy, rz = (-mx * so + mz * co + pz) - c.Cz;
      const float xla = rx * c.sa + rz * c.ca, zla = -(rx * c.ca - rz * c.sa);
      const float xe = xla, ye = ry * c.cth - zla * c.sth, ze = ry * c.sth + zla * c.cth;
      w[v] = -ze;
      ok = ok && (w[v] > NEAR_Z);
      // normal: Ry(y_rot) then view rotation, through the inverse transpose of glScalef(scale) (objects.py:142) = divided by the scale, and NOT
      // renormalised (GL_NORMALIZE / GL_RESCALE_NORMAL are never enabled): whatever length the OBJ file gives it stays.  Pinned on Mesa llvmpipe.
      const float nwx = td.n[v][0] * co + td.n[v][2] * so, nwy = td.n[v][1], nwz = -td.n[v][0] * so + td.n[v][2] * co;
      const float nxl = nwx * c.sa + nwz * c.ca, nzl = -(nwx * c.ca - nwz * c.sa);
      float nex = nxl, ney = nwy * c.cth - nzl * c.sth, nez = nwy * c.sth + nzl * c.cth;
      const float ninv = 1.f / oi.scale;
      nex *= ninv; ney *= ninv; nez *= ninv;
      float ndl;
      if (c.L[3] == 0.f) ndl = nex * c.L[0] + ney * c.L[1] + nez * c.L[2];
      else {
        const float lx = c.L[0] - xe, ly = c.L[1] - ye, lz = c.L[2] - ze;
        ndl = (nex * lx + ney * ly + nez * lz) * rsqrtf(lx * lx + ly * ly + lz * lz);
      }
      ndl = fmaxf(ndl, 0.f);
      const float iw = 1.f / w[v];
      st.iw[v] = iw;
      st.sx[v] = (xe * iw / c.tx + 1.f) * 0.5f * (float)R.W;
      st.sy[v] = (1.f - ye * iw / c.ty) * 0.5f * (float)R.H;
#pragma unroll
      for (int k = 0; k < 3; ++k)
        st.cw[v][k] = fminf(td.c[v][k] * (c.base[k] + c.dif[k] * ndl), 1.f) * 255.f * iw;
      st.uw[v] = td.uv[v][0] * iw; st.vw[v] = td.uv[v][1] * iw;
    }
    st.tex = td.tex; st.pad = 0;
    if (oi.light_tris > 0 && (t - obj_first) < oi.light_tris)          // traffic light card: texture by pattern
      st.tex = A.ob_light[(size_t)obj * N + e] ? oi.light_tex1 : oi.light_tex0;
    if (R.segment) {         // get_mesh(name, segment=True): one flat colour as every chunk's texture (objmesh.py:255-292),
      const uint8_t* sc = R.mesh_seg + 4 * oi.mesh_id;   // MODULATEd with the per-vertex Kd -> fold it into the vertex colours
#pragma unroll
      for (int v = 0; v < 3; ++v)
#pragma unroll
        for (int k = 0; k < 3; ++k) st.cw[v][k] *= (float)sc[k] * (1.f / 255.f);
      st.tex = -1;
    }
    const float area = (st.sx[1] - st.sx[0]) * (st.sy[2] - st.sy[0]) - (st.sx[2] - st.sx[0]) * (st.sy[1] - st.sy[0]);
    ok = ok && (area != 0.f);
    st.inv_area = ok ? 1.f / area : 0.f;
    // screen box padded by DT_TRI_PAD pixels: the four samples sit within 0.375 px of the pixel centre the box is tested with
    st.bx0 = fminf(fminf(st.sx[0], st.sx[1]), st.sx[2]) - DT_TRI_PAD; st.bx1 = fmaxf(fmaxf(st.sx[0], st.sx[1]), st.sx[2]) + DT_TRI_PAD;
    st.by0 = fminf(fminf(st.sy[0], st.sy[1]), st.sy[2]) - DT_TRI_PAD; st.by1 = fmaxf(fmaxf(st.sy[0], st.sy[1]), st.sy[2]) + DT_TRI_PAD;
    if (ok && (st.bx1 < 0.f || st.bx0 > (float)R.W || st.by1 < 0.f || st.by0 > (float)R.H)) { ok = false; st.inv_area = 0.f; }
    if (!ok) { st.bx0 = 1e30f; st.bx1 = -1e30f; st.by0 = 1e30f; st.by1 = -1e30f; }
    st.index = t;
    // culled triangles (outside the view, degenerate, beyond near / far) leave only their inverted box: k_resolve_obj culls on
    // the boxes and reads the 128-byte record of survivors only.  (dt_render_layout sets R.tribox whenever it sets R.stris, so the `!R.tribox` arm
    // below and the test after it are never taken the other way: no pass runs without the stream, and every reader of the records -- k_resolve_obj,
    // render_views.hip's scene_samples4 -- tests a triangle by the stream's box, never by the one a culled triangle's record still holds.)
    if (ok || !R.tribox) out[t] = st;
    if (R.tribox) R.tribox[(size_t)e * R.max_tris + t] = make_float4(st.bx0, st.bx1, st.by0, st.by1);   // the cull stream of k_resolve_obj: 16 B per triangle, contiguous
    if (ok) {
      atomicMin(&s_obox[obj][0], f2ord(st.bx0)); atomicMax(&s_obox[obj][1], f2ord(st.bx1));
      atomicMin(&s_obox[obj][2], f2ord(st.by0)); atomicMax(&s_obox[obj][3], f2ord(st.by1));
    }
  }
  __syncthreads();
  if (tid < m.n_obj) {                      // per-object screen box = union of its live triangles' boxes
    ObjBox ob;
    ob.first = s_first[tid]; ob.pad[0] = ob.pad[1] = 0;
    const int cnt = s_nt[tid];
    const bool live = s_obox[tid][0] != 0x7fffffff;
    ob.bx0 = live ? ord2f(s_obox[tid][0]) : 1e30f; ob.bx1 = live ? ord2f(s_obox[tid][1]) : -1e30f;
    ob.by0 = live ? ord2f(s_obox[tid][2]) : 1e30f; ob.by1 = live ? ord2f(s_obox[tid][3]) : -1e30f;
    ob.count = live ? cnt : 0;
    R.objbox[(size_t)e * DTSIM_MAX_OBJECTS + tid] = ob;
    s_oboxf[tid][0] = ob.bx0; s_oboxf[tid][1] = ob.bx1; s_oboxf[tid][2] = ob.by0; s_oboxf[tid][3] = ob.by1;   // empty when not live
  }
  __syncthreads();
  if (R.objmask) {
    // which objects' screen boxes meet each raster wavefront block (source-pixel boxes of the blocks: k_blk_setup): the
    // raster reads one 8-byte mask per (env, block) instead of walking the env's object boxes
    const int n_blk = ((R.W + DT_TILE_W - 1) / DT_TILE_W) * ((R.H + DT_TILE_H - 1) / DT_TILE_H) * 4;
    const float4* bbx = reinterpret_cast<const float4*>(R.blockbox);
    // The mask must hold every object the rasters' per-pixel test can select: that test takes the pixel centres as fp16 (half an ulp:
    // up to 1 px below 4096) against the box widened by obj_mrg (up to 0.95 px), so the block boxes are widened by 2 px here.  Without
    // the pad a pixel just outside an object's box was queued or not depending on which other pixels share its block -- i.e. on the
    // distortion table, not on the pixel's own ray.
    const float pad = 2.f;
    unsigned long long livem = 0ull;                 // objects with a live screen box (usually one or none)
    for (int o = 0; o < m.n_obj; ++o) livem |= s_oboxf[o][0] <= s_oboxf[o][1] ? 1ull << o : 0ull;
    for (int b = tid; b < n_blk; b += DT_OBJSETUP_T) {
      const float4 bb = bbx[b];                      // x0, x1, y0, y1
      unsigned long long mk = 0ull;
      for (unsigned long long lm = livem; lm; lm &= lm - 1ull) {
        const int o = __builtin_ctzll(lm);
        if (!(bb.y + pad < s_oboxf[o][0] || bb.x - pad > s_oboxf[o][1] || bb.w + pad < s_oboxf[o][2] || bb.z - pad > s_oboxf[o][3])) mk |= 1ull << o;
      }
      R.objmask[(size_t)(pos ? pos[e] : e) * n_blk + b] = mk;   // indexed by position in the render order
    }
  }
}

// ---- per-pixel tables of the shared camera (PixTab, SampTab: render_records.h; env-invariant), built here -----------------

__global__ void k_pix_setup(RenderParams R, const float4* __restrict__ lut, PixTab* __restrict__ pixtab, SampTab* __restrict__ samptab) {
  const int pix = blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= R.W * R.H) return;
  const float aspect = (float)R.W / (float)R.H;
  const float ex_n = 0.375f * 2.f / (float)R.W * 1.01f, ey_n = 0.375f * 2.f / (float)R.H * 1.01f;
  const CamShared cs = default_cam(aspect);
  const float4 l = lut[pix];
  const bool ok = l.z != 0.f;
  const PixInv p = pix_inv(l.x, l.y, ok, cs.tx, cs.ty, cs.sth, cs.cth, cs.Cy, cs.L, ex_n, ey_n);
  const bool cand = (p.flags & (PF_VALID | PF_SKY)) == PF_VALID;
  const bool plain = cand && !(p.flags & PF_ALWAYS_EDGE) && (p.flags & PF_TILE_OK) && (p.flags & PF_GROUND_OK);
  PixTab t;
  t.lr = p.lr; t.lf = p.lf;
  t.lit = !ok ? -1.f : !cand ? 0.f : fminf(fmaf(cs.dif, p.ndl, cs.base), 1.f);
  // one-ray pixel  <=>  cells-to-boundary k > reach + 0.5  <=>  k > floor(reach + 0.5)   (k integer)
  t.mi = plain ? (uint32_t)fminf(floorf(fmaf(p.mrg, R.q_per_m, 0.5f)), 65534.f) : 0xFFFFu;
  t.mi |= (uint32_t)__half_as_ushort(__float2half_ru(fminf(p.mrg, 60000.f))) << 16;
  pixtab[pix] = t;
  SampTab sp;
  const auto &ox = MSAA_POS.x, &oy = MSAA_POS.y;
  const float sxn = 2.f / (float)R.W, syn = 2.f / (float)R.H;
  sp.flags = 0u;
  float dlr[4], dlf[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const Ray r = make_ray(l.x + ox[k] * sxn, l.y - oy[k] * syn, cs.tx, cs.ty, cs.sth, cs.cth);
    dlr[k] = dlf[k] = 0.f;
    if (r.yla < 0.f) {
      const float inv = frcp(-r.yla);
      const float t = cs.Cy * inv, tg = (cs.Cy - GROUND_Y) * inv;
      dlr[k] = fminf(fmaxf(t * r.xe - p.lr, -60000.f), 60000.f); dlf[k] = fminf(fmaxf(t * r.fwd - p.lf, -60000.f), 60000.f);
      if (t >= NEAR_Z && t <= FAR_Z) sp.flags |= 1u << k;
      if (tg >= NEAR_Z && tg <= FAR_Z) sp.flags |= 16u << k;
    }
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    sp.dlr[j] = (uint32_t)__half_as_ushort(__float2half_rn(dlr[2 * j])) | ((uint32_t)__half_as_ushort(__float2half_rn(dlr[2 * j + 1])) << 16);
    sp.dlf[j] = (uint32_t)__half_as_ushort(__float2half_rn(dlf[2 * j])) | ((uint32_t)__half_as_ushort(__float2half_rn(dlf[2 * j + 1])) << 16);
  }
  sp.lr_bits = __float_as_uint(t.lr); sp.lf_bits = __float_as_uint(t.lf); sp.lit_bits = __float_as_uint(t.lit);   // the PixTab's hit and lit factor once more: phase 2 of the exact path reads ONE table
  samptab[pix] = sp;
}

}  // namespace

// Everything a raster of `pipe` reads, on stream s: the render order, the per-env records, the mesh objects' triangles and masks, the per-pixel
// tables; R.work zeroed for the pass.  tables, mask and the returned bits: dt_launch_render's (dtsim_dev.h).
RenderSetup dt_launch_render_setup(hipStream_t s, const SimArrays& A, const RenderParams& R, const EnvRecs& x, int pipe, int tables, const uint8_t* mask) {
  tables &= 3;                                         // bit 2 (returned): this pass ran in k_env_sort's order (DTSIM_FIELD_RENDER_POS)
  const bool quad = pipe == DTSIM_PIPE_V3 || pipe == DTSIM_PIPE_Q, v3dr = pipe == DTSIM_PIPE_V3DR;
  // render order (k_env_sort): the quad pipeline indexes by position (EnvQ, object masks, queue entries); env ids come
  // from EnvQ.env
  int32_t* pos = ((quad || v3dr) && R.envpos && A.N > ENVS_PER_BLOCK) ? R.envpos : nullptr;   // one chunk: the order does not matter
  // masked pass (dtsim_render_masked): the selected envs take positions [0, live) -- always sorted, whatever N --, the others -1; every setup
  // kernel skips them and the SUB rasters stop at live.  The generic rasters render every env instead (same state, same bytes).
  const bool sub = mask && (quad || v3dr) && R.envpos;
  if (sub) {
    pos = R.envpos;
    (void)hipMemsetAsync(R.work, 0, DT_WORK_INTS * sizeof(int32_t), s);          // (before the sort: it writes the live count there)
    hipLaunchKernelGGL(k_env_sort<true>, dim3(1), dim3(1024), 0, s, A, R.maps, pos, mask, R.work + DT_WORK_LIVE);
    tables |= 4;
  } else if (pos) { hipLaunchKernelGGL(k_env_sort<false>, dim3(1), dim3(1024), 0, s, A, R.maps, pos, nullptr, nullptr); tables |= 4; }
#define LAUNCH_CAM(M_) hipLaunchKernelGGL(k_cam_setup<M_>, dim3((A.N + 63) / 64), dim3(64), 0, s, A, R.domain_rand, R.segment,                  \
                     (float)R.W / (float)R.H, x.cams, x.fasts, R.maps, (quad || v3dr) ? x.envq : nullptr, R.qlog2, pos, quad ? x.envv : nullptr,  \
                     v3dr ? x.envd : nullptr, R.W, R.H, R.light, (quad && R.light) ? x.envl : nullptr)
  if (sub) LAUNCH_CAM(true); else LAUNCH_CAM(false);
#undef LAUNCH_CAM
  if (!sub) (void)hipMemsetAsync(R.work, 0, DT_WORK_INTS * sizeof(int32_t), s);   // work-item counts + cursors of k_resolve / k_resolve_obj
  if (R.max_tris > 0) {
    if (!(tables & 2)) hipLaunchKernelGGL(k_blk_setup, dim3((unsigned)dt_raster_tiles(R.W, R.H)), dim3(RB), 0, s, R, reinterpret_cast<const float4*>(R.lut), reinterpret_cast<float4*>(R.blockbox));
    tables |= 2;
    if (sub) hipLaunchKernelGGL(k_obj_setup<true>, dim3(A.N), dim3(DT_OBJSETUP_T), 0, s, A, R, x.cams, pos);
    else hipLaunchKernelGGL(k_obj_setup<false>, dim3(A.N), dim3(DT_OBJSETUP_T), 0, s, A, R, x.cams, pos);
  }

  if (quad && !(tables & 1)) {
    hipLaunchKernelGGL(k_pix_setup, dim3((R.W * R.H + 255) / 256), dim3(256), 0, s, R, reinterpret_cast<const float4*>(R.lut), x.pixtab, x.samptab);
    tables |= 1;
  }
  return RenderSetup{tables, sub, pos != nullptr};
}
