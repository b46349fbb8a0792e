// render_views.hip -- the kernels that read what a render pass (dt_launch_render, render.hip) leaves behind: its frames, its per-env camera records (EnvCam),
// its projected mesh triangles (ScreenTri / ObjBox) and the camera table (lut).  None of them uses the raster's machinery (queues, work
// lists, quad records, workgroup map, per-pixel tables); what they share with the pass is render_scene.h, and the unit is compiled with
// render.hip's flags (build.py), so that classify() and test_tri are the frame's own code here.  In order: k_overlay_lines, scene_samples4
// (the opaque scene at the four samples of a pixel), k_overlay_leds, the rules the camera-map kernels share (out_camera_pixel, EnvEntry, EnvScene,
// Winner / take_nearer, instance_id, tile_texel_class, sample_class, flow_image and the flow's four rules, store_depth), k_depth, k_labels, k_flow*, k_camera_maps, k_bev, k_ipm_*, then
// view_scene and their dt_launch_* (dtsim_dev.h).
#include "dtsim_dev.h"
#include "render_scene.h"
#include "flow_transform.h"
#include <hip/hip_fp16.h>

namespace {

// The camera table's entry of ONE pixel: NDC (nx, ny) and centre (sxp, syp, in pixels) of its rectilinear source pixel; live = false where
// the fisheye leaves the pixel without a source (the frame's black border).  It does not depend on the env.  NO_PIX: a thread past the end.
struct ViewPix { float nx, ny, sxp, syp; bool live; };
#define NO_PIX ViewPix{0.f, 0.f, 0.f, 0.f, false}
__device__ inline ViewPix view_pixel(const float4* __restrict__ lut, const size_t at, const int W, const int H) {
  ViewPix p;
  const float4 l = lut[at];
  p.live = l.z != 0.f; p.nx = l.x; p.ny = l.y;
  src_px(l.x, l.y, W, H, p.sxp, p.syp);
  return p;
}
// The grid of the per-env maps: blocks of 256 threads over the map's `cells` x chunks of DEPTH_ENVS envs.  A thread loops over the envs of its
// chunk, and that loop is ONE copy of its body in every kernel (unroll(disable); why: at k_depth).
#define DEPTH_ENVS DT_ENVS_PER_BLOCK
static inline dim3 view_grid(const int cells, const int N) { return dim3((unsigned)((cells + 255) / 256), (unsigned)((N + DEPTH_ENVS - 1) / DEPTH_ENVS)); }
// Per-env distortion tables (dtsim_set_distortion_luts; k_depth / k_labels with CAL): the table entry of camera pixel `at` for env e is the
// IDENTITY table's entry at s = cal_src[env_cal[e]][at] -- the rectilinear pixel whose colour k_remap_cal put at frames[e][at], read rather than
// recomputed so that its bits are the rectilinear pass's own -- and a dead entry (z = 0) where s = -1 or the thread owns no pixel.  env_cal[e]
// is wave-uniform; the calibration and s are clamped to their tables (the install checked both: the clamps only keep a caller's stale pointer
// from reading outside them on a device others share).
__device__ inline float4 cal_entry(const float4* __restrict__ lut, const int32_t* __restrict__ cal_src, const int32_t* __restrict__ env_cal,
                                   const int n_cal, const int e, const bool in, const size_t at, const int W, const int H) {
  if (!in) return make_float4(0.f, 0.f, 0.f, 0.f);
  const size_t hw = (size_t)W * (size_t)H;
  const int s = cal_src[(size_t)min((unsigned)env_cal[e], (unsigned)(n_cal - 1)) * hw + at];
  return (unsigned)s < (unsigned)hw ? lut[s] : make_float4(0.f, 0.f, 0.f, 0.f);
}

// ---- k_overlay_lines: the reference's GL_LINE overlays as a post-pass on the resolved frames --------------------------------------
// draw_curve (simulator.py:1886-1904, graphics.py:336-349: the lane curves of every drivable tile, 19 segments each, the one most aligned
// with the heading red, the others blue) and draw_bbox (simulator.py:1907-1918, objects.py:131-146: the collision rectangles of the
// objects and of the agent at y = 0.01, red).  The host states the segments in WORLD space (dtsim_draw_lines); here every segment is
// taken through the env's camera (EnvCam: shared or domain-randomised), clipped at the near plane, and rasterised as GL rasterises a
// 1-pixel line under multisampling: the rectangle of width 1 px around the projected segment, coverage per MSAA sample.  The pass works on
// the RESOLVED frame, per OUTPUT pixel (its source pixel comes from the LUT, so the fisheye remap is honoured): a pixel with n of its four
// samples covered becomes ((4 - n) frame + sum of the covering lines' colours) / 4 -- what the multisample resolve gives when the line is
// the nearest thing in the pixel.  Documented deviations from the GL state machine: lines are not depth-tested against
// mesh objects (they lie 1 cm above the tile plane: in front of tiles and ground always); their colour is the glColor lit as a surface
// with normal +y (GL_COLOR_MATERIAL, the normal the tile draw leaves behind), the texel of whatever texture is still bound is not applied;
// where two lines cover one sample the first in the list wins (depth func LESS on equal depths).
struct OvSeg { float ax, ay, bx, by, inv_len2, r, g, b; };     // projected segment in source-pixel space, lit colour 0..255
__global__ __launch_bounds__(256) void k_overlay_lines(RenderParams R, const EnvCam* __restrict__ cams, const float* __restrict__ lines,
                                                       const int first, const int count, const int env) {
  __shared__ OvSeg s_seg[256];
  const int tid = threadIdx.x;
  const int pix = blockIdx.x * 256 + tid;
  const EnvCam c = cams[env];
  const ViewPix p = pix < R.W * R.H ? view_pixel(reinterpret_cast<const float4*>(R.lut), pix, R.W, R.H) : NO_PIX;
  const float sxp = p.sxp, syp = p.syp;
  const bool live = p.live;
  const auto &ox = MSAA_POS.x, &oy = MSAA_POS.y;
  float acc[3] = {0.f, 0.f, 0.f};
  uint32_t covered = 0u;
  for (int base = 0; base < count; base += 256) {
    __syncthreads();
    {                                                  // stage up to 256 projected segments
      OvSeg sg; sg.ax = sg.ay = sg.bx = sg.by = 0.f; sg.inv_len2 = -1.f; sg.r = sg.g = sg.b = 0.f;
      if (base + tid < count) {
        const float* L = lines + (size_t)(first + base + tid) * 9;
        float pe[2][3], lit[2];
#pragma unroll
        for (int v = 0; v < 2; ++v) {
          const float rx = L[3 * v] - c.Cx, ry = L[3 * v + 1] - c.Cy, rz = L[3 * v + 2] - c.Cz;
          const float xla = rx * c.sa + rz * c.ca, zla = -(rx * c.ca - rz * c.sa);
          pe[v][0] = xla; pe[v][1] = ry * c.cth - zla * c.sth; pe[v][2] = ry * c.sth + zla * c.cth;      // eye space, -z forward
        }
        float w0 = -pe[0][2], w1 = -pe[1][2];
        const float wn = NEAR_Z * 1.0001f;
        bool ok = !(w0 < wn && w1 < wn);
        if (ok && (w0 < wn || w1 < wn)) {              // clip the end behind the near plane
          const int vb = w0 < wn ? 0 : 1, vf = 1 - vb;
          const float t = (wn - (-pe[vb][2])) / ((-pe[vf][2]) - (-pe[vb][2]));
#pragma unroll
          for (int k = 0; k < 3; ++k) pe[vb][k] += t * (pe[vf][k] - pe[vb][k]);
          w0 = -pe[0][2]; w1 = -pe[1][2];
        }
        if (ok) {
#pragma unroll
          for (int v = 0; v < 2; ++v) {                // lit as a surface with world normal +y: eye-space normal (0, cth, sth)
            float ndl;
            if (c.L[3] == 0.f) ndl = c.cth * c.L[1] + c.sth * c.L[2];
            else {
              const float lx = c.L[0] - pe[v][0], ly = c.L[1] - pe[v][1], lz = c.L[2] - pe[v][2];
              ndl = (c.cth * ly + c.sth * lz) * rsqrtf(lx * lx + ly * ly + lz * lz);
            }
            lit[v] = fmaxf(ndl, 0.f);
          }
          const float ndl = 0.5f * (lit[0] + lit[1]);  // one colour per segment: the light at its middle
          sg.ax = (pe[0][0] / w0 / c.tx + 1.f) * 0.5f * (float)R.W; sg.ay = (1.f - pe[0][1] / w0 / c.ty) * 0.5f * (float)R.H;
          sg.bx = (pe[1][0] / w1 / c.tx + 1.f) * 0.5f * (float)R.W; sg.by = (1.f - pe[1][1] / w1 / c.ty) * 0.5f * (float)R.H;
          const float dx = sg.bx - sg.ax, dy = sg.by - sg.ay, l2 = dx * dx + dy * dy;
          sg.inv_len2 = l2 > 1e-12f ? 1.f / l2 : -1.f;
          sg.r = 255.f * fminf(L[6] * (c.base[0] + c.dif[0] * ndl), 1.f);
          sg.g = 255.f * fminf(L[7] * (c.base[1] + c.dif[1] * ndl), 1.f);
          sg.b = 255.f * fminf(L[8] * (c.base[2] + c.dif[2] * ndl), 1.f);
        }
      }
      s_seg[tid] = sg;
    }
    __syncthreads();
    if (!live) continue;
    const int n = min(256, count - base);
    for (int i = 0; i < n; ++i) {
      const OvSeg sg = s_seg[i];
      if (sg.inv_len2 < 0.f) continue;
      if (sxp < fminf(sg.ax, sg.bx) - 1.f || sxp > fmaxf(sg.ax, sg.bx) + 1.f || syp < fminf(sg.ay, sg.by) - 1.f || syp > fmaxf(sg.ay, sg.by) + 1.f) continue;
      const float dx = sg.bx - sg.ax, dy = sg.by - sg.ay;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float qx = sxp + ox[q] - sg.ax, qy = syp + oy[q] - sg.ay;
        const float u = (qx * dx + qy * dy) * sg.inv_len2;                       // along the segment, 0..1
        const float cr = qx * dy - qy * dx;                                      // |cross| = distance x length
        const bool in = u >= 0.f && u <= 1.f && cr * cr * sg.inv_len2 <= 0.25f;   // within half a pixel of the line
        if (in && !((covered >> q) & 1u)) { covered |= 1u << q; acc[0] += sg.r; acc[1] += sg.g; acc[2] += sg.b; }
      }
    }
  }
  if (live && covered) {
    const float nf = (float)(4 - __popc(covered));
    uint8_t* dst = R.frames + ((size_t)env * R.W * R.H + pix) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) dst[k] = (uint8_t)(fminf(fmaxf(0.25f * (nf * (float)dst[k] + acc[k]), 0.f), 255.f) + 0.5f);
  }
}

// ---- k_overlay_leds: the additively blended LED spheres of enable_leds as a post-pass on the resolved frames --------------------------
// objects.py:68-121: after a duckiebot's mesh, WorldObj.render_mesh draws per LED a 1 cm gluSphere at alpha 1 and a halo at alpha 0.2 with
// glBlendFunc(GL_SRC_ALPHA, GL_ONE), depth test and depth writes on, lighting on, no texture.  The host states the spheres in WORLD space in
// draw order (dtsim_draw_leds: centre, radius, glColor, alpha).  Per OUTPUT pixel (source pixel through the LUT) and MSAA sample: the depth of
// the opaque scene is recomputed -- the planes by classify(), the meshes by z-buffering the env's projected triangles (ScreenTri, left by the
// render pass's k_obj_setup) -- and every sphere whose FRONT surface is nearer than the sample's depth adds alpha x its lit colour (GL_COLOR_MATERIAL:
// colour x (ambient + diffuse N.L) at the hit, clamped) and writes its depth; the pixel becomes frame + sum / 4.  Additive blending is linear, so
// adding to the resolved frame equals blending into the samples.  Documented deviations (oracle/raster.py overlay_leds states the same
// interpretation): the analytic sphere for the 10 x 10 tessellation, front surfaces only (a back face that gluSphere happens to
// emit before the front face would add a second layer), lit per sample instead of per vertex, and all spheres after ALL opaque objects (GL
// interleaves them with the objects in map order).  Not a hot path: one thread per pixel, the triangle loop only under a sphere's screen box.
struct LedS { float ex, ey, ez, r, cr, cg, cb, a, bx0, bx1, by0, by1; };     // eye-space centre, radius, colour, alpha, source-pixel box

// The opaque scene's eye depth at the four MSAA samples of ONE source pixel of one env (k_overlay_leds, k_depth): centre (nx, ny) in NDC =
// (sxp, syp) in pixels, sample q at NDC (nx + ox[q] sxn, ny - oy[q] syn).  The planes by classify() -- the frame's own ownership test: tile
// present / ground extent / sky --, the meshes by z-buffering the env's projected triangles (boxes / tb: the env's ObjBox and ScreenTri rows that
// the render pass's k_obj_setup left, n_obj of them; boxes null: no mesh objects) for the lanes inside an object's screen box.  depth[q] = t of
// the eye-space ray (dx, dy, -1) t; `sky` where the sample sees the clear colour.
// WHO (k_labels): also who owns each sample -- hits[q] = classify()'s plane hit (class, tile, world hit), obj[q] = the object (the o of the
// ObjBox loop) whose triangle won the sample's z-buffer AND lies strictly nearer than the plane (the colour pass's depth test, shade_msaa),
// else -1.  Without WHO (hits, obj unused, may be null) nothing of that is compiled: the depth arithmetic is the same statements in both.
// tbox: the env's rows of RenderParams.tribox, the screen boxes k_obj_setup writes for EVERY triangle of a live object in every pass (the pass
// allocates the stream whenever it allocates the records: dt_render_layout).  A triangle is tested by ITS BOX IN THAT STREAM, never by the box
// inside its record: the pass rewrites the ScreenTri record of a surviving triangle only, so a triangle it culled (a vertex behind the near
// plane, no area, off the frame) keeps the record of the last pass it survived -- or, on a fresh handle, whatever the allocation held -- and
// its inverted box in the stream is what skips it here, as the colour pass skips it.  Every reader of the records goes through this function,
// so every map of a re-rendered handle is that of a fresh handle in the same state (tests/test_gpu_rerender_maps.py).
template <bool WHO>
__device__ inline void scene_samples4(const EnvCam& c, const MapU& m, const TileLds* tiles, const ObjBox* boxes, const ScreenTri* tb, const float4* tbox,
                                      const int n_obj, const float nx, const float ny, const float sxp, const float syp, const float sxn, const float syn,
                                      const float sky, float depth[4], Hit* hits, int* obj) {
  const auto &ox = MSAA_POS.x, &oy = MSAA_POS.y;
  float wbest[4] = {0.f, 0.f, 0.f, 0.f};
  int tbest[4] = {-1, -1, -1, -1};
  int obest[4] = {-1, -1, -1, -1};
  if (boxes) {
    for (int o = 0; o < n_obj; ++o) {
      const ObjBox ob = boxes[o];
      if (ob.count <= 0 || sxp < ob.bx0 - 1.f || sxp > ob.bx1 + 1.f || syp < ob.by0 - 1.f || syp > ob.by1 + 1.f) continue;
      for (int t = ob.first; t < ob.first + ob.count; ++t) {   // the pass's own cull stream: see the comment above
        const float4 b = tbox[t];
        if (!(sxp < b.x || sxp > b.y || syp < b.z || syp > b.w)) test_tri_inside(tb[t], sxp, syp, wbest, tbest);
      }
      if constexpr (WHO) {
#pragma unroll
        for (int q = 0; q < 4; ++q)                   // the sample's winner so far is one of this object's triangles
          if (tbest[q] >= ob.first && tbest[q] < ob.first + ob.count) obest[q] = o;
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    // the steps stated here round one way wherever they are inlined: the sample position is an explicit fused multiply-add, the mesh depth one
    // IEEE division, the minimum exact (PARITY.md 4, "frames of ONE state rendered again"); classify() and test_tri are the frame's own code
    const Ray rs = make_ray(fmaf(ox[q], sxn, nx), fmaf(-oy[q], syn, ny), c.tx, c.ty, c.sth, c.cth);
    const Hit h = classify(c, m, tiles, rs);
    float d = h.cls == CLS_SKY ? sky : h.t;
    if constexpr (WHO) { hits[q] = h; obj[q] = -1; }
    if (tbest[q] >= 0) {
      const float dm = 1.f / wbest[q];
      if constexpr (WHO) obj[q] = dm < d ? obest[q] : -1;
      d = fminf(d, dm);
    }
    depth[q] = d;
  }
}
__device__ inline void scene_depth4(const EnvCam& c, const MapU& m, const TileLds* tiles, const ObjBox* boxes, const ScreenTri* tb, const float4* tbox,
                                    const int n_obj, const float nx, const float ny, const float sxp, const float syp, const float sxn, const float syn,
                                    const float sky, float depth[4]) {
  scene_samples4<false>(c, m, tiles, boxes, tb, tbox, n_obj, nx, ny, sxp, syp, sxn, syn, sky, depth, nullptr, nullptr);
}

__global__ __launch_bounds__(256) void k_overlay_leds(RenderParams R, const EnvCam* __restrict__ cams, const float* __restrict__ spheres,
                                                      const int first, const int count, const int env) {
  __shared__ LedS s_led[64];
  const int tid = threadIdx.x;
  const int pix = blockIdx.x * 256 + tid;
  const EnvCam c = cams[env];
  const MapU m = map_u(R.maps[c.map_id]);
  const TileLds* tiles = reinterpret_cast<const TileLds*>(R.tile_recs);
  const ViewPix p = pix < R.W * R.H ? view_pixel(reinterpret_cast<const float4*>(R.lut), pix, R.W, R.H) : NO_PIX;
  const float nx = p.nx, ny = p.ny, sxp = p.sxp, syp = p.syp;
  const bool live = p.live;
  const auto &ox = MSAA_POS.x, &oy = MSAA_POS.y;
  const float sxn = 2.f / (float)R.W, syn = 2.f / (float)R.H;
  float add[3] = {0.f, 0.f, 0.f};
  float depth[4] = {0.f, 0.f, 0.f, 0.f};
  bool have_depth = false, any = false;
  for (int base = 0; base < count; base += 64) {
    __syncthreads();
    if (tid < 64) {
      LedS sp; sp.r = -1.f; sp.ex = sp.ey = sp.ez = sp.cr = sp.cg = sp.cb = sp.a = 0.f; sp.bx0 = sp.by0 = 1.f; sp.bx1 = sp.by1 = 0.f;
      if (base + tid < count) {
        const float* S = spheres + (size_t)(first + base + tid) * 8;
        const float rx = S[0] - c.Cx, ry = S[1] - c.Cy, rz = S[2] - c.Cz;
        const float xla = rx * c.sa + rz * c.ca, zla = -(rx * c.ca - rz * c.sa);
        sp.ex = xla; sp.ey = ry * c.cth - zla * c.sth; sp.ez = ry * c.sth + zla * c.cth;                 // eye space, -z forward
        const float w = -sp.ez, r = S[3];
        if (r > 0.f && w + r > NEAR_Z) {
          sp.r = r; sp.cr = S[4]; sp.cg = S[5]; sp.cb = S[6]; sp.a = S[7];
          const float wn = fmaxf(w - r, NEAR_Z);
          const float cx = (sp.ex / w / c.tx + 1.f) * 0.5f * (float)R.W, cy = (1.f - sp.ey / w / c.ty) * 0.5f * (float)R.H;
          const float rad = r / wn / fminf(c.tx / (float)R.W, c.ty / (float)R.H) * 0.5f * 1.5f + 2.f;     // conservative: only prunes
          sp.bx0 = cx - rad; sp.bx1 = cx + rad; sp.by0 = cy - rad; sp.by1 = cy + rad;
          if (!(w > 0.f)) { sp.bx0 = sp.by0 = -1e30f; sp.bx1 = sp.by1 = 1e30f; }                          // centre behind the eye: no box, test everything
        }
      }
      s_led[tid] = sp;
    }
    __syncthreads();
    if (!live) continue;
    const int n = min(64, count - base);
    for (int i = 0; i < n; ++i) {
      const LedS sp = s_led[i];
      if (!(sp.r > 0.f) || sxp < sp.bx0 || sxp > sp.bx1 || syp < sp.by0 || syp > sp.by1) continue;
      if (!have_depth) {                               // the opaque scene's depth at the four samples, once per pixel that any sphere may touch
        have_depth = true;
        const bool obj = R.stris && R.objbox && R.tribox;
        scene_depth4(c, m, tiles, obj ? R.objbox + (size_t)env * DTSIM_MAX_OBJECTS : nullptr, obj ? R.stris + (size_t)env * R.max_tris : nullptr,
                     obj ? R.tribox + (size_t)env * R.max_tris : nullptr, obj ? R.maps[c.map_id].n_obj : 0, nx, ny, sxp, syp, sxn, syn, 3.0e38f, depth);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float dx = (nx + ox[q] * sxn) * c.tx, dy = (ny - oy[q] * syn) * c.ty;       // eye-space ray (dx, dy, -1) t, t = eye depth
        const float a = dx * dx + dy * dy + 1.f;
        const float b = dx * sp.ex + dy * sp.ey - sp.ez;
        const float cc = sp.ex * sp.ex + sp.ey * sp.ey + sp.ez * sp.ez - sp.r * sp.r;
        const float disc = b * b - a * cc;
        if (!(disc > 0.f)) continue;
        const float t = (b - sqrtf(disc)) / a;
        if (!(t >= NEAR_Z && t <= FAR_Z && t < depth[q])) continue;
        const float px = t * dx, py = t * dy, pz = -t;
        const float inv_r = 1.f / sp.r;
        const float nxe = (px - sp.ex) * inv_r, nye = (py - sp.ey) * inv_r, nze = (pz - sp.ez) * inv_r;
        float ndl;
        if (c.L[3] == 0.f) ndl = nxe * c.L[0] + nye * c.L[1] + nze * c.L[2];
        else {
          const float lx = c.L[0] - px, ly = c.L[1] - py, lz = c.L[2] - pz;
          ndl = (nxe * lx + nye * ly + nze * lz) * rsqrtf(lx * lx + ly * ly + lz * lz);
        }
        ndl = fmaxf(ndl, 0.f);
        add[0] += sp.a * 255.f * fminf(sp.cr * (c.base[0] + c.dif[0] * ndl), 1.f);
        add[1] += sp.a * 255.f * fminf(sp.cg * (c.base[1] + c.dif[1] * ndl), 1.f);
        add[2] += sp.a * 255.f * fminf(sp.cb * (c.base[2] + c.dif[2] * ndl), 1.f);
        depth[q] = t;
        any = true;
      }
    }
  }
  if (live && any) {
    uint8_t* dst = R.frames + ((size_t)env * R.W * R.H + pix) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) dst[k] = (uint8_t)(fminf(fmaxf((float)dst[k] + 0.25f * add[k], 0.f), 255.f) + 0.5f);
  }
}

// ---- the rules that the camera-map kernels (k_depth, k_labels, k_flow, k_camera_maps) share, each stated once -------------------------------
// Output pixel `pix` = (i, j) of the [oh][ow] map is camera pixel (i sy + sy / 2, j sx + sx / 2), sy = H / oh, sx = W / ow: point-sampled, only
// those pixels are traced.
__device__ __forceinline__ size_t out_camera_pixel(const int pix, const int W, const int H, const int oh, const int ow) {
  const int sx = W / ow, sy = H / oh;
  const int i = pix / ow, j = pix - i * ow;
  return (size_t)(i * sy + sy / 2) * W + (j * sx + sx / 2);
}
// ... and (e, pix) of an [N][oh * ow] map, or of plane k (0: x, 1: y) of an [N][2][oh * ow] flow map, is element:
__device__ __forceinline__ size_t map_at(const int e, const int n_out, const int pix) { return (size_t)e * (size_t)n_out + (size_t)pix; }
__device__ __forceinline__ size_t flow_at(const int e, const int n_out, const int pix, const int k) { return (2 * (size_t)e + k) * (size_t)n_out + (size_t)pix; }

// The table entry of a thread's camera pixel `at` (in: the thread owns one) for each env of its chunk.  Without CAL it is the shared table's,
// loaded once.  CAL: the entry depends on the env -- env_cal[e], then the calibration's source index, then the identity table's entry there:
// three dependent loads (cal_entry).  pixel(e, e1) is called at the top of the loop body, behind nothing: it hands out env e's entry and
// issues the chain of env e + 1, which is waited for at the top of the next iteration, behind this env's scene.
template <bool CAL>
struct EnvEntry {
  const float4* lut; const int32_t* cal_src; const int32_t* env_cal;
  int n_cal; bool in; size_t at; int W, H;
  ViewPix p;
  float4 l_nxt;
  __device__ __forceinline__ EnvEntry(const float4* lut, const int32_t* cal_src, const int32_t* env_cal, const int n_cal, const bool in, const size_t at,
                             const int W, const int H, const int e0)
      : lut(lut), cal_src(cal_src), env_cal(env_cal), n_cal(n_cal), in(in), at(at), W(W), H(H), p(NO_PIX), l_nxt(make_float4(0.f, 0.f, 0.f, 0.f)) {
    if constexpr (CAL) l_nxt = cal_entry(lut, cal_src, env_cal, n_cal, e0, in, at, W, H);
    else if (in) p = view_pixel(lut, at, W, H);
  }
  __device__ __forceinline__ ViewPix pixel(const int e, const int e1) {
    if constexpr (CAL) {
      const float4 l = l_nxt;
      if (e + 1 < e1) l_nxt = cal_entry(lut, cal_src, env_cal, n_cal, e + 1, in, at, W, H);
      p.live = l.z != 0.f; p.nx = l.x; p.ny = l.y;
      src_px(l.x, l.y, W, H, p.sxp, p.syp);
    }
    return p;
  }
};

// What a pixel reads of env e, all at a wave-uniform index (read-only __restrict__ pointers: scalar loads): its camera record, its map and the
// rows of the pass's ObjBox / ScreenTri / box streams; objbox null: the pass projected no mesh triangles.  The map id is clamped:
// calling a masked form with another mask than the pass's is the caller's error (include/dtsim.h) and its result is undefined -- the record of
// a skipped env is an older state's, or the zeros the scratch starts with -- and the clamp only keeps that error from indexing outside the map
// table on a device others share.
// (The env's rows are member functions, evaluated at scene_samples4's call inside `if (p.live)`: as fields filled before it, +3 instructions, +2 SGPRs.)
struct EnvScene {
  EnvCam c; const RenderMapDev* rm; MapU m;
  int e, max_tris; const ObjBox* objbox; const ScreenTri* stris; const float4* tribox;
  __device__ const ObjBox* boxes() const { return objbox ? objbox + (size_t)e * DTSIM_MAX_OBJECTS : nullptr; }
  __device__ const ScreenTri* tris() const { return objbox ? stris + (size_t)e * max_tris : nullptr; }
  __device__ const float4* tri_boxes() const { return objbox ? tribox + (size_t)e * max_tris : nullptr; }
  __device__ int n_obj() const { return objbox ? rm->n_obj : 0; }
};
__device__ __forceinline__ EnvScene env_scene(const int e, const EnvCam* __restrict__ cams, const RenderMapDev* __restrict__ maps, const int n_maps,
                                     const ObjBox* __restrict__ objbox, const ScreenTri* __restrict__ stris, const float4* __restrict__ tribox,
                                     const int max_tris) {
  EnvScene s;
  s.c = cams[e];
  s.rm = &maps[min((unsigned)s.c.map_id, (unsigned)(n_maps - 1))];
  s.m = map_u(*s.rm);
  s.e = e; s.max_tris = max_tris; s.objbox = objbox; s.stris = stris; s.tribox = tribox;
  return s;
}
// scene_samples4 of that env at that pixel; sky = +inf.
template <bool WHO>
__device__ __forceinline__ void scene_samples4(const EnvScene& s, const TileLds* tiles, const ViewPix& p, const float sxn, const float syn, float depth[4],
                                      Hit* hits, int* obj) {
  scene_samples4<WHO>(s.c, s.m, tiles, s.boxes(), s.tris(), s.tri_boxes(), s.n_obj(), p.nx, p.ny, p.sxp, p.syp, sxn, syn, __builtin_inff(), depth, hits,
                      obj);
}

// The WINNER of a pixel: the sample with the smallest depth, ties to the lowest index; sky = +inf, so it wins only when all four are sky.  d: its
// depth, o: its object or -1, ox / oy: its sample offsets, h: its plane hit; unread members fold away.  A kernel folds samples 1..3 into sample 0
// in its own unrolled loop: a function handed the arrays keeps them in scratch or changes instruction counts (profiles/render_views_isa.txt).
struct Winner { float d; int o; float ox, oy; Hit h; };
__device__ __forceinline__ Winner first_sample(const float d, const int o, const Hit& h) { return {d, o, MSAA_POS.x[0], MSAA_POS.y[0], h}; }
__device__ __forceinline__ void take_nearer(Winner& w, const float d, const int o, const int q, const Hit& h) {
  if (d < w.d) { w.d = d; w.o = o; w.ox = MSAA_POS.x[q]; w.oy = MSAA_POS.y[q]; w.h = h; }
}
// Its instance id: o + 1 of its object (the o of scene_samples4<true>: the env's map's object list), else DTSIM_INSTANCE_NONE.
__device__ __forceinline__ uint32_t instance_id(const int ob) { return ob >= 0 ? (uint32_t)ob + 1u : (uint32_t)DTSIM_INSTANCE_NONE; }

// The class of the nearest texel of a textured tile at tile fraction (fx, fz): the texel coordinates are tile_texel_xy's, the ones tile_color
// filters at, with the half-texel shift taken back: floor(x + 0.5), wrapped.  tex_w, tex_h: the one (power-of-two) size of all tile textures;
// texel_class: dt_pack_label_tables' pool, addressed like R.texels.  A camera pixel (sample_class) and a BEV cell (k_bev) that hit one world
// point name one class because both call this.
__device__ __forceinline__ uint32_t tile_texel_class(const TileLds& tr, const float fx, const float fz, const int tex_w, const int tex_h,
                                            const uint8_t* __restrict__ texel_class) {
  float x, y;
  tile_texel_xy(tr, fx, fz, x, y);
  const int x0 = (int)floorf(x + 0.5f) & (tex_w - 1), y0 = (int)floorf(y + 0.5f) & (tex_h - 1);
  return texel_class[tr.tex_off + (uint32_t)(y0 * (tex_w + 1) + x0)];
}
// Owner -> class, of the winner's object ob (or -1) and plane hit h: the mesh table through the map's object-instance table, the two fixed plane
// classes, or for a tile the class of its texel.
__device__ __forceinline__ uint32_t sample_class(const int ob, const Hit& h, const EnvScene& s, const TileLds* __restrict__ tiles,
                                                 const ObjInstDev* __restrict__ objs, const uint8_t* __restrict__ texel_class,
                                                 const uint8_t* __restrict__ mesh_class, const int n_mesh_class, const int tex_w, const int tex_h) {
  if (ob >= 0) return mesh_class[min((unsigned)objs[s.rm->obj_off + ob].mesh_id, (unsigned)(n_mesh_class - 1))];
  if (h.cls == CLS_SKY) return DTSIM_LABEL_SKY;
  if (h.cls == CLS_GROUND) return DTSIM_LABEL_GROUND;
  const TileLds tr = tiles[s.m.tile_off + h.tj * s.m.gw + h.ti];
  if (!(tr.flags & 2u)) return DTSIM_LABEL_GROUND;     // a present tile without a texture has no texel table
  // the tile fraction, as shade_msaa hands it to tile_color
  return tile_texel_class(tr, h.wx * s.m.its - (float)h.ti, h.wz * s.m.its - (float)h.tj, tex_w, tex_h, texel_class);
}

// An eye-space point on the image: w, the rectilinear (u, v) of dtsim_ipm's step 1 and A(u, v) -- the identity, or with a calibration the
// forward model at (u - 0.5, v - 0.5) (ipm_project.h dt_ipm_forward, in float64: in float32 its 25 operations would take the count of
// roundings R of tests/test_flow_model_host.py past 32).  Both terms of a flow go through this one function, so one point gives one value.
struct FlowPt { double ax, ay; float w, u, v; };
__device__ inline FlowPt flow_image(const float x, const float y, const float z, const float tx, const float ty, const float Wf, const float Hf,
                                    const IpmCal* __restrict__ cal) {
  FlowPt p;
  p.w = -z;
  p.u = (x / p.w / tx + 1.f) * 0.5f * Wf;             // R: 4 roundings (two divisions, the sum, the product by W; x 0.5 is exact)
  p.v = (1.f - y / p.w / ty) * 0.5f * Hf;             //    (the same 4, of the other coordinate)
  p.ax = (double)p.u; p.ay = (double)p.v;
  if (cal) dt_ipm_forward(*cal, p.ax - 0.5, p.ay - 0.5, 0.0, p.ax, p.ay);   // (wave-uniform) R: none, float64
  return p;
}

// The flow of the winner, rule by rule (as ONE function they change k_flow's instruction count: profiles/render_views_isa.txt).
// Its eye-space hit X = d (xe, ye, -1), rebuilt from the sample's own ray (scene_samples4's statement of it) at the sample's depth:
struct Eye3 { float x, y, z; };
__device__ __forceinline__ Eye3 winner_eye_point(const Winner& w, const ViewPix& p, const EnvCam& c, const float sxn, const float syn) {
  const float xe = fmaf(w.ox, sxn, p.nx) * c.tx, ye = fmaf(-w.oy, syn, p.ny) * c.ty;
  return {w.d * xe, w.d * ye, -w.d};
}
// ... the ONE pair (M, t) it moves by: the static one, or the winning object's dynamic slot's (a per-lane read, only on lanes such an object owns):
__device__ __forceinline__ const FlowXf* flow_xf(const FlowRec& rec, const int ob, const RenderMapDev& rm, const ObjInstDev* objs) {
  const FlowXf* xf = &rec.fix;
  if (ob >= 0) {
    const int slot = objs[rm.obj_off + ob].dyn_slot;
    if (slot >= 0) xf = &rec.dyn[min(slot, DTSIM_MAX_DYNAMIC - 1)];
  }
  return xf;
}
// ... M X + t.  R: 3 roundings per coordinate (three fused multiply-adds), x and w both enter u: 6
__device__ __forceinline__ Eye3 flow_apply(const FlowXf* xf, const Eye3& X) {
  return {fmaf(xf->M[0], X.x, fmaf(xf->M[1], X.y, fmaf(xf->M[2], X.z, xf->t[0]))), fmaf(xf->M[3], X.x, fmaf(xf->M[4], X.y, fmaf(xf->M[5], X.z, xf->t[1]))),
          fmaf(xf->M[6], X.x, fmaf(xf->M[7], X.y, fmaf(xf->M[8], X.z, xf->t[2])))};
}
// ... and whether the previous point lies in front of the camera and on the image (a NaN fails every comparison; w, u, v by value: by FlowPt&, k_flow moves).
__device__ __forceinline__ bool flow_valid(const float w, const float u, const float v, const float Wf, const float Hf) {
  return w >= NEAR_Z && u >= 0.f && u < Wf && v >= 0.f && v < Hf;
}

// The depth store of one pixel (to: map_at): float32, or half.
__device__ __forceinline__ void store_depth(void* __restrict__ out, const bool f16, const size_t to, const float d) {
  if (f16) static_cast<__half*>(out)[to] = __float2half_rn(d);
  else static_cast<float*>(out)[to] = d;
}

// ---- k_depth: the depth map of every env's camera frame (dtsim_depth; the quantity: include/dtsim.h) -------------------------------------
// A thread owns one output pixel (out_camera_pixel) -- its table entry (source-pixel NDC, live flag) is loaded once -- and loops over the
// DEPTH_ENVS envs of its chunk (grid: pixel blocks x env chunks); the env's camera record, map and object boxes are wave-uniform (EnvScene),
// and every store is one coalesced row segment of one env's map.  Per env the depth is scene_samples4 without WHO -- the code under the LED
// spheres, i.e. classify() per sample and the z-buffer of the triangles the pass projected -- and the minimum of the four (the winner's
// depth, taken by an fminf tree since nothing else of the winner is wanted).
// One state, one result: the env loop is kept as ONE copy of its body (no unrolling, no peeled iteration), so every env of every chunk, the
// tail chunk included, runs the same instructions on its record, whatever the compiler fuses inside classify() (which is the frame's own
// code and stays as it is, so its products are not restated as explicit fused multiply-adds here); the pixel's part (table entry, sample
// offsets) does not depend on the env.  That the compiler keeps one copy is its choice, not a property of this source: the guarantee rests on
// tests/test_gpu_depth.py::test_env_positions_and_the_tail_chunk_give_the_same_bytes (envs e, e + 64, e + 128 of one state, a second call, a
// second render: byte-identical), which fails if a peeled or versioned copy ever rounds differently.
// CAL (dtsim_set_distortion_luts' tables installed and DTSIM_MAP_ENV_TABLES given; cal_src / env_cal / n_cal are read only then): the same grid,
// thread and loop, but the pixel's entry is the ENV's -- EnvEntry<true> -- and is taken inside the loop body, still one copy of it
// (tests/test_gpu_camera_rand_maps.py holds envs e, e + 64, e + 70 of one state and table to the same bytes).  The scene is sampled as
// without CAL.  CAL = false keeps the instructions it had before the parameter (tools/isa_compare.py; profiles/render_views_isa.txt).
template <bool F16, bool CAL = false>
__global__ __launch_bounds__(256) void k_depth(const EnvCam* __restrict__ cams, const RenderMapDev* __restrict__ maps, const TileLds* __restrict__ tiles,
                                               const float4* __restrict__ lut, const ObjBox* __restrict__ objbox, const ScreenTri* __restrict__ stris,
                                               const float4* __restrict__ tribox, const int max_tris, const int n_maps, const int N, const int W, const int H,
                                               const int oh, const int ow, void* __restrict__ out, const uint8_t* __restrict__ mask,
                                               const int32_t* __restrict__ cal_src, const int32_t* __restrict__ env_cal, const int n_cal) {
  const int n_out = oh * ow;
  const int pix = blockIdx.x * 256 + threadIdx.x;
  const bool in = pix < n_out;
  const int e0 = blockIdx.y * DEPTH_ENVS, e1 = min(N, e0 + DEPTH_ENVS);
  EnvEntry<CAL> entry(lut, cal_src, env_cal, n_cal, in, in ? out_camera_pixel(pix, W, H, oh, ow) : 0, W, H, e0);
  const float sxn = 2.f / (float)W, syn = 2.f / (float)H;
#pragma clang loop unroll(disable)
  for (int e = e0; e < e1; ++e) {
    const ViewPix p = entry.pixel(e, e1);
    if (mask && !mask[e]) continue;                    // (wave-uniform) the masked call: this env's row keeps its bytes
    const EnvScene s = env_scene(e, cams, maps, n_maps, objbox, stris, tribox, max_tris);
    float d = 0.f;
    if (p.live) {
      float ds[4];
      scene_samples4<false>(s, tiles, p, sxn, syn, ds, nullptr, nullptr);
      d = fminf(fminf(ds[0], ds[1]), fminf(ds[2], ds[3]));
    }
    if (in) store_depth(out, F16, map_at(e, n_out, pix), d);
  }
}

// ---- k_labels: the semantic label map of every env's camera frame (dtsim_labels; the quantity: include/dtsim.h) ---------------------------
// The sibling of k_depth: the same grid (output-pixel blocks x env chunks of DEPTH_ENVS), the pixel's table entry loaded once, the env's camera
// record, map and object boxes at a wave-uniform index, the env loop ONE copy of its body (tests/test_gpu_labels.py holds envs e, e + 64,
// e + 128 to the same bytes).  Per env it runs scene_samples4<true> -- k_depth's statements plus who owns each sample --, takes the
// winner and maps its owner to a class (sample_class).
// A thread owns ONE pixel, not four adjacent ones: the pass is bound by the four classify() calls and the triangle loop per pixel and env, not
// by its stores (k_depth takes the same time for half maps as for float32 ones, profiles/depth_timing.txt; k_labels, with a quarter of the
// bytes, takes 1.4 x k_depth's time on planes and the same time under meshes, profiles/labels_timing.txt); four pixels per lane would serialise
// four of those per lane for the sake of one wider store, and a wavefront's 64 byte stores are still one contiguous 64-byte row segment.
// LAB / INST (dtsim_labels: <true, false>; dtsim_instances: <false, true>, or <true, true> when it is given a label map too): which of the two
// maps the launch writes, from the ONE classification of the pixel -- `inst` takes the winner's instance_id, DTSIM_INSTANCE_NONE also for a
// pixel without a source; a second byte store at the same offset, as coalesced as the first.  Without LAB the class mapping -- mesh table,
// tile record, texel gather -- is not compiled, and the plane hits it alone reads are dead.  CAL: as k_depth's.
static_assert(DTSIM_MAX_OBJECTS <= 255, "an instance id o + 1 must fit the map's byte");
template <bool LAB, bool INST, bool CAL = false>
__global__ __launch_bounds__(256) void k_labels(const EnvCam* __restrict__ cams, const RenderMapDev* __restrict__ maps, const TileLds* __restrict__ tiles,
                                                const float4* __restrict__ lut, const ObjBox* __restrict__ objbox, const ScreenTri* __restrict__ stris,
                                                const float4* __restrict__ tribox, const ObjInstDev* __restrict__ objs, const uint8_t* __restrict__ texel_class,
                                                const uint8_t* __restrict__ mesh_class, const int n_mesh_class, const int tex_w, const int tex_h,
                                                const int max_tris, const int n_maps, const int N, const int W, const int H, const int oh, const int ow,
                                                uint8_t* __restrict__ out, uint8_t* __restrict__ inst, const uint8_t* __restrict__ mask,
                                                const int32_t* __restrict__ cal_src, const int32_t* __restrict__ env_cal, const int n_cal) {
  const int n_out = oh * ow;
  const int pix = blockIdx.x * 256 + threadIdx.x;
  const bool in = pix < n_out;
  const int e0 = blockIdx.y * DEPTH_ENVS, e1 = min(N, e0 + DEPTH_ENVS);
  EnvEntry<CAL> entry(lut, cal_src, env_cal, n_cal, in, in ? out_camera_pixel(pix, W, H, oh, ow) : 0, W, H, e0);
  const float sxn = 2.f / (float)W, syn = 2.f / (float)H;
#pragma clang loop unroll(disable)
  for (int e = e0; e < e1; ++e) {
    const ViewPix p = entry.pixel(e, e1);
    if (mask && !mask[e]) continue;                    // (wave-uniform) the masked call: this env's row keeps its bytes
    const EnvScene s = env_scene(e, cams, maps, n_maps, objbox, stris, tribox, max_tris);
    uint32_t cls = DTSIM_LABEL_NONE, who = DTSIM_INSTANCE_NONE;
    if (p.live) {
      float ds[4];
      Hit hs[4];
      int os[4];
      scene_samples4<true>(s, tiles, p, sxn, syn, ds, hs, os);
      Winner w = first_sample(ds[0], os[0], hs[0]);
#pragma unroll
      for (int q = 1; q < 4; ++q) take_nearer(w, ds[q], os[q], q, hs[q]);
      if constexpr (INST) who = instance_id(w.o);
      if constexpr (LAB) cls = sample_class(w.o, w.h, s, tiles, objs, texel_class, mesh_class, n_mesh_class, tex_w, tex_h);
    }
    if (in) {
      const size_t to = map_at(e, n_out, pix);
      if constexpr (LAB) out[to] = (uint8_t)cls;
      if constexpr (INST) inst[to] = (uint8_t)who;
    }
  }
}
// ---- k_flow_mark, k_flow_setup, k_flow: the optical-flow map of dtsim_flow (the quantity: include/dtsim.h; the transform: flow_transform.h) ------
// k_flow_mark: the copy -- a thread per env takes what the flow needs of the CURRENT state out of the state arrays into the handle's FlowMark.
__global__ __launch_bounds__(64) void k_flow_mark(const SimArrays A, FlowMark* __restrict__ marks, const uint8_t* __restrict__ mask) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= A.N || (mask && !mask[e])) return;
  const size_t N = (size_t)A.N;
  FlowMark m;
  m.x = A.pos_x[e]; m.z = A.pos_z[e]; m.ang = A.angle[e];
#pragma unroll
  for (int k = 0; k < 6; ++k) m.cam[k] = A.cam[k * N + e];
  m.episode = A.episode[e]; m.map_id = A.map_id[e]; m.has = 1; m.pad = 0;
  static_assert(DTSIM_MAX_DYNAMIC == 8, "FlowMark and FlowRec hold eight dynamic slots");
#pragma unroll
  for (int k = 0; k < DTSIM_MAX_DYNAMIC; ++k) {
    m.ob[k][0] = A.ob_cx[k * N + e]; m.ob[k][1] = A.ob_cy[k * N + e]; m.ob[k][2] = A.ob_cz[k * N + e]; m.ob[k][3] = A.ob_yrot[k * N + e];
  }
  marks[e] = m;
}
// k_flow_setup: one small launch per dtsim_flow call, a thread per env: dt_flow_record (flow_transform.h) on the mark and the current state
// arrays, in float64, into the env's FlowRec.
__global__ __launch_bounds__(64) void k_flow_setup(const SimArrays A, const FlowMark* __restrict__ marks, FlowRec* __restrict__ recs, const int per_env,
                                                   const int W, const int H, const uint8_t* __restrict__ mask) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= A.N || (mask && !mask[e])) return;
  const size_t N = (size_t)A.N;
  FlowState cur;
  cur.x = A.pos_x[e]; cur.z = A.pos_z[e]; cur.ang = A.angle[e];
#pragma unroll
  for (int k = 0; k < 6; ++k) cur.cam[k] = (double)A.cam[k * N + e];
#pragma unroll
  for (int k = 0; k < DTSIM_MAX_DYNAMIC; ++k) {
    cur.ob[k][0] = A.ob_cx[k * N + e]; cur.ob[k][1] = A.ob_cy[k * N + e]; cur.ob[k][2] = A.ob_cz[k * N + e]; cur.ob[k][3] = A.ob_yrot[k * N + e];
  }
  FlowRec r;
  dt_flow_record(marks[e], cur, A.episode[e], A.map_id[e], per_env != 0, W, H, r);
  recs[e] = r;
}
// k_flow: the sibling of k_labels -- the same grid (output-pixel blocks x env chunks of DEPTH_ENVS), the pixel's table entry loaded once, the
// env's camera record, map, object boxes and FlowRec at a wave-uniform index, the env loop ONE copy of its body (tests/test_gpu_flow.py holds
// envs e, e + 64, e + 128 to the same bytes).  Per env it runs scene_samples4<true>, takes the winner, rebuilds its eye-space hit
// X = d (xe, ye, -1) from the sample's own ray, applies ONE pair (M, t) -- the static one, or the winning object's dynamic slot's, a per-lane
// read of the env's record only on lanes a dynamic object owns -- and puts X and M X + t on the image through flow_image.
// flow = A(prev) - A(cur), rounded to float32 once.
__global__ __launch_bounds__(256) void k_flow(const EnvCam* __restrict__ cams, const RenderMapDev* __restrict__ maps, const TileLds* __restrict__ tiles,
                                              const float4* __restrict__ lut, const ObjBox* __restrict__ objbox, const ScreenTri* __restrict__ stris,
                                              const float4* __restrict__ tribox, const ObjInstDev* __restrict__ objs, const FlowRec* __restrict__ recs,
                                              const IpmCal* __restrict__ cal, const int max_tris, const int n_maps, const int N, const int W, const int H, const int oh, const int ow,
                                              float* __restrict__ flow, uint8_t* __restrict__ valid, const uint8_t* __restrict__ mask) {
  const int n_out = oh * ow;
  const int pix = blockIdx.x * 256 + threadIdx.x;
  const bool in = pix < n_out;
  const ViewPix p = in ? view_pixel(lut, out_camera_pixel(pix, W, H, oh, ow), W, H) : NO_PIX;
  const float sxn = 2.f / (float)W, syn = 2.f / (float)H, Wf = (float)W, Hf = (float)H;
  const int e0 = blockIdx.y * DEPTH_ENVS, e1 = min(N, e0 + DEPTH_ENVS);
#pragma clang loop unroll(disable)
  for (int e = e0; e < e1; ++e) {
    if (mask && !mask[e]) continue;                    // (wave-uniform) the masked call: this env's rows keep their bytes
    const EnvScene s = env_scene(e, cams, maps, n_maps, objbox, stris, tribox, max_tris);
    const FlowRec& rec = recs[e];
    float fu = 0.f, fv = 0.f;
    bool ok = false;
    if (p.live) {
      float ds[4];
      Hit hs[4];
      int os[4];
      scene_samples4<true>(s, tiles, p, sxn, syn, ds, hs, os);
      Winner w = first_sample(ds[0], os[0], hs[0]);
#pragma unroll
      for (int q = 1; q < 4; ++q) take_nearer(w, ds[q], os[q], q, hs[q]);
      if (w.d < __builtin_inff() && rec.valid) {       // not sky (sky = +inf wins only when all four are), and a mark of this episode
        const Eye3 X = winner_eye_point(w, p, s.c, sxn, syn), Xp = flow_apply(flow_xf(rec, w.o, *s.rm, objs), X);
        const FlowPt a = flow_image(X.x, X.y, X.z, rec.txc, rec.tyc, Wf, Hf, cal);
        const FlowPt b = flow_image(Xp.x, Xp.y, Xp.z, rec.txp, rec.typ, Wf, Hf, cal);
        ok = flow_valid(b.w, b.u, b.v, Wf, Hf);
        if (ok) { fu = (float)(b.ax - a.ax); fv = (float)(b.ay - a.ay); }              // R: 1 (the one rounding of the difference)
      }
    }
    if (in) {                                          // the two planes of the env's map: each store a coalesced row segment, as is the byte of `valid`
      flow[flow_at(e, n_out, pix, 0)] = fu;
      flow[flow_at(e, n_out, pix, 1)] = fv;
      if (valid) valid[map_at(e, n_out, pix)] = ok ? 1 : 0;
    }
  }
}

// ---- k_camera_maps: depth, labels, instances and flow of one size from ONE classification of the pixel (dtsim_camera_maps) -------------------
// The sibling of k_labels and k_flow: the same grid (output-pixel blocks x env chunks of DEPTH_ENVS), the pixel's table entry loaded once -- with
// CAL the env's own, as k_depth's --, the env's camera record, map, object boxes and FlowRec at a wave-uniform index, the env loop ONE copy of
// its body (tests/test_gpu_camera_maps.py holds envs e, e + 64, e + 128 to the same bytes), the wave-uniform mask skip.  Per env it runs
// scene_samples4<true> ONCE, and every output is its one winner's:
//   depth      its depth -- the minimum of the four, k_depth's value --, 0 for a pixel without a source; float32, or half (f16, wave-uniform);
//   labels     its sample_class;
//   inst       its instance_id;
//   flow/valid k_flow's body, written out (the one such site: the comment in the body) (FLOW: only then are the float64 forward model and the FlowRec compiled in).
// depth, labels and inst are branched on at run time (kernel arguments: wave-uniform); with FLOW, flow is written and valid if given.  The
// four passes it stands for pay the four classify() calls and the triangle loop once each; this one pays them once (the stores are not the
// cost: k_labels' comment).
// FLOW && CAL does not exist: the flow under per-env tables is refused (dtsim_flow).
template <bool FLOW, bool CAL>
__global__ __launch_bounds__(256) void k_camera_maps(const EnvCam* __restrict__ cams, const RenderMapDev* __restrict__ maps, const TileLds* __restrict__ tiles,
                                                     const float4* __restrict__ lut, const ObjBox* __restrict__ objbox, const ScreenTri* __restrict__ stris,
                                                     const float4* __restrict__ tribox, const ObjInstDev* __restrict__ objs,
                                                     const uint8_t* __restrict__ texel_class, const uint8_t* __restrict__ mesh_class,
                                                     const int n_mesh_class, const int tex_w, const int tex_h, const FlowRec* __restrict__ recs,
                                                     const IpmCal* __restrict__ cal, const int max_tris, const int n_maps, const int N, const int W,
                                                     const int H, const int oh, const int ow, void* __restrict__ depth, const int f16,
                                                     uint8_t* __restrict__ labels, uint8_t* __restrict__ inst, float* __restrict__ flow,
                                                     uint8_t* __restrict__ valid, const uint8_t* __restrict__ mask, const int32_t* __restrict__ cal_src,
                                                     const int32_t* __restrict__ env_cal, const int n_cal) {
  static_assert(!(FLOW && CAL), "the flow under per-env tables is refused");
  const int n_out = oh * ow;
  const int pix = blockIdx.x * 256 + threadIdx.x;
  const bool in = pix < n_out;
  const int e0 = blockIdx.y * DEPTH_ENVS, e1 = min(N, e0 + DEPTH_ENVS);
  EnvEntry<CAL> entry(lut, cal_src, env_cal, n_cal, in, in ? out_camera_pixel(pix, W, H, oh, ow) : 0, W, H, e0);
  const float sxn = 2.f / (float)W, syn = 2.f / (float)H;
#pragma clang loop unroll(disable)
  for (int e = e0; e < e1; ++e) {
    const ViewPix p = entry.pixel(e, e1);
    if (mask && !mask[e]) continue;                    // (wave-uniform) the masked call: this env's rows keep their bytes
    const EnvScene s = env_scene(e, cams, maps, n_maps, objbox, stris, tribox, max_tris);
    float d = 0.f, fu = 0.f, fv = 0.f;
    uint32_t cls = DTSIM_LABEL_NONE, who = DTSIM_INSTANCE_NONE;
    bool ok = false;
    if (p.live) {
      float ds[4];
      Hit hs[4];
      int os[4];
      scene_samples4<true>(s, tiles, p, sxn, syn, ds, hs, os);
      Winner w = first_sample(ds[0], os[0], hs[0]);
#pragma unroll
      for (int q = 1; q < 4; ++q) take_nearer(w, ds[q], os[q], q, hs[q]);
      // THE ONE WRITTEN-OUT SITE of the unit: to the end of the block the winner is read through copies of its members, and instance_id,
      // winner_eye_point, flow_xf, flow_apply and flow_valid are written out.  The copy guards no behaviour: with them called, or w read in place,
      // k_camera_maps<true, *, *> only encode two compares e32 instead of e64, which tools/isa_compare.py counts as other opcodes
      // (profiles/render_views_isa.txt); it can go when tool or compiler stop telling them apart.  Until then a rule's change is made here too.
      const float db = w.d, oxq = w.ox, oyq = w.oy; const int ob = w.o; const Hit& hb = w.h;
      d = db;
      who = ob >= 0 ? (uint32_t)ob + 1u : (uint32_t)DTSIM_INSTANCE_NONE;
      if (labels) cls = sample_class(ob, hb, s, tiles, objs, texel_class, mesh_class, n_mesh_class, tex_w, tex_h);   // (wave-uniform)
      if constexpr (FLOW) {
        const FlowRec& rec = recs[e];
        const float Wf = (float)W, Hf = (float)H;
        if (db < __builtin_inff() && rec.valid) {     // not sky, and a mark of this episode
          const float xe = fmaf(oxq, sxn, p.nx) * s.c.tx, ye = fmaf(-oyq, syn, p.ny) * s.c.ty;
          const float X = db * xe, Y = db * ye, Z = -db;
          const FlowXf* xf = &rec.fix;
          if (ob >= 0) {
            const int slot = objs[s.rm->obj_off + ob].dyn_slot;
            if (slot >= 0) xf = &rec.dyn[min(slot, DTSIM_MAX_DYNAMIC - 1)];
          }
          const float xp = fmaf(xf->M[0], X, fmaf(xf->M[1], Y, fmaf(xf->M[2], Z, xf->t[0])));
          const float yp = fmaf(xf->M[3], X, fmaf(xf->M[4], Y, fmaf(xf->M[5], Z, xf->t[1])));
          const float zp = fmaf(xf->M[6], X, fmaf(xf->M[7], Y, fmaf(xf->M[8], Z, xf->t[2])));
          const FlowPt a = flow_image(X, Y, Z, rec.txc, rec.tyc, Wf, Hf, cal);
          const FlowPt b = flow_image(xp, yp, zp, rec.txp, rec.typ, Wf, Hf, cal);
          ok = b.w >= NEAR_Z && b.u >= 0.f && b.u < Wf && b.v >= 0.f && b.v < Hf;
          if (ok) { fu = (float)(b.ax - a.ax); fv = (float)(b.ay - a.ay); }              // R: 1 (the one rounding of the difference)
        }
      }
    }
    if (in) {
      const size_t to = map_at(e, n_out, pix);
      if (depth) store_depth(depth, f16, to, d);
      if (labels) labels[to] = (uint8_t)cls;
      if (inst) inst[to] = (uint8_t)who;
      if constexpr (FLOW) {
        flow[flow_at(e, n_out, pix, 0)] = fu;
        flow[flow_at(e, n_out, pix, 1)] = fv;
        if (valid) valid[to] = ok ? 1 : 0;
      }
    }
  }
}

// ---- k_bev: the egocentric bird's-eye label map of every env (dtsim_bev; the quantity: include/dtsim.h) ------------------------------------
// The grid of k_depth / k_labels: cell blocks x env chunks of DEPTH_ENVS.  A thread owns ONE cell; its place in the agent's frame -- f cells
// ahead, s cells to the right, both multiples of one half and exact in float32 -- does not depend on the env and is computed once.  The env
// loop is ONE copy of its body (tests/test_gpu_bev.py holds envs e, e + 64 and e + 128 to the same bytes), and a wavefront's 64 byte stores
// are one contiguous segment of one env's map.
// Per (workgroup, env), once, by the first wavefront.  Before the loop its lane l takes env e0 + l of the chunk: the pose in double, sincos of
// the double angle in double (cur_angle is unbounded: a float32 of it would lose the direction), kept in LDS in double for the objects and
// rounded to float32 for the cells, beside what a cell needs of the env's map (the map id clamped as k_depth clamps it) -- one chain of load
// latencies and one sincos for the chunk, not one per env (measured: profiles/bev_timing.txt).  The tile records of all maps (at most
// DTSIM_LDS_TILES of 32 bytes) are staged in dynamic LDS as well: a cell's iteration is a chain of dependent reads -- its env, its tile's
// record, its texel's class -- and with 64 envs in series per thread the pass is bound by that chain's latency, not by its stores.
// In the loop, for an env whose map has objects, lane o brings object o into the agent's frame -- a BevRect: the centre of its collision
// rectangle and the two half-axes u, v in cell units, kept as the dual pair (A, B) with P - centre = a u + b v, a = (P - centre) . A,
// b = (P - centre) . B, so that the cell's test is |a| <= 1 and |b| <= 1 -- from the packed corners of a static object (ocorners) or the env's
// current SimArrays::ob_corners of a dynamic one.  Hidden objects, objects without a mesh and objects whose bounding circle misses the window
// are dropped and the rest compacted in lane order (ballot + prefix count): the list in LDS is in ascending object index, its length is
// wave-uniform, and most envs loop over none.  The list is double-buffered in LDS, so one barrier per such env suffices: the first
// wavefront fills slot (it + 1) & 1 while the others may still read slot it & 1, which is not written again before the next barrier.  An
// env on a map without objects (workgroup-uniform) meets no barrier and no work of the first wavefront at all.
// Per cell: the first rectangle of the list that holds the cell gives the class and the id; else the tile under P = (x, z) + f d + s r
// (float32 from the rounded pose: five roundings, < 1e-5 m below 32 m), found by floorf(w * its) and sampled at the tile fraction
// w * its - tile by tile_texel_class, as sample_class samples it, so a camera label pixel and a cell that hit one world point name one class.
// No camera record, no distortion table, nothing a render pass leaves behind is read.
struct alignas(16) BevRect { float cf, cs, af, as, bf, bs; uint32_t cls, id; };
struct alignas(16) BevEnv {                                        // what a cell needs of its env, in LDS:
  float x, z, dc, ds;                                              // the pose; cell * cos, cell * sin of the angle
  float its; int tile_off, gw, gh;                                 // its map: 1 / tile size, first tile record, grid size
  int n_obj, obj_off, pad[2];                                      // ... object count, first object instance
};
struct alignas(16) BevPose { double x, z, cs, sn; };               // the same in double: the pose, cos and sin of the angle
static_assert(DTSIM_MAX_OBJECTS <= 64, "one lane of the first wavefront per object");
template <bool LAB, bool INST>
__global__ __launch_bounds__(256) void k_bev(const double* __restrict__ pos_x, const double* __restrict__ pos_z, const double* __restrict__ angle,
                                             const int32_t* __restrict__ map_id, const double* __restrict__ ob_corners,
                                             const uint8_t* __restrict__ ob_visible, const RenderMapDev* __restrict__ maps,
                                             const TileLds* __restrict__ tiles, const ObjInstDev* __restrict__ objs, const double* __restrict__ ocorners,
                                             const uint8_t* __restrict__ texel_class, const uint8_t* __restrict__ mesh_class, const int n_mesh_class,
                                             const int tex_w, const int tex_h, const int n_maps, const int n_tile_recs, const int N, const int oh,
                                             const int ow, const double cell, const int rows_behind, uint8_t* __restrict__ out, uint8_t* __restrict__ inst,
                                             const uint8_t* __restrict__ mask) {
  __shared__ BevRect s_rect[2][DTSIM_MAX_OBJECTS];
  __shared__ int s_n[2];
  __shared__ BevEnv s_env[DEPTH_ENVS];
  __shared__ BevPose s_pose[DEPTH_ENVS];
  extern __shared__ __align__(16) unsigned char s_bev_dyn[];          // [n_tile_recs] TileLds: the tile records of all maps
  TileLds* s_tiles = reinterpret_cast<TileLds*>(s_bev_dyn);
  const int n_out = oh * ow;
  const int tid = threadIdx.x;
  const int pix = blockIdx.x * 256 + tid;
  const bool in = pix < n_out;
  const int i = in ? pix / ow : 0, j = in ? pix - i * ow : 0;
  const float f = (float)(oh - rows_behind - i) - 0.5f;               // cells ahead of the agent (row 0 is the farthest)
  const float sd = ((float)j + 0.5f) - 0.5f * (float)ow;              // cells to its right (column 0 is the leftmost)
  // the window in cell units, for the cull
  const double f_lo = -(double)rows_behind, f_hi = (double)(oh - rows_behind), s_hi = 0.5 * (double)ow;
  const double inv_cell = 1.0 / cell;
  const int e0 = blockIdx.y * DEPTH_ENVS, e1 = min(N, e0 + DEPTH_ENVS);
  static_assert(DEPTH_ENVS <= 64, "one lane of the first wavefront per env of the chunk");
  for (int t = tid; t < n_tile_recs; t += 256) s_tiles[t] = tiles[t];
  if (tid < DEPTH_ENVS && e0 + tid < e1) {
    BevPose p;
    p.x = pos_x[e0 + tid]; p.z = pos_z[e0 + tid];
    sincos(angle[e0 + tid], &p.sn, &p.cs);
    s_pose[tid] = p;
    const RenderMapDev rm = maps[min((unsigned)map_id[e0 + tid], (unsigned)(n_maps - 1))];   // (the clamp: as k_depth's)
    BevEnv ev{};
    ev.x = (float)p.x; ev.z = (float)p.z; ev.dc = (float)(cell * p.cs); ev.ds = (float)(cell * p.sn);
    ev.its = rm.inv_tile_size; ev.tile_off = rm.tile_off; ev.gw = rm.grid_w; ev.gh = rm.grid_h;
    ev.n_obj = min(rm.n_obj, DTSIM_MAX_OBJECTS); ev.obj_off = rm.obj_off;
    s_env[tid] = ev;
  }
  __syncthreads();
  int it = 0;
#pragma clang loop unroll(disable)
  for (int e = e0; e < e1; ++e) {
    if (mask && !mask[e]) continue;                    // (workgroup-uniform) the masked call: this env's row keeps its bytes
    const BevEnv ev = s_env[e - e0];
    const int n_obj = __builtin_amdgcn_readfirstlane(ev.n_obj), obj_off = __builtin_amdgcn_readfirstlane(ev.obj_off);
    const int b = it & 1;
    int n_rect = 0;
    if (n_obj > 0) {                                   // (workgroup-uniform)
      ++it;
      if (tid < 64) {
        const BevPose p = s_pose[e - e0];
        const double x = p.x, z = p.z, sn = p.sn, cs = p.cs;
        bool keep = false;
        BevRect r{};
        if (tid < n_obj) {
          const ObjInstDev oi = objs[obj_off + tid];
          if (oi.mesh_id >= 0 && ob_visible[(size_t)tid * N + e]) {
            double c[8];
            if (oi.dyn_slot >= 0) {
              const int d = min(oi.dyn_slot, DTSIM_MAX_DYNAMIC - 1);
#pragma unroll
              for (int k = 0; k < 8; ++k) c[k] = ob_corners[(size_t)(k * DTSIM_MAX_DYNAMIC + d) * N + e];
            } else {
#pragma unroll
              for (int k = 0; k < 8; ++k) c[k] = ocorners[(size_t)(obj_off + tid) * 8 + k];
            }
            // corners 0, 1, 3 in the agent's frame, cell units: ahead = (c - pos) . d, right = (c - pos) . r, d = (cos, -sin), r = (sin, cos)
            double pf[3], ps[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
              const int q = k == 2 ? 3 : k;
              const double dx = c[2 * q] - x, dz = c[2 * q + 1] - z;
              pf[k] = (dx * cs - dz * sn) * inv_cell; ps[k] = (dx * sn + dz * cs) * inv_cell;
            }
            const double uf = 0.5 * (pf[1] - pf[0]), us = 0.5 * (ps[1] - ps[0]), vf = 0.5 * (pf[2] - pf[0]), vs = 0.5 * (ps[2] - ps[0]);
            const double cf = pf[0] + uf + vf, cs_ = ps[0] + us + vs;
            const double det = uf * vs - us * vf;
            const double rad = sqrt(fmax((uf + vf) * (uf + vf) + (us + vs) * (us + vs), (uf - vf) * (uf - vf) + (us - vs) * (us - vs))) + 1.0;
            const double df = fmax(fmax(f_lo - cf, cf - f_hi), 0.0), dsd = fmax(fabs(cs_) - s_hi, 0.0);
            keep = det != 0.0 && df * df + dsd * dsd <= rad * rad;          // (a NaN anywhere: dropped)
            r.cf = (float)cf; r.cs = (float)cs_;
            r.af = (float)(vs / det); r.as = (float)(-vf / det); r.bf = (float)(-us / det); r.bs = (float)(uf / det);
            r.cls = LAB ? (uint32_t)mesh_class[min((unsigned)oi.mesh_id, (unsigned)(n_mesh_class - 1))] : 0u;
            r.id = (uint32_t)tid + 1u;
          }
        }
        const unsigned long long kept = __ballot(keep);
        if (keep) s_rect[b][__popcll(kept & ((1ull << tid) - 1ull))] = r;
        if (tid == 0) s_n[b] = __popcll(kept);
      }
      __syncthreads();
      n_rect = __builtin_amdgcn_readfirstlane(s_n[b]);
    }
    uint32_t cls = DTSIM_LABEL_GROUND, who = DTSIM_INSTANCE_NONE;
    bool hit = false;
    for (int k = 0; k < n_rect; ++k) {                 // (wave-uniform count; LDS broadcast reads)
      const BevRect r = s_rect[b][k];
      const float pf = f - r.cf, ps = sd - r.cs;
      const float a = fmaf(ps, r.as, pf * r.af), bb = fmaf(ps, r.bs, pf * r.bf);
      if (fabsf(a) <= 1.f && fabsf(bb) <= 1.f) { cls = r.cls; who = r.id; hit = true; break; }
    }
    if constexpr (LAB) {
      if (!hit) {
        const float wx = fmaf(sd, ev.ds, fmaf(f, ev.dc, ev.x));
        const float wz = fmaf(sd, ev.dc, fmaf(-f, ev.ds, ev.z));
        const float its = ev.its;
        const float fi = floorf(wx * its), fj = floorf(wz * its);
        if (fi >= 0.f && fj >= 0.f && fi < (float)ev.gw && fj < (float)ev.gh) {
          const int ti = (int)fi, tj = (int)fj;
          const TileLds tr = s_tiles[ev.tile_off + tj * ev.gw + ti];
          // present and textured (else: the ground's class); the tile fraction, as sample_class takes it
          if ((tr.flags & 3u) == 3u) cls = tile_texel_class(tr, wx * its - (float)ti, wz * its - (float)tj, tex_w, tex_h, texel_class);
        }
      }
    }
    if (in) {
      const size_t to = (size_t)e * (size_t)n_out + (size_t)pix;
      if constexpr (LAB) out[to] = (uint8_t)cls;
      if constexpr (INST) inst[to] = (uint8_t)who;
    }
  }
}

// ---- k_ipm_*: the ground-projected camera image of dtsim_ipm (the quantity: include/dtsim.h; its statement: ipm_project.h), on k_bev's grid:
// cell blocks x env chunks of DEPTH_ENVS.
//
// A thread owns IPM_CPT = 4 ADJACENT cells of the map (cells, not rows: the map is one run of oh * ow cells per env), so that what it
// stores per env is whole dwords wherever the layout allows: 12 bytes of an HWC image, one dword of each CHW plane, one dword of `valid`,
// 16 bytes of `src`.  VEC says that it does allow -- oh * ow is a multiple of 4 and every base pointer is aligned (dt_ipm_vec) --, else
// the same cells are stored byte by byte, each behind its own bound.  The env loop is ONE copy of its body.
//   k_ipm_table  : the shared camera with at most one calibration is rigid in the agent's frame, so cell -> source pixel is the same for
//                  every env and every step: computed once, in float64, into the handle's table (dtsim_api.hip caches it on its key).
//   k_ipm_gather : the hot path of that case.  The thread's four table entries stay in registers across the chunk's env loop; per env
//                  it loads 12 scattered frame bytes and stores them coalesced.  No arithmetic but the addresses.
//   k_ipm_env    : per-env cameras (DTSIM_F_DOMAIN_RAND) or several calibrations.  Before the loop lane l of the first wavefront puts the
//                  camera of env e0 + l, built in float64 from the state, and its calibration's index into LDS, as k_bev does with BevPose;
//                  in the loop every cell does the float64 projection and the polynomial itself (near cells move about 4 000 px per
//                  metre: float32 world coordinates would cost 1e-3 px).
// An invalid cell reads pixel 0 of the frame (always there) and selects zero: no divergent load.
#define IPM_CPT 4
struct alignas(4) IpmRgb4 { uint32_t a, b, c; };                    // four HWC pixels

static inline bool dt_ipm_vec(const IpmArgs& a) {
  return (a.oh * a.ow) % IPM_CPT == 0 && ((uintptr_t)a.img & 3) == 0 && ((uintptr_t)a.valid & 3) == 0 && ((uintptr_t)a.src & 15) == 0;
}

// the outputs of env `env` for the thread's cells [cell0, cell0 + IPM_CPT) of n_out, whose source pixels are src[] (-1: invalid), from its frame
template <bool CHW, bool VEC>
__device__ __forceinline__ void ipm_store(const uint8_t* __restrict__ frame, const int32_t (&src)[IPM_CPT], const int cell0, const int n_out,
                                          const size_t env, uint8_t* __restrict__ img, uint8_t* __restrict__ valid, int32_t* __restrict__ srco) {
  if (cell0 >= n_out) return;
  const size_t at = env * (size_t)n_out + (size_t)cell0;
  if (img) {
    uint32_t ch[3] = {0u, 0u, 0u};                                   // byte k of ch[c]: channel c of cell k
#pragma unroll
    for (int k = 0; k < IPM_CPT; ++k) {
      const uint8_t* p = frame + (size_t)max(src[k], 0) * 3;
      const uint32_t r = p[0], g = p[1], b = p[2];
      const bool ok = src[k] >= 0;
      ch[0] |= (ok ? r : 0u) << (8 * k); ch[1] |= (ok ? g : 0u) << (8 * k); ch[2] |= (ok ? b : 0u) << (8 * k);
    }
    if constexpr (CHW) {
      uint8_t* o = img + env * 3 * (size_t)n_out + (size_t)cell0;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if constexpr (VEC) *reinterpret_cast<uint32_t*>(o + (size_t)c * n_out) = ch[c];
        else {
#pragma unroll
          for (int k = 0; k < IPM_CPT; ++k) if (cell0 + k < n_out) o[(size_t)c * n_out + k] = (uint8_t)(ch[c] >> (8 * k));
        }
      }
    } else {
      uint8_t* o = img + at * 3;
      if constexpr (VEC) {
        uint32_t px[IPM_CPT];
#pragma unroll
        for (int k = 0; k < IPM_CPT; ++k)
          px[k] = ((ch[0] >> (8 * k)) & 255u) | (((ch[1] >> (8 * k)) & 255u) << 8) | (((ch[2] >> (8 * k)) & 255u) << 16);
        IpmRgb4 v;                                                   // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
        v.a = px[0] | (px[1] << 24); v.b = (px[1] >> 8) | (px[2] << 16); v.c = (px[2] >> 16) | (px[3] << 8);
        *reinterpret_cast<IpmRgb4*>(o) = v;
      } else {
#pragma unroll
        for (int k = 0; k < IPM_CPT; ++k)
          if (cell0 + k < n_out) {
#pragma unroll
            for (int c = 0; c < 3; ++c) o[3 * k + c] = (uint8_t)(ch[c] >> (8 * k));
          }
      }
    }
  }
  if (valid) {
    if constexpr (VEC) {
      uint32_t v = 0u;
#pragma unroll
      for (int k = 0; k < IPM_CPT; ++k) v |= (src[k] >= 0 ? 1u : 0u) << (8 * k);
      *reinterpret_cast<uint32_t*>(valid + at) = v;
    } else {
#pragma unroll
      for (int k = 0; k < IPM_CPT; ++k) if (cell0 + k < n_out) valid[at + k] = src[k] >= 0 ? 1 : 0;
    }
  }
  if (srco) {
    if constexpr (VEC) *reinterpret_cast<int4*>(srco + at) = make_int4(src[0], src[1], src[2], src[3]);
    else {
#pragma unroll
      for (int k = 0; k < IPM_CPT; ++k) if (cell0 + k < n_out) srco[at + k] = src[k];
    }
  }
}

__global__ __launch_bounds__(256) void k_ipm_table(const IpmCam cam, const IpmCal* __restrict__ cal, const int W, const int H, const int oh,
                                                   const int ow, const double cell, const int rows_behind, int32_t* __restrict__ table) {
  const int at = blockIdx.x * 256 + threadIdx.x;
  if (at >= oh * ow) return;
  const int i = at / ow, j = at - i * ow;
  double f, s;
  dt_ipm_cell(i, j, oh, ow, cell, rows_behind, f, s);
  table[at] = dt_ipm_source(cam, cal, W, H, f, s);
}

template <bool CHW, bool VEC>
__global__ __launch_bounds__(256) void k_ipm_gather(const uint8_t* __restrict__ frames, const int32_t* __restrict__ table, const int N,
                                                    const int n_out, const size_t frame_bytes, uint8_t* __restrict__ img,
                                                    uint8_t* __restrict__ valid, int32_t* __restrict__ srco, const uint8_t* __restrict__ mask) {
  const int cell0 = (blockIdx.x * 256 + threadIdx.x) * IPM_CPT;
  int32_t src[IPM_CPT];
  if constexpr (VEC) {
    const int4 t = cell0 < n_out ? *reinterpret_cast<const int4*>(table + cell0) : make_int4(-1, -1, -1, -1);
    src[0] = t.x; src[1] = t.y; src[2] = t.z; src[3] = t.w;
  } else {
#pragma unroll
    for (int k = 0; k < IPM_CPT; ++k) src[k] = cell0 + k < n_out ? table[cell0 + k] : -1;
  }
  const int e0 = blockIdx.y * DEPTH_ENVS, e1 = min(N, e0 + DEPTH_ENVS);
#pragma clang loop unroll(disable)
  for (int e = e0; e < e1; ++e) {
    if (mask && !mask[e]) continue;                    // (workgroup-uniform) the masked call: this env's rows keep their bytes
    ipm_store<CHW, VEC>(frames + (size_t)e * frame_bytes, src, cell0, n_out, (size_t)e, img, valid, srco);
  }
}

// per_env: DTSIM_F_DOMAIN_RAND -- the cameras of SimArrays::cam; else `shared`, default_cam()'s.  cals: [n_cal] (n_cal = 0: rectilinear),
// env_cal: [N] or null = calibration 0 for every env.
template <bool CHW, bool VEC>
__global__ __launch_bounds__(256) void k_ipm_env(const uint8_t* __restrict__ frames, const double* __restrict__ angle, const float* __restrict__ camp,
                                                 const int per_env, const IpmCam shared, const IpmCal* __restrict__ cals, const int n_cal,
                                                 const int32_t* __restrict__ env_cal, const int N, const int W, const int H, const int oh, const int ow,
                                                 const double cell, const int rows_behind, uint8_t* __restrict__ img, uint8_t* __restrict__ valid,
                                                 int32_t* __restrict__ srco, const uint8_t* __restrict__ mask) {
  __shared__ IpmCam s_cam[DEPTH_ENVS];
  __shared__ int s_cal[DEPTH_ENVS];
  const int n_out = oh * ow;
  const int tid = threadIdx.x;
  const int cell0 = (blockIdx.x * 256 + tid) * IPM_CPT;
  double f[IPM_CPT], sd[IPM_CPT];
#pragma unroll
  for (int k = 0; k < IPM_CPT; ++k) {
    const int at = min(cell0 + k, n_out - 1);
    const int i = at / ow, j = at - i * ow;
    dt_ipm_cell(i, j, oh, ow, cell, rows_behind, f[k], sd[k]);
  }
  const int e0 = blockIdx.y * DEPTH_ENVS, e1 = min(N, e0 + DEPTH_ENVS);
  static_assert(DEPTH_ENVS <= 64, "one lane of the first wavefront per env of the chunk");
  if (tid < DEPTH_ENVS && e0 + tid < e1) {
    const int e = e0 + tid;
    IpmCam c = shared;
    if (per_env) {
      double sa, ca;
      sincos(angle[e], &sa, &ca);                      // of the float64 angle (cur_angle is unbounded)
      const size_t n = (size_t)N;
      const double noise[3] = {(double)camp[3 * n + e], (double)camp[4 * n + e], (double)camp[5 * n + e]};
      c = dt_ipm_camera((double)camp[0 * n + e], (double)camp[1 * n + e], (double)camp[2 * n + e], noise, sa, ca, W, H);
    }
    s_cam[tid] = c;
    s_cal[tid] = n_cal > 0 ? (env_cal ? (int)min((unsigned)env_cal[e], (unsigned)(n_cal - 1)) : 0) : -1;
  }
  __syncthreads();
#pragma clang loop unroll(disable)
  for (int e = e0; e < e1; ++e) {
    if (mask && !mask[e]) continue;                    // (workgroup-uniform)
    const IpmCam c = s_cam[e - e0];
    const int ci = __builtin_amdgcn_readfirstlane(s_cal[e - e0]);
    const IpmCal* cal = ci >= 0 ? cals + ci : nullptr;
    int32_t src[IPM_CPT];
#pragma unroll
    for (int k = 0; k < IPM_CPT; ++k) src[k] = cell0 + k < n_out ? dt_ipm_source(c, cal, W, H, f[k], sd[k]) : -1;
    ipm_store<CHW, VEC>(frames + (size_t)e * ((size_t)W * H * 3), src, cell0, n_out, (size_t)e, img, valid, srco);
  }
}

static inline dim3 dt_ipm_grid(const IpmArgs& a) { return view_grid((a.oh * a.ow + IPM_CPT - 1) / IPM_CPT, a.N); }   // a thread per IPM_CPT cells

// What every camera-map launch hands its kernel of the pass, decided here once: the rows of the projected mesh triangles (objbox / stris: null
// unless the pass projected some; tribox: its box stream, which it leaves whenever it leaves the records) and the per-env tables (null / 0
// unless all three are given -- the CAL instantiations).
struct ViewScene { const float4* lut; const ObjBox* objbox; const ScreenTri* stris; const float4* tribox; const int32_t* cal_src; const int32_t* env_cal; int n_cal; };
static inline ViewScene view_scene(const RenderParams& R, const int32_t* cal_src = nullptr, const int32_t* env_cal = nullptr, const int n_cal = 0) {
  const bool obj = R.stris && R.objbox && R.tribox, cal = cal_src && env_cal && n_cal > 0;
  return {reinterpret_cast<const float4*>(R.lut), obj ? R.objbox : nullptr, obj ? R.stris : nullptr, obj ? R.tribox : nullptr,
          cal ? cal_src : nullptr, cal ? env_cal : nullptr, cal ? n_cal : 0};
}

}  // namespace

void dt_launch_overlay_leds(hipStream_t s, const RenderParams& R, const float* d_spheres, int first, int count, int env) {
  if (count <= 0) return;
  hipLaunchKernelGGL(k_overlay_leds, dim3((unsigned)((R.W * R.H + 255) / 256)), dim3(256), 0, s, R, R.envcam, d_spheres, first, count, env);
}

void dt_launch_depth(hipStream_t s, const RenderParams& R, void* out, int oh, int ow, bool f16, const uint8_t* mask, const int32_t* cal_src,
                     const int32_t* env_cal, int n_cal) {
  if (R.N <= 0) return;
  const ViewScene v = view_scene(R, cal_src, env_cal, n_cal);
  auto k = v.cal_src ? (f16 ? k_depth<true, true> : k_depth<false, true>) : (f16 ? k_depth<true> : k_depth<false>);
  hipLaunchKernelGGL(k, view_grid(oh * ow, R.N), dim3(256), 0, s, R.envcam, R.maps, R.tile_recs, v.lut, v.objbox, v.stris, v.tribox, R.max_tris, R.n_maps,
                     R.N, R.W, R.H, oh, ow, out, mask, v.cal_src, v.env_cal, v.n_cal);
}

void dt_launch_labels(hipStream_t s, const RenderParams& R, const uint8_t* texel_class, const uint8_t* mesh_class, int n_mesh_class, uint8_t* out,
                      uint8_t* inst, int oh, int ow, const uint8_t* mask, const int32_t* cal_src, const int32_t* env_cal, int n_cal) {
  if (R.N <= 0 || (!out && !inst)) return;
  const ViewScene v = view_scene(R, cal_src, env_cal, n_cal);
  auto k = v.cal_src ? (out && inst ? k_labels<true, true, true> : out ? k_labels<true, false, true> : k_labels<false, true, true>)
                     : (out && inst ? k_labels<true, true> : out ? k_labels<true, false> : k_labels<false, true>);
  hipLaunchKernelGGL(k, view_grid(oh * ow, R.N), dim3(256), 0, s, R.envcam, R.maps, R.tile_recs, v.lut, v.objbox, v.stris, v.tribox, R.objs, texel_class,
                     mesh_class, n_mesh_class, R.tex_w, R.tex_h, R.max_tris, R.n_maps, R.N, R.W, R.H, oh, ow, out, inst, mask, v.cal_src, v.env_cal,
                     v.n_cal);
}

void dt_launch_flow_mark(hipStream_t s, const SimArrays& A, FlowMark* marks, const uint8_t* mask) {
  if (A.N <= 0) return;
  hipLaunchKernelGGL(k_flow_mark, dim3((unsigned)((A.N + 63) / 64)), dim3(64), 0, s, A, marks, mask);
}

void dt_launch_flow(hipStream_t s, const RenderParams& R, const SimArrays& A, const FlowMark* marks, FlowRec* recs, bool per_env, const IpmCal* cal,
                    float* flow, uint8_t* valid, int oh, int ow, const uint8_t* mask) {
  if (R.N <= 0) return;
  dt_launch_flow_setup(s, R, A, marks, recs, per_env, mask);
  const ViewScene v = view_scene(R);
  hipLaunchKernelGGL(k_flow, view_grid(oh * ow, R.N), dim3(256), 0, s, R.envcam, R.maps, R.tile_recs, v.lut, v.objbox, v.stris, v.tribox, R.objs, recs, cal,
                     R.max_tris, R.n_maps, R.N, R.W, R.H, oh, ow, flow, valid, mask);
}

void dt_launch_flow_setup(hipStream_t s, const RenderParams& R, const SimArrays& A, const FlowMark* marks, FlowRec* recs, bool per_env,
                          const uint8_t* mask) {
  if (R.N <= 0) return;
  hipLaunchKernelGGL(k_flow_setup, dim3((unsigned)((R.N + 63) / 64)), dim3(64), 0, s, A, marks, recs, per_env ? 1 : 0, R.W, R.H, mask);
}

void dt_launch_camera_maps(hipStream_t s, const RenderParams& R, const CameraMapsOut& o, const uint8_t* texel_class, const uint8_t* mesh_class,
                           int n_mesh_class, const FlowRec* recs, const IpmCal* cal, int oh, int ow, const uint8_t* mask, const int32_t* cal_src,
                           const int32_t* env_cal, int n_cal) {
  if (R.N <= 0 || (!o.depth && !o.labels && !o.inst && !o.flow)) return;
  const ViewScene v = view_scene(R, o.flow ? nullptr : cal_src, env_cal, n_cal);   // (no tables with flow: the caller refused that)
  auto k = o.flow ? k_camera_maps<true, false> : v.cal_src ? k_camera_maps<false, true> : k_camera_maps<false, false>;
  hipLaunchKernelGGL(k, view_grid(oh * ow, R.N), dim3(256), 0, s, R.envcam, R.maps, R.tile_recs, v.lut, v.objbox, v.stris, v.tribox, R.objs, texel_class,
                     mesh_class, n_mesh_class, R.tex_w, R.tex_h, o.flow ? recs : nullptr, o.flow ? cal : nullptr, R.max_tris, R.n_maps, R.N, R.W, R.H, oh,
                     ow, o.depth, o.f16 ? 1 : 0, o.labels, o.inst, o.flow, o.flow ? o.valid : nullptr, mask, v.cal_src, v.env_cal, v.n_cal);
}

void dt_launch_bev(hipStream_t s, const RenderParams& R, const SimArrays& A, const double* ocorners, const uint8_t* texel_class,
                   const uint8_t* mesh_class, int n_mesh_class, uint8_t* cls, uint8_t* inst, int oh, int ow, double cell, int rows_behind,
                   const uint8_t* mask) {
  if (R.N <= 0 || (!cls && !inst)) return;
  const dim3 grid = view_grid(oh * ow, R.N);
  auto k = cls && inst ? k_bev<true, true> : cls ? k_bev<true, false> : k_bev<false, true>;
  static_assert(DTSIM_LDS_TILES * sizeof(TileLds) <= 32768, "the tile records of all maps fit the workgroup's LDS beside its 10 KB of lists");
  const int n_recs = min(R.n_tile_recs, DTSIM_LDS_TILES);   // (dt_pack_maps refuses more)
  hipLaunchKernelGGL(k, grid, dim3(256), (size_t)n_recs * sizeof(TileLds), s, A.pos_x, A.pos_z, A.angle, A.map_id, A.ob_corners, A.ob_visible, R.maps,
                     R.tile_recs, R.objs, ocorners, texel_class, mesh_class, n_mesh_class, R.tex_w, R.tex_h, R.n_maps, n_recs, R.N, oh, ow, cell, rows_behind,
                     cls, inst, mask);
}

void dt_launch_ipm_table(hipStream_t s, int32_t* table, const IpmCal* cal, int W, int H, int oh, int ow, double cell, int rows_behind) {
  hipLaunchKernelGGL(k_ipm_table, dim3((unsigned)((oh * ow + 255) / 256)), dim3(256), 0, s, dt_ipm_shared_camera(W, H), cal, W, H, oh, ow, cell,
                     rows_behind, table);
}

void dt_launch_ipm_gather(hipStream_t s, const IpmArgs& a, const int32_t* table) {
  if (a.N <= 0) return;
  const bool vec = dt_ipm_vec(a);
  auto k = a.chw ? (vec ? k_ipm_gather<true, true> : k_ipm_gather<true, false>) : (vec ? k_ipm_gather<false, true> : k_ipm_gather<false, false>);
  hipLaunchKernelGGL(k, dt_ipm_grid(a), dim3(256), 0, s, a.frames, table, a.N, a.oh * a.ow, (size_t)a.W * a.H * 3, a.img, a.valid, a.src, a.mask);
}

void dt_launch_ipm_env(hipStream_t s, const IpmArgs& a, const SimArrays& A, bool per_env, const IpmCal* cals, int n_cal, const int32_t* env_cal) {
  if (a.N <= 0) return;
  const bool vec = dt_ipm_vec(a);
  auto k = a.chw ? (vec ? k_ipm_env<true, true> : k_ipm_env<true, false>) : (vec ? k_ipm_env<false, true> : k_ipm_env<false, false>);
  hipLaunchKernelGGL(k, dt_ipm_grid(a), dim3(256), 0, s, a.frames, A.angle, A.cam, per_env ? 1 : 0, dt_ipm_shared_camera(a.W, a.H), cals, n_cal, env_cal,
                     a.N, a.W, a.H, a.oh, a.ow, a.cell, a.rows_behind, a.img, a.valid, a.src, a.mask);
}

void dt_launch_overlay_lines(hipStream_t s, const RenderParams& R, const float* d_lines, int first, int count, int env) {
  if (count <= 0) return;
  hipLaunchKernelGGL(k_overlay_lines, dim3((unsigned)((R.W * R.H + 255) / 256)), dim3(256), 0, s, R, R.envcam, d_lines, first, count, env);
}
