// render_records.h -- the records one stage of the render pass writes and another reads: the per-env constants (EnvCam, EnvFast, EnvQ, EnvV,
// EnvL, EnvD: written by render_setup.hip's k_cam_setup, read by the rasters, the exact paths and render_views.hip), the per-pixel tables of the
// shared camera (PixTab, SampTab: k_pix_setup) and the dump slot of the masked frame stores.  Plain C++: it compiles on the host as
// scene_tables.h, raster_map.h and observe_plan.h do, and tests/test_render_records_host.py holds the sizes and offsets to numbers.
// The kernels read several of these as 16-byte pieces or as one scalar load: no size, alignment or offset may change without them.
#ifndef DTSIM_RENDER_RECORDS_H
#define DTSIM_RENDER_RECORDS_H
#include <stddef.h>
#include <stdint.h>

// The LDS tile table of k_raster_v3 / k_raster_v3dr / k_resolve_dr (raster_common.h v3_fill_tile_table): the records' tab3 offsets are in these terms.
#define V3_TAB_PITCH 256                              // table entries per LDS row: the tile byte of Z selects the row
#define V3_MAP_COLS 32                                // columns of one map inside a half row (padded grid width <= 32, up to 4 maps)

struct alignas(16) EnvCam {          // 32 floats = 128 B, written by k_cam_setup
  float Cx, Cy, Cz;      // camera centre (world)
  float sa, ca;          // yaw
  float sth, cth;        // pitch (cam_angle[0])
  float tx, ty;          // tan(fov_y/2)*aspect, tan(fov_y/2)
  float hor[3];          // horizon colour * 255
  float gnd[3];          // ground colour * 255
  float base[3];         // scene ambient 0.3 + light ambient
  float dif[3];          // light diffuse
  float L[4];            // light position, eye space (w=0: direction, pre-normalised)
  float gndl[4];         // max(0, N.L) at the 4 ground-quad corners (-x-z, +x-z, -x+z, +x+z)
  int32_t map_id;
  float pad[2];
};
static_assert(sizeof(EnvCam) == 128, "EnvCam is 128 bytes");

// Everything the fast path needs per env, fully precomputed by k_cam_setup so that the env loop of
// k_raster does no wave-uniform arithmetic on the vector ALU (there is no scalar float ALU on gfx950):
// one 64-byte scalar load per env.
struct alignas(16) EnvFast {
  float A, B, Cxi, Czi;        // yaw rotation straight into tile units: gx = Cxi + lr*A + lf*B, gz = Czi + lr*B - lf*A
  float kg, Cx, Cz, its;       // ground-plane scale (Cy+0.008)/Cy, camera centre, 1/tile_size
  float ts, gw_m, gh_m, pad;   // tile size, grid extent in metres
  uint32_t hor_rgb;            // packed horizon colour
  int32_t gw, gh, tile_off;    // grid size, first tile record of the env's map
};
static_assert(sizeof(EnvFast) == 64, "EnvFast is 64 bytes");

// Per-env constants of the quad-layout fast path (k_raster_q): the tile-plane hit (lr, lf) of a pixel in the yaw-local
// frame goes straight to padded quad coordinates  X = Cx + lr*A + lf*B,  Z = Cz + lr*B - lf*A  (tile units x S, +0.5
// for the GL_LINEAR half-texel shift, + DT_QRING tiles of off-grid ring).  One 64-byte scalar load per env.
struct alignas(16) EnvQ {
  float A, B, Cx, Cz;
  float Xhi, Zhi;              // clamp range [S/2, hi]: centres of the outermost ring cells
  uint32_t tab_b, pitch4;      // the map's padded tile table inside the LDS copy (byte offset), row pitch in bytes (8-byte entries)
  uint32_t hor_rgb;            // packed horizon colour
  uint32_t sky[3];             // the horizon colour as the three dwords of four consecutive pixels (RGBR GBRG BRGB)
  uint32_t reach;              // cells from the camera to the border of the padded grid: hits closer than that need no clamp
  uint32_t env;                // the env (frame index) at this position of the render order (k_env_sort)
  uint32_t tab3;               // k_raster_v3's LDS column offset of the map: byte offset of its V3_MAP_COLS entries inside a table row
  uint32_t qpm_bits;           // quad cells per metre of the env's map (float bits): the exact path's ground-quad test
};
static_assert(sizeof(EnvQ) == 64, "EnvQ is 64 bytes");
// k_raster_v3's per-env constants, in render order: the transform as PAIRS (the scalar operand of a v_pk_fma_f32 is two
// consecutive scalar registers: loaded as pairs they need no s_mov), everything its env loop reads in one 64-byte scalar
// load.  [N + 1] entries: the loop prefetches one past its chunk.
struct alignas(16) EnvV {
  float A2[2], B2[2], Cx2[2], Cz2[2];
  float Xhi, Zhi;
  uint32_t tab3, hor_rgb, reach, env, pad[2];
};
static_assert(sizeof(EnvV) == 64, "EnvV is 64 bytes");
// Per-env light of the shared camera (DTSIM_F_LIGHT_CAPTURE without DTSIM_F_DOMAIN_RAND), in render order, [N + 1] entries: the env's
// eye-space light rotated into the yaw-local frame (right, up, forward) of the shared camera, where the pixel-centre hit on the tile plane is
// (lr, -Cy, lf) and the plane normal (0, 1, 0).  lit / 256 = min(base / 256 + kd8 * rsq((Lr - lr)^2 + (Lf - lf)^2 + h2), 1 / 256)  (env_lit8):
//   position:  Lr, Lf as rotated, h2 = h^2 with h = Lu + Cy (= N.(L - P), the same for every pixel), kd8 = dif * max(h, 0) / 256 (a light
//              at or below the plane: h2 = 1, kd8 = 0 -- unlit, and no 0 * inf where a pixel lies under it);
//   direction: Lr = Lf = 0, h2 = 2^120 -- the pixel's own terms vanish beside it, so the root is 2^-60 for every pixel (a wave-uniform
//              constant) -- and kd8 = dif * max(N.L, 0) * 2^60 / 256.
struct alignas(16) EnvL { float Lr, Lf, h2, kd8; };
static_assert(sizeof(EnvL) == 16, "EnvL is 16 bytes");

// Per-env constants of k_raster_v3dr (index = POSITION in the render order -- k_env_sort -- the frame index is EnvDG.env; written by
// k_cam_setup when domain randomisation is on).  Every value is ONE dword: the packed-fp32 instructions take a scalar for both halves
// (op_sel_hi = 0), so the pairs the first version stored bought nothing and cost 15 scalar registers of a kernel that spills them.
struct EnvDG {                                         // what the geometry / record loads of an env need (prefetched one env ahead): 64 B
  float hx0, hx1, hx2, hz0, hz1, hz2, Cx, Cz;
  float na1, sth;                                                         // -a1, sth
  float Xhi, Zhi;                                                         // clamp range
  uint32_t tab3, env;                                                     // LDS column offset of the map, frame index
  uint32_t pad[2];
};
struct EnvDR {                                         // classification, light, ground quad (read while the records are in flight): 80 B
  float dy, a2, cth, cE, Kr;                                              // dy, a2, cth, cex + eys, 1.05 Cy q
  float tx, inv_lo, inv_hi, ndy;                                          // |xe| scale, one-ray range of inv, -dy
  float kc[3];                                                            // lit_c / 256 per channel (the filter's byte weights sum to 256)
  uint32_t hor_rgb;                                                       // packed horizon colour
  float kg, gx1, gz1, qpm;                                                // ground scale, grid extent in cells (x, z), cells per metre (mixed tile / ground blocks only)
  float kcc[3];                                                           // - 2^23 * kc: what the biased filter sum carries (see the filter)
};
// The same env once more, PACKED for the per-lane gathers of k_resolve_dr (the exact path is bound by the NUMBER of vector memory
// instructions it issues -- 16 cycles of the texture unit each, whatever they hit -- so what a pixel needs sits in as few 16-byte pieces
// as possible): five pieces always, one more for sky samples, four more for ground-quad samples.
struct EnvDX {
  float hx0, hx1, hx2, hz0;            // homography
  float hz1, hz2, Cx, Cz;
  float na1, sth, Xhi, Zhi;            // -a1, sth; clamp range
  uint32_t tab3, env; float kg, qpm;   // LDS column offset of the map, frame index; ground scale, cells per metre
  float Cy, kc[3];                     // camera height; lit / 256 per channel
  float positional, hor[3];            // < 0: the light is positional (per-pixel light term); horizon colour x 255
  float gnd[3], gndl0;                 // ground colour x 255; max(0, N.L) at the ground-quad corners
  float gndl1, gndl2, gndl3, pad0;
  float base[3], dif0;                 // scene + light ambient; light diffuse
  float dif1, dif2, pad1, pad2;
};
static_assert(sizeof(EnvDX) == 160, "ten 16-byte pieces");
struct alignas(64) EnvD { EnvDG g; EnvDR r; EnvDX x; char pad_[16]; };
static_assert(sizeof(EnvDG) == 64 && sizeof(EnvDR) == 80, "a 64-byte and an 80-byte piece (scalar loads: 16 + 13 (+ 4) dwords)");
static_assert(sizeof(EnvD) == 320 && offsetof(EnvD, x) % 16 == 0, "EnvD is 320 bytes; EnvDX is read as 16-byte pieces");

// ---- per-pixel tables of the shared camera (env-invariant; built by k_pix_setup) ----------------------------------
// PixTab: what k_raster_q keeps in registers per pixel.  lit: < 0 source pixel outside the image (BORDER_CONSTANT 0),
// 0 sky for all four samples, > 0 the lit factor min(base + dif * N.L, 1) of the tile plane at the pixel-centre hit.
// mi: low 16 bits = MSAA reach in quad cells (0xFFFF: never a one-ray pixel), high 16 = the reach in metres, fp16 rounded up.
struct alignas(16) PixTab { float lr, lf, lit; uint32_t mi; };
// SampTab: the four MSAA sample hits on the tile plane in the yaw-local frame (k_resolve_q), as fp16 offsets from the
// pixel-centre hit (lr, lf) of the PixTab (a sample sits within a pixel footprint of the centre: an fp16 offset
// places it to 5e-4 of that footprint; for pixels whose centre ray misses the planes the offsets are the hits
// themselves).  flags: bit s = sample s hits the tile plane within [near, far], bit 4+s = it hits the ground plane
// within [near, far] (ground hit = kg * tile-plane hit).
// lr_bits, lf_bits, lit_bits: lr, lf, lit of the PixTab once more (float bits): phase 2 of k_raster_v3's exact path reads ONE table.
struct alignas(16) SampTab { uint32_t dlr[2], dlf[2]; uint32_t flags; uint32_t lr_bits, lf_bits, lit_bits; };
static_assert(sizeof(PixTab) == 16 && sizeof(SampTab) == 32, "table records");

// ---- dtsim_flow (render_views.hip k_flow_mark, k_flow_setup, k_flow; the arithmetic: flow_transform.h) ----------------------------
// FlowMark: what dtsim_flow_mark remembers of one env's state -- the float64 pose, the six camera floats of DTSIM_FIELD_CAMERA, the
// episode and map, and per dynamic slot the centre (x, height, z) and y_rot (degrees) k_obj_setup places the mesh with.  has: 0 = no mark
// (the buffer starts zeroed and dtsim_set_maps / dtsim_set_assets zero it again).
struct FlowMark {
  double x, z, ang;
  float cam[6];
  int32_t episode, map_id, has, pad;
  double ob[8][4];                                    // [DTSIM_MAX_DYNAMIC]: cx, cy, cz, y_rot
};
static_assert(sizeof(FlowMark) == 320, "FlowMark is 320 bytes");
// FlowXf: X_prev_eye = M X_cur_eye + t, row-major, float32 (rounded from float64 after the camera centres were subtracted).
struct alignas(16) FlowXf { float M[9], t[3]; };
// FlowRec: one env's record of a dtsim_flow call, written by k_flow_setup: the pair of static surfaces, then one per dynamic slot with the
// object's motion folded in; the image-plane half-extents of the current and of the previous camera (both from the float64 formula, so equal
// cameras give equal bits); valid: the env has a mark of its current episode and map.
struct alignas(16) FlowRec {
  FlowXf fix;
  float txc, tyc, txp, typ;
  int32_t valid, pad[3];
  FlowXf dyn[8];                                      // [DTSIM_MAX_DYNAMIC]
};
static_assert(sizeof(FlowXf) == 48 && sizeof(FlowRec) == 464 && offsetof(FlowRec, dyn) == 80, "FlowRec: 48 + 32 + 8 x 48 bytes");

// RenderParams.dump: `store` takes the masked lanes of the unconditional frame store (16 B per lane)
struct RenderDump { uint8_t store[64 * 16]; };

#endif
