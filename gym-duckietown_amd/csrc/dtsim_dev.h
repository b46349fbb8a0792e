// Internal device-side layout of libdtsim (not part of the C-ABI).
//
// HBM layout (DESIGN.md "Data layout"):
//   * per-env state is struct-of-arrays, one array per scalar, index = env, all carved
//     from ONE slab so a checkpoint is a single memcpy (SimArrays and the slab's layout: state_fields.h);
//     thread e of the step kernel touches element e of each array => every load/store
//     of a wavefront is one fully coalesced 512-byte (f64) transaction.
//   * per-map tables are one packed blob of 8-byte words per map, copied into LDS by
//     each workgroup of the step kernel (tiles, Bezier control points, static OBBs).
//   * frames are [N][H][W][3] uint8.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/dtsim.h"
#include "ipm_project.h"
#include "observe_plan.h"
#include "render_records.h"
#include "scene_tables.h"
#include "state_fields.h"

// ---- constants of the reference (simulator.py:99-177), evaluated exactly as
// Python evaluates them (IEEE double, same operation order) -------------------
#define DT_CAMERA_FORWARD_DIST 0.066
#define DT_ROBOT_WIDTH (0.13 + 0.02)
#define DT_ROBOT_LENGTH 0.18
#define DT_CENTER_SHIFT (DT_CAMERA_FORWARD_DIST - (DT_ROBOT_LENGTH / 2))
#define DT_SAFETY_RAD_MULT 1.8
#define DT_AGENT_SAFETY_RAD ((DT_ROBOT_LENGTH / 2) * DT_SAFETY_RAD_MULT) /* max(L,W)=L */
#define DT_REWARD_INVALID_POSE (-1000.0)

struct StepParams {
  int32_t n_steps, frame_skip, max_steps, delay_steps;
  int32_t action_mode, actions_f64, auto_reset, n_pool;
  uint32_t step_flags;                  // DTSIM_STEP_*
  int32_t light_capture, domain_rand;   // DTSIM_F_LIGHT_CAPTURE (device-side resets take the new light through the last frame's camera); DTSIM_F_DOMAIN_RAND (that camera carries its noise)
  int32_t lanes;                        // lanes of a wavefront that share one env in k_step (1, 2, 4; physics.hip Coop)
  int32_t camera_rand;                  // DTSIM_LUTS_CAMERA_RAND: device-side resets scale camera height / angle / fov_y (simulator.py:611-614)
  const dtsim_reset_sampler* sampler;   // device copy, or null: device-side reset sampling (N2)
  double delta_time, robot_speed;
  double gain, trim, radius, k, limit;
};

// launchers implemented in physics.hip
void dt_launch_step(hipStream_t s, const SimArrays& A, const MapSet& M, const StepParams& P,
                    const void* actions, const dtsim_init_state* pool);
void dt_launch_reset(hipStream_t s, const SimArrays& A, const MapSet& M, const StepParams& P,
                     const uint8_t* mask, const dtsim_init_state* states);
void dt_launch_query(hipStream_t s, const SimArrays& A, const MapSet& M, const StepParams& P, int n,
                     const int32_t* env_idx, const double* poses, double safety_factor, dtsim_probe* out);

// ---- raster -----------------------------------------------------------------
// One mesh triangle of one env after model/view/projection and per-vertex lighting
// (objects.py:123-148, objmesh.py:360-375): rectilinear pixel coordinates, 1/w, lit colour/w.
struct alignas(16) ScreenTri {
  // first 64 bytes: coverage / depth (all k_resolve's z-buffer pass reads; same layout as render_exact.hip TriCov)
  float bx0, bx1, by0, by1;  // pixel bounding box (+-1 px); empty (bx0 > bx1) when culled
  float sx[3], sy[3], iw[3];
  float inv_area;            // 0 => culled (behind the near plane / degenerate / invisible)
  int32_t index;             // position in the env's triangle order (z-buffer tie break)
  int32_t pad;
  // second 64 bytes: shading attributes, read only for the winning triangle of a sample
  float cw[3][3];            // per-vertex lit colour (0..255) divided by w
  float uw[3], vw[3];        // per-vertex texture coordinates divided by w
  int32_t tex;               // texture index of the material chunk, -1 = untextured
};
static_assert(sizeof(ScreenTri) == 128, "ScreenTri is 128 bytes");
struct ObjBox { float bx0, bx1, by0, by1; int32_t first, count, pad[2]; };          // screen box + triangle range of one object

// raster work decomposition: a workgroup owns a DT_TILE_W x DT_TILE_H pixel tile for DT_ENVS_PER_BLOCK consecutive envs (positions of the render order)
#ifndef DT_WAVE_W
#define DT_WAVE_W 128                      // pixel columns of a wavefront's block (128 x 2 pixels; 64 x 4 measured 2.5 % slower)
#endif
#ifndef DT_PPT
#define DT_PPT 4                           // pixels per lane: a wavefront's block is 64 * DT_PPT pixels
#endif
#ifndef DT_V3_WW
#define DT_V3_WW 128                       // k_raster_v3 (render_v3.hip): pixel columns of ITS wavefront block (128 / 64 / 32); the workgroup tile stays 128 x 8
#endif
#define DT_TILE_W DT_WAVE_W
#define DT_TILE_H (4 * (64 * DT_PPT / DT_WAVE_W))  // 4 wavefronts stacked vertically
#ifndef DT_ENVS_PER_BLOCK
#define DT_ENVS_PER_BLOCK 64                 // envs a raster workgroup loops over (round 6: 32 -> 64 -- the tile tables and per-pixel constants of a workgroup serve twice the envs:
                                             // C3 - 1.9 %, C5 - 2.8 %, C4 +- 0, frames unchanged; a queue entry's env field has six bits: 64 is the limit)
#endif
#ifndef DT_ITEM_B
#define DT_ITEM_B 8                          // 64-entry edge batches per k_resolve work item
#endif
#define DT_ITEMS_PER_WG (4 * (DT_PPT * DT_ENVS_PER_BLOCK) / DT_ITEM_B) // worst case: 4 regions x (64*PPT px x envs / 64) batches
static inline size_t dt_raster_tiles(int W, int H) {
  return (size_t)((W + DT_TILE_W - 1) / DT_TILE_W) * (size_t)((H + DT_TILE_H - 1) / DT_TILE_H);
}
static inline size_t dt_raster_groups(int N, int W, int H) { return dt_raster_tiles(W, H) * (((size_t)N + DT_ENVS_PER_BLOCK - 1) / DT_ENVS_PER_BLOCK); }

struct RenderParams {
  int32_t N, W, H, distortion;
  int32_t domain_rand, n_maps, n_tile_recs;
  int32_t tex_w, tex_h;           // all tile textures share one (power-of-two) size
  const TileLds* tile_recs;       // [n_tile_recs], maps concatenated (RenderMapDev.tile_off)
  uint8_t* frames;
  const float* lut;             // [H*W][4]: source-pixel NDC x, y (of the rectilinear pixel), valid flag, pad
  const uint32_t* texels;       // RGBA8 pool
  const TexDev* tex;
  const RenderMapDev* maps;
  const uint32_t* tiles;
  const ObjInstDev* objs;
  const MeshDev* meshes;
  const TriDev* tris;
  EnvCam* envcam;               // [N] EnvCam written by the setup kernel (the render scratch: dt_render_layout; the records: render_records.h)
  // mesh objects: per-env screen-space triangles written by the object setup kernel
  int32_t max_tris, segment;    // triangle slots per env (max over maps), 0 = no objects anywhere; segment: DTSIM_RENDER_SEGMENT
  ScreenTri* stris;             // [N][max_tris]
  float4* tribox;               // [N][max_tris] screen boxes (bx0, bx1, by0, by1) of the triangles: k_resolve_obj's cull stream
  ObjBox* objbox;               // [N][DTSIM_MAX_OBJECTS]
  float* blockbox;              // [raster tiles * 4][4] source-pixel bounding box of each raster wavefront block (k_blk_setup)
  unsigned long long* objmask;  // [N][raster tiles * 4] objects whose screen box meets the block (bit o), written by k_obj_setup
  uint2* objrange;              // [DTSIM_MAX_MAPS][DTSIM_MAX_OBJECTS] (first, count) of each object's triangles in its map's order (k_blk_setup)
  uint16_t* queue;              // MSAA edge-pixel queue regions, [workgroups][4][256*16]
  int32_t* qcount;              // [workgroups][4]
  uint16_t* qend;               // [workgroups][4][DT_ENVS_PER_BLOCK] queue fill of each region after each env of the chunk (mesh-object renders)
  int32_t* work;                // [DT_WORK_INTS] counts and cursors of the exact paths' work lists, k_raster_v3's ticket counters (the DT_WORK_* slots below); zeroed per render
  uint32_t* items;              // [workgroups * DT_ITEMS_PER_WG] work items: raster workgroup * DT_ITEMS_PER_WG + part
  uint32_t* items2;             // [workgroups * DT_ENVS_PER_BLOCK] work items of k_resolve_obj: raster workgroup * DT_ITEMS_PER_WG + env group
  const uint8_t* mesh_seg;      // [n_meshes][4] flat segmentation colour per mesh (segment renders only)
  // quad-layout fast path (null qtex: the generic k_raster is used)
  const uint8_t* qtex;          // quad blocks, 16 B records
  const uint32_t* qtiles;       // [n_qtiles][2] per padded-table cell: byte offset of its block, mask of the record's offset inside it (cell mask for sizes other than 256); maps concatenated
  int32_t n_qtiles, qlog2;      // qlog2: log2(S), S = tile texture size
  float q_per_m;                // quad cells per metre (S / tile_size), max over maps: scales the MSAA margin
  int32_t qmax_tiles;           // largest padded grid extent over the maps (tiles)
  int32_t* envpos;              // [N] position of each env in the render order (k_env_sort)
  RenderDump* dump;             // masked lanes of the unconditional frame store write here
  PixTab* pixtab;               // [H*W] PixTab (16 B), then [H*W] SampTab (32 B): per-pixel tables of the shared camera (k_pix_setup)
  EnvV* envv;                   // [N + 1] EnvV: k_raster_v3's per-env constants in render order
  EnvD* envd;                   // [N] EnvD (320 B, render order): k_raster_v3dr's per-env constants (domain randomisation)
  int32_t q3_rows;              // k_raster_v3 / k_raster_v3dr: rows of their LDS tile table (largest padded grid height); 0: they cannot run (dt_raster_pipe)
  int32_t light;                // DTSIM_F_LIGHT_CAPTURE with the shared camera: every env lit by its own eye-space light (k_cam_setup, the LIGHT kernels)
};
#define DT_WORK_INTS (32 + 8 * 32)   // RenderParams.work: the slots, then k_raster_v3's ticket counters
#define DT_WORK_ITEMS 0          //   work items of k_resolve / k_resolve_dr in RenderParams.items (the rasters append)
#define DT_WORK_CURSOR 1         //   their grab cursor
#define DT_WORK_OBJ_FRONT 2      //   k_resolve_obj's heavy items, from the front of RenderParams.items2
#define DT_WORK_OBJ_CURSOR 3     //   its grab cursor
#define DT_WORK_OBJ_BACK 6       //   its other items, from the back of items2
#define DT_WORK_LIVE 7           //   envs of a masked pass (k_env_sort<true>), read by the SUB rasters
#define DT_WORK_TICKETS 32       //   k_raster_v3's ticket counters (raster_map.h): XCD x's at DT_WORK_TICKETS + 32 * x, 128 bytes apart and from the slots above
// The render scratch (render.hip dt_render_layout): the allocations RenderParams points into, each a run of arrays -- ENV: per env EnvCam, EnvFast,
// EnvQ, envpos, EnvV [N + 1], EnvD, EnvL [N + 1]; PIX: PixTab, SampTab, RenderDump; QCOUNT: qcount, work; ITEMS: items, items2; STRIS: stris, tribox.
enum RenderSlab { DT_SLAB_ENV, DT_SLAB_PIX, DT_SLAB_QUEUE, DT_SLAB_QCOUNT, DT_SLAB_ITEMS, DT_SLAB_QEND, DT_SLAB_STRIS, DT_SLAB_OBJBOX, DT_SLAB_OBJMASK, DT_SLABS };
// With bytes: bytes[s] = the size of slab s for N envs, W x H frames and max_tris triangle slots per env (0: no such slab).  With R: points
// R's scratch fields (envcam .. objmask; the object arrays only with max_tris > 0) into base[DT_SLABS] (null bases: null arrays).
// Returns the typed records of the ENV and PIX slabs: the arrays the launchers of a pass reach beside RenderParams (the handle keeps them).
struct EnvRecs { EnvCam* cams; EnvFast* fasts; EnvQ* envq; EnvV* envv; EnvD* envd; EnvL* envl; PixTab* pixtab; SampTab* samptab; };
EnvRecs dt_render_layout(int N, int W, int H, int max_tris, size_t* bytes, void* const* base = nullptr, RenderParams* R = nullptr);
// The raster of a pass (DTSIM_PIPE_*) from R, the largest padded tile grid of the maps (grid_rows x grid_cols, DT_QRING ring included) and
// DTSIM_RASTER_OLD (raster_old: k_raster_q / the generic raster instead of k_raster_v3 / k_raster_v3dr); sets R.q3_rows.
int dt_raster_pipe(RenderParams& R, int grid_rows, int grid_cols, bool raster_old);
// One render pass on stream s, the one entry point of dtsim_api.hip: the setup kernels (render_setup.hip), the raster of `pipe` (render.hip,
// render_v3.hip), the exact-path kernels (render_exact.hip).  pipe: dt_raster_pipe's choice for R; x: dt_render_layout's records of R's slabs.
// tables: bit 0 = the per-pixel tables (k_pix_setup), bit 1 = block boxes / object ranges (k_blk_setup) are valid from an earlier launch (they
// depend on the camera LUT and the maps only); returns the bits that are valid after this launch, plus bit 2 when the pass ran in k_env_sort's
// render order (RenderParams.envpos holds it: DTSIM_FIELD_RENDER_POS).
// mask (device, [N] bytes, nonzero = selected): the masked pass of dtsim_render_masked -- the quad-record pipelines render the selected envs
// only (positions [0, live) of k_env_sort<true>'s order, pos = -1 for the others); the generic rasters render every env.
int dt_launch_render(hipStream_t s, const SimArrays& A, const RenderParams& R, const EnvRecs& x, int pipe, int tables, const uint8_t* mask = nullptr);
// Its three steps.  Setup (render_setup.hip): the render order (k_env_sort), R.work zeroed, the per-env records (k_cam_setup), the mesh
// objects (k_blk_setup, k_obj_setup) and the per-pixel tables (k_pix_setup) a raster of `pipe` reads; tables, mask: as above.  Returns
// tables: dt_launch_render's return value; sub: this is a masked pass in render order (the rasters' SUB instantiations over positions
// [0, live)); has_pos: the pass runs in k_env_sort's order (positions become envs through EnvQ.env).
struct RenderSetup { int tables; bool sub, has_pos; };
RenderSetup dt_launch_render_setup(hipStream_t s, const SimArrays& A, const RenderParams& R, const EnvRecs& x, int pipe, int tables, const uint8_t* mask);
// The rasters of render_v3.hip (sub: RenderSetup.sub).  k_raster_v3 (DTSIM_PIPE_V3) resolves its plane-edge pixels inside; k_raster_v3dr (DTSIM_PIPE_V3DR) is followed by k_resolve_dr.
void dt_launch_raster_v3(hipStream_t s, const RenderParams& R, const EnvRecs& x, bool sub);
void dt_launch_raster_v3dr(hipStream_t s, const RenderParams& R, const EnvRecs& x, bool sub);
// Exact path (render_exact.hip): k_resolve on the plane-edge pixels a generic raster queued, k_resolve_obj on the pixels inside mesh-object
// screen boxes (R.max_tris > 0) after any raster.
void dt_launch_render_exact(hipStream_t s, const RenderParams& R, const EnvRecs& x, int pipe, bool has_pos);
// GL_LINE overlays (draw_curve / draw_bbox; render_views.hip k_overlay_lines) as a post-pass on the resolved frame of `env`: d_lines = [..][9] world-space segments + colour
// (device memory), `count` of them from `first` on; uses the EnvCam the last render wrote.
void dt_launch_overlay_lines(hipStream_t s, const RenderParams& R, const float* d_lines, int first, int count, int env);
// the LED spheres of enable_leds (render_views.hip k_overlay_leds): [count] spheres of env `env` from d_spheres[first..], world space, R = the last render pass's parameters
void dt_launch_overlay_leds(hipStream_t s, const RenderParams& R, const float* d_spheres, int first, int count, int env);
// the depth maps of dtsim_depth (render_views.hip k_depth): out = [N][oh][ow] float32 (f16: half), output pixel (i, j) = camera pixel
// (i * (H / oh) + H / oh / 2, j * (W / ow) + W / ow / 2); R = the last render pass's parameters; mask (device, [N] bytes, or null = every
// env): the rows of the other envs are not written.  The caller checked that oh divides H and ow divides W.
// cal_src / env_cal / n_cal: the per-env distortion tables of dtsim_set_distortion_luts (device; dt_launch_remap_cal's) -- env e's pixel then
// takes the entry R.lut (the identity table of the rectilinear pass) holds at cal_src[env_cal[e]][camera pixel], none where that is -1.  Null
// pointers: the single table R.lut, the kernels without the per-env path.
void dt_launch_depth(hipStream_t s, const RenderParams& R, void* out, int oh, int ow, bool f16, const uint8_t* mask, const int32_t* cal_src,
                     const int32_t* env_cal, int n_cal);
// the label maps of dtsim_labels (render_views.hip k_labels): out = [N][oh][ow] bytes, sized, sampled and masked as dt_launch_depth's; texel_class:
// one byte per texel in the layout of R.texels (dt_pack_label_tables), mesh_class: [n_mesh_class] bytes.  inst: the instance map of
// dtsim_instances, same shape, written in the same launch from the same classification.  Either of out / inst may be null (the tables are
// read only with out); they must not overlap.  cal_src / env_cal / n_cal: as dt_launch_depth's.
void dt_launch_labels(hipStream_t s, const RenderParams& R, const uint8_t* texel_class, const uint8_t* mesh_class, int n_mesh_class, uint8_t* out,
                      uint8_t* inst, int oh, int ow, const uint8_t* mask, const int32_t* cal_src, const int32_t* env_cal, int n_cal);
// dtsim_flow_mark (render_views.hip k_flow_mark): the selected envs' current state into marks [N] (mask: device, [N] bytes, or null = every env).
void dt_launch_flow_mark(hipStream_t s, const SimArrays& A, FlowMark* marks, const uint8_t* mask);
// the flow maps of dtsim_flow (render_views.hip k_flow_setup, k_flow): flow = [N][2][oh][ow] float32, valid = [N][oh][ow] bytes or null, sized,
// sampled and masked as dt_launch_depth's.  marks / recs: the handle's [N] FlowMark and FlowRec (the records are rewritten by every call);
// per_env: the cameras of SimArrays::cam (DTSIM_F_DOMAIN_RAND), else the shared one; cal: the calibration whose forward model the fisheye
// frames go through, or null (rectilinear).
void dt_launch_flow(hipStream_t s, const RenderParams& R, const SimArrays& A, const FlowMark* marks, FlowRec* recs, bool per_env, const IpmCal* cal,
                    float* flow, uint8_t* valid, int oh, int ow, const uint8_t* mask);
// dt_launch_flow's first launch alone (k_flow_setup): the selected envs' FlowRec from their marks and the current state.
void dt_launch_flow_setup(hipStream_t s, const RenderParams& R, const SimArrays& A, const FlowMark* marks, FlowRec* recs, bool per_env,
                          const uint8_t* mask);
// the maps of dtsim_camera_maps (render_views.hip k_camera_maps), all [N][oh][ow] of ONE size, sampled and masked as dt_launch_depth's, from one
// classification of the pixel: depth (float32, or half with f16), labels and inst (bytes; the tables of dt_launch_labels are read only with
// labels), flow [N][2][oh][ow] float32 and valid (only with flow).  Any may be null, not all; they must not overlap.  recs: the FlowRec that
// dt_launch_flow_setup wrote in this stream, cal: as dt_launch_flow's (both read only with flow).  cal_src / env_cal / n_cal: as
// dt_launch_depth's, and ignored with flow (the caller refuses that combination).  Reads R.tribox where the pass left it.
struct CameraMapsOut { void* depth; bool f16; uint8_t *labels, *inst; float* flow; uint8_t* valid; };
void dt_launch_camera_maps(hipStream_t s, const RenderParams& R, const CameraMapsOut& o, const uint8_t* texel_class, const uint8_t* mesh_class,
                           int n_mesh_class, const FlowRec* recs, const IpmCal* cal, int oh, int ow, const uint8_t* mask, const int32_t* cal_src,
                           const int32_t* env_cal, int n_cal);
// the bird's-eye maps of dtsim_bev (render_views.hip k_bev): cls / inst = [N][oh][ow] bytes (either may be null, not both), cell metres per cell,
// rows_behind of the oh rows behind the agent.  Of R only the scene of render_scene is read (maps, tile_recs, n_tile_recs, objs, tex_w, tex_h, n_maps) and
// N: no camera, no table of a pass.  ocorners: dt_pack_object_corners' table; texel_class / mesh_class as dt_launch_labels' (read only with
// cls); mask: device, [N] bytes, or null = every env.  The caller checked the sizes (1 .. DTSIM_BEV_MAX_SIDE) and cell (finite, > 0).
void dt_launch_bev(hipStream_t s, const RenderParams& R, const SimArrays& A, const double* ocorners, const uint8_t* texel_class,
                   const uint8_t* mesh_class, int n_mesh_class, uint8_t* cls, uint8_t* inst, int oh, int ow, double cell, int rows_behind,
                   const uint8_t* mask);
// the ground-projected camera image of dtsim_ipm (render_views.hip k_ipm_*; the projection: ipm_project.h).  One call's arguments: img = [N][oh][ow][3]
// bytes, or [N][3][oh][ow] with chw, valid = [N][oh][ow] bytes, src = [N][oh][ow] int32 -- any may be null --, taken from `frames`
// ([N][H][W][3]); mask: device, [N] bytes, or null = every env.  The caller checked the sizes, cell and rows_behind as dtsim_bev's.
struct IpmArgs {
  const uint8_t* frames;
  int N, W, H;
  uint8_t *img, *valid;
  int32_t* src;
  int oh, ow;
  double cell;
  int rows_behind;
  bool chw;
  const uint8_t* mask;
};
// the shared camera's table [oh * ow] of source pixels (-1: invalid); cal: the one calibration (device), or null = rectilinear
void dt_launch_ipm_table(hipStream_t s, int32_t* table, const IpmCal* cal, int W, int H, int oh, int ow, double cell, int rows_behind);
// the shared camera: every env through `table`
void dt_launch_ipm_gather(hipStream_t s, const IpmArgs& a, const int32_t* table);
// per-env cameras (per_env: those of SimArrays::cam, else the shared one) and / or calibrations: cals = [n_cal] (device; 0: rectilinear),
// env_cal = [N] indices into it (device), or null = calibration 0 for every env
void dt_launch_ipm_env(hipStream_t s, const IpmArgs& a, const SimArrays& A, bool per_env, const IpmCal* cals, int n_cal, const int32_t* env_cal);
// camera_rand (remap.hip): frames[e] = scratch[e] gathered through table env_cal[e] of src ([n_cal][H*W] int32, -1 = black); only the
// envs with mask[e] != 0 when mask (device) is given.  Host builders of the tables, bit-identical to dtsim/distortion.py.
void dt_launch_remap_cal(hipStream_t s, const uint8_t* scratch, uint8_t* frames, const int32_t* src, const int32_t* env_cal,
                         const uint8_t* mask, int N, int W, int H);
void dt_build_remap_maps(int W, int H, int n_cal, const double* K, const double* D, const double* ir, float* rx, float* ry);
void dt_fill_pack_remap(int W, int H, int n_cal, float* rx, float* ry, const int32_t* order, const int64_t* order_off, int32_t* src_index);

// observation post-processing (observe.hip).  plan: dt_observe_plan / dt_observe_plan_cubic's (observe_plan.h), P: its parameters with
// the per-call fields and the table pointers set.  mask (device, [N] bytes, nonzero = selected; null = every env): dtsim_observe_masked --
// the rows of other envs are not written
void dt_launch_observe(hipStream_t s, const ObservePlan& plan, const ObserveParams& P, const uint8_t* mask = nullptr);
// row e of src -> row e of dst (row_bytes each) for every e < N with mask[e] != 0 (device pointers; dtsim_copy_rows)
void dt_launch_copy_rows(hipStream_t s, int N, void* dst, const void* src, size_t row_bytes, const uint8_t* mask);
// one box and pixel count per id and env (dtsim_boxes, k_boxes): inst = [N][oh][ow] bytes -> out = [N][DTSIM_MAX_OBJECTS][5] int32; mask:
// device, [N] bytes, or null = every env.  The caller checked that oh * ow fits an int.
void dt_launch_boxes(hipStream_t s, int N, const uint8_t* inst, int oh, int ow, int32_t* out, const uint8_t* mask);
// the observation history (dtsim_obs_push): obs ([N][3][out_h][out_w] uint8) -> the newest slot of stack ([N][depth][3 or 1][out_h][out_w], uint8 or
// float32), the older slots move one down; first / mask: device, [N] bytes, or null (no env starts anew / every env)
void dt_launch_obs_push(hipStream_t s, int N, void* stack, const uint8_t* obs, int depth, int out_h, int out_w, bool f32, bool gray,
                        const uint8_t* first, const uint8_t* mask);
// the weighted frame blend (dtsim_blend_frames): out[j] = sum of w[i] * f[i][j] over D = sum of w[i], rounded half up (uint8) or as one float
// division (f32), for the frame_bytes bytes of every env (mask: device, [N] bytes, or null = every env).  Passed to the kernel by value.
struct BlendArgs {
  const uint8_t* f[DTSIM_BLEND_MAX];   // device pointers, oldest first; entries past n are unused
  uint32_t w[DTSIM_BLEND_MAX];         // 0 .. 255 each, 1 <= D <= 256 (the launcher's caller checked)
  int n;
};
void dt_launch_blend_frames(hipStream_t s, int N, void* out, const BlendArgs& B, size_t frame_bytes, bool f32, const uint8_t* mask);
