// dtsim_api.hip -- C-ABI entry points of libdtsim.so (include/dtsim.h).
// Host-side only: handle management, table packing/upload, stream-ordered launches.
// There is deliberately NO CPU fallback: without a HIP device dtsim_create fails with
// DTSIM_E_NOGPU.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "dtsim_dev.h"
#include <dlfcn.h>
#include <mutex>

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIPCHK(expr)                                                                       \
  do {                                                                                     \
    hipError_t _e = (expr);                                                                \
    if (_e != hipSuccess) return fail(DTSIM_E_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
  } while (0)

struct ProfSlot {
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> free_;
};

// One device allocation of the handle: freed when its owner is replaced or the handle deleted.  The caller synchronises
// h->stream first whenever the stream may still read the old buffer.
struct HipFree {
  void operator()(void* p) const { (void)hipFree(p); }
};
template <typename T>
using DevPtr = std::unique_ptr<T, HipFree>;

// n elements of T into `out`, which keeps what it had on failure
template <typename T>
hipError_t dev_alloc(DevPtr<T>& out, size_t n) {
  T* p = nullptr;
  hipError_t e = hipMalloc(&p, sizeof(T) * n);
  if (e == hipSuccess) out.reset(p);
  return e;
}

// src[0, n) in a new buffer of max(n, min_n) elements (null for none), moved into `out` only on success
template <typename T>
hipError_t dev_upload(DevPtr<T>& out, const T* src, size_t n, size_t min_n = 0) {
  DevPtr<T> p;
  hipError_t e = dev_alloc(p, std::max(n, min_n));
  if (e == hipSuccess && n) e = hipMemcpy(p.get(), src, sizeof(T) * n, hipMemcpyHostToDevice);
  if (e == hipSuccess) out = std::move(p);
  return e;
}

// a staging buffer of n elements in place of `buf`, whose old buffer is released once stream `s` no longer reads it
template <typename T>
hipError_t dev_grow(DevPtr<T>& buf, size_t n, hipStream_t s) {
  DevPtr<T> p;
  hipError_t e = dev_alloc(p, n);
  if (e == hipSuccess && buf) e = hipStreamSynchronize(s);
  if (e == hipSuccess) buf = std::move(p);
  return e;
}

// The plan of the last observation resize of one kind and the device copy of its tables, kept while the next call brings the same tables.
struct ObserveSlot {
  ObservePlan plan;
  DevPtr<int32_t> d_tab;
};

// The assets of the last dtsim_set_assets: the device copies, and on the host what dt_pack_maps and dt_pack_segment_texels need
// later (T.tris is released after the upload).
struct AssetSlot {
  AssetTables T;
  DevPtr<uint32_t> d_texels;
  DevPtr<TexDev> d_tex;
  DevPtr<MeshDev> d_meshes;
  DevPtr<TriDev> d_tris;
};

// The maps of the last dtsim_set_maps: M (blobs, dyn) serves physics, reset, query and the sampler; the rest is the render side,
// packed against the assets of that moment -- a later dtsim_set_assets releases it (renderable = false) until the next dtsim_set_maps.
struct MapSlot : MapScalars {
  DevPtr<uint64_t> d_blobs;
  DevPtr<DynInit> d_dyn;
  bool renderable = false;
  DevPtr<RenderMapDev> d_rmaps;
  DevPtr<uint32_t> d_rtiles;
  DevPtr<TileLds> d_tilerecs;
  DevPtr<ObjInstDev> d_robjs;
  DevPtr<uint8_t> d_qtex;             // quad-layout blocks for k_raster_q
  DevPtr<uint32_t> d_qtiles;
  DevPtr<double> d_ocorners;          // dt_pack_object_corners: the objects' collision rectangles, in d_robjs' order (dtsim_bev)
  DevPtr<char> d_obj[DT_SLABS];       // DT_SLAB_STRIS .. DT_SLAB_OBJMASK of the render scratch (dt_render_layout): only with mesh objects
  void release_render() {
    renderable = false;
    d_rmaps.reset(); d_rtiles.reset(); d_tilerecs.reset(); d_robjs.reset(); d_qtex.reset(); d_qtiles.reset(); d_ocorners.reset();
    for (auto& p : d_obj) p.reset();
  }
};

}  // namespace

struct dtsim {
  dtsim_config cfg{};
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int N = 0;
  // SoA slab
  DevPtr<char> slab;
  size_t slab_bytes = 0;
  SimArrays A{};
  // maps
  bool have_maps = false, have_reset = false;
  MapSlot maps;
  // reset / pool staging
  DevPtr<dtsim_init_state> d_states;
  DevPtr<uint8_t> d_mask;
  DevPtr<dtsim_init_state> d_pool;
  int n_pool = 0;
  // actions staging
  DevPtr<char> d_actions;
  size_t actions_cap = 0;
  // query staging
  DevPtr<int32_t> d_qenv;
  DevPtr<double> d_qpose;
  DevPtr<dtsim_probe> d_qout;
  DevPtr<dtsim_agent_info> d_agent;
  bool rendered = false;          // a render pass has written the per-env cameras (dtsim_draw_lines needs them)
  bool masked = false;            // the last pass was dtsim_render_masked: the post-passes need a full one
  RenderParams last_R{};          // the parameters of that pass (dtsim_draw_leds: projected triangles, tables); last_segment: it was the segment view
  bool last_segment = false;
  bool leds_ok = false;           // last_R still names live buffers (cleared by dtsim_set_assets / dtsim_set_maps / dtsim_set_distortion_lut, which re-allocate)
  DevPtr<float> d_leds;          // dtsim_draw_leds: device copy of the caller's spheres
  int leds_cap = 0;
  DevPtr<float> d_lines;          // dtsim_draw_lines: device copy of the caller's segments
  int lines_cap = 0;
  int render_tables = 0;          // dt_launch_render: which env-invariant tables are valid (camera LUT + maps unchanged)
  int render_pipe = 0;            // DTSIM_PIPE_* of the last render pass (DTSIM_FIELD_RENDER_PIPE)
  int q_cap = 0;
  // render
  DevPtr<uint8_t> frames_own;
  uint8_t* frames = nullptr;      // frames_own, or the caller's memory (dtsim_bind_frames)
  size_t frames_bytes = 0;
  DevPtr<float> d_lut;
  bool have_lut = false;
  // camera_rand (dtsim_set_distortion_luts): per-env remap tables; while n_cal > 0 the raster writes the rectilinear frames into
  // d_scratch (d_lut is the identity) and k_remap_cal gathers them into `frames`
  int n_cal = 0;
  bool camera_rand = false;       // DTSIM_LUTS_CAMERA_RAND: the device reset sampler scales the camera
  DevPtr<int32_t> d_cal_src;      // [n_cal][H*W]
  DevPtr<int32_t> d_env_cal;      // [N]
  DevPtr<uint8_t> d_scratch;      // [N][H][W][3]
  AssetSlot assets;
  DevPtr<uint32_t> d_texels_seg;      // segmented versions, same layout as assets.d_texels (dtsim_set_segment_assets)
  DevPtr<uint8_t> d_mesh_seg;         // [n_meshes][4] flat segmentation colour per mesh
  DevPtr<uint8_t> d_texel_class;      // one class byte per texel in assets.d_texels' layout (dtsim_set_label_assets)
  DevPtr<uint8_t> d_mesh_class;       // [n_meshes] class per mesh
  int n_mesh_class = 0;               // entries of d_mesh_class (at least 1)
  DevPtr<char> d_render[DT_SLABS];    // the render scratch (dt_render_layout): DT_SLAB_ENV .. DT_SLAB_QEND, allocated at dtsim_create (the object slabs: maps.d_obj)
  EnvRecs recs{};                     // the typed per-env records and per-pixel tables inside d_render (dt_render_layout's, set with the slabs)
  bool raster_old = false;            // DTSIM_RASTER_OLD=1 at dtsim_create: neither k_raster_v3 nor k_raster_v3dr (A/B timing only; dt_raster_pipe)
  int step_lanes = 1;                 // lanes of a wavefront per env in k_step (physics.hip Coop): 1, 2 or 4
  DevPtr<dtsim_reset_sampler> d_sampler;      // device copy when a reset sampler is installed
  ObserveSlot obs, obsc;          // dtsim_observe / dtsim_observe_cubic (and their masked forms)
  // dtsim_ipm: the calibrations of dtsim_set_ipm_calibrations, and the shared camera's table of source pixels with the key it was built for
  int n_ipm_cal = 0;
  DevPtr<IpmCal> d_ipm_cal;         // [n_ipm_cal]
  DevPtr<int32_t> d_ipm_env_cal;    // [N], or null: calibration 0 for every env
  DevPtr<int32_t> d_ipm_table;      // [DTSIM_BEV_MAX_SIDE^2]: allocated at the first use and never moved, so a rebuild is stream-ordered
  struct IpmKey { int oh = 0, ow = 0, rows_behind = 0; double cell = 0.0; uint64_t cal = 0; } ipm_key;   // cal = 0: no table yet
  uint64_t ipm_cal_version = 1;     // counts the installs: a new calibration is a new key
  // dtsim_flow: the remembered states of dtsim_flow_mark and the per-env records of a call, both [N], allocated at the first use and never
  // moved; neither is part of SimArrays or the state slab.  lut_fisheye: the single distortion table is not the identity.
  DevPtr<FlowMark> d_flow_mark;
  DevPtr<FlowRec> d_flow_rec;
  bool lut_fisheye = false;
  ProfSlot prof[DTSIM_KERNEL__COUNT];
};

namespace {

StepParams step_params(const dtsim* h, int n_steps) {
  StepParams P{};
  P.n_steps = n_steps;
  P.frame_skip = h->cfg.frame_skip;
  P.max_steps = h->cfg.max_steps;
  P.delay_steps = h->cfg.delay_steps;
  P.action_mode = h->cfg.action_mode;
  P.actions_f64 = (h->cfg.flags & DTSIM_F_ACTIONS_F64) ? 1 : 0;
  P.auto_reset = ((h->cfg.flags & DTSIM_F_AUTO_RESET) && (h->n_pool > 0 || h->d_sampler)) ? 1 : 0;
  P.n_pool = h->n_pool;
  P.sampler = h->d_sampler.get();
  P.delta_time = h->cfg.delta_time;
  P.robot_speed = h->cfg.robot_speed;
  P.gain = h->cfg.gain; P.trim = h->cfg.trim; P.radius = h->cfg.radius; P.k = h->cfg.k; P.limit = h->cfg.limit;
  P.lanes = h->step_lanes;
  P.light_capture = (h->cfg.flags & DTSIM_F_LIGHT_CAPTURE) ? 1 : 0;
  P.domain_rand = (h->cfg.flags & DTSIM_F_DOMAIN_RAND) ? 1 : 0;
  P.camera_rand = h->camera_rand ? 1 : 0;
  return P;
}

// points R's scratch fields into the handle's render slabs (dt_render_layout); returns the slabs' typed records
EnvRecs render_scratch(const dtsim* h, int max_tris, RenderParams* R) {
  void* base[DT_SLABS];
  for (int i = 0; i < DT_SLABS; ++i) base[i] = i < DT_SLAB_STRIS ? h->d_render[i].get() : h->maps.d_obj[i].get();
  return dt_render_layout(h->N, h->cfg.cam_width, h->cfg.cam_height, max_tris, nullptr, base, R);
}

// the scene of a pass: the assets (segment: their segmented texels) and the render side of the maps
void render_scene(const dtsim* h, bool segment, RenderParams* R) {
  const AssetSlot& a = h->assets;
  const MapSlot& m = h->maps;
  R->texels = segment ? h->d_texels_seg.get() : a.d_texels.get(); R->tex = a.d_tex.get();
  R->meshes = a.d_meshes.get(); R->tris = a.d_tris.get();
  R->n_maps = m.M.n_maps;
  R->maps = m.d_rmaps.get(); R->tiles = m.d_rtiles.get(); R->objs = m.d_robjs.get();
  R->max_tris = m.d_obj[DT_SLAB_STRIS] ? m.max_tris : 0;
  R->tile_recs = m.d_tilerecs.get(); R->n_tile_recs = m.n_tilerecs; R->tex_w = m.tex_w; R->tex_h = m.tex_h;
  R->qtex = m.d_qtex.get(); R->qtiles = m.d_qtiles.get(); R->n_qtiles = m.n_qtiles; R->qlog2 = m.qlog2; R->q_per_m = m.q_per_m;
  R->qmax_tiles = std::max(m.grid_rows, m.grid_cols);
}

// the render entry points after a dtsim_set_assets that followed dtsim_set_maps: the maps' render tables indexed the old assets and are gone
int check_renderable(const dtsim* h, const char* who) {
  if (h->have_maps && !h->maps.renderable)
    return fail(DTSIM_E_STATE, "%s: dtsim_set_assets replaced the assets the maps were packed against: call dtsim_set_maps again", who);
  return DTSIM_OK;
}

struct ProfScope {
  dtsim* h; int k; hipEvent_t a = nullptr, b = nullptr; bool on;
  ProfScope(dtsim* h_, int k_) : h(h_), k(k_), on((h_->cfg.flags & DTSIM_F_PROFILE) != 0) {
    if (!on) return;
    ProfSlot& s = h->prof[k];
    if (!s.free_.empty()) { a = s.free_.back().first; b = s.free_.back().second; s.free_.pop_back(); }
    else { (void)hipEventCreate(&a); (void)hipEventCreate(&b); }
    (void)hipEventRecord(a, h->stream);
  }
  ~ProfScope() {
    if (!on) return;
    (void)hipEventRecord(b, h->stream);
    h->prof[k].pending.emplace_back(a, b);
  }
};

}  // namespace

extern "C" {

int dtsim_abi_version(void) { return DTSIM_ABI_VERSION; }
const char* dtsim_last_error(void) { return g_err.c_str(); }

int dtsim_device_count(void) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) return fail(DTSIM_E_NOGPU, "hipGetDeviceCount: %s", hipGetErrorString(e));
  return n;
}

int dtsim_create(const dtsim_config* cfg, dtsim_t** out) {
  if (!cfg || !out) return fail(DTSIM_E_INVALID, "null argument");
  *out = nullptr;
  if (cfg->struct_size != sizeof(dtsim_config))
    return fail(DTSIM_E_INVALID, "dtsim_config.struct_size %u != %zu (ABI mismatch)", cfg->struct_size,
                sizeof(dtsim_config));
  if (cfg->num_envs <= 0) return fail(DTSIM_E_INVALID, "num_envs must be > 0");
  if (cfg->delay_steps < 0 || cfg->delay_steps > DTSIM_MAX_DELAY)
    return fail(DTSIM_E_LIMIT, "delay_steps %d outside [0,%d]", cfg->delay_steps, DTSIM_MAX_DELAY);
  if (cfg->frame_skip < 1 || cfg->delta_time <= 0) return fail(DTSIM_E_INVALID, "bad frame_skip/delta_time");
  if (cfg->cam_width <= 0 || cfg->cam_height <= 0) return fail(DTSIM_E_INVALID, "bad camera size");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(DTSIM_E_NOGPU, "no HIP device visible: libdtsim has no CPU fallback");
  if (cfg->device < 0 || cfg->device >= ndev) return fail(DTSIM_E_INVALID, "device %d out of range", cfg->device);
  HIPCHK(hipSetDevice(cfg->device));
  dtsim* h = new dtsim();
  { const char* ro = getenv("DTSIM_RASTER_OLD"); h->raster_old = ro && ro[0] == '1'; }   // A/B timing aid: k_raster_q instead of k_raster_v3
  // lanes of a wavefront per env in k_step: as many (up to 4) as keep the launch within ~32 K threads -- a small batch is a
  // latency problem (one f64 chain per env, 64 wavefronts on 1024 SIMDs at N = 4096), a large one a throughput problem,
  // where the redundant lanes would cost (profiles/r03_c2_lanes_ab.txt)
  // (tests/test_gpu_step_lanes.py runs one batch size per lane count: move N_LANES_4 / N_LANES_2 / N_LANES_1 there with these thresholds)
  h->step_lanes = cfg->num_envs * 4 <= 32768 ? 4 : cfg->num_envs * 2 <= 32768 ? 2 : 1;
  h->cfg = *cfg;
  h->N = cfg->num_envs;
  if (cfg->stream) { h->stream = (hipStream_t)cfg->stream; }
  else {
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete h; return fail(DTSIM_E_HIP, "hipStreamCreate: %s", hipGetErrorString(e)); }
    h->own_stream = true;
  }
  h->slab_bytes = dt_state_layout(h->A, h->N, nullptr);
  hipError_t e = dev_alloc(h->slab, h->slab_bytes);
  if (e != hipSuccess) { dtsim_destroy(h); return fail(DTSIM_E_HIP, "hipMalloc(state %zu B): %s", h->slab_bytes, hipGetErrorString(e)); }
  (void)hipMemsetAsync(h->slab.get(), 0, h->slab_bytes, h->stream);
  dt_state_layout(h->A, h->N, h->slab.get());
  // map_id = -1 everywhere so the first reset creates the world objects
  (void)hipMemsetAsync(h->A.map_id, 0xFF, sizeof(int32_t) * (size_t)h->N, h->stream);
  e = dev_alloc(h->d_states, (size_t)h->N);
  if (e == hipSuccess) e = dev_alloc(h->d_mask, (size_t)h->N);
  if (e != hipSuccess) { dtsim_destroy(h); return fail(DTSIM_E_HIP, "hipMalloc(reset staging): %s", hipGetErrorString(e)); }
  if (cfg->flags & DTSIM_F_RENDER) {
    h->frames_bytes = (size_t)h->N * cfg->cam_height * cfg->cam_width * 3;
    e = dev_alloc(h->frames_own, h->frames_bytes);
    if (e != hipSuccess) { dtsim_destroy(h); return fail(DTSIM_E_HIP, "hipMalloc(frames %zu B): %s", h->frames_bytes, hipGetErrorString(e)); }
    h->frames = h->frames_own.get();
    e = dev_alloc(h->d_lut, 4 * (size_t)cfg->cam_height * cfg->cam_width);
    size_t bytes[DT_SLABS]; dt_render_layout(h->N, cfg->cam_width, cfg->cam_height, 0, bytes);
    for (int i = DT_SLAB_ENV; i <= DT_SLAB_QEND && e == hipSuccess; ++i) e = dev_alloc(h->d_render[i], bytes[i]);
    // the per-env records start zeroed: a post-pass that is wrongly pointed at an env no pass has written (dtsim_depth_masked with another mask
    // than the pass's: the caller's error, its result undefined) then reads no object and no map index outside the tables
    if (e == hipSuccess) e = hipMemset(h->d_render[DT_SLAB_ENV].get(), 0, bytes[DT_SLAB_ENV]);
    RenderParams R{}; h->recs = render_scratch(h, 0, &R);
    if (e == hipSuccess) e = hipMemset(R.dump, 0, sizeof(RenderDump));
    if (e != hipSuccess) { dtsim_destroy(h); return fail(DTSIM_E_HIP, "hipMalloc(render scratch): %s", hipGetErrorString(e)); }
    if (!(cfg->flags & DTSIM_F_DISTORTION)) {
      // identity LUT: output pixel == rectilinear pixel
      int rc = dtsim_set_distortion_lut(h, nullptr, nullptr);
      if (rc != DTSIM_OK) { dtsim_destroy(h); return rc; }
    }
  }
  *out = h;
  return DTSIM_OK;
}

void dtsim_destroy(dtsim_t* h) {
  if (!h) return;
  (void)hipSetDevice(h->cfg.device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (auto& s : h->prof) {
    for (auto& p : s.pending) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    for (auto& p : s.free_) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
  }
  if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
  delete h;   // frees every device buffer the handle owns
}

// dtsim_set_maps / dtsim_set_assets, once they have succeeded: no env has a mark (stream-ordered, like the marks themselves)
static void drop_flow_marks(dtsim_t* h) {
  if (h->d_flow_mark) (void)hipMemsetAsync(h->d_flow_mark.get(), 0, sizeof(FlowMark) * (size_t)h->N, h->stream);
}

int dtsim_set_assets(dtsim_t* h, const dtsim_texture* textures, int n_textures, const dtsim_mesh* meshes,
                     int n_meshes) {
  if (!h) return fail(DTSIM_E_INVALID, "null handle");
  h->leds_ok = false;
  h->render_tables = 0;           // the cached per-pixel / per-block render tables depend on this
  AssetSlot next;
  std::string err;
  if (int rc = dt_pack_assets(next.T, err, textures, n_textures, meshes, n_meshes)) return fail(rc, "%s", err.c_str());
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(dev_upload(next.d_texels, next.T.pool.data(), next.T.pool.size()));
  HIPCHK(dev_upload(next.d_tex, next.T.tex.data(), next.T.tex.size()));
  HIPCHK(dev_upload(next.d_meshes, next.T.meshes.data(), next.T.meshes.size()));
  HIPCHK(dev_upload(next.d_tris, next.T.tris.data(), next.T.tris.size()));
  next.T.tris = {};
  h->assets = std::move(next);
  h->maps.release_render();       // the installed maps' render tables index the old lists: the render entry points wait for dtsim_set_maps
  h->d_texels_seg.reset();        // mirrors the old list
  h->d_texel_class.reset(); h->d_mesh_class.reset(); h->n_mesh_class = 0;   // so do the label tables
  drop_flow_marks(h);
  return DTSIM_OK;
}

int dtsim_set_segment_assets(dtsim_t* h, const dtsim_texture* textures, int n_textures, const uint8_t* mesh_rgb, int n_meshes) {
  if (!h) return fail(DTSIM_E_INVALID, "null handle");
  std::vector<uint32_t> pool;
  std::vector<uint8_t> rgbx;
  std::string err;
  if (int rc = dt_pack_segment_texels(pool, rgbx, err, textures, n_textures, mesh_rgb, n_meshes, h->assets.T)) return fail(rc, "%s", err.c_str());
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipStreamSynchronize(h->stream));
  DevPtr<uint32_t> d_texels_seg;
  DevPtr<uint8_t> d_mesh_seg;
  HIPCHK(dev_upload(d_texels_seg, pool.data(), pool.size(), 1));
  HIPCHK(dev_upload(d_mesh_seg, rgbx.data(), rgbx.size()));
  h->d_texels_seg = std::move(d_texels_seg); h->d_mesh_seg = std::move(d_mesh_seg);
  return DTSIM_OK;
}

int dtsim_set_label_assets(dtsim_t* h, const uint8_t* const* texel_class, int n_textures, const uint8_t* mesh_class, int n_meshes) {
  if (!h) return fail(DTSIM_E_INVALID, "null handle");
  std::vector<uint8_t> pool, mesh_tab;
  std::string err;
  if (int rc = dt_pack_label_tables(pool, mesh_tab, err, texel_class, n_textures, mesh_class, n_meshes, h->assets.T)) return fail(rc, "%s", err.c_str());
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipStreamSynchronize(h->stream));
  DevPtr<uint8_t> d_texel_class, d_mesh_class;
  HIPCHK(dev_upload(d_texel_class, pool.data(), pool.size(), 1));
  HIPCHK(dev_upload(d_mesh_class, mesh_tab.data(), mesh_tab.size()));
  h->d_texel_class = std::move(d_texel_class); h->d_mesh_class = std::move(d_mesh_class); h->n_mesh_class = (int)mesh_tab.size();
  return DTSIM_OK;
}

int dtsim_set_maps(dtsim_t* h, const dtsim_map* maps, int n_maps) {
  if (!h) return fail(DTSIM_E_INVALID, "null argument");
  h->leds_ok = false;
  h->render_tables = 0;           // the cached per-pixel / per-block render tables depend on this
  MapTables T;
  std::string err;
  if (int rc = dt_pack_maps(T, err, maps, n_maps, h->assets.T, (h->cfg.flags & DTSIM_F_RENDER) != 0)) return fail(rc, "%s", err.c_str());
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipStreamSynchronize(h->stream));
  MapSlot next;
  static_cast<MapScalars&>(next) = T;
  HIPCHK(dev_upload(next.d_blobs, T.blobs.data(), T.blobs.size()));
  HIPCHK(dev_upload(next.d_dyn, T.dyn.data(), T.dyn.size()));
  HIPCHK(dev_upload(next.d_rmaps, T.rmaps.data(), T.rmaps.size()));
  HIPCHK(dev_upload(next.d_rtiles, T.rtiles.data(), T.rtiles.size(), 1));
  HIPCHK(dev_upload(next.d_robjs, T.robjs.data(), T.robjs.size(), 1));
  HIPCHK(dev_upload(next.d_tilerecs, T.trecs.data(), T.trecs.size(), 1));
  HIPCHK(dev_upload(next.d_qtex, reinterpret_cast<const uint8_t*>(T.qblocks.data()), T.qblocks.size() * 4));
  HIPCHK(dev_upload(next.d_qtiles, T.qtiles.data(), T.qtiles.size()));
  HIPCHK(dev_upload(next.d_ocorners, T.ocorners.data(), T.ocorners.size(), 8));
  size_t bytes[DT_SLABS]; dt_render_layout(h->N, h->cfg.cam_width, h->cfg.cam_height, T.max_tris, bytes);
  for (int i = DT_SLAB_STRIS; i <= DT_SLAB_OBJMASK; ++i)     // the object slabs: only with mesh objects
    if (bytes[i] && (h->cfg.flags & DTSIM_F_RENDER)) HIPCHK(dev_alloc(next.d_obj[i], bytes[i]));
  if (next.d_obj[DT_SLAB_OBJBOX]) HIPCHK(hipMemset(next.d_obj[DT_SLAB_OBJBOX].get(), 0, bytes[DT_SLAB_OBJBOX]));   // no object boxes until a pass writes them (as the records of dtsim_create)
  // worlds must be re-created against the new maps
  HIPCHK(hipMemsetAsync(h->A.map_id, 0xFF, sizeof(int32_t) * (size_t)h->N, h->stream));
  next.M.blobs = next.d_blobs.get();
  next.M.dyn = next.d_dyn.get();
  next.renderable = true;
  h->maps = std::move(next);
  h->have_maps = true;
  h->have_reset = false;
  drop_flow_marks(h);
  return DTSIM_OK;
}

// one distortion table for every env again (the sampler switch stays: it is dtsim_set_distortion_luts' to set)
static void drop_luts(dtsim_t* h) {
  h->d_cal_src.reset(); h->d_env_cal.reset(); h->d_scratch.reset();
  h->n_cal = 0;
}

int dtsim_set_distortion_lut(dtsim_t* h, const float* rmapx, const float* rmapy) {
  if (!h) return fail(DTSIM_E_INVALID, "null handle");
  h->leds_ok = false;
  h->render_tables = 0;           // the cached per-pixel / per-block render tables depend on this
  if (!h->d_lut) return fail(DTSIM_E_STATE, "handle created without DTSIM_F_RENDER");
  if ((rmapx == nullptr) != (rmapy == nullptr)) return fail(DTSIM_E_INVALID, "rmapx/rmapy must both be given");
  if (rmapx && !(h->cfg.flags & DTSIM_F_DISTORTION)) return fail(DTSIM_E_STATE, "handle created without DTSIM_F_DISTORTION");
  HIPCHK(hipSetDevice(h->cfg.device));
  const int W = h->cfg.cam_width, H = h->cfg.cam_height;
  std::vector<float> lut;
  dt_pack_lut(W, H, rmapx, rmapy, lut);
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(dev_upload(h->d_lut, lut.data(), lut.size()));
  drop_luts(h);
  h->have_lut = true;
  h->lut_fisheye = rmapx != nullptr;
  return DTSIM_OK;
}

int dtsim_set_distortion_luts(dtsim_t* h, int n_cal, const int32_t* src_index, const int32_t* env_cal, uint32_t flags) {
  if (!h) return fail(DTSIM_E_INVALID, "null handle");
  if (flags & ~(uint32_t)DTSIM_LUTS_CAMERA_RAND) return fail(DTSIM_E_INVALID, "unknown flags 0x%x", flags);
  if (!h->d_lut) return fail(DTSIM_E_STATE, "handle created without DTSIM_F_RENDER");
  if (n_cal == 0) {                                   // uninstall: the caller installs a single table with dtsim_set_distortion_lut
    if (src_index || env_cal) return fail(DTSIM_E_INVALID, "n_cal = 0 takes no tables");
    if ((flags & DTSIM_LUTS_CAMERA_RAND) && (h->cfg.flags & DTSIM_F_LIGHT_CAPTURE))
      return fail(DTSIM_E_STATE, "DTSIM_LUTS_CAMERA_RAND with DTSIM_F_LIGHT_CAPTURE is not supported");
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    drop_luts(h);
    h->camera_rand = (flags & DTSIM_LUTS_CAMERA_RAND) != 0;
    return DTSIM_OK;
  }
  if (n_cal < 0 || !src_index || !env_cal) return fail(DTSIM_E_INVALID, "n_cal %d, src_index %p, env_cal %p", n_cal, (const void*)src_index, (const void*)env_cal);
  if (!(h->cfg.flags & DTSIM_F_DISTORTION)) return fail(DTSIM_E_STATE, "handle created without DTSIM_F_DISTORTION");
  if (h->cfg.flags & DTSIM_F_LIGHT_CAPTURE) return fail(DTSIM_E_STATE, "per-env distortion tables with DTSIM_F_LIGHT_CAPTURE are not supported");
  const int W = h->cfg.cam_width, H = h->cfg.cam_height;
  const size_t hw = (size_t)W * H;
  for (int e = 0; e < h->N; ++e)
    if (env_cal[e] < 0 || env_cal[e] >= n_cal) return fail(DTSIM_E_INVALID, "env_cal[%d] = %d outside [0, %d)", e, env_cal[e], n_cal);
  for (size_t i = 0; i < (size_t)n_cal * hw; ++i)     // every gather of k_remap_cal stays inside the env's scratch frame
    if (src_index[i] < -1 || src_index[i] >= (int64_t)hw) return fail(DTSIM_E_INVALID, "src_index[%zu] = %d outside [-1, %zu)", i, src_index[i], hw);
  HIPCHK(hipSetDevice(h->cfg.device));
  DevPtr<int32_t> d_src, d_cal;
  DevPtr<uint8_t> d_scr;
  HIPCHK(dev_upload(d_src, src_index, hw * n_cal));
  HIPCHK(dev_upload(d_cal, env_cal, (size_t)h->N));
  HIPCHK(dev_alloc(d_scr, h->frames_bytes));
  // the raster renders rectilinear frames while the tables are installed (this also drops the previous per-env tables)
  if (int rc = dtsim_set_distortion_lut(h, nullptr, nullptr)) return rc;
  h->d_cal_src = std::move(d_src); h->d_env_cal = std::move(d_cal); h->d_scratch = std::move(d_scr);
  h->n_cal = n_cal;
  h->camera_rand = (flags & DTSIM_LUTS_CAMERA_RAND) != 0;
  return DTSIM_OK;
}

int dtsim_build_remap_maps(int width, int height, int n_cal, const double* K, const double* D, const double* inv_new_K, float* rmapx, float* rmapy) {
  if (width < 5 || height < 5 || n_cal < 0 || (n_cal && (!K || !D || !inv_new_K || !rmapx || !rmapy)))
    return fail(DTSIM_E_INVALID, "dtsim_build_remap_maps: %d x %d, n_cal %d, null tables", width, height, n_cal);
  dt_build_remap_maps(width, height, n_cal, K, D, inv_new_K, rmapx, rmapy);
  return DTSIM_OK;
}

int dtsim_fill_pack_remap(int width, int height, int n_cal, float* rmapx, float* rmapy, const int32_t* hole_order, const int64_t* hole_off,
                          int32_t* src_index) {
  if (width <= 0 || height <= 0 || n_cal < 0 || (n_cal && (!rmapx || !rmapy || !hole_off)))
    return fail(DTSIM_E_INVALID, "dtsim_fill_pack_remap: %d x %d, n_cal %d, null tables", width, height, n_cal);
  const int64_t hw = (int64_t)width * height;
  for (int i = 0; i < n_cal; ++i) {
    if (hole_off[i] < 0 || hole_off[i + 1] < hole_off[i] || (hole_off[i + 1] > hole_off[i] && !hole_order))
      return fail(DTSIM_E_INVALID, "hole_off[%d..%d] = %lld, %lld", i, i + 1, (long long)hole_off[i], (long long)hole_off[i + 1]);
    for (int64_t k = hole_off[i]; k < hole_off[i + 1]; ++k)
      if (hole_order[k] < 0 || hole_order[k] >= hw) return fail(DTSIM_E_INVALID, "hole_order[%lld] = %d outside the image", (long long)k, hole_order[k]);
  }
  dt_fill_pack_remap(width, height, n_cal, rmapx, rmapy, hole_order, hole_off, src_index);
  return DTSIM_OK;
}

static int check_states(const dtsim* h, const dtsim_init_state* st, int n, const uint8_t* mask) {
  for (int e = 0; e < n; ++e) {
    if (mask && !mask[e]) continue;
    const int mid = st[e].map_id & ~DTSIM_MAP_RELOAD;
    if (st[e].map_id < 0 || mid >= h->maps.M.n_maps) return fail(DTSIM_E_INVALID, "state %d: map_id %d out of range", e, st[e].map_id);
  }
  return DTSIM_OK;
}

int dtsim_set_reset_sampler(dtsim_t* h, const dtsim_reset_sampler* sampler) {
  if (!h) return fail(DTSIM_E_INVALID, "null handle");
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (!sampler) {
    h->d_sampler.reset();
    return DTSIM_OK;
  }
  if (!h->have_maps) return fail(DTSIM_E_STATE, "dtsim_set_reset_sampler before dtsim_set_maps");
  if (sampler->max_attempts <= 0 || !(sampler->accept_start_angle_deg > 0))
    return fail(DTSIM_E_INVALID, "sampler: max_attempts %d, accept_start_angle_deg %g", sampler->max_attempts, sampler->accept_start_angle_deg);
  for (int m = 0; m < h->maps.M.n_maps; ++m) {
    const int i = sampler->start_tile[m][0], j = sampler->start_tile[m][1];
    if (i < 0) continue;
    if (i >= h->maps.grid_w[m] || j < 0 || j >= h->maps.grid_h[m]) return fail(DTSIM_E_INVALID, "sampler: start tile (%d,%d) outside map %d", i, j, m);
  }
  HIPCHK(dev_upload(h->d_sampler, sampler, 1));
  return DTSIM_OK;
}

int dtsim_reset_done(dtsim_t* h) {
  if (!h) return fail(DTSIM_E_INVALID, "null handle");
  if (!h->have_reset) return fail(DTSIM_E_STATE, "dtsim_reset_done before the first dtsim_reset");
  if (!h->d_sampler) return fail(DTSIM_E_STATE, "dtsim_reset_done needs dtsim_set_reset_sampler");
  h->rendered = false;
  HIPCHK(hipSetDevice(h->cfg.device));
  {
    ProfScope ps(h, DTSIM_KERNEL_RESET);
    dt_launch_reset(h->stream, h->A, h->maps.M, step_params(h, 0), h->A.done, nullptr);   // mask = the done flags, on the device
  }
  HIPCHK(hipGetLastError());
  return DTSIM_OK;
}

int dtsim_reset(dtsim_t* h, const uint8_t* mask, const dtsim_init_state* states) {
  if (!h) return fail(DTSIM_E_INVALID, "null argument");
  if (!h->have_maps) return fail(DTSIM_E_STATE, "dtsim_reset before dtsim_set_maps");
  h->rendered = false;                               // the state moves on: the post-passes (dtsim_draw_lines / dtsim_draw_leds) need a new dtsim_render
  if (!states) {                                     // device-side sampling
    if (!h->d_sampler) return fail(DTSIM_E_STATE, "dtsim_reset(states = NULL) needs dtsim_set_reset_sampler");
    HIPCHK(hipSetDevice(h->cfg.device));
    if (mask) HIPCHK(hipMemcpyAsync(h->d_mask.get(), mask, (size_t)h->N, hipMemcpyHostToDevice, h->stream));
    {
      ProfScope ps(h, DTSIM_KERNEL_RESET);
      dt_launch_reset(h->stream, h->A, h->maps.M, step_params(h, 0), mask ? h->d_mask.get() : nullptr, nullptr);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    h->have_reset = true;
    return DTSIM_OK;
  }
  int rc = check_states(h, states, h->N, mask);
  if (rc) return rc;
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipMemcpyAsync(h->d_states.get(), states, sizeof(dtsim_init_state) * (size_t)h->N, hipMemcpyHostToDevice, h->stream));
  if (mask) HIPCHK(hipMemcpyAsync(h->d_mask.get(), mask, (size_t)h->N, hipMemcpyHostToDevice, h->stream));
  {
    ProfScope ps(h, DTSIM_KERNEL_RESET);
    dt_launch_reset(h->stream, h->A, h->maps.M, step_params(h, 0), mask ? h->d_mask.get() : nullptr, h->d_states.get());
  }
  HIPCHK(hipGetLastError());
  // the host buffers may be reused by the caller as soon as we return
  HIPCHK(hipStreamSynchronize(h->stream));
  h->have_reset = true;
  return DTSIM_OK;
}

int dtsim_set_spawn_pool(dtsim_t* h, const dtsim_init_state* pool, int n_pool) {
  if (!h || !pool || n_pool <= 0) return fail(DTSIM_E_INVALID, "bad pool");
  if (!h->have_maps) return fail(DTSIM_E_STATE, "dtsim_set_spawn_pool before dtsim_set_maps");
  int rc = check_states(h, pool, n_pool, nullptr);
  if (rc) return rc;
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(dev_upload(h->d_pool, pool, (size_t)n_pool));
  h->n_pool = n_pool;
  return DTSIM_OK;
}

int dtsim_step(dtsim_t* h, const void* actions, int n_steps, int actions_on_device) {
  return dtsim_step_ex(h, actions, n_steps, actions_on_device, 0u);
}

int dtsim_step_ex(dtsim_t* h, const void* actions, int n_steps, int actions_on_device, uint32_t flags) {
  if (!h || !actions || n_steps <= 0) return fail(DTSIM_E_INVALID, "bad argument");
  if (flags & ~(uint32_t)(DTSIM_STEP_ONE_UPDATE | DTSIM_STEP_POSE_ONLY)) return fail(DTSIM_E_INVALID, "unknown step flags 0x%x", flags);
  if (!h->have_maps || !h->have_reset) return fail(DTSIM_E_STATE, "dtsim_step before dtsim_set_maps/dtsim_reset");
  h->rendered = false;                               // the cameras / projected triangles of the last render pass describe the state before this step
  HIPCHK(hipSetDevice(h->cfg.device));
  const size_t esz = (h->cfg.flags & DTSIM_F_ACTIONS_F64) ? 8 : 4;
  const size_t bytes = (size_t)n_steps * h->N * 2 * esz;
  const void* dptr = actions;
  if (!actions_on_device) {
    if (bytes > h->actions_cap) {
      HIPCHK(dev_grow(h->d_actions, bytes, h->stream));
      h->actions_cap = bytes;
    }
    // pageable host memory: hipMemcpyAsync stages synchronously, so the caller may
    // reuse `actions` on return
    HIPCHK(hipMemcpyAsync(h->d_actions.get(), actions, bytes, hipMemcpyHostToDevice, h->stream));
    dptr = h->d_actions.get();
  }
  {
    ProfScope ps(h, DTSIM_KERNEL_STEP);
    StepParams sp = step_params(h, n_steps);
    sp.step_flags = flags;
    dt_launch_step(h->stream, h->A, h->maps.M, sp, dptr, h->d_pool.get());
  }
  HIPCHK(hipGetLastError());
  return DTSIM_OK;
}

int dtsim_render(dtsim_t* h) { return dtsim_render_ex(h, 0u); }

static int render_pass(dtsim_t* h, uint32_t flags, const uint8_t* mask);
int dtsim_render_ex(dtsim_t* h, uint32_t flags) { return render_pass(h, flags, nullptr); }
int dtsim_render_masked(dtsim_t* h, uint32_t flags, const uint8_t* mask) {
  if (!mask) return fail(DTSIM_E_INVALID, "dtsim_render_masked: null mask");
  return render_pass(h, flags, mask);
}

// mask: dtsim_render_masked's device mask, or null for the full pass
static int render_pass(dtsim_t* h, uint32_t flags, const uint8_t* mask) {
  if (!h) return fail(DTSIM_E_INVALID, "null handle");
  if (flags & ~(uint32_t)(DTSIM_RENDER_SEGMENT | DTSIM_RENDER_GL_FILTER)) return fail(DTSIM_E_INVALID, "unknown render flags 0x%x", flags);
  const bool segment = (flags & DTSIM_RENDER_SEGMENT) != 0;
  if (segment && !h->d_texels_seg) return fail(DTSIM_E_STATE, "DTSIM_RENDER_SEGMENT before dtsim_set_segment_assets");
  if (!h->frames) return fail(DTSIM_E_STATE, "handle created without DTSIM_F_RENDER");
  if (!h->have_maps || !h->have_reset) return fail(DTSIM_E_STATE, "dtsim_render before dtsim_set_maps/dtsim_reset");
  if (!h->have_lut) return fail(DTSIM_E_STATE, "DTSIM_F_DISTORTION set but dtsim_set_distortion_lut was not called");
  if (int rc = check_renderable(h, "dtsim_render")) return rc;
  HIPCHK(hipSetDevice(h->cfg.device));
  RenderParams R{};
  R.N = h->N; R.W = h->cfg.cam_width; R.H = h->cfg.cam_height;
  R.distortion = (h->cfg.flags & DTSIM_F_DISTORTION) ? 1 : 0;
  R.domain_rand = (h->cfg.flags & DTSIM_F_DOMAIN_RAND) ? 1 : 0;
  R.frames = h->n_cal ? h->d_scratch.get() : h->frames;   // camera_rand: the rectilinear frames, gathered into `frames` below
  R.lut = h->d_lut.get();
  R.segment = segment ? 1 : 0; R.mesh_seg = h->d_mesh_seg.get();
  render_scene(h, segment, &R);
  render_scratch(h, R.max_tris, &R);                     // (its typed records are h->recs, kept since dtsim_create: the ENV and PIX slabs do not move)
  R.light = ((h->cfg.flags & DTSIM_F_LIGHT_CAPTURE) && !R.domain_rand) ? 1 : 0;   // (the per-env camera path lights from EnvCam anyway)
  if (flags & DTSIM_RENDER_GL_FILTER) R.qtex = nullptr;   // no quad records: the generic raster (llvmpipe's GL_LINEAR arithmetic) takes the pass
  const int pipe = dt_raster_pipe(R, h->maps.grid_rows, h->maps.grid_cols, h->raster_old);
  {
    ProfScope ps(h, DTSIM_KERNEL_RENDER);
    h->render_tables = dt_launch_render(h->stream, h->A, R, h->recs, pipe, h->render_tables, mask);
    h->render_pipe = pipe | (R.light ? DTSIM_PIPE_ENV_LIGHT : 0);
    if (h->n_cal) dt_launch_remap_cal(h->stream, h->d_scratch.get(), h->frames, h->d_cal_src.get(), h->d_env_cal.get(), mask, h->N, R.W, R.H);
  }
  HIPCHK(hipGetLastError());
  h->rendered = true; h->last_R = R; h->last_segment = segment; h->leds_ok = true; h->masked = mask != nullptr;
  return DTSIM_OK;
}

// The shared body of dtsim_draw_lines / dtsim_draw_leds: `n` host records of `width` floats, grouped by env_idx (null: all env 0), are
// uploaded into the handle's buffer `buf` (capacity `cap`, in records; grown to at least min_cap) and drawn onto the frames with one
// `launch` per env that has records.  prepare(h, &R): the entry point's own state precondition -- false refuses the call, `need` says
// why -- and the RenderParams of its launches.
static int overlay_run(dtsim_t* h, const char* who, const float* recs, int width, const int32_t* env_idx, int n, DevPtr<float> dtsim::*buf,
                       int dtsim::*cap, int min_cap, const char* need, bool (*prepare)(const dtsim*, RenderParams*),
                       void (*launch)(hipStream_t, const RenderParams&, const float*, int first, int count, int env)) {
  if (!h || (n > 0 && !recs)) return fail(DTSIM_E_INVALID, "%s: null argument", who);
  if (n < 0) return fail(DTSIM_E_INVALID, "%s: n = %d", who, n);
  if (!h->frames) return fail(DTSIM_E_STATE, "%s: handle created without DTSIM_F_RENDER", who);
  if (int rc = check_renderable(h, who)) return rc;
  RenderParams R{};
  if (!prepare(h, &R)) return fail(DTSIM_E_STATE, "%s %s", who, need);
  if (h->masked) return fail(DTSIM_E_STATE, "%s after dtsim_render_masked: the post-passes need a full dtsim_render", who);
  if (h->n_cal) return fail(DTSIM_E_STATE, "%s with per-env distortion tables installed (the overlays read the single table)", who);
  if (n == 0) return DTSIM_OK;
  for (int i = 0; i < n; ++i) {
    const int e = env_idx ? env_idx[i] : 0;
    if (e < 0 || e >= h->N) return fail(DTSIM_E_INVALID, "%s: env_idx[%d] = %d out of range [0, %d)", who, i, e, h->N);
    if (env_idx && i && env_idx[i] < env_idx[i - 1]) return fail(DTSIM_E_INVALID, "%s: env_idx must be non-decreasing (records grouped by env, in draw order)", who);
  }
  HIPCHK(hipSetDevice(h->cfg.device));
  if (h->*cap < n) {
    const int grown = std::max(n, min_cap);
    HIPCHK(dev_grow(h->*buf, width * (size_t)grown, h->stream));
    h->*cap = grown;
  }
  float* d_recs = (h->*buf).get();
  HIPCHK(hipMemcpyAsync(d_recs, recs, sizeof(float) * width * (size_t)n, hipMemcpyHostToDevice, h->stream));
  int i0 = 0;
  while (i0 < n) {                                    // one launch per env that has records
    const int e = env_idx ? env_idx[i0] : 0;
    int i1 = i0;
    while (i1 < n && (env_idx ? env_idx[i1] : 0) == e) ++i1;
    launch(h->stream, R, d_recs, i0, i1 - i0, e);
    i0 = i1;
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));           // `recs` is pageable host memory: the copy must have left it
  return DTSIM_OK;
}

int dtsim_draw_lines(dtsim_t* h, const float* lines, const int32_t* env_idx, int n) {
  return overlay_run(h, "dtsim_draw_lines", lines, 9, env_idx, n, &dtsim::d_lines, &dtsim::lines_cap, 1024,
                     "before the first dtsim_render (the pass writes the cameras the lines go through)",
                     [](const dtsim* h, RenderParams* R) {
                       if (!h->have_maps || !h->have_reset || !h->have_lut || !h->rendered) return false;
                       R->N = h->N; R->W = h->cfg.cam_width; R->H = h->cfg.cam_height; R->frames = h->frames; R->lut = h->d_lut.get();
                       render_scratch(h, 0, R);      // (the overlays read the EnvCam records the pass wrote)
                       return true;
                     }, dt_launch_overlay_lines);
}

int dtsim_draw_leds(dtsim_t* h, const float* spheres, const int32_t* env_idx, int n) {
  return overlay_run(h, "dtsim_draw_leds", spheres, 8, env_idx, n, &dtsim::d_leds, &dtsim::leds_cap, 256,
                     "needs a preceding dtsim_render (colour view): it tests the spheres against that pass's scene",
                     [](const dtsim* h, RenderParams* R) {
                       if (!h->rendered || !h->leds_ok || h->last_segment) return false;
                       *R = h->last_R;
                       R->frames = h->frames;        // (dtsim_bind_frames may have moved the output since the pass)
                       return true;
                     }, dt_launch_overlay_leds);
}

// The checks dtsim_depth, dtsim_labels and their masked forms share: the arguments (flags: only the bits of `allowed`), then the state -- a
// colour pass of the current state whose cameras and projected triangles the post-pass reads.  masked: the masked form (its device mask must be given).
// Per-env distortion tables: refused unless the caller asked for them with DTSIM_MAP_ENV_TABLES (every entry point allows that bit).
static int map_pass_check(dtsim_t* h, const char* who, const void* out, int oh, int ow, uint32_t flags, uint32_t allowed, bool masked, const uint8_t* mask) {
  if (!h || !out || (masked && !mask)) return fail(DTSIM_E_INVALID, "%s: null argument", who);
  if (flags & ~(allowed | (uint32_t)DTSIM_MAP_ENV_TABLES)) return fail(DTSIM_E_INVALID, "%s: unknown flags 0x%x", who, flags);
  const int W = h->cfg.cam_width, H = h->cfg.cam_height;
  if (oh <= 0 || ow <= 0 || H % oh || W % ow)
    return fail(DTSIM_E_INVALID, "%s: a %d x %d map of %d x %d frames (the map is point-sampled: each size must divide the camera's)", who, ow, oh, W, H);
  if (!h->frames) return fail(DTSIM_E_STATE, "handle created without DTSIM_F_RENDER");
  if (int rc = check_renderable(h, who)) return rc;
  if (!h->rendered || !h->leds_ok || h->last_segment)
    return fail(DTSIM_E_STATE, "%s needs a preceding dtsim_render (colour view) of the current state: it reads that pass's cameras and projected triangles", who);
  // the masked pass of the quad-record pipelines writes neither the camera (k_cam_setup) nor the triangles (k_obj_setup) of an unselected env
  if (h->masked && !masked) return fail(DTSIM_E_STATE, "%s after dtsim_render_masked: only the masked form, with the pass's mask", who);
  if (h->n_cal && !(flags & DTSIM_MAP_ENV_TABLES))
    return fail(DTSIM_E_STATE, "%s with per-env distortion tables installed (without DTSIM_MAP_ENV_TABLES it reads the single table)", who);
  return DTSIM_OK;
}

// The per-env tables a camera post-pass reads: the installed ones when the call asked for them (DTSIM_MAP_ENV_TABLES), else none -- the flag
// without installed tables changes nothing.
struct EnvTables { const int32_t *src, *env_cal; int n; };
static EnvTables env_tables(const dtsim* h, uint32_t flags) {
  if (!(flags & DTSIM_MAP_ENV_TABLES) || !h->n_cal) return EnvTables{nullptr, nullptr, 0};
  return EnvTables{h->d_cal_src.get(), h->d_env_cal.get(), h->n_cal};
}

// The shared body of the camera post-passes -- dtsim_depth, dtsim_labels, dtsim_instances and their masked forms: map_pass_check with `out`,
// the output the entry point cannot do without; the label tables where the launch reads them (`tables`: how the refusal reads, null when
// it reads none); then `launch`.
extern "C++" {
template <class Launch>
static int map_pass_run(dtsim_t* h, const char* who, const void* out, int oh, int ow, uint32_t flags, uint32_t allowed, bool masked,
                        const uint8_t* mask, const char* tables, Launch launch) {
  if (int rc = map_pass_check(h, who, out, oh, ow, flags, allowed, masked, mask)) return rc;
  if (tables && (!h->d_texel_class || !h->d_mesh_class)) return fail(DTSIM_E_STATE, "%s %s", who, tables);
  HIPCHK(hipSetDevice(h->cfg.device));
  launch();
  HIPCHK(hipGetLastError());
  return DTSIM_OK;
}
}  // extern "C++"

static void depth_launch(const dtsim* h, void* out, int oh, int ow, uint32_t flags, const uint8_t* mask) {
  const EnvTables t = env_tables(h, flags);
  dt_launch_depth(h->stream, h->last_R, out, oh, ow, (flags & DTSIM_DEPTH_F16) != 0, mask, t.src, t.env_cal, t.n);
}

int dtsim_depth(dtsim_t* h, void* out, int oh, int ow, uint32_t flags) {
  return map_pass_run(h, "dtsim_depth", out, oh, ow, flags, (uint32_t)DTSIM_DEPTH_F16, false, nullptr, nullptr,
                      [=] { depth_launch(h, out, oh, ow, flags, nullptr); });
}
int dtsim_depth_masked(dtsim_t* h, void* out, int oh, int ow, uint32_t flags, const uint8_t* mask) {
  return map_pass_run(h, "dtsim_depth_masked", out, oh, ow, flags, (uint32_t)DTSIM_DEPTH_F16, true, mask, nullptr,
                      [=] { depth_launch(h, out, oh, ow, flags, mask); });
}

// (one kernel classifies for dtsim_labels and dtsim_instances: it fills whichever of the two maps is given)
static void labels_launch(const dtsim* h, uint8_t* labels, uint8_t* inst, int oh, int ow, uint32_t flags, const uint8_t* mask) {
  const EnvTables t = env_tables(h, flags);
  dt_launch_labels(h->stream, h->last_R, h->d_texel_class.get(), h->d_mesh_class.get(), h->n_mesh_class, labels, inst, oh, ow, mask, t.src, t.env_cal,
                   t.n);
}

int dtsim_labels(dtsim_t* h, uint8_t* out, int oh, int ow, uint32_t flags) {
  return map_pass_run(h, "dtsim_labels", out, oh, ow, flags, 0u, false, nullptr, "before dtsim_set_label_assets",
                      [=] { labels_launch(h, out, nullptr, oh, ow, flags, nullptr); });
}
int dtsim_labels_masked(dtsim_t* h, uint8_t* out, int oh, int ow, uint32_t flags, const uint8_t* mask) {
  return map_pass_run(h, "dtsim_labels_masked", out, oh, ow, flags, 0u, true, mask, "before dtsim_set_label_assets",
                      [=] { labels_launch(h, out, nullptr, oh, ow, flags, mask); });
}

// (the label tables only when a label map is asked for too)
int dtsim_instances(dtsim_t* h, uint8_t* inst, uint8_t* labels, int oh, int ow, uint32_t flags) {
  return map_pass_run(h, "dtsim_instances", inst, oh, ow, flags, 0u, false, nullptr, labels ? "with a label map before dtsim_set_label_assets" : nullptr,
                      [=] { labels_launch(h, labels, inst, oh, ow, flags, nullptr); });
}
int dtsim_instances_masked(dtsim_t* h, uint8_t* inst, uint8_t* labels, int oh, int ow, uint32_t flags, const uint8_t* mask) {
  return map_pass_run(h, "dtsim_instances_masked", inst, oh, ow, flags, 0u, true, mask, labels ? "with a label map before dtsim_set_label_assets" : nullptr,
                      [=] { labels_launch(h, labels, inst, oh, ow, flags, mask); });
}

// The handle's FlowMark and FlowRec arrays, allocated at the first use; the marks start as "none".
static int flow_buffers(dtsim_t* h) {
  if (h->d_flow_mark && h->d_flow_rec) return DTSIM_OK;
  DevPtr<FlowMark> marks;
  DevPtr<FlowRec> recs;
  HIPCHK(dev_alloc(marks, (size_t)h->N));
  HIPCHK(dev_alloc(recs, (size_t)h->N));
  HIPCHK(hipMemsetAsync(marks.get(), 0, sizeof(FlowMark) * (size_t)h->N, h->stream));
  HIPCHK(hipMemsetAsync(recs.get(), 0, sizeof(FlowRec) * (size_t)h->N, h->stream));
  h->d_flow_mark = std::move(marks); h->d_flow_rec = std::move(recs);
  return DTSIM_OK;
}

int dtsim_flow_mark(dtsim_t* h, const uint8_t* mask) {
  if (!h) return fail(DTSIM_E_INVALID, "dtsim_flow_mark: null handle");
  if (!h->have_maps || !h->have_reset) return fail(DTSIM_E_STATE, "dtsim_flow_mark before dtsim_set_maps and dtsim_reset: there is no state to remember");
  HIPCHK(hipSetDevice(h->cfg.device));
  if (int rc = flow_buffers(h)) return rc;
  dt_launch_flow_mark(h->stream, h->A, h->d_flow_mark.get(), mask);
  HIPCHK(hipGetLastError());
  return DTSIM_OK;
}

// dtsim_flow and its masked form: dtsim_depth's checks (map_pass_check) with no flag allowed, then the calibration a fisheye handle needs.
static int flow_run(dtsim_t* h, const char* who, float* flow, uint8_t* valid, int oh, int ow, uint32_t flags, bool masked, const uint8_t* mask) {
  if (!h || !flow || (masked && !mask)) return fail(DTSIM_E_INVALID, "%s: null argument", who);
  if (flags) return fail(DTSIM_E_INVALID, "%s: flags 0x%x (must be 0)", who, flags);
  if ((const void*)flow == (const void*)valid) return fail(DTSIM_E_INVALID, "%s: flow and valid are one buffer", who);
  if (int rc = map_pass_check(h, who, flow, oh, ow, 0u, 0u, masked, mask)) return rc;
  if (h->lut_fisheye && h->n_ipm_cal < 1)
    return fail(DTSIM_E_STATE, "%s on fisheye frames before dtsim_set_ipm_calibrations (the flow goes through the calibration's forward model)", who);
  HIPCHK(hipSetDevice(h->cfg.device));
  if (int rc = flow_buffers(h)) return rc;
  dt_launch_flow(h->stream, h->last_R, h->A, h->d_flow_mark.get(), h->d_flow_rec.get(), (h->cfg.flags & DTSIM_F_DOMAIN_RAND) != 0,
                 h->lut_fisheye ? h->d_ipm_cal.get() : nullptr, flow, valid, oh, ow, mask);
  HIPCHK(hipGetLastError());
  return DTSIM_OK;
}
int dtsim_flow(dtsim_t* h, float* flow, uint8_t* valid, int oh, int ow, uint32_t flags) {
  return flow_run(h, "dtsim_flow", flow, valid, oh, ow, flags, false, nullptr);
}
int dtsim_flow_masked(dtsim_t* h, float* flow, uint8_t* valid, int oh, int ow, uint32_t flags, const uint8_t* mask) {
  return flow_run(h, "dtsim_flow_masked", flow, valid, oh, ow, flags, true, mask);
}

// dtsim_camera_maps and its masked form: the argument checks of its own (which outputs, that they do not overlap), dtsim_depth's checks
// (map_pass_check), the label tables with `labels`, and with `flow` everything dtsim_flow refuses -- installed per-env tables whatever the
// flags say, a fisheye handle without its calibration -- plus a handle no dtsim_flow_mark has been called on.
static int camera_maps_run(dtsim_t* h, const char* who, const dtsim_camera_maps_out* out, int oh, int ow, uint32_t flags, bool masked,
                           const uint8_t* mask) {
  if (!h || !out || (masked && !mask)) return fail(DTSIM_E_INVALID, "%s: null argument", who);
  if (!out->depth && !out->labels && !out->instances && !out->flow && !out->flow_valid) return fail(DTSIM_E_INVALID, "%s: no output", who);
  if (out->flow_valid && !out->flow) return fail(DTSIM_E_INVALID, "%s: flow_valid without flow", who);
  if (oh > 0 && ow > 0) {                              // (a bad size is map_pass_check's to name)
    const size_t px = (size_t)h->N * (size_t)oh * (size_t)ow;
    const struct { const void* p; size_t bytes; } span[5] = {{out->depth, px * ((flags & DTSIM_DEPTH_F16) ? 2 : 4)}, {out->labels, px},
                                                             {out->instances, px}, {out->flow, px * 8}, {out->flow_valid, px}};
    for (int a = 0; a < 5; ++a)
      for (int b = a + 1; b < 5; ++b) {
        const uintptr_t pa = (uintptr_t)span[a].p, pb = (uintptr_t)span[b].p;
        if (pa && pb && pa < pb + span[b].bytes && pb < pa + span[a].bytes) return fail(DTSIM_E_INVALID, "%s: outputs %d and %d overlap", who, a, b);
      }
  }
  const void* any = out->depth ? out->depth : out->labels ? (const void*)out->labels : out->instances ? (const void*)out->instances : (const void*)out->flow;
  if (out->flow && h->n_cal)                           // (dtsim_flow's refusal and code; DTSIM_MAP_ENV_TABLES does not lift it)
    flags &= ~(uint32_t)DTSIM_MAP_ENV_TABLES;
  if (int rc = map_pass_check(h, who, any, oh, ow, flags, (uint32_t)DTSIM_DEPTH_F16, masked, mask)) return rc;
  if (out->labels && (!h->d_texel_class || !h->d_mesh_class)) return fail(DTSIM_E_STATE, "%s with a label map before dtsim_set_label_assets", who);
  if (out->flow) {
    if (h->lut_fisheye && h->n_ipm_cal < 1)
      return fail(DTSIM_E_STATE, "%s with flow on fisheye frames before dtsim_set_ipm_calibrations (the flow goes through the calibration's forward model)", who);
    if (!h->d_flow_mark || !h->d_flow_rec) return fail(DTSIM_E_STATE, "%s with flow before the first dtsim_flow_mark", who);
  }
  HIPCHK(hipSetDevice(h->cfg.device));
  const EnvTables t = env_tables(h, flags);
  if (out->flow)
    dt_launch_flow_setup(h->stream, h->last_R, h->A, h->d_flow_mark.get(), h->d_flow_rec.get(), (h->cfg.flags & DTSIM_F_DOMAIN_RAND) != 0, mask);
  {
    ProfScope ps(h, DTSIM_KERNEL_CAMERA_MAPS);
    const CameraMapsOut o{out->depth, (flags & DTSIM_DEPTH_F16) != 0, out->labels, out->instances, out->flow, out->flow_valid};
    dt_launch_camera_maps(h->stream, h->last_R, o, h->d_texel_class.get(), h->d_mesh_class.get(), h->n_mesh_class, h->d_flow_rec.get(),
                          h->lut_fisheye ? h->d_ipm_cal.get() : nullptr, oh, ow, mask, t.src, t.env_cal, t.n);
  }
  HIPCHK(hipGetLastError());
  return DTSIM_OK;
}
int dtsim_camera_maps(dtsim_t* h, const dtsim_camera_maps_out* out, int oh, int ow, uint32_t flags) {
  return camera_maps_run(h, "dtsim_camera_maps", out, oh, ow, flags, false, nullptr);
}
int dtsim_camera_maps_masked(dtsim_t* h, const dtsim_camera_maps_out* out, int oh, int ow, uint32_t flags, const uint8_t* mask) {
  return camera_maps_run(h, "dtsim_camera_maps_masked", out, oh, ow, flags, true, mask);
}

int dtsim_boxes(dtsim_t* h, const uint8_t* inst, int oh, int ow, int32_t* out, uint32_t flags, const uint8_t* mask) {
  if (!h || !inst || !out) return fail(DTSIM_E_INVALID, "dtsim_boxes: null argument");
  if (flags) return fail(DTSIM_E_INVALID, "dtsim_boxes: unknown flags 0x%x", flags);
  if (oh <= 0 || ow <= 0 || (int64_t)oh * ow > INT32_MAX) return fail(DTSIM_E_INVALID, "dtsim_boxes: a %d x %d map", ow, oh);
  HIPCHK(hipSetDevice(h->cfg.device));
  dt_launch_boxes(h->stream, h->N, inst, oh, ow, out, mask);
  HIPCHK(hipGetLastError());
  return DTSIM_OK;
}

int dtsim_bev(dtsim_t* h, uint8_t* cls, uint8_t* inst, int oh, int ow, double cell, int rows_behind, uint32_t flags, const uint8_t* mask) {
  if (!h || (!cls && !inst)) return fail(DTSIM_E_INVALID, "dtsim_bev: null argument");
  if (cls == inst) return fail(DTSIM_E_INVALID, "dtsim_bev: cls and inst are one buffer");
  if (flags) return fail(DTSIM_E_INVALID, "dtsim_bev: unknown flags 0x%x", flags);
  if (oh < 1 || ow < 1 || oh > DTSIM_BEV_MAX_SIDE || ow > DTSIM_BEV_MAX_SIDE)
    return fail(DTSIM_E_INVALID, "dtsim_bev: a %d x %d map (each size 1 .. %d)", ow, oh, DTSIM_BEV_MAX_SIDE);
  if (!std::isfinite(cell) || !(cell > 0.0)) return fail(DTSIM_E_INVALID, "dtsim_bev: cell %g (metres per cell: finite, > 0)", cell);
  if (rows_behind < 0 || rows_behind > oh) return fail(DTSIM_E_INVALID, "dtsim_bev: rows_behind %d outside [0, %d]", rows_behind, oh);
  // the render tables: the tile records, the object instances and the texel pool the class pool mirrors (no pass of the raster is needed)
  if (!h->frames || !h->have_maps || !h->maps.renderable || !h->maps.d_rmaps || !h->maps.d_tilerecs || !h->maps.d_robjs || !h->maps.d_ocorners)
    return fail(DTSIM_E_INVALID, "dtsim_bev: the handle holds no render tables (DTSIM_F_RENDER, dtsim_set_assets, then dtsim_set_maps)");
  if (cls && (!h->d_texel_class || !h->d_mesh_class)) return fail(DTSIM_E_INVALID, "dtsim_bev with a class map before dtsim_set_label_assets");
  HIPCHK(hipSetDevice(h->cfg.device));
  RenderParams R{};
  R.N = h->N;
  render_scene(h, false, &R);
  dt_launch_bev(h->stream, R, h->A, h->maps.d_ocorners.get(), h->d_texel_class.get(), h->d_mesh_class.get(), h->n_mesh_class, cls, inst, oh, ow, cell,
                rows_behind, mask);
  HIPCHK(hipGetLastError());
  return DTSIM_OK;
}

int dtsim_set_ipm_calibrations(dtsim_t* h, int n_cal, const double* K, const double* D, const double* new_K, const int32_t* env_cal) {
  if (!h) return fail(DTSIM_E_INVALID, "dtsim_set_ipm_calibrations: null handle");
  if (n_cal < 0) return fail(DTSIM_E_INVALID, "dtsim_set_ipm_calibrations: n_cal %d", n_cal);
  if (n_cal == 0 && (K || D || new_K || env_cal)) return fail(DTSIM_E_INVALID, "dtsim_set_ipm_calibrations: n_cal = 0 takes no tables");
  if (n_cal > 0 && (!K || !D || !new_K)) return fail(DTSIM_E_INVALID, "dtsim_set_ipm_calibrations: null K, D or new_K");
  if (n_cal > 1 && !env_cal) return fail(DTSIM_E_INVALID, "dtsim_set_ipm_calibrations: %d calibrations need env_cal", n_cal);
  if (!h->frames) return fail(DTSIM_E_STATE, "dtsim_set_ipm_calibrations: handle created without DTSIM_F_RENDER");
  std::vector<IpmCal> cals((size_t)n_cal);
  for (int i = 0; i < n_cal; ++i)
    if (!dt_ipm_pack_cal(cals[i], K + 9 * (size_t)i, D + 5 * (size_t)i, new_K + 9 * (size_t)i))
      return fail(DTSIM_E_INVALID, "dtsim_set_ipm_calibrations: calibration %d holds a value that is not finite, or its new_K has no inverse", i);
  if (env_cal)
    for (int e = 0; e < h->N; ++e)
      if (env_cal[e] < 0 || env_cal[e] >= n_cal) return fail(DTSIM_E_INVALID, "dtsim_set_ipm_calibrations: env_cal[%d] = %d outside [0, %d)", e, env_cal[e], n_cal);
  HIPCHK(hipSetDevice(h->cfg.device));
  DevPtr<IpmCal> d_cal;
  DevPtr<int32_t> d_env;
  if (n_cal) HIPCHK(dev_upload(d_cal, cals.data(), cals.size()));
  if (env_cal) HIPCHK(dev_upload(d_env, env_cal, (size_t)h->N));
  HIPCHK(hipStreamSynchronize(h->stream));           // the stream may still read the old tables
  h->d_ipm_cal = std::move(d_cal); h->d_ipm_env_cal = std::move(d_env);
  h->n_ipm_cal = n_cal;
  ++h->ipm_cal_version;
  return DTSIM_OK;
}

int dtsim_ipm(dtsim_t* h, uint8_t* img, uint8_t* valid, int32_t* src, int oh, int ow, double cell, int rows_behind, uint32_t flags,
              const uint8_t* mask) {
  if (!h || (!img && !valid && !src)) return fail(DTSIM_E_INVALID, "dtsim_ipm: null argument");
  const void *pi = img, *pv = valid, *ps = src;
  if ((pi && (pi == pv || pi == ps)) || (pv && pv == ps)) return fail(DTSIM_E_INVALID, "dtsim_ipm: two outputs are one buffer");
  if (flags & ~(uint32_t)DTSIM_IPM_CHW) return fail(DTSIM_E_INVALID, "dtsim_ipm: unknown flags 0x%x", flags);
  if (oh < 1 || ow < 1 || oh > DTSIM_BEV_MAX_SIDE || ow > DTSIM_BEV_MAX_SIDE)
    return fail(DTSIM_E_INVALID, "dtsim_ipm: a %d x %d map (each size 1 .. %d)", ow, oh, DTSIM_BEV_MAX_SIDE);
  if (!std::isfinite(cell) || !(cell > 0.0)) return fail(DTSIM_E_INVALID, "dtsim_ipm: cell %g (metres per cell: finite, > 0)", cell);
  if (rows_behind < 0 || rows_behind > oh) return fail(DTSIM_E_INVALID, "dtsim_ipm: rows_behind %d outside [0, %d]", rows_behind, oh);
  if (!h->frames) return fail(DTSIM_E_STATE, "dtsim_ipm: handle created without DTSIM_F_RENDER");
  if (!h->have_reset) return fail(DTSIM_E_STATE, "dtsim_ipm before dtsim_reset");
  HIPCHK(hipSetDevice(h->cfg.device));
  IpmArgs a{};
  a.frames = h->frames; a.N = h->N; a.W = h->cfg.cam_width; a.H = h->cfg.cam_height;
  a.img = img; a.valid = valid; a.src = src; a.oh = oh; a.ow = ow; a.cell = cell; a.rows_behind = rows_behind;
  a.chw = (flags & DTSIM_IPM_CHW) != 0; a.mask = mask;
  const bool per_env = (h->cfg.flags & DTSIM_F_DOMAIN_RAND) != 0;
  if (!per_env && h->n_ipm_cal <= 1) {               // the shared camera is rigid in the agent's frame: one table for every env and step
    if (!h->d_ipm_table) HIPCHK(dev_alloc(h->d_ipm_table, (size_t)DTSIM_BEV_MAX_SIDE * DTSIM_BEV_MAX_SIDE));
    dtsim::IpmKey& k = h->ipm_key;
    if (k.cal != h->ipm_cal_version || k.oh != oh || k.ow != ow || k.rows_behind != rows_behind || k.cell != cell) {
      dt_launch_ipm_table(h->stream, h->d_ipm_table.get(), h->d_ipm_cal.get(), a.W, a.H, oh, ow, cell, rows_behind);
      k.cal = h->ipm_cal_version; k.oh = oh; k.ow = ow; k.rows_behind = rows_behind; k.cell = cell;
    }
    dt_launch_ipm_gather(h->stream, a, h->d_ipm_table.get());
  } else {
    dt_launch_ipm_env(h->stream, a, h->A, per_env, h->d_ipm_cal.get(), h->n_ipm_cal, h->d_ipm_env_cal.get());
  }
  HIPCHK(hipGetLastError());
  return DTSIM_OK;
}

void* dtsim_frames_devptr(dtsim_t* h) { return h ? h->frames : nullptr; }
size_t dtsim_frames_bytes(const dtsim_t* h) { return h ? h->frames_bytes : 0; }

int dtsim_bind_frames(dtsim_t* h, void* devptr) {
  if (!h) return fail(DTSIM_E_INVALID, "null handle");
  if (!h->frames_own) return fail(DTSIM_E_STATE, "handle created without DTSIM_F_RENDER");
  h->frames = devptr ? (uint8_t*)devptr : h->frames_own.get();
  return DTSIM_OK;
}

// ---- RCCL all-gather of the frame batch (include/dtsim.h) ---------------------------------
// librccl is resolved at first use: the product path of a single GPU never loads it.
namespace {
typedef int (*nccl_allgather_fn)(const void*, void*, size_t, int /*ncclDataType_t*/, void* /*ncclComm_t*/, hipStream_t);
typedef const char* (*nccl_errstr_fn)(int);
nccl_allgather_fn g_nccl_allgather = nullptr;
nccl_errstr_fn g_nccl_errstr = nullptr;
std::once_flag g_nccl_once;
std::string g_nccl_why;                               // why the library / symbol could not be had (kept: dlerror() is one-shot)
void resolve_rccl() {
  std::call_once(g_nccl_once, [] {
    void* lib = nullptr;
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);    // (the process's own copy when torch already loaded it)
      if (lib) break;
      if (const char* e = dlerror()) g_nccl_why = e;
    }
    if (!lib) return;
    g_nccl_allgather = reinterpret_cast<nccl_allgather_fn>(dlsym(lib, "ncclAllGather"));
    g_nccl_errstr = reinterpret_cast<nccl_errstr_fn>(dlsym(lib, "ncclGetErrorString"));
    if (!g_nccl_allgather) { const char* e = dlerror(); g_nccl_why = e ? e : "ncclAllGather not exported"; }
  });
}
}  // namespace

int dtsim_allgather_frames(dtsim_t* h, void* nccl_comm, void* recv, const void* send, size_t send_bytes) {
  if (!h || !nccl_comm || !recv) return fail(DTSIM_E_INVALID, "bad argument");
  if (!send) {
    if (!h->frames) return fail(DTSIM_E_STATE, "handle created without DTSIM_F_RENDER");
    send = h->frames;
    send_bytes = dtsim_frames_bytes(h);
  }
  if (send_bytes == 0) return fail(DTSIM_E_INVALID, "empty send buffer");
  resolve_rccl();
  if (!g_nccl_allgather)
    return fail(DTSIM_E_STATE, "librccl.so (ncclAllGather) could not be loaded: %s", g_nccl_why.empty() ? "library or symbol not found" : g_nccl_why.c_str());
  HIPCHK(hipSetDevice(h->cfg.device));
  const int rc = g_nccl_allgather(send, recv, send_bytes, /*ncclUint8*/ 1, nccl_comm, h->stream);
  if (rc != 0) return fail(DTSIM_E_HIP, "ncclAllGather: %s", g_nccl_errstr ? g_nccl_errstr(rc) : "error");
  return DTSIM_OK;
}

// The shared body of the four observation entry points.  cubic: dtsim_observe_cubic's tables (first_x / taps_x / first_y / taps_y, four taps)
// into h->obsc, else dtsim_observe's into h->obs; mask: the masked forms' device mask, or null for every env.
static int observe_run(dtsim_t* h, bool cubic, void* out, int out_h, int out_w, int flags, const uint8_t* mask,
                       const int32_t* bounds_x, const int32_t* taps_x, int ksize_x, const int32_t* bounds_y, const int32_t* taps_y, int ksize_y) {
  if (!h || !out) return fail(DTSIM_E_INVALID, "bad argument");
  if (!h->frames) return fail(DTSIM_E_STATE, "handle created without DTSIM_F_RENDER");
  const int W = h->cfg.cam_width, H = h->cfg.cam_height;
  ObserveSlot& slot = cubic ? h->obsc : h->obs;
  ObservePlan next;
  std::string err;
  int rc = cubic ? dt_observe_pack_cubic(next, err, W, H, h->N, out_h, out_w, bounds_x, taps_x, bounds_y, taps_y)
                 : dt_observe_pack(next, err, W, H, h->N, out_h, out_w, bounds_x, taps_x, ksize_x, bounds_y, taps_y, ksize_y);
  if (rc != DTSIM_OK) return fail(rc, "%s", err.c_str());
  HIPCHK(hipSetDevice(h->cfg.device));
  if (!slot.d_tab || !next.same_tables(slot.plan)) {
    // other tables than the slot's (the same output size may come with other tables): plan them -- the A/B switches are read here,
    // once per plan -- and replace the slot only when all of it succeeded
    rc = cubic ? dt_observe_plan_cubic(next, err)
               : dt_observe_plan(next, err, getenv("DTSIM_OBSERVE_STAGED") != nullptr, getenv("DTSIM_OBSERVE_GENERIC") != nullptr);
    if (rc != DTSIM_OK) return fail(rc, "%s", err.c_str());
    HIPCHK(hipStreamSynchronize(h->stream));         // the stream may still read the old tables
    HIPCHK(dev_upload(slot.d_tab, next.tab.data(), next.tab.size()));
    slot.plan = std::move(next);
  }
  const ObservePlan& plan = slot.plan;
  ObserveParams P = plan.P;
  P.chw = (flags & DTSIM_OBS_CHW) ? 1 : 0; P.f32 = (flags & DTSIM_OBS_F32) ? 1 : 0;
  P.frames = h->frames; P.out = out;
  const int32_t* tab = slot.d_tab.get();
  P.bx = tab + plan.off_bx; P.kkx = tab + plan.off_kkx; P.by = tab + plan.off_by; P.kky = tab + plan.off_kky;
  {
    ProfScope ps(h, DTSIM_KERNEL_OBSERVE);
    dt_launch_observe(h->stream, plan, P, mask);
  }
  HIPCHK(hipGetLastError());
  return DTSIM_OK;
}

int dtsim_observe(dtsim_t* h, void* out, int out_h, int out_w, int flags,
                  const int32_t* bounds_x, const int32_t* taps_x, int ksize_x,
                  const int32_t* bounds_y, const int32_t* taps_y, int ksize_y) {
  return observe_run(h, false, out, out_h, out_w, flags, nullptr, bounds_x, taps_x, ksize_x, bounds_y, taps_y, ksize_y);
}
int dtsim_observe_masked(dtsim_t* h, void* out, int out_h, int out_w, int flags, const uint8_t* mask,
                         const int32_t* bounds_x, const int32_t* taps_x, int ksize_x,
                         const int32_t* bounds_y, const int32_t* taps_y, int ksize_y) {
  if (!mask) return fail(DTSIM_E_INVALID, "dtsim_observe_masked: null mask");
  return observe_run(h, false, out, out_h, out_w, flags, mask, bounds_x, taps_x, ksize_x, bounds_y, taps_y, ksize_y);
}
int dtsim_observe_cubic(dtsim_t* h, void* out, int out_h, int out_w, int flags,
                        const int32_t* first_x, const int32_t* taps_x, const int32_t* first_y, const int32_t* taps_y) {
  return observe_run(h, true, out, out_h, out_w, flags, nullptr, first_x, taps_x, 4, first_y, taps_y, 4);
}
int dtsim_observe_cubic_masked(dtsim_t* h, void* out, int out_h, int out_w, int flags, const uint8_t* mask,
                               const int32_t* first_x, const int32_t* taps_x, const int32_t* first_y, const int32_t* taps_y) {
  if (!mask) return fail(DTSIM_E_INVALID, "dtsim_observe_cubic_masked: null mask");
  return observe_run(h, true, out, out_h, out_w, flags, mask, first_x, taps_x, 4, first_y, taps_y, 4);
}

int dtsim_copy_rows(dtsim_t* h, void* dst, const void* src, size_t row_bytes, const uint8_t* mask) {
  if (!h || !dst || !src || !mask) return fail(DTSIM_E_INVALID, "dtsim_copy_rows: null argument");
  if (row_bytes == 0) return DTSIM_OK;
  HIPCHK(hipSetDevice(h->cfg.device));
  dt_launch_copy_rows(h->stream, h->N, dst, src, row_bytes, mask);
  HIPCHK(hipGetLastError());
  return DTSIM_OK;
}

int dtsim_obs_push(dtsim_t* h, void* stack, const uint8_t* obs, int depth, int out_h, int out_w, int flags, const uint8_t* first, const uint8_t* mask) {
  if (!h || !stack || !obs) return fail(DTSIM_E_INVALID, "dtsim_obs_push: null argument");
  if (depth < 1 || depth > DTSIM_OBS_MAX_DEPTH) return fail(DTSIM_E_INVALID, "dtsim_obs_push: depth %d outside 1 .. %d", depth, DTSIM_OBS_MAX_DEPTH);
  if (out_h <= 0 || out_w <= 0) return fail(DTSIM_E_INVALID, "dtsim_obs_push: output size %dx%d", out_w, out_h);
  if (!(flags & DTSIM_OBS_CHW)) return fail(DTSIM_E_INVALID, "dtsim_obs_push: stacks are CHW (DTSIM_OBS_CHW)");
  if (flags & ~(DTSIM_OBS_CHW | DTSIM_OBS_F32 | DTSIM_OBS_GRAY)) return fail(DTSIM_E_INVALID, "dtsim_obs_push: unknown flags 0x%x", flags);
  HIPCHK(hipSetDevice(h->cfg.device));
  dt_launch_obs_push(h->stream, h->N, stack, obs, depth, out_h, out_w, (flags & DTSIM_OBS_F32) != 0, (flags & DTSIM_OBS_GRAY) != 0, first, mask);
  HIPCHK(hipGetLastError());
  return DTSIM_OK;
}

int dtsim_blend_frames(dtsim_t* h, void* out, const void* const* frames, const uint32_t* weights, int n, int flags, const uint8_t* mask) {
  if (!h || !out || !frames || !weights) return fail(DTSIM_E_INVALID, "dtsim_blend_frames: null argument");
  if (n < 1 || n > DTSIM_BLEND_MAX) return fail(DTSIM_E_INVALID, "dtsim_blend_frames: n = %d outside 1 .. %d", n, DTSIM_BLEND_MAX);
  if (flags & ~DTSIM_OBS_F32) return fail(DTSIM_E_INVALID, "dtsim_blend_frames: unknown flags 0x%x", flags);
  BlendArgs B{};
  B.n = n;
  uint32_t D = 0;
  for (int i = 0; i < n; ++i) {
    if (!frames[i]) return fail(DTSIM_E_INVALID, "dtsim_blend_frames: frames[%d] is null", i);
    if (weights[i] > 255u) return fail(DTSIM_E_INVALID, "dtsim_blend_frames: weights[%d] = %u above 255", i, weights[i]);
    B.f[i] = static_cast<const uint8_t*>(frames[i]); B.w[i] = weights[i];
    D += weights[i];
  }
  if (D < 1 || D > 256) return fail(DTSIM_E_INVALID, "dtsim_blend_frames: the weights sum to %u, outside 1 .. 256", D);
  if (!h->frames) return fail(DTSIM_E_STATE, "handle created without DTSIM_F_RENDER");
  HIPCHK(hipSetDevice(h->cfg.device));
  dt_launch_blend_frames(h->stream, h->N, out, B, (size_t)h->cfg.cam_height * h->cfg.cam_width * 3, (flags & DTSIM_OBS_F32) != 0, mask);
  HIPCHK(hipGetLastError());
  return DTSIM_OK;
}

int dtsim_query(dtsim_t* h, int n, const int32_t* env_idx, const double* poses, double safety_factor,
                dtsim_probe* out) {
  if (!h || n <= 0 || !env_idx || !poses || !out) return fail(DTSIM_E_INVALID, "bad argument");
  if (!h->have_maps || !h->have_reset) return fail(DTSIM_E_STATE, "dtsim_query before dtsim_set_maps/dtsim_reset");
  for (int i = 0; i < n; ++i)
    if (env_idx[i] < 0 || env_idx[i] >= h->N) return fail(DTSIM_E_INVALID, "env_idx[%d]=%d out of range", i, env_idx[i]);
  HIPCHK(hipSetDevice(h->cfg.device));
  if (n > h->q_cap) {
    const int cap = n < 256 ? 256 : n;
    HIPCHK(dev_grow(h->d_qenv, cap, h->stream));
    HIPCHK(dev_grow(h->d_qpose, 3 * (size_t)cap, h->stream));
    HIPCHK(dev_grow(h->d_qout, cap, h->stream));
    h->q_cap = cap;
  }
  HIPCHK(hipMemcpyAsync(h->d_qenv.get(), env_idx, sizeof(int32_t) * n, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->d_qpose.get(), poses, sizeof(double) * 3 * n, hipMemcpyHostToDevice, h->stream));
  {
    ProfScope ps(h, DTSIM_KERNEL_QUERY);
    dt_launch_query(h->stream, h->A, h->maps.M, step_params(h, 0), n, h->d_qenv.get(), h->d_qpose.get(), safety_factor, h->d_qout.get());
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, h->d_qout.get(), sizeof(dtsim_probe) * n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return DTSIM_OK;
}

// ---- field access -------------------------------------------------------------
namespace {
__global__ void k_agent_info(SimArrays A, int e, dtsim_agent_info* out) {
  const size_t N = A.N;
  dtsim_agent_info r;
  r.pos[0] = A.pos_x[e]; r.pos[1] = 0.0; r.pos[2] = A.pos_z[e];
  r.angle = A.angle[e]; r.speed = A.speed[e]; r.timestamp = A.timestamp[e];
  r.wheels[0] = A.wheels[e]; r.wheels[1] = A.wheels[N + e];
  for (int k = 0; k < 4; ++k) r.lane[k] = A.lane[(size_t)k * N + e];
  r.prox = A.prox[e]; r.reward = A.reward[e];
  r.tile[0] = A.tile_i[e]; r.tile[1] = A.tile_j[e]; r.step_count = A.step_count[e];
  r.in_lane = A.in_lane[e]; r.done = A.done[e]; r.done_code = A.done_code[e]; r.pad = 0;
  *out = r;
}

// dtsim_read / dtsim_write: a field of state_fields.h's table, one hipMemcpy per plane through the interleave of its public layout
int field_xfer(dtsim* h, int field, void* host, size_t bytes, bool to_host) {
  if (!h || !host) return fail(DTSIM_E_INVALID, "null argument");
  const StateField* f = dt_state_field(field);
  const size_t N = (size_t)h->N, need = f ? dt_field_bytes(*f, N, h->slab_bytes) : 0;
  if (need == 0) return fail(DTSIM_E_INVALID, "unknown field %d", field);
  if (bytes != need) return fail(DTSIM_E_INVALID, "field %d: %zu bytes given, %zu expected", field, bytes, need);
  hipError_t e0 = hipSetDevice(h->cfg.device);
  if (e0 == hipSuccess) e0 = hipStreamSynchronize(h->stream);
  if (e0 != hipSuccess) return fail(DTSIM_E_HIP, "sync: %s", hipGetErrorString(e0));
  if (!to_host && !f->writable) return fail(DTSIM_E_INVALID, "%s is read-only", f->name);
  switch (field) {                                    // what is no view of the slab's arrays
    case DTSIM_FIELD_STATE_BLOB: {
      hipError_t e = to_host ? hipMemcpy(host, h->slab.get(), need, hipMemcpyDeviceToHost)
                             : hipMemcpy(h->slab.get(), host, need, hipMemcpyHostToDevice);
      if (e != hipSuccess) return fail(DTSIM_E_HIP, "hipMemcpy blob: %s", hipGetErrorString(e));
      return DTSIM_OK;
    }
    case DTSIM_FIELD_RENDER_PIPE: {
      int32_t* out = static_cast<int32_t*>(host);
      for (size_t i = 0; i < N; ++i) out[i] = (int32_t)h->render_pipe;
      return DTSIM_OK;
    }
    case DTSIM_FIELD_RENDER_POS: {                    // the identity until a render pass ran in k_env_sort's order
      int32_t* out = static_cast<int32_t*>(host);
      if (h->render_tables & 4) {
        RenderParams R{}; render_scratch(h, 0, &R);
        hipError_t e = hipMemcpy(out, R.envpos, N * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return fail(DTSIM_E_HIP, "hipMemcpy render order: %s", hipGetErrorString(e));
      } else {
        for (size_t i = 0; i < N; ++i) out[i] = (int32_t)i;
      }
      return DTSIM_OK;
    }
  }
  const int comps = dt_field_comps(*f);
  std::vector<char> tmp(N * f->elem);
  for (int c = 0; c < comps; ++c) {
    char* plane = dt_field_plane(h->A, *f, c);
    if (to_host) {
      hipError_t e = plane ? hipMemcpy(tmp.data(), plane, tmp.size(), hipMemcpyDeviceToHost) : hipSuccess;
      if (e != hipSuccess) return fail(DTSIM_E_HIP, "hipMemcpy D2H: %s", hipGetErrorString(e));
      dt_plane_to_public(host, plane ? tmp.data() : nullptr, N, comps, c, f->elem);
    } else if (plane) {
      dt_public_to_plane(tmp.data(), host, N, comps, c, f->elem);
      hipError_t e = hipMemcpy(plane, tmp.data(), tmp.size(), hipMemcpyHostToDevice);
      if (e != hipSuccess) return fail(DTSIM_E_HIP, "hipMemcpy H2D: %s", hipGetErrorString(e));
    }
  }
  return DTSIM_OK;
}
}  // namespace

int dtsim_read_agent(dtsim_t* h, int env, dtsim_agent_info* out) {
  if (!h || !out) return fail(DTSIM_E_INVALID, "null argument");
  if (env < 0 || env >= h->N) return fail(DTSIM_E_INVALID, "env %d out of range [0, %d)", env, h->N);
  HIPCHK(hipSetDevice(h->cfg.device));
  if (!h->d_agent) HIPCHK(dev_alloc(h->d_agent, 1));
  hipLaunchKernelGGL(k_agent_info, dim3(1), dim3(1), 0, h->stream, h->A, env, h->d_agent.get());
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, h->d_agent.get(), sizeof(dtsim_agent_info), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return DTSIM_OK;
}

int dtsim_read(dtsim_t* h, int field, void* dst, size_t bytes) { return field_xfer(h, field, dst, bytes, true); }
int dtsim_write(dtsim_t* h, int field, const void* src, size_t bytes) {
  if (h) h->rendered = false;                        // (any field may move the scene: the post-passes wait for the next dtsim_render)
  return field_xfer(h, field, const_cast<void*>(src), bytes, false);
}

void* dtsim_field_devptr(dtsim_t* h, int field) {
  const StateField* f = h ? dt_state_field(field) : nullptr;
  if (!f || !f->view) return nullptr;
  return f->outer ? dt_field_plane(h->A, *f, 0) : h->slab.get();   // POS: the x plane; the z plane is pos_z
}

size_t dtsim_field_bytes(const dtsim_t* h, int field) {
  const StateField* f = h ? dt_state_field(field) : nullptr;
  return f ? dt_field_bytes(*f, (size_t)h->N, h->slab_bytes) : 0;
}
size_t dtsim_state_bytes(const dtsim_t* h) { return h ? h->slab_bytes : 0; }

int dtsim_sync(dtsim_t* h) {
  if (!h) return fail(DTSIM_E_INVALID, "null handle");
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipStreamSynchronize(h->stream));
  return DTSIM_OK;
}

void* dtsim_stream(dtsim_t* h) { return h ? (void*)h->stream : nullptr; }

int dtsim_profile_read(dtsim_t* h, int kernel, int* n_launches, double* total_ms) {
  if (!h || kernel < 0 || kernel >= DTSIM_KERNEL__COUNT || !n_launches || !total_ms) return fail(DTSIM_E_INVALID, "bad argument");
  if (!(h->cfg.flags & DTSIM_F_PROFILE)) return fail(DTSIM_E_STATE, "handle created without DTSIM_F_PROFILE");
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipStreamSynchronize(h->stream));
  ProfSlot& s = h->prof[kernel];
  double tot = 0;
  for (auto& p : s.pending) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, p.first, p.second));
    tot += ms;
    s.free_.push_back(p);
  }
  *n_launches = (int)s.pending.size();
  *total_ms = tot;
  s.pending.clear();
  return DTSIM_OK;
}

}  // extern "C"
