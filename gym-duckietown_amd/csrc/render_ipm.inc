// render_ipm.inc -- the ground-projected camera image of dtsim_ipm (the quantity: include/dtsim.h; its statement: ipm_project.h).  Included
// by render.hip after k_bev, whose grid it shares: cell blocks x env chunks of DEPTH_ENVS.
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
#include "ipm_project.h"
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

static inline dim3 dt_ipm_grid(const IpmArgs& a) {
  return dim3((unsigned)((a.oh * a.ow + 256 * IPM_CPT - 1) / (256 * IPM_CPT)), (unsigned)((a.N + DEPTH_ENVS - 1) / DEPTH_ENVS));
}
