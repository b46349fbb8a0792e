// remap.hip -- per-env fisheye of camera_rand (include/dtsim.h: dtsim_set_distortion_luts, dtsim_build_remap_maps,
// dtsim_fill_pack_remap).
//
// Device: k_remap_cal gathers each env's frame out of the rectilinear scratch batch through the env's calibration table
// (cv2.remap(INTER_NEAREST), distortion.py:118-124, with BORDER_CONSTANT black where the table holds -1).
// Host: the tables themselves, bit-identical to the numpy statement in dtsim/distortion.py (rectify_maps, invert_map,
// fill_holes) for any K and D.  This unit is compiled with -ffp-contract=off: every f64 / f32 operation below is one
// separately rounded IEEE operation in numpy's order, nothing is fused or reassociated.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "dtsim_dev.h"

namespace {

// ---- device: frames[e][p] = scratch[e][src[env_cal[e]][p]] (0 where the index is -1) ----------------------------------
// One workgroup per (env, band of REMAP_T * 4 pixels): the sources of a band lie on a few nearby rows of the env's scratch
// frame, so the byte gathers hit in L2.  VEC (H * W % 4 == 0): 4 pixels per lane, one 16-byte table load, 3 dword stores.
constexpr int REMAP_T = 256;

template <bool VEC>
__global__ __launch_bounds__(REMAP_T) void k_remap_cal(const uint8_t* __restrict__ scratch, uint8_t* __restrict__ frames,
                                                       const int32_t* __restrict__ src, const int32_t* __restrict__ env_cal,
                                                       const uint8_t* __restrict__ mask, int hw, int bands) {
  const int e = blockIdx.x / bands, band = blockIdx.x - e * bands;
  if (mask && !mask[e]) return;
  const int32_t* tab = src + (size_t)env_cal[e] * hw;
  const uint8_t* in = scratch + (size_t)e * hw * 3;
  if (VEC) {
    const int q = band * REMAP_T + threadIdx.x;      // pixel quad
    if (q * 4 >= hw) return;
    const int4 s = reinterpret_cast<const int4*>(tab)[q];
    const int si[4] = {s.x, s.y, s.z, s.w};
    uint32_t px[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      px[k] = 0u;
      if (si[k] >= 0) {
        const uint8_t* p = in + (size_t)si[k] * 3;
        px[k] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
      }
    }
    uint32_t* out = reinterpret_cast<uint32_t*>(frames + ((size_t)e * hw + (size_t)q * 4) * 3);
    out[0] = px[0] | (px[1] << 24);
    out[1] = (px[1] >> 8) | (px[2] << 16);
    out[2] = (px[2] >> 16) | (px[3] << 8);
  } else {
    const int p = band * REMAP_T + threadIdx.x;
    if (p >= hw) return;
    const int si = tab[p];
    uint8_t* o = frames + ((size_t)e * hw + p) * 3;
    if (si >= 0) {
      const uint8_t* q = in + (size_t)si * 3;
      o[0] = q[0]; o[1] = q[1]; o[2] = q[2];
    } else {
      o[0] = o[1] = o[2] = 0;
    }
  }
}

// ---- host: the tables -----------------------------------------------------------------------------------------------------
// rectify_maps (cv::initUndistortRectifyMap as restated in dtsim/distortion.py): the accumulated f64 row walk of
// np.add.accumulate, then the plumb-bob model, in numpy's evaluation order.
void rectify(int W, int H, const double* K, const double* D, const double* ir, float* mapx, float* mapy) {
  const double fx = K[0], u0 = K[2], fy = K[4], v0 = K[5];
  const double k1 = D[0], k2 = D[1], p1 = D[2], p2 = D[3], k3 = D[4];
  for (int r = 0; r < H; ++r) {
    const double rd = (double)r;
    double X = rd * ir[1] + ir[2], Y = rd * ir[4] + ir[5], Wh = rd * ir[7] + ir[8];
    for (int c = 0; c < W; ++c) {
      if (c) { X = X + ir[0]; Y = Y + ir[3]; Wh = Wh + ir[6]; }
      const double w = 1.0 / Wh;
      const double x = X * w, y = Y * w;
      const double x2 = x * x, y2 = y * y;
      const double r2 = x2 + y2, _2xy = (2.0 * x) * y;
      const double kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2;
      const double xd = (x * kr + p1 * _2xy) + p2 * (r2 + 2.0 * x2);
      const double yd = (y * kr + p1 * (r2 + 2.0 * y2)) + p2 * _2xy;
      mapx[(size_t)r * W + c] = (float)(fx * xd + u0);
      mapy[(size_t)r * W + c] = (float)(fy * yd + v0);
    }
  }
}

// numpy's float32 -> int32 cast on x86 (cvttss2si): truncation, 0x80000000 for NaN / out of range
inline int32_t f2i_trunc(float v) { return (v > -2147483648.f && v < 2147483648.f) ? (int32_t)v : INT32_MIN; }

// invert_map: 9 passes of the non-accumulating fancy `+=` (each pass reads the sums from before it; of several sources
// with one target the last in row-major order wins), then ax / aw in float32 (NaN where nothing landed).  The sums are
// integers below 2^24, exact in float32 as in numpy's float64 intermediate.
void invert(int W, int H, const float* mapx, const float* mapy, float* rx, float* ry) {
  const size_t n = (size_t)W * H;
  std::vector<float> aw(n, 0.f), ax(n, 0.f), ay(n, 0.f), sw, sx, sy;
  std::vector<int32_t> xd(n), yd(n);
  for (size_t i = 0; i < n; ++i) {
    xd[i] = std::min(std::max(f2i_trunc(mapx[i]), 2), W - 2);
    yd[i] = std::min(std::max(f2i_trunc(mapy[i]), 2), H - 2);
  }
  static const int off[9][3] = {{-1, -1, 7}, {-1, 0, 10}, {-1, 1, 7}, {0, -1, 10}, {0, 0, 20}, {0, 1, 10}, {1, -1, 7}, {1, 0, 10}, {1, 1, 7}};
  for (const auto& o : off) {
    sw = aw; sx = ax; sy = ay;
    for (int r = 0; r < H; ++r)
      for (int c = 0; c < W; ++c) {
        const size_t i = (size_t)r * W + c;
        const int ty = yd[i] + o[0], tx = xd[i] + o[1];
        if (ty < 0 || ty >= H || tx < 0 || tx >= W) continue;   // (clipped to [1, dim - 1]: never taken)
        const size_t t = (size_t)ty * W + tx;
        aw[t] = sw[t] + (float)o[2];
        ax[t] = (float)((double)sx[t] + (double)(o[2] * c));
        ay[t] = (float)((double)sy[t] + (double)(o[2] * r));
      }
  }
  for (size_t i = 0; i < n; ++i) {
    if (aw[i] > 0.f) { rx[i] = ax[i] / aw[i]; ry[i] = ay[i] / aw[i]; }
    else rx[i] = ry[i] = NAN;
  }
}

// fill_holes: passes over the holes in the caller's visiting order (the iteration order of the reference's Python set;
// removals do not reorder a set, so every pass visits the remaining holes in the first pass's order), the first
// non-NaN neighbour of the reference's offset list, values filled earlier in a pass feeding later holes.
void fill(int W, int H, float* rx, float* ry, const int32_t* order, int64_t n_holes) {
  std::vector<std::pair<int, int>> deltas;
  for (int i = 0; i < 5; ++i)
    for (int j = 0; j < 5; ++j)
      if (std::hypot((double)(i - 3), (double)(j - 3)) <= 2.0) deltas.emplace_back(i - 3, j - 3);
  std::stable_sort(deltas.begin(), deltas.end(), [](const std::pair<int, int>& a, const std::pair<int, int>& b) {
    return std::hypot((double)a.first, (double)a.second) < std::hypot((double)b.first, (double)b.second);
  });
  std::vector<int32_t> cur(order, order + n_holes), next;
  while (!cur.empty()) {
    size_t filled = 0;
    next.clear();
    for (const int32_t idx : cur) {
      const int i = idx / W, j = idx % W;
      bool done = false;
      for (const auto& d : deltas) {
        const int u = i + d.first, v = j + d.second;
        if (u >= 0 && u < H && v >= 0 && v < W && !std::isnan(rx[(size_t)u * W + v])) {
          rx[idx] = rx[(size_t)u * W + v]; ry[idx] = ry[(size_t)u * W + v];
          ++filled; done = true;
          break;
        }
      }
      if (!done) next.push_back(idx);
    }
    if (!filled) break;
    cur.swap(next);
  }
}

// one int32 source index per output pixel: cvRound (round half to even) of the float map, -1 outside the image
void pack(int W, int H, const float* rx, const float* ry, int32_t* out) {
  for (size_t i = 0; i < (size_t)W * H; ++i) {
    const float fx = rx[i], fy = ry[i];
    int32_t v = -1;
    if (!std::isnan(fx) && !std::isnan(fy) && std::fabs(fx) < 1e9f && std::fabs(fy) < 1e9f) {
      const long sx = std::lrint((double)fx), sy = std::lrint((double)fy);
      if (sx >= 0 && sx < W && sy >= 0 && sy < H) v = (int32_t)(sy * W + sx);
    }
    out[i] = v;
  }
}

template <class F> void parallel_tables(int n, F f) {
  const int nt = std::max(1, std::min({n, 16, (int)std::max(1u, std::thread::hardware_concurrency())}));
  std::vector<std::thread> pool;
  for (int t = 0; t < nt; ++t)
    pool.emplace_back([&, t] { for (int i = t; i < n; i += nt) f(i); });
  for (auto& th : pool) th.join();
}

}  // namespace

void dt_build_remap_maps(int W, int H, int n_cal, const double* K, const double* D, const double* ir, float* rx, float* ry) {
  const size_t n = (size_t)W * H;
  parallel_tables(n_cal, [&](int i) {
    std::vector<float> mx(n), my(n);
    rectify(W, H, K + 9 * i, D + 5 * i, ir + 9 * i, mx.data(), my.data());
    invert(W, H, mx.data(), my.data(), rx + n * i, ry + n * i);
  });
}

void dt_fill_pack_remap(int W, int H, int n_cal, float* rx, float* ry, const int32_t* order, const int64_t* order_off, int32_t* src_index) {
  const size_t n = (size_t)W * H;
  parallel_tables(n_cal, [&](int i) {
    fill(W, H, rx + n * i, ry + n * i, order + order_off[i], order_off[i + 1] - order_off[i]);
    if (src_index) pack(W, H, rx + n * i, ry + n * i, src_index + n * i);
  });
}

void dt_launch_remap_cal(hipStream_t s, const uint8_t* scratch, uint8_t* frames, const int32_t* src, const int32_t* env_cal,
                         const uint8_t* mask, int N, int W, int H) {
  const int hw = W * H;
  if (hw % 4 == 0) {
    const int bands = (hw / 4 + REMAP_T - 1) / REMAP_T;
    hipLaunchKernelGGL(k_remap_cal<true>, dim3((unsigned)((size_t)N * bands)), dim3(REMAP_T), 0, s, scratch, frames, src, env_cal, mask, hw, bands);
  } else {
    const int bands = (hw + REMAP_T - 1) / REMAP_T;
    hipLaunchKernelGGL(k_remap_cal<false>, dim3((unsigned)((size_t)N * bands)), dim3(REMAP_T), 0, s, scratch, frames, src, env_cal, mask, hw, bands);
  }
}
