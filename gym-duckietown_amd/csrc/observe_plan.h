// observe_plan.h -- the host-side plan of the observation resize (dtsim_observe*, observe.hip): the kernel argument, the packed
// resampling tables, the kernel a shape launches and its LDS.  Plain C++17 without a HIP header, so a host program can include it
// (tests/test_observe_paths_host.py drives the planner with g++).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/dtsim.h"

#ifndef DT_OBS_STAGE_ROWS
#define DT_OBS_STAGE_ROWS 8    // input rows k_observe stages in LDS per horizontal step
#endif
#ifndef DT_OBS_LDS_KB
#define DT_OBS_LDS_KB 48       // k_observe's LDS budget
#endif
#ifndef DT_OBS_MAX_RPB
#define DT_OBS_MAX_RPB 8       // output rows per k_observe workgroup at most: enough rows, and the grid stays large
#endif
// the k_observe_pow2<HN, SY> instantiations (hn dwords per column window, vertical scale): the planner chooses the kernel only for
// these pairs, the launcher launches them
#define DT_OBS_POW2_LIST(X) X(7, 2) X(7, 4) X(7, 8) X(12, 2) X(12, 4) X(12, 8)

// observation post-processing (observe.hip): Pillow-exact bilinear resize + layout + normalisation
struct ObserveParams {
  int32_t N, H, W, oh, ow;
  int32_t kx, ky;               // taps per output column / row in the tables
  int32_t rows_per_block;       // output rows per workgroup
  int32_t max_rows_in;          // input rows any workgroup needs (sizes the LDS intermediate)
  int32_t chw, f32;             // layout (0: [N,h,w,3], 1: [N,3,h,w]) and dtype (0: uint8, 1: float32 / 255)
  const uint8_t* frames;        // [N,H,W,3]
  void* out;
  const int32_t* bx;            // [ow][2] first tap, tap count   (dtsim/resample.py coeffs)
  const int32_t* kkx;           // [ow][kx] 22-bit fixed-point taps
  const int32_t* by;            // [oh][2]
  const int32_t* kky;           // [oh][ky]
  // (OpenCV INTER_CUBIC, k_observe_cubic: bx / by = [ow] / [oh] first of the four taps, borders replicate; kkx / kky = [..][4] 11-bit taps)
  // power-of-two down-scaling (640 -> 160 / 80, 480 -> 240 / 120 / 60): away from the borders every output column (row) has the
  // SAME taps, and they are small integers times a power of two (the triangle filter of scale S normalises to (1, 3, .., 2S-1,
  // 2S-1, .., 1) / 2S^2).  hfast: 0 off, else S: the 2S taps x 3 channels of a column sit in `hn` aligned dwords starting `hoff`
  // bytes from 3 S ox; hw[c][d] holds channel c's tap weights at their byte positions of dword d (zeros elsewhere): three
  // chains of v_dot4_u32_u8 filter a column.  vfast: 0 off, else S: vw[t] the 2S row weights, applied to four bytes at a time
  // in two 16-bit lanes.  hsh / vsh: the fixed-point shift that is left (22 - log2 of the common factor).
  int32_t hfast, hn, hoff, hsh;
  int32_t vfast, vsh;
  uint32_t hw[3][12];
  uint32_t vw[16];
};

enum ObserveKernel {
  DT_OBS_STAGED,   // k_observe: rows staged in LDS, any tables (with the fast taps where the plan has them)
  DT_OBS_POW2,     // k_observe_pow2<P.hn, P.vfast> + k_observe_border
  DT_OBS_CUBIC,    // k_observe_cubic
};

struct ObservePlan {
  std::vector<int32_t> tab;     // [bx | kkx | by | kky] as the kernels read them; with P's output size and tap counts, the cache key
  size_t off_bx = 0, off_kkx = 0, off_by = 0, off_kky = 0;   // the four parts, in elements of `tab`
  ObserveParams P{};            // everything but frames, out, chw, f32 and the four table pointers
  ObserveKernel kernel = DT_OBS_STAGED;
  size_t lds = 0;               // dynamic LDS bytes of the launch
  bool same_tables(const ObservePlan& o) const {
    return P.oh == o.P.oh && P.ow == o.P.ow && P.kx == o.P.kx && P.ky == o.P.ky && tab == o.tab;
  }
};

// k_observe's dynamic LDS with an intermediate of `rows` input rows: [DT_OBS_STAGE_ROWS dword-padded input rows + 32 B | rows x ow x 3
// bytes, dword-padded | the column tables [ow][2 + 9] of the 9-tap window path | 16 B].  fit_rows (optional): the rows that keep it within
// DT_OBS_LDS_KB, with kMargin set aside for the padding and the tail.  (Where the fixed parts alone exceed the budget -- 24 W + 44 ow
// bytes through the 9-tap path, e.g. 640 -> 800 columns -- the unsigned difference wraps, every row count "fits" and the launch asks for more.)
inline size_t dt_observe_lds(int W, int ow, int kx, int rows, size_t* fit_rows = nullptr) {
  constexpr size_t kTail = 16, kMargin = 32;
  static_assert(kMargin >= kTail + 3, "the margin covers the tail and the dword padding of the rows");
  const size_t stage = DT_OBS_STAGE_ROWS * (((size_t)W * 3 + 3) / 4) * 4 + 32;
  const size_t tabs = (ow != W && kx <= 9) ? (size_t)ow * (2 + 9) * 4 : 0;
  if (fit_rows) *fit_rows = ((size_t)DT_OBS_LDS_KB * 1024 - stage - tabs - kMargin) / ((size_t)ow * 3);
  return stage + (((size_t)rows * ow * 3 + 3) & ~(size_t)3) + tabs + kTail;
}

inline int dt_observe_fail(std::string& err, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  err = buf;
  return code;
}

// ---- bilinear (Pillow) ---------------------------------------------------------------------------------------------------------
// Every call: the arguments' presence, and the caller's tables (dtsim/resample.py coeffs; none for an axis that keeps its size) packed
// into p.tab with P.N .. P.ky.  A plan whose same_tables() holds for the packed one is already the plan of this call; else
// dt_observe_plan completes the packed one.
inline int dt_observe_pack(ObservePlan& p, std::string& err, int W, int H, int N, int out_h, int out_w,
                           const int32_t* bounds_x, const int32_t* taps_x, int ksize_x,
                           const int32_t* bounds_y, const int32_t* taps_y, int ksize_y) {
  if (out_h <= 0 || out_w <= 0) return dt_observe_fail(err, DTSIM_E_INVALID, "output size %dx%d", out_w, out_h);
  if ((out_w != W && (!bounds_x || !taps_x || ksize_x <= 0)) || (out_h != H && (!bounds_y || !taps_y || ksize_y <= 0)))
    return dt_observe_fail(err, DTSIM_E_INVALID, "resampling tables missing for a resized axis");
  p = ObservePlan{};
  std::vector<int32_t>& tab = p.tab;
  if (out_w != W) {
    tab.insert(tab.end(), bounds_x, bounds_x + 2 * (size_t)out_w);
    p.off_kkx = tab.size();
    tab.insert(tab.end(), taps_x, taps_x + (size_t)out_w * ksize_x);
  } else ksize_x = 0;
  p.off_by = tab.size();
  if (out_h != H) {
    tab.insert(tab.end(), bounds_y, bounds_y + 2 * (size_t)out_h);
    p.off_kky = tab.size();
    tab.insert(tab.end(), taps_y, taps_y + (size_t)out_h * ksize_y);
  } else {                                             // rows pass through: row i reads input row i
    for (int i = 0; i < out_h; ++i) { tab.push_back(i); tab.push_back(1); }
    p.off_kky = tab.size();
    ksize_y = 0;
  }
  p.P.N = N; p.P.H = H; p.P.W = W; p.P.oh = out_h; p.P.ow = out_w; p.P.kx = ksize_x; p.P.ky = ksize_y;
  return DTSIM_OK;
}

// the `uniform` test of a power-of-two axis: every interior output coordinate has the same 2S small-integer taps (times a power of
// two) starting at S o - S / 2; w: the 2S integers, *sh: the shift that is left
inline bool dt_observe_uniform(const int32_t* bounds, const int32_t* taps, int ksize, int n_in, int n_out, int S, uint32_t* w, int* sh) {
  if (n_out < 3 || n_out * S != n_in || 2 * S > ksize || 2 * S > 16) return false;
  const int32_t* k1 = taps + (size_t)1 * ksize;
  int common = 22;                                  // trailing zero bits shared by the taps of column 1
  for (int t = 0; t < 2 * S; ++t) { if (k1[t] <= 0) return false; common = std::min(common, __builtin_ctz((unsigned)k1[t])); }
  long long sum = 0;
  for (int t = 0; t < 2 * S; ++t) { const int q = k1[t] >> common; if (q > 255) return false; w[t] = (uint32_t)q; sum += q; }
  if (sum != (1ll << (22 - common)) || 22 - common < 1 || 22 - common > 7) return false;   // two-lane sums must stay below 2^16
  for (int o = 1; o < n_out - 1; ++o) {
    if (bounds[2 * o] != S * o - S / 2 || bounds[2 * o + 1] != 2 * S) return false;
    for (int t = 0; t < 2 * S; ++t) if (taps[(size_t)o * ksize + t] != k1[t]) return false;
  }
  *sh = 22 - common;
  return true;
}

// Completes a packed plan: validates the tables, searches the rows per workgroup, derives the power-of-two fast paths and chooses the
// kernel.  generic (DTSIM_OBSERVE_GENERIC): no fast paths, the table-driven ones only; staged (DTSIM_OBSERVE_STAGED): the fast taps stay,
// in k_observe.  DTSIM_OK, or the error with its message in err.
inline int dt_observe_plan(ObservePlan& p, std::string& err, bool staged, bool generic) {
  ObserveParams& P = p.P;
  const int W = P.W, H = P.H, out_w = P.ow, out_h = P.oh, ksize_x = P.kx, ksize_y = P.ky;
  const int32_t *bounds_x = p.tab.data() + p.off_bx, *taps_x = p.tab.data() + p.off_kkx;
  const int32_t *by = p.tab.data() + p.off_by, *taps_y = p.tab.data() + p.off_kky;
  for (int i = 0; i < out_h; ++i)
    if (by[2 * i] < 0 || by[2 * i + 1] <= 0 || by[2 * i] + by[2 * i + 1] > H || (i && by[2 * i] < by[2 * i - 2]))
      return dt_observe_fail(err, DTSIM_E_INVALID, "bounds_y[%d] = (%d, %d) out of range / not monotone", i, by[2 * i], by[2 * i + 1]);
  if (out_w != W)
    for (int i = 0; i < out_w; ++i)
      if (bounds_x[2 * i] < 0 || bounds_x[2 * i + 1] <= 0 || bounds_x[2 * i + 1] > ksize_x || bounds_x[2 * i] + bounds_x[2 * i + 1] > W)
        return dt_observe_fail(err, DTSIM_E_INVALID, "bounds_x[%d] = (%d, %d) out of range", i, bounds_x[2 * i], bounds_x[2 * i + 1]);
  if (out_h != H)
    for (int i = 0; i < out_h; ++i) if (by[2 * i + 1] > ksize_y) return dt_observe_fail(err, DTSIM_E_INVALID, "bounds_y[%d] count > ksize_y", i);
  // rows per workgroup: as many output rows as keep the uint8 intermediate (+ staging) within the LDS budget
  size_t fit_rows = 0;
  dt_observe_lds(W, out_w, ksize_x, 0, &fit_rows);
  const int max_rows = (int)std::min<size_t>((size_t)H, fit_rows);
  for (int cand = 1; cand <= out_h; ++cand) {
    int worst = 0;
    for (int o0 = 0; o0 < out_h; o0 += cand) {
      const int o1 = std::min(o0 + cand, out_h) - 1;
      worst = std::max(worst, by[2 * o1] + by[2 * o1 + 1] - by[2 * o0]);
    }
    if (worst > max_rows) break;
    P.rows_per_block = cand; P.max_rows_in = worst;
    if (cand >= DT_OBS_MAX_RPB) break;
  }
  if (P.rows_per_block == 0)
    return dt_observe_fail(err, DTSIM_E_LIMIT, "observation %dx%d: one output row needs more input rows than fit in LDS", out_w, out_h);
  // power-of-two down-scaling: interior columns / rows with identical small-integer taps (the dot4 / two-lane paths)
  if (!generic && out_w != W && ((size_t)W * 3) % 4 == 0) {
    for (int S : {4, 8}) {
      uint32_t w[16]; int sh = 0;
      if (!dt_observe_uniform(bounds_x, taps_x, ksize_x, W, out_w, S, w, &sh)) continue;
      const int start = -3 * S / 2;                  // first byte of a column's window relative to 3 S ox
      P.hfast = S; P.hsh = sh;
      P.hoff = start & ~3;                           // (two's complement: rounds towards minus infinity)
      P.hn = (3 * 2 * S + (start - P.hoff) + 3) / 4; // 7 (S = 4) or 12 (S = 8): the two window sizes the kernels unroll
      for (int b = 0; b < 3 * 2 * S; ++b) {
        const int pos = b + (start - P.hoff);
        P.hw[b % 3][pos / 4] |= w[b / 3] << (8 * (pos % 4));
      }
      break;
    }
  }
  if (!generic && out_h != H && ((size_t)out_w * 3) % 4 == 0) {
    for (int S : {2, 4, 8}) {
      uint32_t w[16]; int sh = 0;
      if (!dt_observe_uniform(by, taps_y, ksize_y, H, out_h, S, w, &sh)) continue;
      P.vfast = S; P.vsh = sh;
      for (int t = 0; t < 2 * S; ++t) P.vw[t] = w[t];
      break;
    }
  }
#define DT_OBS_HAS(HN_, SY_) || (P.hn == HN_ && P.vfast == SY_)
  const bool pow2 = P.hfast && P.vfast && out_w >= 3 && out_h >= 3 && !staged && (false DT_OBS_POW2_LIST(DT_OBS_HAS));
#undef DT_OBS_HAS
  p.kernel = pow2 ? DT_OBS_POW2 : DT_OBS_STAGED;
  p.lds = pow2 ? 0 : dt_observe_lds(W, out_w, ksize_x, P.max_rows_in);
  return DTSIM_OK;
}

// ---- OpenCV INTER_CUBIC ---------------------------------------------------------------------------------------------------------
// as dt_observe_pack, for the tables of dtsim/resample.py cubic_coeffs: [first_x | taps_x [ow][4] | first_y | taps_y [oh][4]]
inline int dt_observe_pack_cubic(ObservePlan& p, std::string& err, int W, int H, int N, int out_h, int out_w,
                                 const int32_t* first_x, const int32_t* taps_x, const int32_t* first_y, const int32_t* taps_y) {
  if (!first_x || !taps_x || !first_y || !taps_y) return dt_observe_fail(err, DTSIM_E_INVALID, "bad argument");
  if (out_h <= 0 || out_w <= 0) return dt_observe_fail(err, DTSIM_E_INVALID, "output size %dx%d", out_w, out_h);
  p = ObservePlan{};
  std::vector<int32_t>& tab = p.tab;
  tab.insert(tab.end(), first_x, first_x + out_w);
  p.off_kkx = tab.size();
  tab.insert(tab.end(), taps_x, taps_x + 4 * (size_t)out_w);
  p.off_by = tab.size();
  tab.insert(tab.end(), first_y, first_y + out_h);
  p.off_kky = tab.size();
  tab.insert(tab.end(), taps_y, taps_y + 4 * (size_t)out_h);
  p.P.N = N; p.P.H = H; p.P.W = W; p.P.oh = out_h; p.P.ow = out_w; p.P.kx = 4; p.P.ky = 4;
  return DTSIM_OK;
}

// as dt_observe_plan: validates the packed tables; the kernel is k_observe_cubic with one int32 row of 3 W sums in LDS
inline int dt_observe_plan_cubic(ObservePlan& p, std::string& err) {
  const int W = p.P.W, H = p.P.H, out_w = p.P.ow, out_h = p.P.oh;
  const int32_t *first_x = p.tab.data() + p.off_bx, *taps_x = p.tab.data() + p.off_kkx;
  const int32_t *first_y = p.tab.data() + p.off_by, *taps_y = p.tab.data() + p.off_kky;
  p.lds = (size_t)W * 3 * sizeof(int32_t) + 16;
  if (p.lds > 64 * 1024) return dt_observe_fail(err, DTSIM_E_LIMIT, "frame rows of %d pixels do not fit the kernel's LDS row", W);
  for (int i = 0; i < out_w; ++i)
    if (first_x[i] < -3 || first_x[i] >= W) return dt_observe_fail(err, DTSIM_E_INVALID, "first_x[%d] = %d out of range", i, first_x[i]);
  for (int i = 0; i < out_h; ++i)
    if (first_y[i] < -3 || first_y[i] >= H) return dt_observe_fail(err, DTSIM_E_INVALID, "first_y[%d] = %d out of range", i, first_y[i]);
  for (size_t i = 0; i < 4 * (size_t)out_w; ++i)
    if (taps_x[i] < -32768 || taps_x[i] > 32767) return dt_observe_fail(err, DTSIM_E_INVALID, "taps_x[%zu] is not a 16-bit tap", i);
  for (size_t i = 0; i < 4 * (size_t)out_h; ++i)
    if (taps_y[i] < -32768 || taps_y[i] > 32767) return dt_observe_fail(err, DTSIM_E_INVALID, "taps_y[%zu] is not a 16-bit tap", i);
  p.kernel = DT_OBS_CUBIC;
  return DTSIM_OK;
}
