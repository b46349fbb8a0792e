// observe.hip -- learner-side observation post-processing on the device.
//
// Replaces, for the whole frame batch at once, what the reference's learners do per env on the host:
//   learning/utils/wrappers.py:38-54  ResizeWrapper   (scipy imresize == PIL Image.resize BILINEAR)
//   learning/utils/wrappers.py:57-69  NormalizeWrapper (/ 255 -> float32)
//   learning/utils/wrappers.py:72-86  ImgWrapper       (HWC -> CHW)
// The resize is Pillow's antialiased two-pass resampler in 8-bit fixed point (22-bit coefficients,
// uint8 intermediate after the horizontal pass); the coefficient tables come from the host
// (dtsim/resample.py, pinned bit-exact against PIL) so the device result is bit-identical to
// `Image.resize`.  HBM-read bound: every frame byte is read once (plus the row overlap between
// neighbouring row blocks), the output is 16x smaller at 640x480 -> 160x120.
#include "dtsim_dev.h"
#include <algorithm>

namespace {

#define OB 256                 // threads per workgroup
#ifndef OBS_STAGE_ROWS
#define OBS_STAGE_ROWS DT_OBS_STAGE_ROWS   // input rows staged in LDS per horizontal step
#endif
#define PREC 22                // Pillow PRECISION_BITS (32 - 8 - 2)

__device__ inline uint32_t clip8(int32_t acc) {
  const int32_t v = acc >> PREC;
  return (uint32_t)min(max(v, 0), 255);
}

// ---- vertical pass + layout / normalisation.  PER = 4 consecutive intermediate bytes per thread when the
// rows are dword-sized (compile-time, so the accumulators stay in registers), else 1.
template <int PER>
__device__ inline void observe_vertical_t(const ObserveParams& P, const uint8_t* s_tmp, int e, int oy0, int oy1, int y_first, int tid) {
  const int tmp_row_bytes = P.ow * 3, per_row = tmp_row_bytes / PER;
  const int n_out = (oy1 - oy0) * per_row;
  for (int i = tid; i < n_out; i += OB) {
    const int oy = oy0 + i / per_row, j0 = (i % per_row) * PER;
    uint32_t v[PER];
    if (PER == 4 && P.vfast && oy > 0 && oy < P.oh - 1) {
      // uniform small-integer taps: four bytes per step in two 16-bit lanes (sum of the weights = 2^vsh: a lane never carries)
      const int S = P.vfast;
      const uint8_t* p = s_tmp + (size_t)(S * oy - S / 2 - y_first) * tmp_row_bytes + j0;
      uint32_t lo = 0x00010001u << (P.vsh - 1), hi = lo;                  // the rounding half
      for (int t = 0; t < 2 * S; ++t) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(p + (size_t)t * tmp_row_bytes);
        lo = __umul24(w & 0x00FF00FFu, P.vw[t]) + lo;
        hi = __umul24((w >> 8) & 0x00FF00FFu, P.vw[t]) + hi;
      }
      lo = (lo >> P.vsh) & 0x00FF00FFu; hi = (hi >> P.vsh) & 0x00FF00FFu;
      const uint32_t packed = lo | (hi << 8);
      if (!P.chw && !P.f32) {
        *reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(P.out) + ((size_t)e * P.oh + oy) * tmp_row_bytes + j0) = packed;
        continue;
      }
#pragma unroll
      for (int q = 0; q < PER; ++q) v[q] = (packed >> (8 * q)) & 255u;
    } else if (P.oh == P.H) {
#pragma unroll
      for (int q = 0; q < PER; ++q) v[q] = s_tmp[(size_t)(oy - y_first) * tmp_row_bytes + j0 + q];
    } else {
      const int y0 = P.by[2 * oy], n = P.by[2 * oy + 1];
      const int32_t* k = P.kky + oy * P.ky;
      const uint8_t* p = s_tmp + (size_t)(y0 - y_first) * tmp_row_bytes + j0;
      int32_t a[PER];
#pragma unroll
      for (int q = 0; q < PER; ++q) a[q] = 1 << (PREC - 1);
      for (int t = 0; t < n; ++t) {
        const uint32_t kt = (uint32_t)k[t];
        if (PER == 4) {
          const uint32_t w = *reinterpret_cast<const uint32_t*>(p + (size_t)t * tmp_row_bytes);
#pragma unroll
          for (int q = 0; q < PER; ++q) a[q] += (int32_t)__umul24((w >> (8 * q)) & 255u, kt);
        } else {
          a[0] += (int32_t)__umul24((uint32_t)p[(size_t)t * tmp_row_bytes], kt);
        }
      }
#pragma unroll
      for (int q = 0; q < PER; ++q) v[q] = clip8(a[q]);
    }
    if (PER == 4 && !P.chw && !P.f32) {                // HWC uint8: one dword store
      *reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(P.out) + ((size_t)e * P.oh + oy) * tmp_row_bytes + j0) =
          v[0] | (v[1 % PER] << 8) | (v[2 % PER] << 16) | (v[3 % PER] << 24);
      continue;
    }
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int j = j0 + q, ox = j / 3, c = j % 3;
      const size_t o = P.chw ? (((size_t)e * 3 + c) * P.oh + oy) * P.ow + ox : ((size_t)e * P.oh + oy) * tmp_row_bytes + j;
      if (P.f32) reinterpret_cast<float*>(P.out)[o] = (float)v[q] / 255.0f;     // NormalizeWrapper: (obs - 0) / (255 - 0)
      else reinterpret_cast<uint8_t*>(P.out)[o] = (uint8_t)v[q];
    }
  }
}
__device__ inline void observe_vertical(const ObserveParams& P, const uint8_t* s_tmp, int e, int oy0, int oy1, int y_first, int tid) {
  if (((P.ow * 3) & 3) == 0) observe_vertical_t<4>(P, s_tmp, e, oy0, oy1, y_first, tid);
  else observe_vertical_t<1>(P, s_tmp, e, oy0, oy1, y_first, tid);
}

// MASKED (dtsim_observe_masked): the workgroups / threads of envs with mask[e] == 0 leave at once (the grid stays sized for N); the
// unmasked instantiations do not read `mask`.
template <bool MASKED = false>
__global__ __launch_bounds__(OB) void k_observe(ObserveParams P, const uint8_t* __restrict__ mask) {
  extern __shared__ uint32_t s_mem[];
  const int tid = threadIdx.x;
  const int n_blocks = (P.oh + P.rows_per_block - 1) / P.rows_per_block;
  const int e = blockIdx.x / n_blocks, blk = blockIdx.x % n_blocks;
  if (MASKED && !mask[e]) return;                    // (the whole workgroup: one env)
  const int oy0 = blk * P.rows_per_block, oy1 = min(oy0 + P.rows_per_block, P.oh);
  const int y_first = P.by[2 * oy0], y_last = P.by[2 * (oy1 - 1)] + P.by[2 * (oy1 - 1) + 1];
  const int rows_in = y_last - y_first;
  const int in_row_bytes = P.W * 3, in_row_words = (in_row_bytes + 3) >> 2;
  const int tmp_row_bytes = P.ow * 3;
  uint8_t* s_row = reinterpret_cast<uint8_t*>(s_mem);                               // [OBS_STAGE_ROWS][in_row_words * 4] (+32 B slack)
  uint8_t* s_tmp = s_row + (size_t)OBS_STAGE_ROWS * in_row_words * 4 + 32;          // [max_rows_in][ow * 3]
  int32_t* s_bx = reinterpret_cast<int32_t*>(s_tmp + (((size_t)P.max_rows_in * tmp_row_bytes + 3) & ~(size_t)3));   // [ow][2]
  int32_t* s_kx = s_bx + 2 * P.ow;                                                  // [ow][9] (fast path only)
  if (P.ow != P.W && P.kx <= 9 && !P.hfast) {
    for (int i = tid; i < 2 * P.ow; i += OB) s_bx[i] = P.bx[i];
    for (int i = tid; i < 9 * P.ow; i += OB) s_kx[i] = (i % 9) < P.kx ? P.kkx[(i / 9) * P.kx + (i % 9)] : 0;
  }
  const uint8_t* frame = P.frames + (size_t)e * P.H * in_row_bytes;
  const bool aligned = (in_row_bytes & 3) == 0;

  // ---- horizontal pass (skipped when the width is unchanged: Pillow then resamples rows only).
  // The rows of stage s+1 are prefetched into registers while stage s is filtered from LDS, so the
  // global-load latency is off the critical path (one stage = OBS_STAGE_ROWS rows).
  constexpr int PF = 16;                               // prefetch registers per thread
  const bool pipelined = aligned && OBS_STAGE_ROWS * in_row_words <= PF * OB;
  uint32_t pf[PF];
  auto prefetch = [&](int r0) {
    const int nr = min(OBS_STAGE_ROWS, rows_in - r0);
#pragma unroll
    for (int q = 0; q < PF; ++q) {
      const int i = tid + q * OB;
      if (i < nr * in_row_words) {
        const int rr = i / in_row_words, wd = i % in_row_words;
        pf[q] = reinterpret_cast<const uint32_t*>(frame + (size_t)(y_first + r0 + rr) * in_row_bytes)[wd];
      }
    }
  };
  if (pipelined && rows_in > 0) prefetch(0);
  for (int r0 = 0; r0 < rows_in; r0 += OBS_STAGE_ROWS) {
    const int nr = min(OBS_STAGE_ROWS, rows_in - r0);
    if (pipelined) {
#pragma unroll
      for (int q = 0; q < PF; ++q) {
        const int i = tid + q * OB;
        if (i < nr * in_row_words) reinterpret_cast<uint32_t*>(s_row)[i] = pf[q];    // rows are contiguous: i == rr * in_row_words + wd
      }
    } else if (aligned) {                            // coalesced dword loads of whole rows
      for (int i = tid; i < nr * in_row_words; i += OB) {
        const int rr = i / in_row_words, wd = i % in_row_words;
        reinterpret_cast<uint32_t*>(s_row)[rr * in_row_words + wd] =
            reinterpret_cast<const uint32_t*>(frame + (size_t)(y_first + r0 + rr) * in_row_bytes)[wd];
      }
    } else {
      for (int i = tid; i < nr * in_row_bytes; i += OB) {
        const int rr = i / in_row_bytes, bb = i % in_row_bytes;
        s_row[rr * in_row_words * 4 + bb] = frame[(size_t)(y_first + r0 + rr) * in_row_bytes + bb];
      }
    }
    __syncthreads();
    if (pipelined && r0 + OBS_STAGE_ROWS < rows_in) prefetch(r0 + OBS_STAGE_ROWS);
    if (P.hfast) {
      // power-of-two scale: every interior column has the same taps; three chains of v_dot4_u32_u8 over the column's aligned
      // dwords with the channel's weights at their byte positions (kernel arguments: scalar registers)
      const int S = P.hfast, sh = P.hsh;
      for (int i = tid; i < nr * P.ow; i += OB) {
        const int rr = i / P.ow, ox = i % P.ow;
        uint8_t* dst = s_tmp + (size_t)(r0 + rr) * tmp_row_bytes + ox * 3;
        if (ox == 0 || ox == P.ow - 1) {             // border columns: clipped, renormalised taps from the tables
          const uint8_t* src = s_row + rr * in_row_words * 4;
          const int x0 = P.bx[2 * ox], n = P.bx[2 * ox + 1];
          const int32_t* k = P.kkx + ox * P.kx;
          int32_t a0 = 1 << (PREC - 1), a1 = a0, a2 = a0;
          const uint8_t* p = src + x0 * 3;
          for (int t = 0; t < n; ++t) {
            const int32_t kt = k[t];
            a0 += (int32_t)p[3 * t] * kt; a1 += (int32_t)p[3 * t + 1] * kt; a2 += (int32_t)p[3 * t + 2] * kt;
          }
          dst[0] = (uint8_t)clip8(a0); dst[1] = (uint8_t)clip8(a1); dst[2] = (uint8_t)clip8(a2);
          continue;
        }
        const uint32_t* wsrc = reinterpret_cast<const uint32_t*>(s_row + rr * in_row_words * 4) + ((3 * S * ox + P.hoff) >> 2);
        uint32_t a0 = 1u << (sh - 1), a1 = a0, a2 = a0;
        if (P.hn == 7) {
#pragma unroll
          for (int d = 0; d < 7; ++d) {
            const uint32_t w = wsrc[d];
            a0 = __builtin_amdgcn_udot4(w, P.hw[0][d], a0, false); a1 = __builtin_amdgcn_udot4(w, P.hw[1][d], a1, false); a2 = __builtin_amdgcn_udot4(w, P.hw[2][d], a2, false);
          }
        } else {
#pragma unroll
          for (int d = 0; d < 12; ++d) {
            const uint32_t w = wsrc[d];
            a0 = __builtin_amdgcn_udot4(w, P.hw[0][d], a0, false); a1 = __builtin_amdgcn_udot4(w, P.hw[1][d], a1, false); a2 = __builtin_amdgcn_udot4(w, P.hw[2][d], a2, false);
          }
        }
        dst[0] = (uint8_t)(a0 >> sh); dst[1] = (uint8_t)(a1 >> sh); dst[2] = (uint8_t)(a2 >> sh);
      }
    } else if (P.ow != P.W && P.kx <= 9) {
      // fast path (e.g. 640 -> 160: 8 taps): the 27 bytes of the 9-tap window come from 8 dword LDS reads,
      // are byte-aligned with v_alignbyte and multiplied out with 24-bit integer MADs
      for (int i = tid; i < nr * P.ow; i += OB) {
        const int rr = i / P.ow, ox = i % P.ow;
        const int x0 = s_bx[2 * ox];
        const int32_t* k = s_kx + ox * 9;
        const uint32_t* wsrc = reinterpret_cast<const uint32_t*>(s_row + rr * in_row_words * 4);
        const int b0 = x0 * 3, w0 = b0 >> 2;
        const uint32_t sh = (uint32_t)(b0 & 3);
        uint32_t w[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) w[q] = wsrc[w0 + q];               // may run past the row: those taps are 0
        uint32_t a[7];
#pragma unroll
        for (int q = 0; q < 7; ++q) a[q] = __builtin_amdgcn_alignbyte(w[q + 1], w[q], sh);   // bytes b0+4q .. b0+4q+3
        int32_t acc[3] = {1 << (PREC - 1), 1 << (PREC - 1), 1 << (PREC - 1)};
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          const int32_t kt = k[t];
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const int b = 3 * t + c;
            acc[c] += (int32_t)__umul24((a[b >> 2] >> (8 * (b & 3))) & 255u, (uint32_t)kt);
          }
        }
        uint8_t* dst = s_tmp + (size_t)(r0 + rr) * tmp_row_bytes + ox * 3;
        dst[0] = (uint8_t)clip8(acc[0]); dst[1] = (uint8_t)clip8(acc[1]); dst[2] = (uint8_t)clip8(acc[2]);
      }
    } else {
      for (int i = tid; i < nr * P.ow; i += OB) {
        const int rr = i / P.ow, ox = i % P.ow;
        const uint8_t* src = s_row + rr * in_row_words * 4;
        uint8_t* dst = s_tmp + (size_t)(r0 + rr) * tmp_row_bytes + ox * 3;
        if (P.ow == P.W) { dst[0] = src[ox * 3]; dst[1] = src[ox * 3 + 1]; dst[2] = src[ox * 3 + 2]; continue; }
        const int x0 = P.bx[2 * ox], n = P.bx[2 * ox + 1];
        const int32_t* k = P.kkx + ox * P.kx;
        int32_t a0 = 1 << (PREC - 1), a1 = a0, a2 = a0;
        const uint8_t* p = src + x0 * 3;
        for (int t = 0; t < n; ++t) {
          const int32_t kt = k[t];
          a0 += (int32_t)p[3 * t] * kt; a1 += (int32_t)p[3 * t + 1] * kt; a2 += (int32_t)p[3 * t + 2] * kt;
        }
        dst[0] = (uint8_t)clip8(a0); dst[1] = (uint8_t)clip8(a1); dst[2] = (uint8_t)clip8(a2);
      }
    }
    __syncthreads();
  }

  observe_vertical(P, s_tmp, e, oy0, oy1, y_first, tid);
}

// ---- power-of-two down-scaling on both axes (640 x 480 -> 160 x 120, 80 x 60, 160 x 240 ...): no staging at all ----------
// Away from the borders every output pixel has the same small-integer taps (ObserveParams::hw / vw).  A thread owns R = 4
// vertically adjacent output pixels of one column: it walks the (R + 1) SY input rows they need once, filters each row's
// window with three v_dot4_u32_u8 chains straight from global memory (HN aligned dwords; neighbouring threads read
// neighbouring windows, the rows are shared through L1 / L2), rounds to the uint8 intermediate Pillow keeps, and adds it to
// the one or two outputs the row belongs to.  The frame is read from HBM once; nothing is synchronised.  Border rows /
// columns (clipped, renormalised taps) are k_observe_border's.
template <int HN, int SY, bool MASKED = false>
__global__ __launch_bounds__(OB) void k_observe_pow2(ObserveParams P, const uint8_t* __restrict__ mask) {
  constexpr int R = 4;
  const int wi = P.ow - 2, G = (P.oh - 2 + R - 1) / R;
  const int per_env = G * wi;
  const int idx = blockIdx.x * OB + threadIdx.x;
  const int e = idx / per_env, rem = idx - e * per_env;
  if (e >= P.N) return;
  if (MASKED && !mask[e]) return;
  const int g = rem / wi, ox = 1 + (rem - g * wi);
  const int oy0 = 1 + g * R;
  const int SX = P.hfast;
  const int in_row_bytes = P.W * 3;
  const uint8_t* col = P.frames + (size_t)e * P.H * in_row_bytes + (3 * SX * ox + P.hoff);
  const int ybase = SY * oy0 - SY / 2;
  uint32_t acc[R][3];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[r][c] = 1u << (P.vsh - 1);
  const uint32_t hhalf = 1u << (P.hsh - 1);
#pragma unroll
  for (int t = 0; t < (R + 1) * SY; ++t) {
    const int y = min(ybase + t, P.H - 1);             // rows past the frame only feed outputs that are not stored
    const uint32_t* wsrc = reinterpret_cast<const uint32_t*>(col + (size_t)y * in_row_bytes);
    uint32_t a0 = hhalf, a1 = hhalf, a2 = hhalf;
#pragma unroll
    for (int d = 0; d < HN; ++d) {
      const uint32_t w = wsrc[d];
      a0 = __builtin_amdgcn_udot4(w, P.hw[0][d], a0, false); a1 = __builtin_amdgcn_udot4(w, P.hw[1][d], a1, false); a2 = __builtin_amdgcn_udot4(w, P.hw[2][d], a2, false);
    }
    a0 >>= P.hsh; a1 >>= P.hsh; a2 >>= P.hsh;         // Pillow's uint8 intermediate
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int tt = t - SY * r;                       // compile-time: which tap of output r this row is
      if (tt >= 0 && tt < 2 * SY) {
        acc[r][0] = __umul24(a0, P.vw[tt]) + acc[r][0]; acc[r][1] = __umul24(a1, P.vw[tt]) + acc[r][1]; acc[r][2] = __umul24(a2, P.vw[tt]) + acc[r][2];
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int oy = oy0 + r;
    if (oy > P.oh - 2) break;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const uint32_t v = acc[r][c] >> P.vsh;
      const size_t o = P.chw ? (((size_t)e * 3 + c) * P.oh + oy) * P.ow + ox : (((size_t)e * P.oh + oy) * P.ow + ox) * 3 + c;
      if (P.f32) reinterpret_cast<float*>(P.out)[o] = (float)v / 255.0f;
      else reinterpret_cast<uint8_t*>(P.out)[o] = (uint8_t)v;
    }
  }
}

// the border pixels of the same output (first / last row and column): Pillow's two passes per pixel from the tables
template <bool MASKED = false>
__global__ __launch_bounds__(OB) void k_observe_border(ObserveParams P, const uint8_t* __restrict__ mask) {
  const int nb = 2 * P.ow + 2 * (P.oh - 2);
  const int idx = blockIdx.x * OB + threadIdx.x;
  const int e = idx / nb, b = idx - e * nb;
  if (e >= P.N) return;
  if (MASKED && !mask[e]) return;
  int oy, ox;
  if (b < P.ow) { oy = 0; ox = b; }
  else if (b < 2 * P.ow) { oy = P.oh - 1; ox = b - P.ow; }
  else { const int q = b - 2 * P.ow; oy = 1 + (q >> 1); ox = (q & 1) ? P.ow - 1 : 0; }
  const int in_row_bytes = P.W * 3;
  const uint8_t* frame = P.frames + (size_t)e * P.H * in_row_bytes;
  const int x0 = P.bx[2 * ox], nx = P.bx[2 * ox + 1], y0 = P.by[2 * oy], ny = P.by[2 * oy + 1];
  const int32_t* kx = P.kkx + ox * P.kx;
  const int32_t* ky = P.kky + oy * P.ky;
  int32_t acc[3] = {1 << (PREC - 1), 1 << (PREC - 1), 1 << (PREC - 1)};
  for (int t = 0; t < ny; ++t) {
    const uint8_t* p = frame + (size_t)(y0 + t) * in_row_bytes + x0 * 3;
    int32_t a[3] = {1 << (PREC - 1), 1 << (PREC - 1), 1 << (PREC - 1)};
    for (int j = 0; j < nx; ++j) {
      const int32_t kj = kx[j];
      a[0] += (int32_t)p[3 * j] * kj; a[1] += (int32_t)p[3 * j + 1] * kj; a[2] += (int32_t)p[3 * j + 2] * kj;
    }
    const int32_t kt = ky[t];
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] += (int32_t)clip8(a[c]) * kt;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const uint32_t v = clip8(acc[c]);
    const size_t o = P.chw ? (((size_t)e * 3 + c) * P.oh + oy) * P.ow + ox : (((size_t)e * P.oh + oy) * P.ow + ox) * 3 + c;
    if (P.f32) reinterpret_cast<float*>(P.out)[o] = (float)v / 255.0f;
    else reinterpret_cast<uint8_t*>(P.out)[o] = (uint8_t)v;
  }
}

// ---- OpenCV INTER_CUBIC (the reference's own ResizeWrapper, wrappers.py:129-138; dtsim/resample.py cubic_coeffs) ----
// One workgroup per (env, output row).  The four source rows of the output row (replicated at the borders) are combined
// FIRST, vertically: thread t sums the same dword of the four rows with the row's four 11-bit taps, byte by byte, into
// int32 -- coalesced dword loads, every needed frame byte read once -- and leaves the 3 W sums in LDS; then thread ox sums
// four of them per channel with the column's taps.  OpenCV filters rows first and columns second, keeping int32 rows
// without rounding: both orders are the same exact integer sum (|sum| < 2^31 for 8-bit pixels), and the single rounding
// is saturate_cast<uchar>((v + 2^21) >> 22).
template <bool MASKED = false>
__global__ __launch_bounds__(OB) void k_observe_cubic(ObserveParams P, const uint8_t* __restrict__ mask) {
  extern __shared__ uint32_t s_mem[];
  int32_t* s_v = reinterpret_cast<int32_t*>(s_mem);          // [W * 3] vertical sums
  const int tid = threadIdx.x;
  const int e = blockIdx.x / P.oh, oy = blockIdx.x % P.oh;
  if (MASKED && !mask[e]) return;                    // (the whole workgroup: one env)
  const int in_row_bytes = P.W * 3;
  const uint8_t* frame = P.frames + (size_t)e * P.H * in_row_bytes;
  const int y0 = P.by[oy];                               // first of the four rows (may be < 0)
  const int32_t* ky = P.kky + 4 * oy;
  const int32_t k0 = ky[0], k1 = ky[1], k2 = ky[2], k3 = ky[3];
  const uint8_t* r0 = frame + (size_t)min(max(y0, 0), P.H - 1) * in_row_bytes;
  const uint8_t* r1 = frame + (size_t)min(max(y0 + 1, 0), P.H - 1) * in_row_bytes;
  const uint8_t* r2 = frame + (size_t)min(max(y0 + 2, 0), P.H - 1) * in_row_bytes;
  const uint8_t* r3 = frame + (size_t)min(max(y0 + 3, 0), P.H - 1) * in_row_bytes;
  if ((in_row_bytes & 3) == 0) {
    for (int i = tid; i < in_row_bytes / 4; i += OB) {
      const uint32_t a = reinterpret_cast<const uint32_t*>(r0)[i], b = reinterpret_cast<const uint32_t*>(r1)[i];
      const uint32_t c = reinterpret_cast<const uint32_t*>(r2)[i], d = reinterpret_cast<const uint32_t*>(r3)[i];
      int4 v;
      v.x = (int32_t)(a & 255u) * k0 + (int32_t)(b & 255u) * k1 + (int32_t)(c & 255u) * k2 + (int32_t)(d & 255u) * k3;
      v.y = (int32_t)((a >> 8) & 255u) * k0 + (int32_t)((b >> 8) & 255u) * k1 + (int32_t)((c >> 8) & 255u) * k2 + (int32_t)((d >> 8) & 255u) * k3;
      v.z = (int32_t)((a >> 16) & 255u) * k0 + (int32_t)((b >> 16) & 255u) * k1 + (int32_t)((c >> 16) & 255u) * k2 + (int32_t)((d >> 16) & 255u) * k3;
      v.w = (int32_t)(a >> 24) * k0 + (int32_t)(b >> 24) * k1 + (int32_t)(c >> 24) * k2 + (int32_t)(d >> 24) * k3;
      reinterpret_cast<int4*>(s_v)[i] = v;
    }
  } else {
    for (int i = tid; i < in_row_bytes; i += OB) s_v[i] = (int32_t)r0[i] * k0 + (int32_t)r1[i] * k1 + (int32_t)r2[i] * k2 + (int32_t)r3[i] * k3;
  }
  __syncthreads();
  for (int ox = tid; ox < P.ow; ox += OB) {
    const int x0 = P.bx[ox];
    const int32_t* kx = P.kkx + 4 * ox;
    int32_t acc[3] = {0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = min(max(x0 + j, 0), P.W - 1);
      const int32_t kj = kx[j];
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] += s_v[x * 3 + c] * kj;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const uint32_t v = (uint32_t)min(max((acc[c] + (1 << 21)) >> 22, 0), 255);
      const size_t o = P.chw ? (((size_t)e * 3 + c) * P.oh + oy) * P.ow + ox : (((size_t)e * P.oh + oy) * P.ow + ox) * 3 + c;
      if (P.f32) reinterpret_cast<float*>(P.out)[o] = (float)v / 255.0f;
      else reinterpret_cast<uint8_t*>(P.out)[o] = (uint8_t)v;
    }
  }
}

// Row e of src -> row e of dst for every env with mask[e] != 0 (final observations / frames).  Grid: N x blocks_per_row workgroups; chunk c
// of a row = bytes [16 c, 16 c + 16), the row's workgroups stride over its chunks -- 16-byte loads and stores when both bases and the row
// size are 16-byte aligned (vec), else the chunk's bytes one by one.  Unselected rows leave at once.
__global__ __launch_bounds__(256) void k_copy_rows(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, size_t row_bytes, int blocks_per_row,
                                                   const uint8_t* __restrict__ mask, int vec) {
  const int e = blockIdx.x / blocks_per_row;
  if (!mask[e]) return;
  uint8_t* d = dst + (size_t)e * row_bytes;
  const uint8_t* p = src + (size_t)e * row_bytes;
  const size_t stride = (size_t)blocks_per_row * 256 * 16;
  for (size_t off = ((size_t)(blockIdx.x % blocks_per_row) * 256 + threadIdx.x) * 16; off < row_bytes; off += stride) {
    if (vec) { *reinterpret_cast<uint4*>(d + off) = *reinterpret_cast<const uint4*>(p + off); continue; }
    const size_t n = row_bytes - off < 16 ? row_bytes - off : 16;
    for (size_t i = 0; i < n; ++i) d[off + i] = p[off + i];
  }
}

// ---- dtsim_boxes: one box and pixel count per id of an [N][oh][ow] byte map -------------------------------------------------------------
// s_box[k] = x0, y0, x1, y1, n of id k + 1: min / max / add atomics of the workgroup's LDS, integers, so the order of arrival does not show.
#define BOX_IDS DTSIM_MAX_OBJECTS
// `len` pixels of `id` in row `row` from column `col` on (one row: the caller cuts a run at the row's end); other ids (0, above BOX_IDS): nothing
__device__ inline void box_run(int (*s_box)[5], const uint32_t id, const int row, const int col, const int len) {
  if (id - 1u >= (uint32_t)BOX_IDS || len <= 0) return;
  int* b = s_box[id - 1u];
  atomicMin(&b[0], col); atomicMin(&b[1], row); atomicMax(&b[2], col + len); atomicMax(&b[3], row + 1); atomicAdd(&b[4], len);
}

// One workgroup per env (a masked env's leaves at once, wave-uniformly).  The env's n = oh * ow bytes: the `head` bytes up to the first 16-byte
// boundary of its address and the bytes after the last whole 16-byte chunk one per lane, the chunks between as one 16-byte load each, chunk c
// of the workgroup's stride to lane c.  A lane skips an all-zero chunk (one OR), and an all-zero word of another; within its chunk it merges the
// pixels of one id that follow each other in one row -- (row, col) of the chunk's first pixel by one division, then counted on, so a chunk
// may span any number of rows (ow < 16) -- into one box_run: five LDS atomics per run, not per pixel.  After the barrier the table goes out as
// 5 BOX_IDS consecutive ints, the rows of absent ids zeroed.  No global atomics: one map gives one result, bit for bit.
__global__ __launch_bounds__(256) void k_boxes(const uint8_t* __restrict__ inst, const int oh, const int ow, int32_t* __restrict__ out,
                                               const uint8_t* __restrict__ mask) {
  __shared__ int s_box[BOX_IDS][5];
  const int e = blockIdx.x, tid = threadIdx.x;
  if (mask && !mask[e]) return;
  for (int i = tid; i < BOX_IDS; i += 256) { s_box[i][0] = s_box[i][1] = 0x7fffffff; s_box[i][2] = s_box[i][3] = s_box[i][4] = 0; }
  __syncthreads();
  const int n = oh * ow;
  const uint8_t* p = inst + (size_t)e * (size_t)n;
  const int head = min(n, (int)((16u - (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u));
  const int chunks = (n - head) >> 4, tail0 = head + (chunks << 4);
  if (tid < head) box_run(s_box, p[tid], tid / ow, tid % ow, 1);
  if (tid < n - tail0) { const int q = tail0 + tid; box_run(s_box, p[q], q / ow, q % ow, 1); }
  for (int c = tid; c < chunks; c += 256) {
    const int q0 = head + (c << 4);
    const uint4 v = *reinterpret_cast<const uint4*>(p + q0);
    if ((v.x | v.y | v.z | v.w) == 0u) continue;
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    int row = q0 / ow, col = q0 - row * ow;
    uint32_t cur = 0;                                  // the run: `len` pixels of `cur` from (row, start) on
    int start = 0, len = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (w[k] == 0u) {                                // four empty pixels: close the run, count on
        box_run(s_box, cur, row, start, len);
        cur = 0; len = 0;
        col += 4;
        while (col >= ow) { col -= ow; ++row; }
        continue;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t id = (w[k] >> (8 * j)) & 255u;
        if (id != cur) { box_run(s_box, cur, row, start, len); cur = id; start = col; len = 0; }
        ++len;
        if (++col == ow) { box_run(s_box, cur, row, start, len); cur = 0; len = 0; col = 0; ++row; }
      }
    }
    box_run(s_box, cur, row, start, len);
  }
  __syncthreads();
  int32_t* o = out + (size_t)e * (BOX_IDS * 5);
  for (int i = tid; i < BOX_IDS * 5; i += 256) o[i] = s_box[i / 5][4] ? s_box[i / 5][i % 5] : 0;
}

// ---- observation history (dtsim_obs_push): stack[e] =[depth][C][oh * ow] slots of T, oldest first; obs[e] = [3][oh * ow] uint8 ----
// ObsBytes<n>: n consecutive bytes as one access (1, 4 or 16 bytes: byte, dword, four dwords).
template <int NB> struct ObsBytes;
template <> struct ObsBytes<1> { using type = uint8_t; };
template <> struct ObsBytes<4> { using type = uint32_t; };
template <> struct ObsBytes<16> { typedef uint32_t type __attribute__((ext_vector_type(4))); };

// Pillow's convert("L") (ImagingConvert rgb2l: L24 with the rounding half), on the resized uint8 values
__device__ inline uint32_t gray_l(uint32_t r, uint32_t g, uint32_t b) { return (19595u * r + 38470u * g + 7471u * b + 0x8000u) >> 16; }

// One env's push, in place.  Item i of a slot = its elements [VP i, VP i + VP) (VP = 1, or 16 bytes' worth); a thread loads item i of slots
// 1 .. depth - 1 (all loads first), then stores them one slot down and the converted observation into the last slot -- or the observation into
// every slot when the env starts anew.  It touches item i only, in every slot: no two threads meet.  `row` may alias itself across slots
// (not __restrict__); obs does not overlap it.
template <typename T, bool GRAY, int VP>
__device__ inline void obs_push_items(T* row, const uint8_t* __restrict__ obs_e, size_t slot, size_t plane, int depth, bool anew, size_t i0, size_t stride) {
  using A = typename ObsBytes<VP * (int)sizeof(T)>::type;     // VP elements of a slot
  using L = typename ObsBytes<VP>::type;                      // their VP bytes of one plane of obs
  const size_t items = slot / VP;
  for (size_t i = i0; i < items; i += stride) {
    union { L l; uint8_t b[VP]; } in[GRAY ? 3 : 1];
    in[0].l = *reinterpret_cast<const L*>(obs_e + i * VP);
    if (GRAY) {
      in[1].l = *reinterpret_cast<const L*>(obs_e + plane + i * VP);
      in[2 % (GRAY ? 3 : 1)].l = *reinterpret_cast<const L*>(obs_e + 2 * plane + i * VP);
    }
    union { A a; T t[VP]; } nv;
#pragma unroll
    for (int q = 0; q < VP; ++q) {
      const uint32_t v = GRAY ? gray_l(in[0].b[q], in[1 % (GRAY ? 3 : 1)].b[q], in[2 % (GRAY ? 3 : 1)].b[q]) : in[0].b[q];
      if (sizeof(T) == 4) nv.t[q] = (T)((float)v / 255.0f);   // NormalizeWrapper, as k_observe*
      else nv.t[q] = (T)v;
    }
    A* s0 = reinterpret_cast<A*>(row) + i;
    if (anew) {
      for (int k = 0; k < depth; ++k) s0[(size_t)k * items] = nv.a;
      continue;
    }
    A keep[DTSIM_OBS_MAX_DEPTH - 1];
#pragma unroll
    for (int k = 0; k < DTSIM_OBS_MAX_DEPTH - 1; ++k)
      if (k < depth - 1) keep[k] = s0[(size_t)(k + 1) * items];
#pragma unroll
    for (int k = 0; k < DTSIM_OBS_MAX_DEPTH - 1; ++k)
      if (k < depth - 1) s0[(size_t)k * items] = keep[k];
    s0[(size_t)(depth - 1) * items] = nv.a;
  }
}

// Grid: N x blocks_per_env workgroups, an env's workgroups stride over its items.  vec: 16-byte slot accesses (the launcher checked the bases
// and the slot size), else element by element.  Workgroups of envs with mask[e] == 0 leave at once (mask null: every env); first[e] != 0
// (first null: none) replicates the observation into every slot.
template <typename T, bool GRAY>
__global__ __launch_bounds__(256) void k_obs_push(T* stack, const uint8_t* __restrict__ obs, size_t plane, int depth, int blocks_per_env,
                                                  const uint8_t* __restrict__ first, const uint8_t* __restrict__ mask, int vec) {
  const int e = blockIdx.x / blocks_per_env;
  if (mask && !mask[e]) return;
  const bool anew = first && first[e];
  const size_t slot = (GRAY ? 1 : 3) * plane;
  T* row = stack + (size_t)e * depth * slot;
  const uint8_t* obs_e = obs + (size_t)e * 3 * plane;
  const size_t i0 = (size_t)(blockIdx.x % blocks_per_env) * 256 + threadIdx.x, stride = (size_t)blocks_per_env * 256;
  if (vec) obs_push_items<T, GRAY, 16 / (int)sizeof(T)>(row, obs_e, slot, plane, depth, anew, i0, stride);
  else obs_push_items<T, GRAY, 1>(row, obs_e, slot, plane, depth, anew, i0, stride);
}

// ---- weighted frame blend (dtsim_blend_frames): out[j] = sum over i of w[i] f[i][j], over D = sum of w[i] ----
// S / D rounded half up is (S + D / 2) / D in integer division (for odd D the dropped half never reaches the next multiple of D).  With
// x = S + D / 2 < 2^16 + 2^7, D <= 256 and M = 2^25 / D + 1 = (2^25 + r) / D, 0 < r <= D: x M / 2^25 = x / D + x r / (2^25 D), and x r < 2^25, so
// the excess stays below 1 / D and the floor is that of x / D.  ((x << 7) M) >> 32 is one v_mul_hi_u32 (x << 7 < 2^24).
__device__ inline uint32_t blend_round(uint32_t S, uint32_t half, uint32_t M) { return __umulhi((S + half) << 7, M); }

// One env's blend.  Chunk c of a frame = bytes [16 c, 16 c + 16); the env's workgroups stride over the chunks.  vec: one 16-byte load per input, all
// issued before the first use, four bytes at a time in two 16-bit lanes per multiply-add (a lane holds at most 255 D < 2^16: it never carries), one
// 16-byte store (uint8) or four (float32); else the chunk's bytes one by one.  out may be one of the inputs (uint8): an element's inputs are all
// loaded before it is stored, and no other thread touches it.  NF = B.n, the number of inputs (compile-time: straight-line code, the loads back to back).
// The float32 instantiations load the inputs nontemporally (measured, profiles/motion_blur_timing.txt: 5 % faster there, 1 % slower with uint8 out).
template <typename T, int NF>
__global__ __launch_bounds__(256) void k_blend_frames(T* out, BlendArgs B, size_t frame_bytes, int blocks_per_env, const uint8_t* __restrict__ mask, int vec,
                                                      uint32_t D, uint32_t M) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  const int e = blockIdx.x / blocks_per_env;
  if (mask && !mask[e]) return;
  const size_t base = (size_t)e * frame_bytes;
  const uint32_t half = D >> 1;
  const float fD = (float)D;
  const size_t stride = (size_t)blocks_per_env * 256 * 16;
  for (size_t off = ((size_t)(blockIdx.x % blocks_per_env) * 256 + threadIdx.x) * 16; off < frame_bytes; off += stride) {
    if (vec) {
      u32x4 v[NF];
#pragma unroll
      for (int k = 0; k < NF; ++k) {
        const u32x4* p = reinterpret_cast<const u32x4*>(B.f[k] + base + off);
        v[k] = sizeof(T) == 4 ? __builtin_nontemporal_load(p) : *p;
      }
      u32x4 packed;
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        uint32_t lo = 0, hi = 0;                       // the sums of bytes 0 and 2 / of bytes 1 and 3 of dword d
#pragma unroll
        for (int k = 0; k < NF; ++k) {
          lo = __umul24(v[k][d] & 0x00FF00FFu, B.w[k]) + lo;
          hi = __umul24((v[k][d] >> 8) & 0x00FF00FFu, B.w[k]) + hi;
        }
        if (sizeof(T) == 4) {                          // one IEEE division per element
          f32x4 q;
          q[0] = (float)(lo & 0xFFFFu) / fD; q[1] = (float)(hi & 0xFFFFu) / fD; q[2] = (float)(lo >> 16) / fD; q[3] = (float)(hi >> 16) / fD;
          reinterpret_cast<f32x4*>(out + base + off)[d] = q;
        } else {
          packed[d] = blend_round(lo & 0xFFFFu, half, M) | (blend_round(hi & 0xFFFFu, half, M) << 8) | (blend_round(lo >> 16, half, M) << 16) |
                      (blend_round(hi >> 16, half, M) << 24);
        }
      }
      if (sizeof(T) == 1) *reinterpret_cast<u32x4*>(out + base + off) = packed;
      continue;
    }
    const size_t n = frame_bytes - off < 16 ? frame_bytes - off : 16;
    for (size_t i = off; i < off + n; ++i) {
      uint32_t S = 0;
#pragma unroll
      for (int k = 0; k < NF; ++k) S = __umul24((uint32_t)B.f[k][base + i], B.w[k]) + S;
      if (sizeof(T) == 4) out[base + i] = (T)((float)S / fD);
      else out[base + i] = (T)blend_round(S, half, M);
    }
  }
}

}  // namespace

// the instantiation for B.n inputs (NF counts down from DTSIM_BLEND_MAX to it)
template <typename T, int NF = DTSIM_BLEND_MAX>
static void blend_launch(hipStream_t s, dim3 grid, T* out, const BlendArgs& B, size_t frame_bytes, int per_env, const uint8_t* mask, int vec, uint32_t D, uint32_t M) {
  if (B.n == NF) hipLaunchKernelGGL((k_blend_frames<T, NF>), grid, dim3(256), 0, s, out, B, frame_bytes, per_env, mask, vec, D, M);
  else if constexpr (NF > 1) blend_launch<T, NF - 1>(s, grid, out, B, frame_bytes, per_env, mask, vec, D, M);
}

void dt_launch_blend_frames(hipStream_t s, int N, void* out, const BlendArgs& B, size_t frame_bytes, bool f32, const uint8_t* mask) {
  const size_t chunks = (frame_bytes + 15) / 16;
  const int per_env = (int)std::min<size_t>((chunks + 255) / 256, 16);   // (as dt_launch_copy_rows)
  uintptr_t bits = reinterpret_cast<uintptr_t>(out) | frame_bytes;
  uint32_t D = 0;
  for (int i = 0; i < B.n; ++i) { bits |= reinterpret_cast<uintptr_t>(B.f[i]); D += B.w[i]; }
  const int vec = (bits & 15) == 0;
  const uint32_t M = (1u << 25) / D + 1;
  const dim3 grid((unsigned)((size_t)N * per_env));
  if (f32) blend_launch(s, grid, static_cast<float*>(out), B, frame_bytes, per_env, mask, vec, D, M);
  else blend_launch(s, grid, static_cast<uint8_t*>(out), B, frame_bytes, per_env, mask, vec, D, M);
}

void dt_launch_copy_rows(hipStream_t s, int N, void* dst, const void* src, size_t row_bytes, const uint8_t* mask) {
  const size_t chunks = (row_bytes + 15) / 16;
  const int per_row = (int)std::min<size_t>((chunks + 255) / 256, 16);   // (a selected row: up to 16 workgroups; the grid stays small when few are)
  const int vec = ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src) | row_bytes) & 15) == 0;
  hipLaunchKernelGGL(k_copy_rows, dim3((unsigned)((size_t)N * per_row)), dim3(256), 0, s, static_cast<uint8_t*>(dst), static_cast<const uint8_t*>(src),
                     row_bytes, per_row, mask, vec);
}

void dt_launch_boxes(hipStream_t s, int N, const uint8_t* inst, int oh, int ow, int32_t* out, const uint8_t* mask) {
  if (N <= 0) return;
  hipLaunchKernelGGL(k_boxes, dim3((unsigned)N), dim3(256), 0, s, inst, oh, ow, out, mask);
}

void dt_launch_obs_push(hipStream_t s, int N, void* stack, const uint8_t* obs, int depth, int out_h, int out_w, bool f32, bool gray,
                        const uint8_t* first, const uint8_t* mask) {
  const size_t plane = (size_t)out_h * out_w, slot = (gray ? 1 : 3) * plane, esz = f32 ? 4 : 1;
  // 16-byte slot accesses with the matching 4 (float32) or 16 (uint8) bytes per plane of obs: every slot (and, in grey, every plane of obs)
  // then starts on such a boundary
  const int vec = (reinterpret_cast<uintptr_t>(stack) & 15) == 0 && (slot * esz & 15) == 0 && (reinterpret_cast<uintptr_t>(obs) & (16 / esz - 1)) == 0;
  const size_t items = vec ? slot * esz / 16 : slot;
  const int per_env = (int)std::min<size_t>((items + 255) / 256, 16);    // (as dt_launch_copy_rows: the grid stays small when few envs are selected)
  const dim3 grid((unsigned)((size_t)N * per_env)), block(256);
  if (f32) {
    float* st = static_cast<float*>(stack);
    if (gray) hipLaunchKernelGGL((k_obs_push<float, true>), grid, block, 0, s, st, obs, plane, depth, per_env, first, mask, vec);
    else hipLaunchKernelGGL((k_obs_push<float, false>), grid, block, 0, s, st, obs, plane, depth, per_env, first, mask, vec);
  } else {
    uint8_t* st = static_cast<uint8_t*>(stack);
    if (gray) hipLaunchKernelGGL((k_obs_push<uint8_t, true>), grid, block, 0, s, st, obs, plane, depth, per_env, first, mask, vec);
    else hipLaunchKernelGGL((k_obs_push<uint8_t, false>), grid, block, 0, s, st, obs, plane, depth, per_env, first, mask, vec);
  }
}

void dt_launch_observe(hipStream_t s, const ObservePlan& plan, const ObserveParams& P, const uint8_t* mask) {
  using Kernel = void (*)(ObserveParams, const uint8_t*);
  auto launch = [&](Kernel k, size_t blocks) { hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(OB), plan.lds, s, P, mask); };
  switch (plan.kernel) {
    case DT_OBS_CUBIC:
      launch(mask ? k_observe_cubic<true> : k_observe_cubic<false>, (size_t)P.N * P.oh);
      break;
    case DT_OBS_POW2: {                                // interior pixels, four rows of a column per thread; then the border pixels
      const size_t n_in = (size_t)P.N * ((P.oh - 2 + 3) / 4) * (P.ow - 2), n_b = (size_t)P.N * (2 * P.ow + 2 * (P.oh - 2));
#define DT_OBS_LAUNCH(HN_, SY_) \
      if (P.hn == HN_ && P.vfast == SY_) launch(mask ? k_observe_pow2<HN_, SY_, true> : k_observe_pow2<HN_, SY_, false>, (n_in + OB - 1) / OB);
      DT_OBS_POW2_LIST(DT_OBS_LAUNCH)
#undef DT_OBS_LAUNCH
      launch(mask ? k_observe_border<true> : k_observe_border<false>, (n_b + OB - 1) / OB);
      break;
    }
    case DT_OBS_STAGED:
      launch(mask ? k_observe<true> : k_observe<false>, (size_t)P.N * ((P.oh + P.rows_per_block - 1) / P.rows_per_block));
      break;
  }
}
