// render_v3.hip -- the rasters of the BASELINE configurations (256 x 256 tile textures), one unit beside render.hip: k_raster_v3 with its exact path
// resolve_region_v3 (first half, below), then k_raster_v3dr with its exact path k_resolve_dr (second half, with its own header further down),
// and one launcher per pipe with the dynamic-LDS sizes beside it (end of the file).
// k_raster_v3: the quad-record one-ray path of k_raster_q (render.hip) on an instruction diet
// (shares EnvCam / EnvFast / EnvQ / PixTab / SampTab -- render_records.h -- and the queue protocol with k_raster_q).
// The workgroup map, the LDS tile table fill, the object masks and spxy are raster_common.h's ("scaffolding shared by the rasters"), and so are resolve_region_v3's
// entry decode, sample ownership, ground-quad rules and store_rgb ("... by the exact paths"); the queue appends, push_obj, the transpose and the hand-over epilogue are this kernel's own copies.
//
// Replaces the same reference code as k_raster_q: simulator.py:1853-1884 (tile quads, GL_LINEAR / GL_REPEAT),
// simulator.py:1806-1812 (ground quad), graphics.py:172-251 (4x MSAA resolve), distortion.py:85-125 (remap, folded in).
//
// As built (what changed against k_raster_q, profiles/r02: 43.7 VALU instructions per pixel -> 36.9):
//   * tile table in LDS rows of 1 KB: block byte offset at (tz << 10 | tx << 2) + map column offset, the record-offset mask 512
//     bytes behind it, so that the address is ONE v_perm (both tile bytes) + one v_lshl_add and both come back from one
//     ds_read2_b32;
//   * (round 6) the quad coordinates are snapped to 256ths of a texel by one packed add of 32768 (raster_common.h, Q8_SNAP) -- GL's own
//     coordinate precision -- and tile, cell and fraction are bytes of the sum's bit pattern: no v_cvt_flr_i32 / v_fract; the byte-weight
//     filter (quad_weights8) takes the fractions as 0..255.  Every floating-point step that feeds the snap or the weights is written with
//     explicit fused multiply-adds under `fp contract(off)`: the peeled first env, the loop and the exact path must round alike;
//   * the env loop exists in two instantiations: blocks of candidate pixels only (no clear-colour / border selects at all)
//     and mixed blocks (horizon band, image border); clamping into the padded grid is a third, wave-uniform choice per env;
//   * output: the colour bytes (bits 16..23 of the three filter sums) go to the wavefront's LDS transpose buffer with
//     ds_write_b8_d16_hi -- no packing instructions at all -- and come back as 16-byte pieces of the block's two frame rows
//     (48 lanes x 16 B, stored through a buffer descriptor whose base is the env's frame: scalar address arithmetic);
//   * pixel <-> lane map: a slot (= one record-load instruction) is a 32 x 2 pixel SUB-BLOCK of the 128 x 2 wavefront block,
//     the four slots side by side: the 64 records of one load come from a compact patch of the texture -- fewer distinct cache
//     lines per instruction, which is what the texture unit charges for (tools/ubench/fmt_load.hip: ~ 18 cycles for a gather
//     whose lanes share 8 lines, ~ 115 when every lane has its own; tools/gather_lines_model.py: 15 lines on average).
// Variants that were built, measured and REMOVED again (the numbers are in profiles/, the code in the git history): full dummy
// blocks for off-grid tiles, a per-(block, env) ground-only class, a two-stage software pipeline, the exact path pooled per
// workgroup, lane <-> four consecutive pixels, 64-pixel row slots, dword transposes, the v_dot2_u32_u16 filter on
// format-converting loads, a late wait on the transpose read-back, a persistent launch, other frame-tile launch orders
// (profiles/r03_variants_ab.txt, r04_variants_ab.txt, r04_wave_spans.txt, r05_variants_ab.txt).
#include "raster_common.h"

// Buffer stores through a raw descriptor (k_raster_v3 / k_raster_v3dr frame rows): clang has no builtin with a scalar-base form, the LLVM
// intrinsics are reached by name (their immediates must be literals after inlining).
typedef int v3_i32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t v3_u32x3 __attribute__((ext_vector_type(3)));
__device__ void v3_buf_store_v3i32(v3_u32x3 data, v3_i32x4 rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.store.v3i32");
typedef uint32_t v3_u32x4 __attribute__((ext_vector_type(4)));
__device__ void v3_buf_store_v4i32(v3_u32x4 data, v3_i32x4 rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.store.v4i32");
#define V3_RSRC_W3 0x00027000      // raw buffer descriptor word 3
__device__ inline v3_i32x4 v3_rsrc(const void* p, uint32_t bytes) {
  v3_i32x4 r;
  r.x = (int)(uint32_t)reinterpret_cast<uintptr_t>(p); r.y = (int)((reinterpret_cast<uintptr_t>(p) >> 32) & 0xFFFFu); r.z = (int)bytes; r.w = V3_RSRC_W3;
  return r;
}

namespace {

#ifndef DT_V3_WAVES
#define DT_V3_WAVES 6              // wavefronts per SIMD: 80 VGPRs without scratch (round 4: 5 -> 6 with the buffer-descriptor store)
#endif
#ifndef DT_V3_WAVES_OBJ
#define DT_V3_WAVES_OBJ (DT_V3_WAVES - 1)   // the mesh-object instantiation: 111 VGPRs; one more wavefront spills 76 B and is 1.7 % slower
#endif
#define DT_V3_SW (DT_V3_WW / 4)                       // pixel columns of a slot's sub-block (four slots side by side)
#define V3_ROWS (WAVE_PIX / DT_V3_WW)                 // rows of a wavefront block
#define V3_WX (DT_TILE_W / DT_V3_WW)                  // wavefront blocks side by side in the workgroup tile
static_assert(PPT == 4 && DT_V3_WW == 128 && DT_V3_WW == WAVE_W && DT_TILE_W % DT_V3_WW == 0 && (RB / 64) % V3_WX == 0 &&
              V3_ROWS * ((RB / 64) / V3_WX) == DT_TILE_H, "k_raster_v3 / k_raster_v3dr: 128 x 2 wavefront blocks tiling the 128 x 8 workgroup tile "
              "(the generic k_resolve / k_resolve_obj decode the queue entries as row-major pixel numbers of such a block)");
#define V3_SEL_TILE 0x0c0c0602u                       // v_perm: (byte 2 of Z) << 8 | byte 2 of X -- the tile bytes of the snapped coordinates (Q8_SNAP)
#define V3_WAVE_LDS RQ_LIST                           // dwords of LDS per wavefront: the transpose buffer
// pixel number (row-major in the wavefront block) of slot k of lane l; V3_XO*: byte distance of slot k from slot 0 in the transpose buffer
static_assert(DT_V3_WW == 4 * DT_V3_SW && 64 % DT_V3_SW == 0, "four slots side by side");
#define V3_PIX(k, l) (((l) / DT_V3_SW) * DT_V3_WW + (k) * DT_V3_SW + ((l) % DT_V3_SW))
#define V3_XP_LANE(l) (((l) / DT_V3_SW) * DT_V3_WW + ((l) % DT_V3_SW))
#define V3_XO1 "96"                                   // 3 * DT_V3_SW bytes per slot (DT_V3_WW = 128)
#define V3_XO1G "97"
#define V3_XO1B "98"
#define V3_XO2 "192"
#define V3_XO2G "193"
#define V3_XO2B "194"
#define V3_XO3 "288"
#define V3_XO3G "289"
#define V3_XO3B "290"
#define V3_ROW16 (DT_V3_WW * 3 / 16)                  // 16-byte pieces of a block row

struct U4 { uint32_t a, b, c, d; };                   // k_raster_v3's row fragment: 16 bytes on 48 lanes (12 bytes, d unused, when the image is not a whole number of blocks wide)
#define V3_XPOSE_WAIT " s_waitcnt lgkmcnt(0)"

// One pixel's colour as two dwords: R in byte 0 and B in byte 2 of `rb` -- what ds_write_b8 / ds_write_b8_d16_hi can store without
// a shift -- and G in byte 1 of `g`, where the byte-weight filter (quad_filter, raster_common.h) leaves each channel of its dot products:
// rb = v_perm(vb, vr), g = vg; the transpose brings the greens of two pixels into bytes 0 and 2 of one register with one v_perm.
struct C3 { uint32_t rb, g; };
__device__ inline C3 c3_of_rgb(const uint32_t rgb) { return C3{rgb, rgb}; }   // rgb = 0x00BBGGRR

struct GndK { float Cx, Cz, sa, ca, kg, gnd[3], base[3], dif[3], gndl[4], pad[2]; };   // ground-quad constants of one env

// ---- resolve_region_v3: exact path of k_raster_v3 -----------------------------------------------------------------------------
// Called by every wavefront of k_raster_v3 at the end of its env loop on ITS OWN queue region, as resolve_region_q (render.hip) is by
// k_raster_q, with two differences:
//   * no interior test (round 6): every entry takes the four samples, and the queue entries ARE the list -- no compaction, no LDS round
//     trip.  The test resolved 30 % of the entries with one record but cost as much as the four-sample phase (a table gather, a record
//     gather and two patches per entry, latency-bound): without it the exact path is 0.10 ms shorter (profiles/r06_variants_ab.txt
//     block E); an interior pixel's four samples give the one-ray colour anyway;
//   * no list of distinct primitives (round 3).  The colour of a pixel is the sum over its four samples of the shade of the sample's
//     primitive AT THE PIXEL CENTRE (GL: graphics.py:172-251), so every tile sample adds the integer filter of ITS tile's record at the
//     centre cell (same cell index and weights for every tile: the blocks share one cell grid; a sample that is not on a tile reads the
//     all-zero record 0) to one accumulator per channel -- 6 v_dot4 per sample, exact -- and sky / ground samples add their colour once
//     per count.  Tile look-ups go by v_perm like the env loop's; the +-50 m ground-quad test is made in quad coordinates.
// s_qt: k_raster_v3's LDS tile table (block offset at (tz << 10 | tx << 2) + the map's column offset EnvQ.tab3, the record-offset
// mask 512 bytes behind it); s_envq: the EnvQ records of the chunk's 64 positions, staged in LDS by the workgroup -- an entry's constants
// are three ds_read_b128 instead of three 16-byte gathers through the texture unit; (bx0, by0): the origin of the wavefront's block.
// LIGHT: per-env lights (EnvL in render order, envl): the lit factor of the tile plane is env_lit8's, per entry.
template <bool LIGHT>
__device__ inline void resolve_region_v3(const RenderParams& R, const EnvCam* __restrict__ cams, const SampTab* __restrict__ samptab,
                                         const uint8_t* __restrict__ qtex, const uint32_t* s_qt, const uint16_t* w_queue, const int n,
                                         const int e0, const int bx0, const int by0, const int lane, const uint4* s_envq,
                                         const EnvL* __restrict__ envl) {
  const int npix = R.W * R.H;
  const float Sf = (float)(1 << R.qlog2), lo = 0.5f * Sf;
  const char* qtb = reinterpret_cast<const char*>(s_qt);
  for (int r0 = 0; r0 < n; r0 += RQ_LIST) {          // wave-uniform: rounds of up to RQ_LIST entries
    const int n_list = min(n - r0, RQ_LIST);
    for (int l0 = 0; l0 < n_list; l0 += 64) {          // wave-uniform
      const bool have = l0 + lane < n_list;
      // the entries were written by this wavefront a moment ago: bypass the (possibly stale) L1 line
      const uint32_t ent = have ? (uint32_t)__builtin_nontemporal_load(w_queue + r0 + l0 + lane) : 0u;
      const int lp = qe_pixel(ent), el = qe_envpos(ent);
      const int pix = have ? (by0 + lp / DT_V3_WW) * R.W + bx0 + lp % DT_V3_WW : 0;
      const SampTab sp = samptab[pix];
      PixTab pt;                                       // the PixTab's hit and lit factor, from the SampTab (one table, two 16-byte loads: {dlr[2], dlf[2]}, {flags, lr_bits, lf_bits, lit_bits})
      pt.lr = __uint_as_float(sp.lr_bits); pt.lf = __uint_as_float(sp.lf_bits); pt.lit = __uint_as_float(sp.lit_bits); pt.mi = 0u;
      // the env's constants as three of EnvQ's four 16-byte pieces -- [0] = {A, B, Cx, Cz}, [1] = {Xhi, Zhi, tab_b, pitch4}, ([2] = {hor_rgb, sky[3]},)
      // [3] = {reach, env, tab3, qpm_bits} -- (round 5: the exact path is bound by the NUMBER of vector-memory instructions it issues)
      const uint4* fl = s_envq + el * 4;
      const uint4 a4 = fl[0];
      const float4 qa = make_float4(__uint_as_float(a4.x), __uint_as_float(a4.y), __uint_as_float(a4.z), __uint_as_float(a4.w));
      const uint4 qb = fl[1], qd = fl[3];
      const float A = qa.x, B = qa.y, Cx = qa.z, Cz = qa.w, Xhi = __uint_as_float(qb.x), Zhi = __uint_as_float(qb.y);
      const uint32_t tab = qd.z;
      const int e = (int)qd.y;
      const float4* c4 = reinterpret_cast<const float4*>(cams + e);   // EnvCam as 16-byte pieces: [2] = {ty, hor[3]}, [3] = {gnd[3], base0}, [4] = {base1, base2, dif0, dif1}, [5] = {dif2, L..}, [6] = {L3, gndl[0..2]}, [7] = {gndl3, ..}
      const float wCy = default_cam((float)R.W / (float)R.H).Cy;      // shared camera: the same height for every env (what k_cam_setup wrote)
      const float kg = (wCy - GROUND_Y) / wCy;
      const float qpm = __uint_as_float(qd.w);                           // quad cells per metre of the env's map
      const float goff = (float)DT_QRING * Sf + 0.5f, ghalf = GROUND_HALF * qpm;   // world 0 and 50 m in padded quad coordinates
      const float Xu = fmaf(pt.lf, B, fmaf(pt.lr, A, Cx)), Zu = fmaf(pt.lf, -A, fmaf(pt.lr, B, Cz));
      const uint32_t xic = q8_bits(Xu), zic = q8_bits(Zu);              // the centre's snapped coordinates: q8_rec256 works on these bits
      float lit8 = (pt.lit > 0.f ? pt.lit : 0.55f) * Q8_LIT;
      if constexpr (LIGHT) { if (pt.lit > 0.f) lit8 = env_lit8(envl[min(e0 + el, R.N - 1)], pt.lr, pt.lf, env_base8()); }
      const uint32_t W8 = quad_weights8(q8_frac(xic), q8_frac(zic), lit8);
      uint32_t aS[3] = {0u, 0u, 0u};                   // sum over the samples of the byte-weight filter of each sample's record
      int n_sky = 0, n_gnd = 0;
      float gX = 0.f, gZ = 0.f;                        // ground hit (quad coordinates) of the lowest-index ground sample
      uint4 rec = make_uint4(0u, 0u, 0u, 0u);
      uint32_t raddr_prev = 0u;
#pragma unroll
      for (int s = 3; s >= 0; --s) {
        const uint32_t hr = sp.dlr[s >> 1], hf = sp.dlf[s >> 1];
        const float slr = pt.lr + __half2float(__ushort_as_half((unsigned short)((s & 1) ? hr >> 16 : hr)));
        const float slf = pt.lf + __half2float(__ushort_as_half((unsigned short)((s & 1) ? hf >> 16 : hf)));
        const float Xs = fmaf(slf, B, fmaf(slr, A, Cx)), Zs = fmaf(slf, -A, fmaf(slr, B, Cz));
        uint32_t tb, sel;
        const bool s_in = v3_sample_owner(Xs, Zs, lo, Xhi, Zhi, qtb, tab, tb, sel);
        const bool is_tile = have & (((sp.flags >> s) & 1u) != 0u) & s_in & (tb != 0u);
        const float Xg = ground_quad_at(kg, Xs, Cx), Zg = ground_quad_at(kg, Zs, Cz);
        const bool is_gnd = have & !is_tile & (((sp.flags >> (4 + s)) & 1u) != 0u) & ground_quad_in(Xg, goff, ghalf) & ground_quad_in(Zg, goff, ghalf);
        n_gnd += is_gnd; n_sky += !(is_tile | is_gnd);
        if (is_gnd) { gX = Xg; gZ = Zg; }
        // one record per DISTINCT tile among the pixel's samples (round 4: the path is texture-unit heavy, its gathers fully divergent;
        // the samples of most edge pixels share a tile, or are not on a tile at all): a lane loads only when its address changes
        const uint32_t raddr = is_tile ? (tb | q8_rec256(xic, zic, sel)) : 0u;
        if (s == 3 || raddr != raddr_prev) rec = *reinterpret_cast<const uint4*>(qtex + raddr);
        raddr_prev = raddr;
        aS[0] = __builtin_amdgcn_udot4(rec.x, W8, aS[0], false);
        aS[1] = __builtin_amdgcn_udot4(rec.y, W8, aS[1], false);
        aS[2] = __builtin_amdgcn_udot4(rec.z, W8, aS[2], false);
      }
      float acc[3];
      float4 hc = make_float4(0.f, 0.f, 0.f, 0.f);
      if (__ballot(n_sky > 0)) hc = c4[2];             // wave-uniform: the horizon colour only where some sample sees the sky
      acc[0] = fmaf((float)n_sky, hc.y, (float)aS[0] * (1.f / 256.f));
      acc[1] = fmaf((float)n_sky, hc.z, (float)aS[1] * (1.f / 256.f));
      acc[2] = fmaf((float)n_sky, hc.w, (float)aS[2] * (1.f / 256.f));
      if (__ballot(n_gnd > 0)) {                       // wave-uniform: shade the ground quad (lit at its corners, bilinear)
        if (pt.lit > 0.f && (pt.lr != 0.f || pt.lf != 0.f)) { gX = fmaf(kg, Xu - Cx, Cx); gZ = fmaf(kg, Zu - Cz, Cz); }   // the centre ray hits the planes
        const float hs = 0.5f / ghalf;
        const float a_ = fminf(fmaxf(fmaf(gX - goff, hs, 0.5f), 0.f), 1.f), b_ = fminf(fmaxf(fmaf(gZ - goff, hs, 0.5f), 0.f), 1.f);
        const float4 q3 = c4[3], q4 = c4[4], q5 = c4[5], q6 = c4[6], q7 = c4[7];
        const float ndl = ground_corner_ndl(a_, b_, q6.y, q6.z, q6.w, q7.x);
        const float ng = (float)n_gnd;
        acc[0] += ng * ground_lit(q3.x, q3.w, q4.z, ndl);
        acc[1] += ng * ground_lit(q3.y, q4.x, q4.w, ndl);
        acc[2] += ng * ground_lit(q3.z, q4.y, q5.x, ndl);
      }
      const float o[3] = {0.25f * acc[0], 0.25f * acc[1], 0.25f * acc[2]};
      if (have) store_rgb(R.frames, npix, e, pix, pack_rgb(o));
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

// LIGHT (DTSIM_F_LIGHT_CAPTURE): every env lit by its own light (envl: EnvL in render order, [N + 1]) -- the lit factor of a (pixel, env) is
// env_lit8's, two pixels per packed operation, in place of the PixTab's shared one; the PixTab's lit keeps its class role (< 0 outside the
// image, 0 sky, > 0 candidate).  Without LIGHT envl is not read.  SUB: the masked pass, as k_raster_q<.., SUB>.
template <bool OBJ, bool LIGHT = false, bool SUB = false>
__global__ __launch_bounds__(RB) __attribute__((amdgpu_waves_per_eu(OBJ ? DT_V3_WAVES_OBJ : DT_V3_WAVES, OBJ ? DT_V3_WAVES_OBJ : DT_V3_WAVES)))
void k_raster_v3(RenderParams R, const EnvCam* __restrict__ cams, const EnvFast* __restrict__ fasts, const EnvQ* __restrict__ envq,
                 const EnvV* __restrict__ envv, uint8_t* __restrict__ frames, const uint8_t* __restrict__ qtex, const float4* __restrict__ lut,
                 const PixTab* __restrict__ pixtab, const SampTab* __restrict__ samptab, const uint32_t* __restrict__ qtiles,
                 uint16_t* __restrict__ queue, int32_t* __restrict__ qcount, const EnvL* __restrict__ envl) {
  extern __shared__ uint32_t s_mem[];
  uint32_t* s_qt = s_mem;                             // [q3_rows][V3_TAB_PITCH] block byte offsets
  const int tid = threadIdx.x;
  const int npix = R.W * R.H;
  const int tiles_x = (R.W + DT_TILE_W - 1) / DT_TILE_W, n_tiles = tiles_x * ((R.H + DT_TILE_H - 1) / DT_TILE_H);
  RasterWg wg = raster_wg<SUB, /*SCALAR=*/true, /*TICKET=*/!SUB>(R, n_tiles, blockIdx.x);   // (tile and chunk in scalar registers: the env loop's counter and the EnvQ addresses follow)
  if (!wg.live && !wg.claims) return;
  int* s_claim = reinterpret_cast<int*>(s_mem + R.q3_rows * V3_TAB_PITCH);   // two words of the first transpose buffer, idle until the env loop
  const int ticket = wg.claims ? raster_claim_issue(R, blockIdx.x, tid, wg) : 0;   // (the table fill does not depend on the item: it hides the round trip)
  v3_fill_tile_table(R, qtiles, s_qt, tid);
  if (wg.claims) {                                     // workgroup-uniform
    raster_claim_finish(R, n_tiles, blockIdx.x, ticket, s_claim, tid, wg);
    if (!wg.live) return;                              // every list is dry
  }
  const int NL = wg.NL, tile = wg.tile, rwg = wg.rwg(n_tiles), e0 = wg.e0(), e1 = wg.e1();
  // the EnvQ records of the chunk's positions (the exact path reads them per entry: resolve_region_v3), 16 bytes per thread
  uint4* s_envq = reinterpret_cast<uint4*>(s_mem + R.q3_rows * V3_TAB_PITCH + (RB / 64) * V3_WAVE_LDS);
  static_assert(ENVS_PER_BLOCK * 4 <= RB, "one 16-byte piece per thread");
  if (tid < ENVS_PER_BLOCK * 4) s_envq[tid] = reinterpret_cast<const uint4*>(envq + min(e0 + tid / 4, NL - 1))[tid & 3];
  __syncthreads();

  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;   // wave index in a scalar register: block origin, queue region, LDS slices
  const int bx0 = (tile % tiles_x) * DT_TILE_W + (wave % V3_WX) * DT_V3_WW;   // origin of the wavefront's block
  const int by0 = (tile / tiles_x) * DT_TILE_H + (wave / V3_WX) * V3_ROWS;
  const float lo = 0.5f * 256.f;

  // per-pixel invariants (shared camera) from the PixTab
  float lr[PPT], lf[PPT], lit[PPT];
  uint32_t Mi[PPT];
  bool cand[PPT], gok[PPT], valid[PPT];
  uint32_t spxy[PPT];
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    PixTab t{0.f, 0.f, -1.f, 0xFFFFu};
    const int x = bx0 + V3_PIX(k, lane) % DT_V3_WW, y = by0 + V3_PIX(k, lane) / DT_V3_WW;
    const bool inimg = x < R.W && y < R.H;
    if (inimg) t = pixtab[y * R.W + x];
    lr[k] = t.lr; lf[k] = t.lf; lit[k] = fmaxf(t.lit, 0.f) * Q8_LIT; Mi[k] = t.mi;   // lit / 256: the fractions below are bytes (quad_weights8)
    valid[k] = t.lit >= 0.f; cand[k] = t.lit > 0.f; gok[k] = (t.mi & 0xFFFFu) != 0xFFFFu;
    spxy[k] = 0u;
    if (OBJ && inimg) spxy[k] = spxy_pack(lut[y * R.W + x], R.W, R.H);
  }
  bool any_cand = false;
#pragma unroll
  for (int k = 0; k < PPT; ++k) any_cand |= cand[k];

  uint16_t* w_queue = queue + ((size_t)rwg * (RB / 64) + wave) * QREGION;
  int qn = 0, qo = 0;                                  // plane-edge entries (front of the region), object-box entries (back)
  int qend_v = 0;
  uint32_t* w_lds = s_mem + R.q3_rows * V3_TAB_PITCH + wave * V3_WAVE_LDS;   // transpose buffer
  // the lane STORES pixels 4 * lane .. 4 * lane + 3 of the block (12 bytes), whatever the compute map
  const int st_x = bx0 + (lane * 4) % DT_V3_WW, st_y = by0 + (lane * 4) / DT_V3_WW;
  const bool st_ok = st_x < R.W && st_y < R.H;       // W % 4 == 0 (launch precondition): all four pixels or none
  const size_t st_off = ((size_t)st_y * R.W + st_x) * 3;

  ChunkObjMasks<OBJ> objmasks;
  objmasks.load(R, e0, e1, n_tiles * 4, tile * 4 + wave, lane);
  // pixels of the block inside the screen boxes of the objects in `om` -> appended from the far end of the region; oem[k]: their lanes
  auto push_obj = [&](const int e, const uint32_t env, unsigned long long om, unsigned long long oem[PPT], const unsigned long long em[PPT]) __attribute__((always_inline)) {
    const ObjBox* boxes = R.objbox + (size_t)env * DTSIM_MAX_OBJECTS;
    bool oedge[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) oedge[k] = false;
    // the pixel centres are kept as fp16 (spxy): the margin covers the MSAA sample offset (0.375 px) + their rounding (half an fp16
    // ulp of the largest coordinate: 0.25 px below 1024, 0.5 below 2048, 1 below 4096) - the 0.5 px the triangle boxes are padded by
    const float obj_mrg = (R.W > 2048 || R.H > 2048) ? 0.95f : (R.W > 1024 || R.H > 1024) ? 0.45f : 0.3f;
    float sx[PPT], sy[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) spxy_unpack(spxy[k], sx[k], sy[k]);
    while (om) {                                     // wave-uniform
      const int o = __builtin_ctzll(om);
      const ObjBox ob = boxes[o];
      om &= om - 1ull;
#pragma unroll
      for (int k = 0; k < PPT; ++k)
        if (valid[k] && sx[k] >= ob.bx0 - obj_mrg && sx[k] <= ob.bx1 + obj_mrg && sy[k] >= ob.by0 - obj_mrg && sy[k] <= ob.by1 + obj_mrg) oedge[k] = true;
    }
    bool any_oedge = false;
#pragma unroll
    for (int k = 0; k < PPT; ++k) any_oedge |= oedge[k];
    if (__ballot(any_oedge)) {
      const uint32_t etag = (uint32_t)(e - e0) << 8;
#pragma unroll
      for (int k = 0; k < PPT; ++k) {
        const bool ek = oedge[k];
        const unsigned long long mk = __ballot(ek);
        oem[k] = mk;
        if (ek) {
          const int rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u));
          w_queue[QREGION - 1 - (qo + rank)] = (uint16_t)(etag | (__builtin_amdgcn_inverse_ballot_w64(em[k]) ? QE_PLANE_EDGE : 0u) | (uint32_t)V3_PIX(k, lane));
        }
        qo += __popcll(mk);
      }
    }
  };
  // Frame rows go out through a buffer descriptor: base = the env's frame (64-bit SCALAR arithmetic), the lane's byte offset in one
  // register for the whole kernel; lanes without pixels carry an offset beyond num_records and the bounds check drops them.
  const uint32_t st_voff = st_ok ? (uint32_t)st_off : 0x80000000u;
  const uint32_t frame_bytes = (uint32_t)npix * 3u;
  // 16-byte pieces: the block's two rows are 384 bytes each = 24 lanes x 16 bytes; lane l < 48 stores bytes 16 * (l % 24) .. of row l / 24
  const bool wide = __builtin_amdgcn_readfirstlane((int)(R.W % DT_V3_WW == 0 && R.H % V3_ROWS == 0)) != 0;   // wave-uniform: every block lies inside the image
  const uint32_t st_voff16 = lane < 48 ? (uint32_t)(((size_t)(by0 + lane / V3_ROW16) * R.W + bx0) * 3u) + (uint32_t)(lane % V3_ROW16) * 16u : 0x80000000u;
  auto store = [&](const uint32_t env, const U4& o) __attribute__((always_inline)) {
    const v3_i32x4 fr = v3_rsrc(frames + (size_t)env * frame_bytes, frame_bytes);
    if (wide) v3_buf_store_v4i32(v3_u32x4{o.a, o.b, o.c, o.d}, fr, (int)st_voff16, 0, 2);   // wave-uniform; aux 2 = nt
    else v3_buf_store_v3i32(v3_u32x3{o.a, o.b, o.c}, fr, (int)st_voff, 0, 2);
  };
  // ---- pixel colours (byte 2 of three dwords each) of the four slots -> the lane's 12 bytes of the frame row
  // (LDS byte addresses for the inline DS instructions: the low half of a flat LDS pointer is the LDS offset)
  const uint32_t xp_wr = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(w_lds)) + (uint32_t)V3_XP_LANE(lane) * 3u;    // slot 0's R
  // read-back: the lane's 12 bytes -- or, in the 16-byte form, bytes 16 * (lane % 48) .. (lanes 48..63 re-read and never store)
  const uint32_t xp_rd = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(w_lds)) + (wide ? (uint32_t)(lane % 48) * 16u : (uint32_t)lane * 12u);
  auto transpose = [&](const C3 c[PPT]) __attribute__((always_inline)) -> U4 {
    U4 out;
    out.d = 0u;
    // slot k of lane l is pixel k * 64 + l: byte address 3 * (k * 64 + l) + channel.  DS operations of one wavefront
    // execute in order, so the reads below see the writes; the read waits for its data itself (the compiler does not
    // track the counters of inline assembly).
    uint2 rd01, rd23;                                // (operand numbering: two outputs + a filler input keep the first colour at %4)
    const uint32_t g01 = __builtin_amdgcn_perm(c[1].g, c[0].g, 0x0c050c01u), g23 = __builtin_amdgcn_perm(c[3].g, c[2].g, 0x0c050c01u);   // greens: slot 0 | slot 1 << 16, slot 2 | slot 3 << 16
    asm volatile(
        "ds_write_b8 %3, %4\n ds_write_b8 %3, %5 offset:1\n ds_write_b8_d16_hi %3, %4 offset:2\n"
        "ds_write_b8 %3, %6 offset:" V3_XO1 "\n ds_write_b8_d16_hi %3, %5 offset:" V3_XO1G "\n ds_write_b8_d16_hi %3, %6 offset:" V3_XO1B "\n"
        "ds_write_b8 %3, %7 offset:" V3_XO2 "\n ds_write_b8 %3, %8 offset:" V3_XO2G "\n ds_write_b8_d16_hi %3, %7 offset:" V3_XO2B "\n"
        "ds_write_b8 %3, %9 offset:" V3_XO3 "\n ds_write_b8_d16_hi %3, %8 offset:" V3_XO3G "\n ds_write_b8_d16_hi %3, %9 offset:" V3_XO3B "\n"
        "ds_read2_b32 %0, %10 offset1:1\n ds_read2_b32 %1, %10 offset0:2 offset1:3\n" V3_XPOSE_WAIT
        : "=&v"(rd01), "=&v"(rd23)
        : "v"(xp_wr), "v"(xp_wr), "v"(c[0].rb), "v"(g01), "v"(c[1].rb), "v"(c[2].rb), "v"(g23), "v"(c[3].rb), "v"(xp_rd)
        : "memory");
    out.a = rd01.x; out.b = rd01.y; out.c = rd23.x; out.d = rd23.y;
    return out;
  };

  const bool wave_sky = !__ballot(any_cand);
  if (wave_sky) {
    // ---- all sky / border for every env: the horizon colour pattern, masked where the source pixel lies outside the image
    C3 vm[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) vm[k] = c3_of_rgb(valid[k] ? 0x00FFFFFFu : 0u);
    U4 m = transpose(vm);
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(m.a), "+v"(m.b), "+v"(m.c), "+v"(m.d));
    // v_perm selectors that lay the horizon colour 0x00BBGGRR over the lane's bytes: byte j of the fragment is channel (ph + j) % 3,
    // ph = the fragment's first byte in the row modulo 3 (0 in the 12-byte form: RGBR GBRG BRGB; (lane % 24) % 3 in the 16-byte form)
    uint32_t hsel[4];
    {
      const uint32_t ph = wide ? (uint32_t)((lane % V3_ROW16) % 3) : 0u;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        uint32_t v = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) v |= ((ph + 4u * i + j) % 3u) << (8 * j);
        hsel[i] = v;
      }
    }
    for (int e = e0; e < e1; ++e) {
      const EnvV f = envv[e];
      const unsigned long long om = objmasks.of(e);
      const uint32_t s0 = __builtin_amdgcn_perm(f.hor_rgb, f.hor_rgb, hsel[0]), s1 = __builtin_amdgcn_perm(f.hor_rgb, f.hor_rgb, hsel[1]),
                     s2 = __builtin_amdgcn_perm(f.hor_rgb, f.hor_rgb, hsel[2]), s3 = __builtin_amdgcn_perm(f.hor_rgb, f.hor_rgb, hsel[3]);
      if (OBJ && om) {                                 // wave-uniform: objects in front of the sky only add queue entries (the sky pixel is final unless covered)
        unsigned long long oem[PPT] = {0ull, 0ull, 0ull, 0ull};
        const unsigned long long noe[PPT] = {0ull, 0ull, 0ull, 0ull};   // sky / border pixels are no plane edges
        push_obj(e, f.env, om, oem, noe);
      }
      store(f.env, U4{s0 & m.a, s1 & m.b, s2 & m.c, s3 & m.d});
      if (OBJ) qend_v = lane >= e - e0 ? qo : qend_v;
    }
    if (lane == 0) qcount[rwg * (RB / 64) + wave] = OBJ ? qo : 0;
  } else {
    typedef float f2 __attribute__((ext_vector_type(2)));
    f2 lr2[PPT / 2], lf2[PPT / 2], lit2[PPT / 2];
#pragma unroll
    for (int j = 0; j < PPT / 2; ++j) {
      lr2[j] = f2{lr[2 * j], lr[2 * j + 1]}; lf2[j] = f2{lf[2 * j], lf[2 * j + 1]}; lit2[j] = f2{lit[2 * j], lit[2 * j + 1]};
    }
    const char* s_qtb = reinterpret_cast<const char*>(s_qt);
    unsigned long long candm[PPT], validm[PPT], plainm[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) { candm[k] = __ballot(cand[k]); validm[k] = __ballot(valid[k]); plainm[k] = __ballot(gok[k]); }
    bool mixed = false;                                 // wave-uniform
#pragma unroll
    for (int k = 0; k < PPT; ++k) mixed |= candm[k] != ~0ull;
    uint32_t blk_reach;                                // farthest tile-plane hit of the block from the camera, cells
    {
      float r2 = 0.f;
#pragma unroll
      for (int k = 0; k < PPT; ++k) r2 = fmaxf(r2, lr[k] * lr[k] + lf[k] * lf[k]);
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) r2 = fmaxf(r2, __shfl_xor(r2, d));
      const float r = fsqrt_(r2) * R.q_per_m * 1.0001f + 1.f;
      blk_reach = (uint32_t)__builtin_amdgcn_readfirstlane((int)(r < 1.0e9f ? (uint32_t)r : 0x7FFFFFFFu));
    }
    typedef uint4 Rec;
    struct QStage { Rec q[PPT]; f2 ax2[PPT / 2], az2[PPT / 2]; };
    auto issue_t = [&](const EnvV& f, QStage& st, auto clamp_tag) __attribute__((always_inline)) {
      constexpr bool CLAMP = decltype(clamp_tag)::value;
      const f2 vA = f2{f.A2[0], f.A2[1]}, vB = f2{f.B2[0], f.B2[1]}, vCx = f2{f.Cx2[0], f.Cx2[1]}, vCz = f2{f.Cz2[0], f.Cz2[1]};
      const f2 vK = f2{Q8_SNAP, Q8_SNAP};
#pragma unroll
      for (int j = 0; j < PPT / 2; ++j) {
        // + Q8_SNAP (one more packed add, after the two fused ones: ONE rounding): the sum's bit pattern IS the fixed-point coordinate --
        // byte 0 the fraction in 256ths of a texel (GL's own precision: llvmpipe rounds its coordinates to 8 fractional bits), byte 1
        // the cell, byte 2 the tile -- no v_cvt_flr, no v_fract
        // (explicit fused multiply-adds in the exact path's order -- resolve_region_v3's Xu, Zu: since the snap makes the last bit of these sums
        // visible, every copy of the loop and the exact path must round them the same way; -ffp-contract=fast alone leaves that to the compiler)
        const f2 X2 = fma2(lf2[j], vB, fma2(lr2[j], vA, vCx)) + vK;
        const f2 Z2 = fma2(lf2[j], -vA, fma2(lr2[j], vB, vCz)) + vK;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int k = 2 * j + h;
          float X = h ? X2.y : X2.x, Z = h ? Z2.y : Z2.x;
          if (CLAMP) { X = med3f(X, lo + Q8_SNAP, f.Xhi + Q8_SNAP); Z = med3f(Z, lo + Q8_SNAP, f.Zhi + Q8_SNAP); }
          const uint32_t xi = __float_as_uint(X), zi = __float_as_uint(Z);
          if (h) { st.ax2[j].y = (float)(xi & 255u); st.az2[j].y = (float)(zi & 255u); }
          else { st.ax2[j].x = (float)(xi & 255u); st.az2[j].x = (float)(zi & 255u); }
          // tile -> block offset (LDS): row = tile byte of Z, column = tile byte of X + the map's column offset
          const uint32_t ta = (__builtin_amdgcn_perm(zi, xi, V3_SEL_TILE) << 2) + f.tab3;
          const uint32_t* tp = reinterpret_cast<const uint32_t*>(s_qtb + ta);
          const uint32_t tb = tp[0], sel = tp[V3_TAB_PITCH / 2];      // one ds_read2_b32: block offset, record-offset mask
          const uint32_t cell = q8_rec256(xi, zi, sel);                 // byte offset of the cell's record in its block (4 x 2 cells per line)
          st.q[k] = *reinterpret_cast<const uint4*>(qtex + (tb | cell));
        }
      }
    };
    auto issue = [&](const EnvV& f, QStage& st) __attribute__((always_inline)) {
#if DT_Q_PRIO
      __builtin_amdgcn_s_setprio(DT_Q_PRIO);
#endif
      if (f.reach > blk_reach) issue_t(f, st, std::false_type{});       // wave-uniform, scalar compare
      else issue_t(f, st, std::true_type{});
#if DT_Q_PRIO
      __builtin_amdgcn_s_setprio(0);
#endif
    };
    // ground-quad colour of one pixel (simulator.py:1806-1812; lit at the quad's corners, bilinear)
    auto ground_rgb = [&](const GndK& c, const float lrk, const float lfk) __attribute__((always_inline)) -> uint32_t {
      const float wx = c.Cx + lrk * c.sa + lfk * c.ca, wz = c.Cz + lrk * c.ca - lfk * c.sa;
      const float wxg = fmaf(c.kg, wx - c.Cx, c.Cx), wzg = fmaf(c.kg, wz - c.Cz, c.Cz);
      const float a = fminf(fmaxf((wxg + GROUND_HALF) * (0.5f / GROUND_HALF), 0.f), 1.f);
      const float b = fminf(fmaxf((wzg + GROUND_HALF) * (0.5f / GROUND_HALF), 0.f), 1.f);
      const float ndl = ground_corner_ndl(a, b, c.gndl[0], c.gndl[1], c.gndl[2], c.gndl[3]);
      uint32_t rgb = 0;
      rgb = __builtin_amdgcn_cvt_pk_u8_f32(ground_lit(c.gnd[0], c.base[0], c.dif[0], ndl), 0, rgb);
      rgb = __builtin_amdgcn_cvt_pk_u8_f32(ground_lit(c.gnd[1], c.base[1], c.dif[1], ndl), 1, rgb);
      rgb = __builtin_amdgcn_cvt_pk_u8_f32(ground_lit(c.gnd[2], c.base[2], c.dif[2], ndl), 2, rgb);
      return rgb;
    };
    // plane-edge pixels -> the front of the wavefront's queue region.  The lane sets are SCALAR masks (they come from
    // compares and ballots): the append runs under exec = mask, rank = mbcnt: four vector instructions per slot that has any.
    auto append_edges = [&](const int e, const unsigned long long em[PPT]) __attribute__((always_inline)) {
      const uint32_t etag = (uint32_t)(e - e0) << 8;
#pragma unroll
      for (int k = 0; k < PPT; ++k) {
        const unsigned long long mk = em[k];
        if (!mk) continue;                             // wave-uniform
        if (__builtin_amdgcn_inverse_ballot_w64(mk)) {
          const int rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u));
          w_queue[qn + rank] = (uint16_t)(etag | (uint32_t)V3_PIX(k, lane));
        }
        qn += __popcll(mk);
      }
    };
    auto finish = [&](const int e, const uint32_t env, const uint32_t hor_rgb, const QStage& st, unsigned long long om, auto mixed_tag) __attribute__((always_inline)) -> U4 {
      constexpr bool MIXED = decltype(mixed_tag)::value;
      C3 c[PPT];
      unsigned long long fastm[PPT];
      const Rec* q = st.q;
      unsigned long long slow = 0ull;
#pragma unroll
      for (int j = 0; j < PPT / 2; ++j) {
        if (j) __builtin_amdgcn_sched_barrier(0);
        // bilinear weights with the lit factor folded in (quad_weights8: fractions in 256ths, lit2 = lit / 256), two pixels per packed op
        // (quad_weights8's operations exactly -- which products are fused is part of the definition: the peeled first env, the loop and the
        // exact path must give a pixel the same bytes)
        f2 w00, w10, w01, w11;
        {
#pragma clang fp contract(off)
          f2 I2 = lit2[j];
          if constexpr (LIGHT) I2 = env_lit8_2(envl[e], lr2[j], lf2[j]);
          const f2 c256 = f2{256.f, 256.f};
          const f2 u = st.ax2[j] * I2, v = fma2(I2, c256, -u);
          w11 = u * st.az2[j]; w01 = v * st.az2[j];
          w10 = fma2(u, c256, -w11); w00 = fma2(v, c256, -w01);
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int k = 2 * j + h;
          const unsigned long long fm = __ballot((q[k].w & 0xFFFFu) > (Mi[k] & 0xFFFFu));
          fastm[k] = fm;
          slow |= candm[k] & ~fm;
          uint32_t W = __builtin_amdgcn_cvt_pk_u8_f32(h ? w00.y : w00.x, 0, 0u);
          W = __builtin_amdgcn_cvt_pk_u8_f32(h ? w10.y : w10.x, 1, W);
          W = __builtin_amdgcn_cvt_pk_u8_f32(h ? w01.y : w01.x, 2, W);
          W = __builtin_amdgcn_cvt_pk_u8_f32(h ? w11.y : w11.x, 3, W);
          const uint32_t vr = __builtin_amdgcn_udot4(q[k].x, W, 128u, false), vg = __builtin_amdgcn_udot4(q[k].y, W, 128u, false),
                         vb = __builtin_amdgcn_udot4(q[k].z, W, 128u, false);          // the channel is byte 1 of each sum
          c[k].rb = __builtin_amdgcn_perm(vb, vr, 0x0c050c01u);                        // R -> byte 0, B -> byte 2
          c[k].g = vg;                                                                 // (byte 1: the transpose pairs two pixels' greens in one v_perm)
        }
      }
      if (MIXED) {                                     // horizon band / image border: clear colour, BORDER_CONSTANT 0
        const C3 hc = c3_of_rgb(hor_rgb);
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
          c[k].rb = cand[k] ? c[k].rb : valid[k] ? hc.rb : 0u; c[k].g = cand[k] ? c[k].g : valid[k] ? hc.g : 0u;
        }
      }
      if (!slow && !(OBJ && om)) return transpose(c);  // wave-uniform: every candidate pixel of the block is a certain tile interior
      unsigned long long em[PPT] = {0ull, 0ull, 0ull, 0ull}, oem[PPT] = {0ull, 0ull, 0ull, 0ull};   // edge / object-box lanes per slot (scalar)
      if (slow) {                                      // wave-uniform: some candidate pixel is not a certain tile interior
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
          const unsigned long long sk = candm[k] & ~fastm[k];
          if (!sk) continue;                           // wave-uniform
          em[k] = sk;
          // off-grid cell: the ground quad, if every sample stays off the grid and inside the quad; else the exact path
          const unsigned long long gm = sk & __ballot((q[k].w >> 16) != 0u) & plainm[k];
          if (gm) {
            uint32_t mik = Mi[k];
            asm volatile("" : "+v"(mik));              // keep the conversion here: hoisted out of the env loop it costs a register pair per slot (spills)
            const float mrgk = __half2float(__ushort_as_half((unsigned short)(mik >> 16)));
            const EnvFast g = fasts[env];              // scalar loads, only on this path (mixed tile / ground blocks)
            const EnvCam cc = cams[env];
            GndK K;
            K.Cx = cc.Cx; K.Cz = cc.Cz; K.sa = cc.sa; K.ca = cc.ca; K.kg = g.kg;
#pragma unroll
            for (int t = 0; t < 3; ++t) { K.gnd[t] = cc.gnd[t]; K.base[t] = cc.base[t]; K.dif[t] = cc.dif[t]; }
#pragma unroll
            for (int t = 0; t < 4; ++t) K.gndl[t] = cc.gndl[t];
            const float wx = K.Cx + lr[k] * K.sa + lf[k] * K.ca, wz = K.Cz + lr[k] * K.ca - lf[k] * K.sa;
            const float wxg = fmaf(K.kg, wx - K.Cx, K.Cx), wzg = fmaf(K.kg, wz - K.Cz, K.Cz);
            const bool clear = (wx < -mrgk) | (wx > g.gw_m + mrgk) | (wz < -mrgk) | (wz > g.gh_m + mrgk);
            const bool inq = (fabsf(wxg) + 2.f * mrgk < GROUND_HALF) & (fabsf(wzg) + 2.f * mrgk < GROUND_HALF);
            const bool gfast = __builtin_amdgcn_inverse_ballot_w64(gm) & clear & inq;
            const C3 gc = c3_of_rgb(ground_rgb(K, lr[k], lf[k]));
            c[k].rb = gfast ? gc.rb : c[k].rb; c[k].g = gfast ? gc.g : c[k].g;
            em[k] = sk & ~__ballot(gfast);
          }
        }
      }
      if (OBJ && om) {                                 // wave-uniform: some object's screen box meets this block
        push_obj(e, env, om, oem, em);
#pragma unroll
        for (int k = 0; k < PPT; ++k) em[k] &= ~oem[k];
      }
      const U4 out = transpose(c);
      append_edges(e, em);
      return out;
    };
    auto run = [&](auto mixed_tag) __attribute__((always_inline)) {
      // one stage, deferred store: the 12 bytes of env e-1 are held in registers and stored right after the loads of
      // env e have been issued (k_raster_q's loop)
      QStage sa;
      const EnvV* fp = envv + e0;                      // [N + 1] entries: the prefetch may run one past the chunk
      EnvV f = fp[0];
      issue(f, sa);
      uint32_t hor = f.hor_rgb, env = f.env, env_prev;
      f = fp[1]; ++fp;
      U4 held = finish(e0, env, hor, sa, objmasks.of(e0), mixed_tag);
      if (OBJ) qend_v = qo;
      for (int e = e0 + 1; e < e1; ++e) {
        env_prev = env; hor = f.hor_rgb; env = f.env;
        issue(f, sa);
        store(env_prev, held);
        f = fp[1]; ++fp;
        held = finish(e, env, hor, sa, objmasks.of(e), mixed_tag);
        if (OBJ) qend_v = lane >= e - e0 ? qo : qend_v;
      }
      store(env, held);
    };
    if (mixed) run(std::true_type{}); else run(std::false_type{});
    if (lane == 0) qcount[rwg * (RB / 64) + wave] = OBJ ? qo : qn;
    if (qn > 0) {
      __builtin_amdgcn_s_waitcnt(0);                   // queue stores have left the wavefront
      resolve_region_v3<LIGHT>(R, cams, samptab, qtex, s_qt, w_queue, qn, e0, bx0, by0, lane, s_envq, envl);
    }
  }
  if (OBJ) {
    if (lane < ENVS_PER_BLOCK) R.qend[((size_t)rwg * (RB / 64) + wave) * ENVS_PER_BLOCK + lane] = (uint16_t)qend_v;
    __shared__ envmask_t s_og[RB / 64], s_oh[RB / 64];
    envmask_t oh = 0ull;
    const envmask_t og = obj_groups_of(qend_v, lane, &oh);
    if (lane == 0) { s_og[wave] = og; s_oh[wave] = oh; }
    __syncthreads();
    if (tid == 0) {
      envmask_t g = 0ull, gh = 0ull;
#pragma unroll
      for (int r = 0; r < RB / 64; ++r) { g |= s_og[r]; gh |= s_oh[r]; }
      if (g) push_obj_items(R, (uint32_t)rwg, g, gh);
    }
  }
}

// ==== k_raster_v3dr: domain randomisation (per-env camera, light, colours) on the quad records of k_raster_v3 ====
// The workgroup map, the LDS tile table fill, the object masks and spxy are raster_common.h's ("scaffolding shared by the rasters"), and so are k_resolve_dr's
// grabs, entry decode, sample ownership, ground-quad rules and store_rgb ("... by the exact paths"); the queue appends, push_obj, the transpose, the hand-over epilogue and k_resolve_dr's item / batch lookup are this half's own copies.
//
// Reference: simulator.py:565-614 (the per-reset camera / light / colour perturbations), :1761-1803 (projection and
// model-view per env), :1853-1884 (tile quads, GL_LINEAR / GL_REPEAT), graphics.py:172-251 (4x MSAA).
//
// The generic per-env-camera raster (k_raster<DR=1>) recomputes ray, plane hit, tile record, affine texture map and a
// float bilinear fetch from the RGBA pool per (pixel, env): 130 vector instructions per pixel
// (profiles/r03_c4_pmc_summary.txt).  Here the per-env camera is a HOMOGRAPHY from the pixel's rectilinear NDC (nx, ny)
// -- env-invariant, two registers per pixel -- straight to padded quad coordinates:
//     den = sth - a1 ny                (= -yla: > 0 below the horizon)          inv = 1 / den
//     X = Cx + inv (hx0 nx + hx1 ny + hx2)        Z = Cz + inv (hz0 nx + hz1 ny + hz2)
// with hx0 = Cy tx A, hx1 = Cy a2 B, hx2 = Cy cth B, hz0 = Cy tx B, hz1 = -Cy a2 A, hz2 = -Cy cth A  (A, B, Cx, Cz: the
// env's yaw / position map of EnvQ; a1 = ty cth, a2 = ty sth), all per-env scalars prepared by k_cam_setup (EnvD).  From
// there on the pixel is k_raster_v3's: v_perm tile look-up, one 16-byte record, integer filter.  What the shared camera
// had in tables is per (pixel, env) here:
//   * MSAA reach, as an upper bound in cells: (kappa (|xe| + |fwd|) + cex + eys) * 1.05 Cy q / den, kappa = rho + 4/3 rho^2,
//     rho = dy / den  (pix_inv_dr's bound with the L1 norm in place of the L2 norm: a larger reach only sends more pixels
//     to the exact path; the tighter max(a + s / 3, a / 3 + s) of pix_inv's two sample vectors was measured: 2.96 -> 2.84 % of
//     C4's pixels on the exact path for two more instructions per pixel, + 0.1 ms on the raster -- not kept);
//   * classification: candidate  <=>  den > -dy (a pixel without a source carries NaN coordinates: its den is NaN and it is never a
//     candidate -- no validity masks in scalar registers);  one-ray eligible  <=>  inv_lo <= inv <= inv_hi (near / far / horizon-band
//     limits folded into two per-env bounds, conservative);  fast  <=>  eligible and meta > reach + 0.5;
//   * light: the DR light is a direction (simulator.py:565-584), so the tile plane's lit factor is a per-env constant PER
//     CHANNEL (ambient / diffuse are perturbed per channel): the byte-weight filter (quad_weights8) runs unlit, its sum accumulated onto
//     2^23 so that it reads as a float, and each channel is one fused multiply-add + v_cvt_pk_u8_f32.  An env whose light is positional gets
//     inv_hi < 0: nothing is eligible and every candidate pixel takes the exact path (k_resolve_dr), which handles it.
// Plane-edge pixels go to the wavefront's queue region and are resolved by k_resolve_dr (below: the same records through the env's
// homography, its own persistent launch); pixels inside mesh-object boxes to k_resolve_obj -- the queue protocol of k_raster<DR=1, OBJ>.

template <bool OBJ, bool SUB = false>   // SUB: the masked pass, as k_raster_q<.., SUB>
#ifndef DT_V3DR_WAVES_MIN
#define DT_V3DR_WAVES_MIN 6              // round 3: (5, 6) -> (6, 6): C4 pass 4.24 - 4.31 -> 4.08 - 4.13 ms on one box (4 / 5 / 7 wavefronts: 4.34 / 4.30 / 4.29)
#define DT_V3DR_WAVES_MAX 6
#endif
__global__ __launch_bounds__(RB) __attribute__((amdgpu_waves_per_eu(DT_V3DR_WAVES_MIN, DT_V3DR_WAVES_MAX)))
void k_raster_v3dr(RenderParams R, const EnvCam* __restrict__ cams, const EnvD* __restrict__ envd, uint8_t* __restrict__ frames,
                   const uint8_t* __restrict__ qtex, const float4* __restrict__ lut, const uint32_t* __restrict__ qtiles,
                   uint16_t* __restrict__ queue, int32_t* __restrict__ qcount) {
  extern __shared__ uint32_t s_mem[];
  uint32_t* s_qt = s_mem;
  const int tid = threadIdx.x;
  const int npix = R.W * R.H;
  const int tiles_x = (R.W + DT_TILE_W - 1) / DT_TILE_W, n_tiles = tiles_x * ((R.H + DT_TILE_H - 1) / DT_TILE_H);
  const RasterWg wg = raster_wg<SUB, /*SCALAR=*/true>(R, n_tiles, blockIdx.x);   // (tile and chunk in scalar registers: the env loop's counter and the EnvD addresses follow)
  if (!wg.live) return;
  const int tile = wg.tile, rwg = wg.rwg(n_tiles), e0 = wg.e0(), e1 = wg.e1();
  v3_fill_tile_table(R, qtiles, s_qt, tid);
  __syncthreads();

  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int bx0 = (tile % tiles_x) * DT_TILE_W, by0 = (tile / tiles_x) * DT_TILE_H + wave * V3_ROWS;
  const float lo = 0.5f * 256.f;
  typedef float f2 __attribute__((ext_vector_type(2)));

  // per-pixel invariants: the rectilinear NDC of the pixel's source (the fisheye remap folded in).  A pixel without a source (outside the
  // image, or remapped from outside: BORDER_CONSTANT 0) carries NaN in both: its den is NaN, so it is never a candidate, and its source
  // position (spxy, fp16) is NaN, so it is in no object box -- no validity mask lives in scalar registers across the env loop (the kernel
  // spills those: every mask read back cost a v_readlane pair per pixel and env).
  float nx[PPT], ny[PPT];
  uint32_t spxy[PPT];
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    const int x = bx0 + V3_PIX(k, lane) % DT_V3_WW, y = by0 + V3_PIX(k, lane) / DT_V3_WW;
    const bool inimg = x < R.W && y < R.H;
    float4 l = make_float4(0.f, 0.f, 0.f, 0.f);
    if (inimg) l = lut[y * R.W + x];
    const bool ok = l.z != 0.f;
    nx[k] = ok ? l.x : __builtin_nanf(""); ny[k] = ok ? l.y : __builtin_nanf("");
    spxy[k] = 0x7E007E00u;
    if (OBJ && ok) spxy[k] = spxy_pack(l, R.W, R.H);
  }
  f2 nx2[PPT / 2], ny2[PPT / 2];
#pragma unroll
  for (int j = 0; j < PPT / 2; ++j) { nx2[j] = f2{nx[2 * j], nx[2 * j + 1]}; ny2[j] = f2{ny[2 * j], ny[2 * j + 1]}; }

  uint16_t* w_queue = queue + ((size_t)rwg * (RB / 64) + wave) * QREGION;
  int qn = 0, qo = 0, qend_v = 0;
  uint32_t* w_lds = s_mem + R.q3_rows * V3_TAB_PITCH + wave * RQ_LIST;     // the wavefront's transpose buffer
  const int st_x = bx0 + (lane * 4) % DT_V3_WW, st_y = by0 + (lane * 4) / DT_V3_WW;
  const bool st_ok = st_x < R.W && st_y < R.H;
  const size_t st_off = ((size_t)st_y * R.W + st_x) * 3;
  // (as k_raster_v3: the env's frame as a buffer descriptor -- scalar base arithmetic, the lane's offset in one register; lanes
  // without pixels carry an offset beyond num_records and are dropped)
  const uint32_t st_voff = st_ok ? (uint32_t)st_off : 0x80000000u;
  const uint32_t frame_bytes = (uint32_t)npix * 3u;
  auto store = [&](const uint32_t env, const U3& o) __attribute__((always_inline)) {
    const v3_i32x4 fr = v3_rsrc(frames + (size_t)env * frame_bytes, frame_bytes);
    v3_buf_store_v3i32(v3_u32x3{o.a, o.b, o.c}, fr, (int)st_voff, 0, 2);   // aux 2 = nt
  };
  // four pixels 0x00BBGGRR (slot k of lane l = pixel k * 64 + l) -> the lane's 12 bytes: dword transpose through LDS
  auto transpose = [&](const uint32_t px[PPT]) __attribute__((always_inline)) -> U3 {
#pragma unroll
    for (int k = 0; k < PPT; ++k) w_lds[V3_PIX(k, lane)] = px[k];   // row-major pixel number in the block, whatever the lane map
    const uint4 o = *reinterpret_cast<const uint4*>(w_lds + lane * 4);
    return U3{__builtin_amdgcn_perm(o.y, o.x, 0x04020100u), __builtin_amdgcn_perm(o.z, o.y, 0x05040201u), __builtin_amdgcn_perm(o.w, o.z, 0x06050402u)};
  };

  ChunkObjMasks<OBJ> objmasks;
  objmasks.load(R, e0, e1, n_tiles * 4, tile * 4 + wave, lane);
  auto push_obj = [&](const int e, const uint32_t env, unsigned long long om, unsigned long long oem[PPT], const unsigned long long em[PPT]) __attribute__((always_inline)) {
    const ObjBox* boxes = R.objbox + (size_t)env * DTSIM_MAX_OBJECTS;
    bool oedge[PPT];
    // (margin: MSAA sample offset + the fp16 rounding of the pixel centres kept in spxy - the triangle boxes' pad; at k_raster_v3's push_obj)
    const float obj_mrg = (R.W > 2048 || R.H > 2048) ? 0.95f : (R.W > 1024 || R.H > 1024) ? 0.45f : 0.3f;
    float sx[PPT], sy[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      oedge[k] = false;
      spxy_unpack(spxy[k], sx[k], sy[k]);
    }
    while (om) {                                     // wave-uniform
      const int o = __builtin_ctzll(om);
      const ObjBox ob = boxes[o];
      om &= om - 1ull;
#pragma unroll
      for (int k = 0; k < PPT; ++k)
        oedge[k] |= sx[k] >= ob.bx0 - obj_mrg && sx[k] <= ob.bx1 + obj_mrg && sy[k] >= ob.by0 - obj_mrg && sy[k] <= ob.by1 + obj_mrg;
    }
    const uint32_t etag = (uint32_t)(e - e0) << 8;
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      const bool ek = oedge[k];
      const unsigned long long mk = __ballot(ek);
      oem[k] = mk;
      if (ek) {
        const int rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u));
        w_queue[QREGION - 1 - (qo + rank)] = (uint16_t)(etag | (__builtin_amdgcn_inverse_ballot_w64(em[k]) ? QE_PLANE_EDGE : 0u) | (uint32_t)V3_PIX(k, lane));
      }
      qo += __popcll(mk);
    }
  };
  const char* s_qtb = reinterpret_cast<const char*>(s_qt);

  EnvDG g = envd[e0].g;                              // scalar loads (wave-uniform address); e = position in the render order
  U3 held{0u, 0u, 0u};
  uint32_t env_held = 0u;
  for (int e = e0; e < e1; ++e) {
    const unsigned long long om = objmasks.of(e);
    uint4 q[PPT];
    f2 ax2[PPT / 2], az2[PPT / 2], inv2[PPT / 2], den2[PPT / 2], X2[PPT / 2], Z2[PPT / 2];
    const f2 vna1 = f2{g.na1, g.na1}, vsth = f2{g.sth, g.sth};
    const f2 vhx0 = f2{g.hx0, g.hx0}, vhx1 = f2{g.hx1, g.hx1}, vhx2 = f2{g.hx2, g.hx2};
    const f2 vhz0 = f2{g.hz0, g.hz0}, vhz1 = f2{g.hz1, g.hz1}, vhz2 = f2{g.hz2, g.hz2};
    const f2 vCx = f2{g.Cx, g.Cx}, vCz = f2{g.Cz, g.Cz}, vK = f2{Q8_SNAP, Q8_SNAP};
    const uint32_t env = g.env;
    // ---- geometry + record loads
#pragma unroll
    for (int j = 0; j < PPT / 2; ++j) {
      den2[j] = fma2(ny2[j], vna1, vsth);            // = -yla   (explicit fused multiply-adds, k_resolve_dr's: the snap below makes the last bit visible)
      inv2[j] = f2{frcp(den2[j].x), frcp(den2[j].y)};
      const f2 numX = fma2(nx2[j], vhx0, fma2(ny2[j], vhx1, vhx2)), numZ = fma2(nx2[j], vhz0, fma2(ny2[j], vhz1, vhz2));
      // (+ Q8_SNAP in a separate add: ONE rounding of the coordinate to 256ths of a texel, and the sum's bits are the fixed-point coordinate:
      // byte 0 the fraction, byte 1 the cell, byte 2 the tile; raster_common.h, quad_weights8)
      X2[j] = fma2(inv2[j], numX, vCx) + vK; Z2[j] = fma2(inv2[j], numZ, vCz) + vK;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int k = 2 * j + h;
        // clamp into the padded grid (also tames the rays at / above the horizon: inf, nan -> lo)
        const float X = med3f(h ? X2[j].y : X2[j].x, lo + Q8_SNAP, g.Xhi + Q8_SNAP), Z = med3f(h ? Z2[j].y : Z2[j].x, lo + Q8_SNAP, g.Zhi + Q8_SNAP);
        const uint32_t xi = __float_as_uint(X), zi = __float_as_uint(Z);
        if (h) { ax2[j].y = q8_frac(xi); az2[j].y = q8_frac(zi); X2[j].y = X; Z2[j].y = Z; }
        else { ax2[j].x = q8_frac(xi); az2[j].x = q8_frac(zi); X2[j].x = X; Z2[j].x = Z; }
        const uint32_t ta = (__builtin_amdgcn_perm(zi, xi, V3_SEL_TILE) << 2) + g.tab3;
        const uint32_t* tp = reinterpret_cast<const uint32_t*>(s_qtb + ta);
        const uint32_t tb = tp[0], sel = tp[V3_TAB_PITCH / 2];
        q[k] = *reinterpret_cast<const uint4*>(qtex + (tb | q8_rec256(xi, zi, sel)));
      }
    }
    // the frame bytes of the env before go out behind these loads (a load is never waited for behind a younger store); the
    // second half of this env's constants and the first half of the next env's are read while the records are in flight
    if (e > e0) store(env_held, held);
    const EnvDR d = envd[e].r;
    g = envd[min(e + 1, e1 - 1)].g;
    // ---- classification: candidate / one-ray eligible / MSAA reach (cells) per (pixel, env)
    unsigned long long candm[PPT], plainm[PPT], fastm[PPT];
    float reach[PPT];                                // reach + 0.5, cells
    {
      const f2 vdy = f2{d.dy, d.dy}, va2 = f2{d.a2, d.a2}, vcth = f2{d.cth, d.cth}, vcE = f2{d.cE, d.cE}, vKr = f2{d.Kr, d.Kr};
#pragma unroll
      for (int j = 0; j < PPT / 2; ++j) {
        const f2 rho = inv2[j] * vdy;
        const f2 kap = (rho * 1.3334f) * rho + rho;
        const f2 fw = ny2[j] * va2 + vcth;
        const f2 g = f2{fmaf(fabsf(nx[2 * j]), d.tx, fabsf(fw.x)), fmaf(fabsf(nx[2 * j + 1]), d.tx, fabsf(fw.y))};
        const f2 m = kap * g + vcE;
        const f2 r = (m * inv2[j]) * vKr + 0.5f;
        reach[2 * j] = r.x; reach[2 * j + 1] = r.y;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int k = 2 * j + h;
          const float dn = h ? den2[j].y : den2[j].x, iv = h ? inv2[j].y : inv2[j].x;
          candm[k] = __ballot(dn > d.ndy);              // (NaN for a pixel without a source)
          plainm[k] = candm[k] & __ballot(iv >= d.inv_lo) & __ballot(iv <= d.inv_hi);   // two compares, ANDed on the scalar unit (one bool expression costs a v_cndmask + v_cmp pair)
        }
      }
    }
    // ---- unlit byte-weight filter (quad_weights8, raster_common.h: one v_dot4_u32_u8 per channel), then the per-channel light in float
    uint32_t px[PPT];
    unsigned long long slow = 0ull;
#pragma unroll
    for (int j = 0; j < PPT / 2; ++j) {
      // (quad_weights8 with l = 1 / 256: every step is exact in fp32 -- the fractions are 8-bit integers)
      const f2 u = ax2[j], v = 256.f - u, bz = az2[j] * Q8_LIT;
      const f2 w11 = u * bz, w01 = v * bz;
      const f2 w10 = u - w11, w00 = v - w01;
      f2 F2[3];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int k = 2 * j + h;
        const unsigned long long fm = plainm[k] & __ballot((float)(q[k].w & 0xFFFFu) > reach[k]);
        fastm[k] = fm;
        slow |= candm[k] & ~fm;
        uint32_t W = __builtin_amdgcn_cvt_pk_u8_f32(h ? w00.y : w00.x, 0, 0u);
        W = __builtin_amdgcn_cvt_pk_u8_f32(h ? w10.y : w10.x, 1, W);
        W = __builtin_amdgcn_cvt_pk_u8_f32(h ? w01.y : w01.x, 2, W);
        W = __builtin_amdgcn_cvt_pk_u8_f32(h ? w11.y : w11.x, 3, W);
        // The filter sum S (< 2^16) leaves the dot product as a FLOAT: accumulated onto 0x4B000000 the result reads 2^23 + S, exactly -- so
        // S kc is one fused multiply-add, kc S' - 2^23 kc, without an integer-to-float conversion; the multiply-adds run PACKED over the pixel
        // pair below (one scalar factor per channel for both).
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const uint32_t qq = ch == 0 ? q[k].x : ch == 1 ? q[k].y : q[k].z;
          const float Sf = __uint_as_float(__builtin_amdgcn_udot4(qq, W, 0x4B000000u, false));
          if (h) F2[ch].y = Sf; else F2[ch].x = Sf;
        }
      }
      {
        uint32_t rgb0 = 0u, rgb1 = 0u;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const float kc1 = d.kc[ch], kcc = d.kcc[ch];
          const f2 vv = F2[ch] * f2{kc1, kc1} + f2{kcc, kcc};
          rgb0 = __builtin_amdgcn_cvt_pk_u8_f32(vv.x, ch, rgb0);
          rgb1 = __builtin_amdgcn_cvt_pk_u8_f32(vv.y, ch, rgb1);
        }
        px[2 * j] = rgb0; px[2 * j + 1] = rgb1;
      }
    }
    if ((candm[0] & candm[1] & candm[2] & candm[3]) != ~0ull) {   // wave-uniform: the block reaches the horizon / the image border for this env
#pragma unroll
      for (int k = 0; k < PPT; ++k) {
        // not a candidate: clear colour, or 0 where the pixel has no source (BORDER_CONSTANT; den is NaN there -- a value of THIS env, so
        // the test cannot be hoisted into one more scalar mask); edge pixels are patched later
        const float dn = (k & 1) ? den2[k / 2].y : den2[k / 2].x;
        px[k] = __builtin_amdgcn_inverse_ballot_w64(candm[k]) ? px[k] : (dn == dn ? d.hor_rgb : 0u);
      }
    }
    unsigned long long em[PPT] = {0ull, 0ull, 0ull, 0ull}, oem[PPT] = {0ull, 0ull, 0ull, 0ull};
    if (slow) {                                      // wave-uniform: some candidate pixel is not a certain tile interior
      const float goff = (float)DT_QRING * 256.f + 0.5f;   // world 0 in padded quad coordinates
#pragma unroll
      for (int k = 0; k < PPT; ++k) {
        const unsigned long long sk = candm[k] & ~fastm[k];
        if (!sk) continue;                           // wave-uniform
        em[k] = sk;
        // off-grid cell of a one-ray eligible pixel: the ground quad, if every sample stays off the grid and inside the quad
        const unsigned long long gm = sk & plainm[k] & __ballot((q[k].w >> 16) != 0u);
        if (gm) {
          const EnvCam c = cams[env];                // scalar loads, only here (ground beyond the map)
          const float X = ((k & 1) ? X2[k / 2].y : X2[k / 2].x) - Q8_SNAP, Z = ((k & 1) ? Z2[k / 2].y : Z2[k / 2].x) - Q8_SNAP;   // (snapped to 256ths of a cell)
          const float ux = X - goff, uz = Z - goff, rc = reach[k];       // hit relative to the grid origin, reach: cells
          const bool clear = (ux < -rc) | (ux > d.gx1 + rc) | (uz < -rc) | (uz > d.gz1 + rc);
          const float Xc = (k & 1) ? vCx.y : vCx.x, Zc = (k & 1) ? vCz.y : vCz.x;
          const float Xg = fmaf(d.kg, X - Xc, Xc) - goff, Zg = fmaf(d.kg, Z - Zc, Zc) - goff;   // ground-quad hit, cells from world 0
          const float gh = GROUND_HALF * d.qpm;
          const bool inq = (fabsf(Xg) + 2.f * rc < gh) & (fabsf(Zg) + 2.f * rc < gh);
          const bool gfast = __builtin_amdgcn_inverse_ballot_w64(gm) & clear & inq;
          const float hs = 0.5f / gh;
          const float a_ = fminf(fmaxf(fmaf(Xg, hs, 0.5f), 0.f), 1.f), b_ = fminf(fmaxf(fmaf(Zg, hs, 0.5f), 0.f), 1.f);
          const float ndl = ground_corner_ndl(a_, b_, c.gndl[0], c.gndl[1], c.gndl[2], c.gndl[3]);
          uint32_t rgb = 0u;                         // (ground_lit, written out: the call reordered scalar moves of the masked instantiation)
          rgb = __builtin_amdgcn_cvt_pk_u8_f32(c.gnd[0] * fminf(c.base[0] + c.dif[0] * ndl, 1.f), 0, rgb);
          rgb = __builtin_amdgcn_cvt_pk_u8_f32(c.gnd[1] * fminf(c.base[1] + c.dif[1] * ndl, 1.f), 1, rgb);
          rgb = __builtin_amdgcn_cvt_pk_u8_f32(c.gnd[2] * fminf(c.base[2] + c.dif[2] * ndl, 1.f), 2, rgb);
          px[k] = gfast ? rgb : px[k];
          em[k] = sk & ~__ballot(gfast);
        }
      }
    }
    if (OBJ && om) {
      push_obj(e, env, om, oem, em);
#pragma unroll
      for (int k = 0; k < PPT; ++k) em[k] &= ~oem[k];
    }
    held = transpose(px); env_held = env;
    {
      const uint32_t etag = (uint32_t)(e - e0) << 8;
#pragma unroll
      for (int k = 0; k < PPT; ++k) {
        const unsigned long long mk = em[k];
        if (!mk) continue;
        if (__builtin_amdgcn_inverse_ballot_w64(mk)) {
          const int rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u));
          w_queue[qn + rank] = (uint16_t)(etag | (uint32_t)V3_PIX(k, lane));
        }
        qn += __popcll(mk);
      }
    }
    if (OBJ) qend_v = lane >= e - e0 ? qo : qend_v;
  }
  store(env_held, held);
  // hand-over: the plane-edge entries (front of the regions) to k_resolve_dr, the object-box entries (back) to k_resolve_obj, by env group
  if (lane == 0) qcount[rwg * (RB / 64) + wave] = qn;
  if (OBJ && lane < ENVS_PER_BLOCK) R.qend[((size_t)rwg * (RB / 64) + wave) * ENVS_PER_BLOCK + lane] = (uint16_t)qend_v;
  __shared__ int s_nb[RB / 64];
  __shared__ envmask_t s_no[RB / 64], s_nh[RB / 64];
  envmask_t oh = 0ull;
  const envmask_t og = OBJ ? obj_groups_of(qend_v, lane, &oh) : 0ull;
  if (lane == 0) { s_nb[wave] = (qn + 63) >> 6; s_no[wave] = og; s_nh[wave] = oh; }
  __syncthreads();
  if (tid == 0) {
    int nb = 0;
    envmask_t no = 0ull, nh = 0ull;
#pragma unroll
    for (int r = 0; r < RB / 64; ++r) { nb += s_nb[r]; no |= s_no[r]; nh |= s_nh[r]; }
    if (nb > 0) {
      const int ni = (nb + ITEM_B - 1) / ITEM_B;
      const int pos = atomicAdd(R.work + DT_WORK_ITEMS, ni);
      for (int i = 0; i < ni; ++i) R.items[pos + i] = (uint32_t)rwg * ITEMS_PER_WG + (uint32_t)i;
    }
    if (OBJ && no) push_obj_items(R, (uint32_t)rwg, no, nh);
  }
}

// The pixel centre of an exact-path entry in padded quad coordinates, as q8_rec256 / quad_weights8 take it (cell and fraction inside the SAMPLE's
// tile).  Inside the padded grid: itself.  Past it -- a sample on the last tiles of a grid whose border lies metres away, the centre of its pixel
// further out than the DT_QRING ring: one image row under the horizon -- wrapped by whole tiles, as GL_REPEAT wraps the texture coordinate that GL
// extrapolates to the centre (a clamp to the ring's edge put the border's cell there: 43 pixels of a row off by 28 - 37 at a border 9 m away).
// nan, or too far for a fraction to be left: lo.
__device__ inline float dr_centre_wrap(float u, float lo, float hi) {
  if (u >= lo && u <= hi) return u;
  if (!(fabsf(u) < 4194304.f)) return lo;
  return u - 256.f * floorf(u * (1.f / 256.f)) + 256.f;
}

// ---- k_resolve_dr: the exact path of the plane-edge pixels k_raster_v3dr queues (round 5) -----------------------------
// Replaces the generic k_resolve behind k_raster_v3dr: same work items (one per 8 queue batches of a raster workgroup, persistent
// wavefronts, static first grab), but a pixel is resolved the way resolve_region_v3 (above) resolves one for the shared camera --
// on the quad records and the LDS tile table, with the env's HOMOGRAPHY in place of the per-pixel sample table:
//   * the four MSAA samples (graphics.py:172-251: coverage and depth per sample) go from their rectilinear NDC straight to padded quad
//     coordinates (EnvDG), one reciprocal each; the tile that OWNS a sample is looked up with one v_perm + one ds_read2;
//     near / far through t = Cy / den (tile plane) and kg t (ground quad);
//   * shading once per primitive AT THE PIXEL CENTRE: every tile sample adds the integer filter of ITS tile's record at the centre
//     cell (one cell grid and one weight set for all tiles), a record is loaded only when a sample's tile differs from the one before;
//     the DR light is a direction, so the lit factor is the env's per-channel constant kc (a positional light -- only when the
//     caller wrote one -- is evaluated per pixel from the EnvCam); ground-quad and sky samples add their colour per count.
// The generic kernel spent 59 vector instructions per sample on classify() alone (ray, two plane hits, tile record, affine texture
// map) and shaded through the float bilinear fetch of the RGBA pool: 595 instructions per 64-pixel batch against ~ 330 here.
// Reference: simulator.py:565-614, 1761-1803 (per-env camera), :1806-1812 (ground quad), :1853-1884 (tiles).
#ifndef DT_RESDR_WAVES
#define DT_RESDR_WAVES 6            // wavefronts per SIMD k_resolve_dr is compiled for
#endif
__global__ __launch_bounds__(RB) __attribute__((amdgpu_waves_per_eu(DT_RESDR_WAVES, DT_RESDR_WAVES)))
void k_resolve_dr(RenderParams R, const EnvCam* __restrict__ cams, const EnvD* __restrict__ envd, const uint8_t* __restrict__ qtex,
                  const float4* __restrict__ lut, const uint32_t* __restrict__ qtiles, const uint16_t* __restrict__ queue,
                  const int32_t* __restrict__ qcount) {
  extern __shared__ uint32_t s_mem[];
  uint32_t* s_qt = s_mem;
  const int tid = threadIdx.x;
  const int npix = R.W * R.H;
  const int tiles_x = (R.W + DT_TILE_W - 1) / DT_TILE_W, n_tiles = tiles_x * ((R.H + DT_TILE_H - 1) / DT_TILE_H);
  const int wave = tid >> 6, lane = tid & 63;
  v3_fill_tile_table(R, qtiles, s_qt, tid);
  __syncthreads();
  const char* qtb = reinterpret_cast<const char*>(s_qt);
  const float lo = 0.5f * 256.f;
  const float goff = (float)DT_QRING * 256.f + 0.5f;   // world 0 in padded quad coordinates
  const float sxn = 2.f / (float)R.W, syn = 2.f / (float)R.H;
  const int n_items = R.work[DT_WORK_ITEMS];         // written by the raster launch
  const int n_grabs = work_n_grabs(n_items);
  bool first_grab = true;
  while (true) {
    int g = wave * (int)gridDim.x + (int)blockIdx.x;
    if (!first_grab) g = work_next_grab(R, DT_WORK_CURSOR, g, lane);
    first_grab = false;
    if (g >= n_grabs) break;
    for (int it = g; it < n_items; it += n_grabs) {  // wave-uniform
      const uint32_t item = R.items[it];
      const int rwg = (int)(item / ITEMS_PER_WG), part = (int)(item % ITEMS_PER_WG);
      const int tile = rwg % n_tiles, chunk = rwg / n_tiles;
      const int e0 = chunk * ENVS_PER_BLOCK;
      const int tile_x0 = (tile % tiles_x) * DT_TILE_W, tile_y0 = (tile / tiles_x) * DT_TILE_H;
      static_assert(RB / 64 == 4, "region lookup assumes 4 wavefronts");
      int rn[4], rb[5];
      rb[0] = 0;
#pragma unroll
      for (int r = 0; r < 4; ++r) { rn[r] = qcount[rwg * 4 + r]; rb[r + 1] = rb[r] + ((rn[r] + 63) >> 6); }
      const int b_end = min(rb[4], (part + 1) * ITEM_B);
      for (int b = part * ITEM_B; b < b_end; ++b) {  // wave-uniform
        const int reg = (b >= rb[1]) + (b >= rb[2]) + (b >= rb[3]);
        const int q0 = (b - (reg == 0 ? rb[0] : reg == 1 ? rb[1] : reg == 2 ? rb[2] : rb[3])) * 64;
        const int n = reg == 0 ? rn[0] : reg == 1 ? rn[1] : reg == 2 ? rn[2] : rn[3];
        const uint16_t* w_queue = queue + ((size_t)rwg * 4 + reg) * QREGION;
        const int wave_y0 = tile_y0 + reg * (WAVE_PIX / WAVE_W);
        const bool have = q0 + lane < n;
        const uint32_t ent = have ? w_queue[q0 + lane] : 0u;
        const int el = qe_envpos(ent), lp = qe_pixel(ent);
        const int pix = (wave_y0 + lp / WAVE_W) * R.W + tile_x0 + lp % WAVE_W;      // entries only exist for in-image pixels
        const float4 l = lut[pix];
        const float nx = l.x, ny = l.y;
        const float4* X = reinterpret_cast<const float4*>(&envd[min(e0 + el, R.N - 1)].x);   // position in the render order
        // the env's constants: five 16-byte gathers over at most 32 distinct records (entries of a region are env-major: a batch holds few envs)
        const float4 g0 = X[0], g1 = X[1], g2 = X[2], g4 = X[4];
        const uint4 g3 = *reinterpret_cast<const uint4*>(X + 3);
        const float hx0 = g0.x, hx1 = g0.y, hx2 = g0.z, hz0 = g0.w, hz1 = g1.x, hz2 = g1.y, Cx = g1.z, Cz = g1.w;
        const float na1 = g2.x, sth = g2.y, Xhi = g2.z, Zhi = g2.w;
        const uint32_t tab = g3.x;
        const int e = (int)g3.y;                       // frame index
        const float kg = __uint_as_float(g3.z), qpm = __uint_as_float(g3.w), Cy = g4.x;
        const float ghalf = GROUND_HALF * qpm;
        // pixel centre: den = -yla; above the horizon the centre hit is not used (no tile sample exists then)
        const float den_c = fmaf(ny, na1, sth);
        const bool c_down = den_c > 0.f;
        const float inv_c = c_down ? frcp(den_c) : 0.f;
        const float Xu = fmaf(inv_c, fmaf(nx, hx0, fmaf(ny, hx1, hx2)), Cx), Zu = fmaf(inv_c, fmaf(nx, hz0, fmaf(ny, hz1, hz2)), Cz);
        const uint32_t xic = q8_bits(dr_centre_wrap(Xu, lo, Xhi)), zic = q8_bits(dr_centre_wrap(Zu, lo, Zhi));   // the centre's snapped coordinates (q8_rec256 works on these bits)
        const uint32_t W8 = quad_weights8(q8_frac(xic), q8_frac(zic), Q8_LIT);   // unlit byte weights (sum 256): the light is applied per channel below
        uint32_t aS[3] = {0u, 0u, 0u};
        int n_sky = 0, n_gnd = 0;
        float gX = 0.f, gZ = 0.f;                      // ground hit (quad coordinates) of the lowest-index ground sample
        uint32_t raddr[4];
        const auto &ox = MSAA_POS.x, &oy = MSAA_POS.y;
#pragma unroll
        for (int s = 3; s >= 0; --s) {
          const float nxs = fmaf(ox[s], sxn, nx), nys = fmaf(-oy[s], syn, ny);
          const float den = fmaf(nys, na1, sth);
          const bool down = den > 0.f;
          const float inv = down ? frcp(den) : 0.f;
          const float t = Cy * inv, tg = kg * t;
          const float Xs = fmaf(inv, fmaf(nxs, hx0, fmaf(nys, hx1, hx2)), Cx), Zs = fmaf(inv, fmaf(nxs, hz0, fmaf(nys, hz1, hz2)), Cz);
          uint32_t tb, sel;
          const bool s_in = v3_sample_owner(Xs, Zs, lo, Xhi, Zhi, qtb, tab, tb, sel);
          const bool is_tile = have & down & (t >= NEAR_Z) & (t <= FAR_Z) & s_in & (tb != 0u);
          const float Xg = ground_quad_at(kg, Xs, Cx), Zg = ground_quad_at(kg, Zs, Cz);
          const bool is_gnd = have & !is_tile & down & (tg >= NEAR_Z) & (tg <= FAR_Z) & ground_quad_in(Xg, goff, ghalf) & ground_quad_in(Zg, goff, ghalf);
          n_gnd += is_gnd; n_sky += !(is_tile | is_gnd);
          if (is_gnd) { gX = Xg; gZ = Zg; }
          raddr[s] = is_tile ? (tb | q8_rec256(xic, zic, sel)) : 0u;
        }
        // one record per DISTINCT tile among the pixel's samples, all loads in flight together (the kernel waits on round trips, not on issue):
        // a lane loads for sample s only when its address differs from sample s + 1's
        uint4 rec[4];
        rec[3] = *reinterpret_cast<const uint4*>(qtex + raddr[3]);
#pragma unroll
        for (int s = 2; s >= 0; --s) {
          rec[s] = make_uint4(0u, 0u, 0u, 0u);
          if (raddr[s] != raddr[s + 1]) rec[s] = *reinterpret_cast<const uint4*>(qtex + raddr[s]);
        }
#pragma unroll
        for (int s = 3; s >= 0; --s) {
          if (s < 3 && raddr[s] == raddr[s + 1]) rec[s] = rec[s + 1];
          aS[0] = __builtin_amdgcn_udot4(rec[s].x, W8, aS[0], false);
          aS[1] = __builtin_amdgcn_udot4(rec[s].y, W8, aS[1], false);
          aS[2] = __builtin_amdgcn_udot4(rec[s].z, W8, aS[2], false);
        }
        float kc[3] = {g4.y, g4.z, g4.w};              // lit factor / 256 per channel (directional light: the env's constant)
        float acc[3];
        {
          const float4 pf = X[5];
          if (__ballot(have && pf.x < 0.f)) {          // wave-uniform, rare: a positional light (not what domain randomisation draws) -> per pixel
            if (pf.x < 0.f) {
              const EnvCam* c = cams + e;
              const Ray rc = make_ray(nx, ny, c->tx, c->ty, c->sth, c->cth);
              const float L[4] = {c->L[0], c->L[1], c->L[2], c->L[3]};
              const float ndl = plane_ndl(L, c->sth, c->cth, rc, Cy * inv_c);
#pragma unroll
              for (int k = 0; k < 3; ++k) kc[k] = fminf(c->base[k] + c->dif[k] * ndl, 1.f) * (1.f / 256.f);
            }
          }
#pragma unroll
          for (int k = 0; k < 3; ++k) acc[k] = (float)aS[k] * kc[k];
          acc[0] = fmaf((float)n_sky, pf.y, acc[0]); acc[1] = fmaf((float)n_sky, pf.z, acc[1]); acc[2] = fmaf((float)n_sky, pf.w, acc[2]);
        }
        if (__ballot(n_gnd > 0)) {                     // wave-uniform: shade the ground quad (lit at its corners, bilinear)
          if (c_down) { gX = fmaf(kg, Xu - Cx, Cx); gZ = fmaf(kg, Zu - Cz, Cz); }   // the centre ray hits the planes: shade at its ground hit
          const float hs = 0.5f / ghalf;
          const float a_ = fminf(fmaxf(fmaf(gX - goff, hs, 0.5f), 0.f), 1.f), b_ = fminf(fmaxf(fmaf(gZ - goff, hs, 0.5f), 0.f), 1.f);
          const float4 q6 = X[6], q7 = X[7], q8 = X[8], q9 = X[9];   // gnd[3], gndl0 | gndl1..3 | base[3], dif0 | dif1, dif2
          const float ndl = ground_corner_ndl(a_, b_, q6.w, q7.x, q7.y, q7.z);
          const float ng = (float)n_gnd;
          acc[0] += ng * ground_lit(q6.x, q8.x, q8.w, ndl);
          acc[1] += ng * ground_lit(q6.y, q8.y, q9.x, ndl);
          acc[2] += ng * ground_lit(q6.z, q8.z, q9.y, ndl);
        }
        const float o[3] = {0.25f * acc[0], 0.25f * acc[1], 0.25f * acc[2]};
        if (have) store_rgb(R.frames, npix, e, pix, pack_rgb(o));
      }
    }
  }
}


}  // namespace

// ---- the launchers, one per pipe.  sub: the masked pass (the SUB instantiations over positions [0, live): the grid is sized for R.N).
static size_t v3_lds_tab(const RenderParams& R) { return (size_t)R.q3_rows * V3_TAB_PITCH * 4; }   // the LDS tile table (v3_fill_tile_table)

template <bool SUB> static void launch_raster_v3(hipStream_t s, const RenderParams& R, const EnvRecs& x) {
  const int n_chunks = (R.N + ENVS_PER_BLOCK - 1) / ENVS_PER_BLOCK;
  const dim3 gridq((unsigned)raster_wg_grid(dt_raster_tiles(R.W, R.H), n_chunks));   // the quad-record rasters' XCD-affine map (raster_wg)
  const dim3 gridv3(SUB ? gridq.x : (unsigned)raster_ticket_grid(dt_raster_tiles(R.W, R.H), n_chunks, DT_RASTER_TICKET_UNITS));   // the full pass: + the thieves
  const size_t lds3 = v3_lds_tab(R) + (size_t)(RB / 64) * V3_WAVE_LDS * 4 + (size_t)ENVS_PER_BLOCK * sizeof(EnvQ);   // + per-wavefront buffers, the chunk's EnvQ records
#define LAUNCH_V3(OBJ_) do { if (R.light) hipLaunchKernelGGL((k_raster_v3<OBJ_, true, SUB>), gridv3, dim3(RB), lds3, s, R, x.cams, x.fasts, x.envq, x.envv, R.frames, \
                                           R.qtex, reinterpret_cast<const float4*>(R.lut), x.pixtab, x.samptab, R.qtiles, R.queue, R.qcount, x.envl); \
                                else hipLaunchKernelGGL((k_raster_v3<OBJ_, false, SUB>), gridv3, dim3(RB), lds3, s, R, x.cams, x.fasts, x.envq, x.envv, R.frames, R.qtex, \
                                           reinterpret_cast<const float4*>(R.lut), x.pixtab, x.samptab, R.qtiles, R.queue, R.qcount, nullptr); } while (0)
  if (R.max_tris > 0) LAUNCH_V3(true); else LAUNCH_V3(false);
#undef LAUNCH_V3
}
void dt_launch_raster_v3(hipStream_t s, const RenderParams& R, const EnvRecs& x, bool sub) {
  if (sub) launch_raster_v3<true>(s, R, x); else launch_raster_v3<false>(s, R, x);
}

// k_raster_v3dr, then its plane-edge pixels: k_resolve_dr, on the quad records through the env's homography (persistent wavefronts pulling
// work items: exactly the resident workgroups, as the generic exact paths)
template <bool SUB> static void launch_raster_v3dr(hipStream_t s, const RenderParams& R, const EnvRecs& x) {
  const int n_chunks = (R.N + ENVS_PER_BLOCK - 1) / ENVS_PER_BLOCK;
  const dim3 gridq((unsigned)raster_wg_grid(dt_raster_tiles(R.W, R.H), n_chunks));
  const size_t lds_tab = v3_lds_tab(R);
  const size_t ldsd = lds_tab + (size_t)(RB / 64) * RQ_LIST * 4;        // + the wavefronts' transpose buffers (w_lds)
  if (R.max_tris > 0) hipLaunchKernelGGL((k_raster_v3dr<true, SUB>), gridq, dim3(RB), ldsd, s, R, x.cams, x.envd, R.frames, R.qtex, reinterpret_cast<const float4*>(R.lut), R.qtiles, R.queue, R.qcount);
  else hipLaunchKernelGGL((k_raster_v3dr<false, SUB>), gridq, dim3(RB), ldsd, s, R, x.cams, x.envd, R.frames, R.qtex, reinterpret_cast<const float4*>(R.lut), R.qtiles, R.queue, R.qcount);
  const dim3 rgrid((unsigned)std::min<size_t>((unsigned)(dt_raster_tiles(R.W, R.H) * n_chunks), resident_blocks(k_resolve_dr, lds_tab)));
  hipLaunchKernelGGL(k_resolve_dr, rgrid, dim3(RB), lds_tab, s, R, x.cams, x.envd, R.qtex, reinterpret_cast<const float4*>(R.lut), R.qtiles, R.queue, R.qcount);
}
void dt_launch_raster_v3dr(hipStream_t s, const RenderParams& R, const EnvRecs& x, bool sub) {
  if (sub) launch_raster_v3dr<true>(s, R, x); else launch_raster_v3dr<false>(s, R, x);
}
