// render_v3.inc -- k_raster_v3: the quad-record one-ray path of k_raster_q on an instruction diet (included by render.hip
// inside its anonymous namespace; shares EnvCam / EnvFast / EnvQ / PixTab / SampTab and the queue protocol with k_raster_q).
// The workgroup map, the LDS tile table fill, the object masks and spxy are render.hip's ("scaffolding shared by the rasters"), and so are resolve_region_v3's
// entry decode, sample ownership, ground-quad rules and store_rgb ("... by the exact paths"); the queue appends, push_obj, the transpose and the hand-over epilogue are this kernel's own copies.
//
// Replaces the same reference code as k_raster_q: simulator.py:1853-1884 (tile quads, GL_LINEAR / GL_REPEAT),
// simulator.py:1806-1812 (ground quad), graphics.py:172-251 (4x MSAA resolve), distortion.py:85-125 (remap, folded in).
//
// As built (what changed against k_raster_q, profiles/r02: 43.7 VALU instructions per pixel -> 36.9):
//   * tile table in LDS rows of 1 KB: block byte offset at (tz << 10 | tx << 2) + map column offset, the record-offset mask 512
//     bytes behind it, so that the address is ONE v_perm (both tile bytes) + one v_lshl_add and both come back from one
//     ds_read2_b32;
//   * (round 6) the quad coordinates are snapped to 256ths of a texel by one packed add of 32768 (render.hip, Q8_SNAP) -- GL's own
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
#define V3_MAX_ROWS 24                                // padded grid height <= 24 (24 KB of LDS)
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
// a shift -- and G in byte 1 of `g`, where the byte-weight filter (quad_filter, render.hip) leaves each channel of its dot products:
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
// s_qt: k_raster_v3's LDS tile table (block offset at (tz << 10 | tx << 2) + the map's column offset EnvQ.pad[0], the record-offset
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
      PixTab pt;                                       // the PixTab's hit and lit factor, from the SampTab (one table, two 16-byte loads)
      pt.lr = __uint_as_float(sp.pad[0]); pt.lf = __uint_as_float(sp.pad[1]); pt.lit = __uint_as_float(sp.pad[2]); pt.mi = 0u;
      // the env's constants as three 16-byte pieces (round 5: the exact path is bound by the NUMBER of vector-memory instructions it issues)
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
