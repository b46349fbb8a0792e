// render_v3dr.inc -- k_raster_v3dr: domain randomisation (per-env camera, light, colours) on the quad records of
// k_raster_v3 (included by render.hip inside its anonymous namespace, after render_v3.inc).
// The workgroup map, the LDS tile table fill, the object masks and spxy are render.hip's ("scaffolding shared by the rasters"), and so are k_resolve_dr's
// grabs, entry decode, sample ownership, ground-quad rules and store_rgb ("... by the exact paths"); the queue appends, push_obj, the transpose, the hand-over epilogue and k_resolve_dr's item / batch lookup are this file's own copies.
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

__device__ inline void fill_envd(EnvD& D, const EnvCam& c, const EnvQ& q, const RenderMapDev& m, float q_cells, int H, int W) {
  const float S = q_cells;                           // cells per tile (256)
  const float a1 = c.ty * c.cth, a2 = c.ty * c.sth;
  const float ey = (0.375f * 2.f / (float)H * 1.01f) * c.ty, cex = (0.375f * 2.f / (float)W * 1.01f) * c.tx;
  const float dy = ey * fabsf(c.cth), eys = ey * fabsf(c.sth);
  const float qpm = m.inv_tile_size * S;
  EnvDG& g = D.g; EnvDR& d = D.r;
  g.hx0 = c.Cy * c.tx * q.A; g.hx1 = c.Cy * a2 * q.B; g.hx2 = c.Cy * c.cth * q.B;
  g.hz0 = c.Cy * c.tx * q.B; g.hz1 = -c.Cy * a2 * q.A; g.hz2 = -c.Cy * c.cth * q.A;
  g.Cx = q.Cx; g.Cz = q.Cz;
  g.na1 = -a1; g.sth = c.sth;
  g.Xhi = q.Xhi; g.Zhi = q.Zhi; g.tab3 = q.pad[0]; g.env = q.env; g.pad[0] = g.pad[1] = 0u;
  d.dy = dy; d.a2 = a2; d.cth = c.cth; d.cE = cex + eys; d.Kr = 1.05f * c.Cy * qpm;
  d.tx = c.tx; d.ndy = -dy;
  const float kgc = (c.Cy - GROUND_Y) / c.Cy;
  // one-ray range of inv = 1 / den (t = Cy inv, rho = dy inv): rho <= 1/4, tg (1 + 2 rho) <= 0.98 far (with rho <= 1/4:
  // 1.5 tg), t (1 - 2 rho) >= 1.02 near (with rho <= 1/4: t / 2) -- pix_inv_dr's PF_ALWAYS_EDGE / PF_TILE_OK / PF_GROUND_OK,
  // conservatively
  d.inv_lo = 2.04f * NEAR_Z / c.Cy;
  d.inv_hi = fminf(0.25f / dy, 0.98f * FAR_Z / (1.5f * kgc * c.Cy));
  const float ndl = fmaxf(c.cth * c.L[1] + c.sth * c.L[2], 0.f);   // directional light on the tile plane (eye-space normal (0, cth, sth))
  if (c.L[3] != 0.f) d.inv_hi = -1.f;                // positional light: per-pixel light term -> everything to the exact path
  for (int k = 0; k < 3; ++k) d.kc[k] = fminf(c.base[k] + c.dif[k] * ndl, 1.f) * (1.f / 256.f);
  d.hor_rgb = q.hor_rgb;
  d.kg = kgc; d.gx1 = (float)m.grid_w * S; d.gz1 = (float)m.grid_h * S; d.qpm = qpm;
  for (int k = 0; k < 3; ++k) d.kcc[k] = -8388608.f * d.kc[k];
  EnvDX& x = D.x;
  x.hx0 = g.hx0; x.hx1 = g.hx1; x.hx2 = g.hx2; x.hz0 = g.hz0; x.hz1 = g.hz1; x.hz2 = g.hz2; x.Cx = q.Cx; x.Cz = q.Cz;
  x.na1 = -a1; x.sth = c.sth; x.Xhi = q.Xhi; x.Zhi = q.Zhi; x.tab3 = g.tab3; x.env = g.env; x.kg = kgc; x.qpm = qpm;
  x.Cy = c.Cy; x.positional = c.L[3] != 0.f ? -1.f : 1.f;
  for (int k = 0; k < 3; ++k) { x.kc[k] = d.kc[k]; x.hor[k] = c.hor[k]; x.gnd[k] = c.gnd[k]; x.base[k] = c.base[k]; }
  x.gndl0 = c.gndl[0]; x.gndl1 = c.gndl[1]; x.gndl2 = c.gndl[2]; x.gndl3 = c.gndl[3]; x.dif0 = c.dif[0]; x.dif1 = c.dif[1]; x.dif2 = c.dif[2];
  x.pad0 = x.pad1 = x.pad2 = 0.f;
  for (int k = 0; k < 16; ++k) D.pad_[k] = 0;
}

__device__ inline void fill_envd_at(EnvD* arr, int idx, const EnvCam& c, const EnvQ& q, const RenderMapDev& m, float q_cells, int H, int W) {
  EnvD d;
  fill_envd(d, c, q, m, q_cells, H, W);
  arr[idx] = d;
}

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
  [[maybe_unused]] uint8_t* const st_base = st_ok ? frames + st_off : reinterpret_cast<uint8_t*>(R.dump) + lane * 16;
  [[maybe_unused]] const uint32_t st_stride = st_ok ? (uint32_t)npix * 3u : 0u;
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
    // (margin: MSAA sample offset + the fp16 rounding of the pixel centres kept in spxy - the triangle boxes' pad; render_v3.inc)
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
      // byte 0 the fraction, byte 1 the cell, byte 2 the tile; render.hip, quad_weights8)
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
    // ---- unlit byte-weight filter (quad_weights8, render.hip: one v_dot4_u32_u8 per channel), then the per-channel light in float
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
// wavefronts, static first grab), but a pixel is resolved the way resolve_region_v3 (render_v3.inc) resolves one for the shared camera --
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
