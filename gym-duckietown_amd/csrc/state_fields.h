// state_fields.h -- the per-env simulation state of a handle, stated once: the struct of device arrays the kernels take (SimArrays),
// the slab those arrays are carved from (DT_STATE_ARRAYS, dt_state_layout: the checkpoint format of DTSIM_FIELD_STATE_BLOB) and the
// public fields of dtsim_read / dtsim_write / dtsim_field_devptr as views of them (DT_STATE_FIELDS).  Plain C++17 without a HIP header,
// so a host program can include it (tests/test_state_fields_host.py lays out, scatters and gathers with g++).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/dtsim.h"

// ---- per-env SoA ------------------------------------------------------------
struct SimArrays {
  int32_t N;
  // pose + dynamics (duckietown_world state, restated)
  double *pos_x, *pos_z, *angle;
  double *q_x, *q_y, *q_c, *q_s, *vel_u, *vel_w;
  double *ring;            // [DTSIM_MAX_DELAY][2][N]  delayed [left,right] duty
  double *war, *wal;       // angular input gains (trim)
  double *wheel_dist;
  double *timestamp, *speed;
  double *reward;
  double *lane;            // [4][N]
  double *prox;
  double *wheels;          // [2][N]
  // dynamic objects [slot][N]
  double *ob_cx, *ob_cz, *ob_sx, *ob_sz;
  double *ob_corners;      // [8][DTSIM_MAX_DYNAMIC][N]
  double *ob_vel, *ob_wait, *ob_time, *ob_angle, *ob_wiggle, *ob_yrot;
  // render / DR parameters (f32, consumed by the raster)
  float *cam;              // [6][N] height, pitch(rad), fov_y(rad), noise x,y,z
  float *colors;           // [16][N] horizon rgb, ground rgb, ambient rgb, diffuse rgb, light xyzw
  int32_t *ring_head, *step_count, *tile_i, *tile_j, *map_id, *episode;
  uint8_t *done, *done_code, *in_lane;
  uint8_t *ob_active;      // [DTSIM_MAX_DYNAMIC][N]
  uint8_t *ob_visible;     // [DTSIM_MAX_OBJECTS][N]
  uint8_t *ob_light;       // [DTSIM_MAX_OBJECTS][N] TrafficLightObj.pattern
  double *ob_cy;           // [DTSIM_MAX_DYNAMIC][N] centre height (CheckerboardObj; 0 for the others)
  double *ob_ext;          // [5][DTSIM_MAX_DYNAMIC][N] DuckiebotObj follow_dist, radius, wheel_dist, robot_width, robot_length
  double *tl_time;         // [N] TrafficLightObj.time (object clock: not reset with the env, objects.py:441,459)
};

// ---- the slab ---------------------------------------------------------------
// One row per array, in slab order: the array of row r starts where row r - 1 ends, each rounded up to 256 bytes.  This order is the
// checkpoint format (tl_time, ob_cy and ob_ext were added last and stay last); the order of SimArrays' members is the kernel argument's.
struct StateArray { uint16_t member, elem, planes; };   // offsetof(SimArrays, member); bytes per element; [planes][N]
#define DT_M(m) offsetof(SimArrays, m)
#define DT_E(m) sizeof(*SimArrays().m)
#define DT_ARRAY(m, planes) {DT_M(m), DT_E(m), planes}
static constexpr StateArray DT_STATE_ARRAYS[] = {
  DT_ARRAY(pos_x, 1), DT_ARRAY(pos_z, 1), DT_ARRAY(angle, 1),
  DT_ARRAY(q_x, 1), DT_ARRAY(q_y, 1), DT_ARRAY(q_c, 1), DT_ARRAY(q_s, 1), DT_ARRAY(vel_u, 1), DT_ARRAY(vel_w, 1),
  DT_ARRAY(ring, DTSIM_MAX_DELAY * 2),
  DT_ARRAY(war, 1), DT_ARRAY(wal, 1), DT_ARRAY(wheel_dist, 1), DT_ARRAY(timestamp, 1), DT_ARRAY(speed, 1), DT_ARRAY(reward, 1),
  DT_ARRAY(lane, 4), DT_ARRAY(prox, 1), DT_ARRAY(wheels, 2),
  DT_ARRAY(ob_cx, DTSIM_MAX_DYNAMIC), DT_ARRAY(ob_cz, DTSIM_MAX_DYNAMIC), DT_ARRAY(ob_sx, DTSIM_MAX_DYNAMIC), DT_ARRAY(ob_sz, DTSIM_MAX_DYNAMIC),
  DT_ARRAY(ob_corners, DTSIM_MAX_DYNAMIC * 8),
  DT_ARRAY(ob_vel, DTSIM_MAX_DYNAMIC), DT_ARRAY(ob_wait, DTSIM_MAX_DYNAMIC), DT_ARRAY(ob_time, DTSIM_MAX_DYNAMIC), DT_ARRAY(ob_angle, DTSIM_MAX_DYNAMIC),
  DT_ARRAY(ob_wiggle, DTSIM_MAX_DYNAMIC), DT_ARRAY(ob_yrot, DTSIM_MAX_DYNAMIC),
  DT_ARRAY(cam, 6), DT_ARRAY(colors, 16),
  DT_ARRAY(ring_head, 1), DT_ARRAY(step_count, 1), DT_ARRAY(tile_i, 1), DT_ARRAY(tile_j, 1), DT_ARRAY(map_id, 1), DT_ARRAY(episode, 1),
  DT_ARRAY(done, 1), DT_ARRAY(done_code, 1), DT_ARRAY(in_lane, 1),
  DT_ARRAY(ob_active, DTSIM_MAX_DYNAMIC), DT_ARRAY(ob_visible, DTSIM_MAX_OBJECTS), DT_ARRAY(ob_light, DTSIM_MAX_OBJECTS),
  DT_ARRAY(tl_time, 1), DT_ARRAY(ob_cy, DTSIM_MAX_DYNAMIC), DT_ARRAY(ob_ext, DTSIM_MAX_DYNAMIC * 5),
};
constexpr size_t DT_STATE_N_ARRAYS = sizeof(DT_STATE_ARRAYS) / sizeof(DT_STATE_ARRAYS[0]);
constexpr bool dt_state_arrays_cover() {   // every pointer member of SimArrays (all of it behind N) has exactly one row
  for (size_t m = DT_M(pos_x); m < sizeof(SimArrays); m += sizeof(void*)) {
    int rows = 0;
    for (const StateArray& a : DT_STATE_ARRAYS) rows += a.member == m;
    if (rows != 1) return false;
  }
  return sizeof(SimArrays) == DT_M(pos_x) + DT_STATE_N_ARRAYS * sizeof(void*);
}
static_assert(dt_state_arrays_cover(), "DT_STATE_ARRAYS needs one row per pointer member of SimArrays");

inline char* dt_state_array(const SimArrays& A, size_t member) { char* p; memcpy(&p, reinterpret_cast<const char*>(&A) + member, sizeof p); return p; }
// Points A's arrays into the slab at `base` for N envs (null base: null arrays) and returns the slab's size.
inline size_t dt_state_layout(SimArrays& A, int N, char* base) {
  A.N = N;
  size_t off = 0;
  for (const StateArray& a : DT_STATE_ARRAYS) {
    char* p = base ? base + off : nullptr;
    memcpy(reinterpret_cast<char*>(&A) + a.member, &p, sizeof p);
    off += ((size_t)N * a.planes * a.elem + 255) & ~size_t(255);
  }
  return off;
}

// ---- the public fields ------------------------------------------------------
// The public layout of a field is [N][outer][inner] elements of `elem` bytes; the device holds planes of [N].  Component c = d * inner + k
// is plane d + k * kstep of the array src[k]; src[k] == 0: no array -- the component reads 0 and ignores writes.  outer == 0: the field is
// the slab itself.  A row without an array is no view of the slab (the render order and raster of the last pass: dtsim_api.hip).
// view: dtsim_field_devptr offers the device memory, the planes of src[0] from the first component's on ([outer][N]; POS: the x plane).
// It is stated, not derived: planes of two arrays that happen to be adjacent (tile_i, tile_j at N = 64) are no view.
struct StateField {
  int id;
  const char* name;
  uint16_t elem, outer, inner, kstep;
  bool writable, view;
  uint16_t src[5];
};
#define DT_ROW(F, elem, outer, inner, kstep, writable, view, ...) {DTSIM_FIELD_##F, "DTSIM_FIELD_" #F, elem, outer, inner, kstep, writable, view, {__VA_ARGS__}}
#define DT_FIELD(F, m, outer, inner, kstep, view, ...) DT_ROW(F, DT_E(m), outer, inner, kstep, true, view, __VA_ARGS__)
#define DT_RUN(F, m, comps) DT_FIELD(F, m, comps, 1, 0, true, DT_M(m))                       // comps planes of one array
#define DT_RENDER(F) DT_ROW(F, 4, 1, 1, 0, false, false, 0)                                   // int32 [N], read-only, not in the slab
static constexpr StateField DT_STATE_FIELDS[] = {
  DT_FIELD(POS, pos_x, 1, 3, 0, true, DT_M(pos_x), 0, DT_M(pos_z)),                           // y reads 0
  DT_RUN(ANGLE, angle, 1), DT_RUN(REWARD, reward, 1), DT_RUN(DONE, done, 1), DT_RUN(DONE_CODE, done_code, 1), DT_RUN(STEP_COUNT, step_count, 1),
  DT_FIELD(TILE, tile_i, 1, 2, 0, false, DT_M(tile_i), DT_M(tile_j)),
  DT_RUN(LANE, lane, 4), DT_RUN(IN_LANE, in_lane, 1), DT_RUN(PROX, prox, 1), DT_RUN(SPEED, speed, 1), DT_RUN(TIMESTAMP, timestamp, 1),
  DT_RUN(WHEELS, wheels, 2), DT_RUN(MAP_ID, map_id, 1),
  DT_FIELD(OBJ_CENTER, ob_cx, DTSIM_MAX_DYNAMIC, 2, 0, false, DT_M(ob_cx), DT_M(ob_cz)),
  DT_RUN(OBJ_ACTIVE, ob_active, DTSIM_MAX_DYNAMIC), DT_RUN(OBJ_YROT, ob_yrot, DTSIM_MAX_DYNAMIC),
  DT_FIELD(OBJ_PARAMS, ob_vel, DTSIM_MAX_DYNAMIC, 3, 0, false, DT_M(ob_vel), DT_M(ob_wait), DT_M(ob_wiggle)),
  DT_RUN(OBJ_VISIBLE, ob_visible, DTSIM_MAX_OBJECTS), DT_RUN(EPISODE, episode, 1),
  DT_ROW(STATE_BLOB, 1, 0, 0, 0, true, true, 0),                                              // the slab, dtsim_state_bytes() of it
  DT_RUN(OBJ_LIGHT, ob_light, DTSIM_MAX_OBJECTS), DT_RUN(OBJ_Y, ob_cy, DTSIM_MAX_DYNAMIC),
  DT_FIELD(OBJ_EXTRA, ob_ext, DTSIM_MAX_DYNAMIC, 5, DTSIM_MAX_DYNAMIC, false,                 // [5][slot][N] on the device, [slot][5] in public
           DT_M(ob_ext), DT_M(ob_ext), DT_M(ob_ext), DT_M(ob_ext), DT_M(ob_ext)),
  DT_RUN(CAMERA, cam, 6), DT_RUN(COLORS, colors, 16), DT_RUN(WHEEL_DIST, wheel_dist, 1),
  DT_RENDER(RENDER_POS), DT_RENDER(RENDER_PIPE),
};
constexpr bool dt_state_fields_in_order() {
  int n = 0;
  for (const StateField& f : DT_STATE_FIELDS) if (f.id != n++) return false;
  return n == DTSIM_FIELD__COUNT;
}
static_assert(dt_state_fields_in_order(), "DT_STATE_FIELDS needs one row per DTSIM_FIELD_*, in the order of their values");

inline const StateField* dt_state_field(int field) { return field >= 0 && field < DTSIM_FIELD__COUNT ? &DT_STATE_FIELDS[field] : nullptr; }
inline int dt_field_comps(const StateField& f) { return f.outer * f.inner; }
inline size_t dt_field_bytes(const StateField& f, size_t N, size_t slab_bytes) { return f.outer ? N * dt_field_comps(f) * f.elem : slab_bytes; }
// the [N] plane of component c in A's slab, or null where the component has no array
inline char* dt_field_plane(const SimArrays& A, const StateField& f, int c) {
  const int d = c / f.inner, k = c % f.inner;
  return f.src[k] ? dt_state_array(A, f.src[k]) + (size_t)(d + k * f.kstep) * (size_t)A.N * f.elem : nullptr;
}
// host memory: an [N] plane (null: zeros) into component c of the public [N][comps] layout, and that component back into a plane
inline void dt_plane_to_public(void* pub, const void* plane, size_t N, int comps, int c, size_t elem) {
  for (size_t i = 0; i < N; ++i) {
    char* dst = static_cast<char*>(pub) + (i * comps + c) * elem;
    if (plane) memcpy(dst, static_cast<const char*>(plane) + i * elem, elem);
    else memset(dst, 0, elem);
  }
}
inline void dt_public_to_plane(void* plane, const void* pub, size_t N, int comps, int c, size_t elem) {
  for (size_t i = 0; i < N; ++i) memcpy(static_cast<char*>(plane) + i * elem, static_cast<const char*>(pub) + (i * comps + c) * elem, elem);
}
