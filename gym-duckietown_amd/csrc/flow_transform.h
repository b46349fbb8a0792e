// flow_transform.h -- the per-env transform of dtsim_flow (the quantity: include/dtsim.h), stated once for the device (render_views.hip
// k_flow_setup) and for host programs: from the remembered state (FlowMark) and the current one, in float64, the float32 record (FlowRec,
// render_records.h) that takes an eye-space point of the current camera to the eye space of the previous one.  Plain C++ without a HIP
// header, as ipm_project.h, whose camera (dt_ipm_camera: dtsim_ipm's step 1) it uses; tests/test_flow_model_host.py compiles it with g++
// under the sanitizers.
//
// Eye coordinates of a world point P (oracle/raster.py Camera.to_eye): E = V (P - C), V = Rx Y with
//   Y  = [[sa, 0, ca], [0, 1, 0], [-ca, 0, sa]]          the yaw: along the agent's right, up and backward axes
//   Rx = [[1, 0, 0], [0, cth, -sth], [0, sth, cth]]      the pitch
// A static point: E_prev = Vp (Vc^T E + Cc - Cp) = M E + t,  M = Vp Vc^T,  t = Vp (Cc - Cp).
// A point of mesh object o, which k_obj_setup places as pos + Ry(y_rot) (scale model), Ry(a) = [[cos a, 0, sin a], [0, 1, 0], [-sin a, 0, cos a]]:
//   P_prev = pos_p + Ro (P - pos_c), Ro = Ry(y_rot_p - y_rot_c), so  M_o = Vp Ro Vc^T,  t_o = Vp (Ro (Cc - pos_c) + pos_p - Cp).
// EXACTNESS.  Nothing is formed as a product of two rotations that ought to cancel.  Every rotation difference is taken as an ANGLE
// difference in float64 first (yaw, pitch, y_rot: exactly 0 where nothing turned) and enters as R - I = [[g, 0, s], [0, 0, 0], [-s, 0, g]]
// with g = -2 sin^2(a / 2), s = sin a, both exactly 0 at a = 0:
//   M   = Rx(pitch_p - pitch_c) + Rx_p (D - I) Rx_c^T,     D = Yp Yc^T, the yaw by ang_p - ang_c
//   M_o = M + Vp (Ro - I) Vc^T
//   d   = Cc - Cp  (positions, noise and the 0.066 m offsets subtracted in float64, term by term);  t = Vp d
//   d_o = d + (Ro - I)(Cc - pos_c) + (pos_p - pos_c);  t_o = Vp d_o
// so a state that equals its mark gives M = I and t = 0 in every bit, an object that stands still gives its env's static pair, and no
// per-pixel arithmetic subtracts metres from metres.
#pragma once
#include "ipm_project.h"
#include "render_records.h"

// One state as the transform reads it: the pose, the camera (height, pitch, fov_y, noise x y z: the floats of DTSIM_FIELD_CAMERA promoted,
// or the shared camera's constants), the dynamic slots (cx, cy, cz, y_rot in degrees).
struct FlowState {
  double x, z, ang;
  double cam[6];
  double ob[8][4];
};

DT_IPM_HD inline void dt_flow_shared_camera(double cam[6]) {       // dt_ipm_shared_camera's constants
  cam[0] = 0.108; cam[1] = 19.15 * (3.141592653589793 / 180.0); cam[2] = 75.0 * (3.141592653589793 / 180.0);
  cam[3] = cam[4] = cam[5] = 0.0;
}

// What the object pairs need of the env beside the static pair, in float64.
struct FlowFrame { double Vp[9], Vc[9], M[9], d[3], Cc[3]; };

DT_IPM_HD inline void dt_flow_mul33(const double* a, const double* b, bool b_transposed, double* out) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double s = 0.0;
      for (int k = 0; k < 3; ++k) s += a[3 * i + k] * (b_transposed ? b[3 * j + k] : b[3 * k + j]);
      out[3 * i + j] = s;
    }
}
DT_IPM_HD inline void dt_flow_mul3(const double* a, const double* v, double* out) {
  for (int i = 0; i < 3; ++i) out[i] = a[3 * i] * v[0] + a[3 * i + 1] * v[1] + a[3 * i + 2] * v[2];
}
DT_IPM_HD inline void dt_flow_round(const double* M, const double* t, FlowXf& x) {
  for (int i = 0; i < 9; ++i) x.M[i] = (float)M[i];
  for (int i = 0; i < 3; ++i) x.t[i] = (float)t[i];
}

// The static pair and the two cameras' half-extents of `rec`, and the frame the object pairs are formed in.
DT_IPM_HD inline void dt_flow_static(const FlowState& cur, const FlowState& prev, int W, int H, FlowRec& rec, FlowFrame& f) {
  double sac, cac, sap, cap;
  sac = sin(cur.ang); cac = cos(cur.ang); sap = sin(prev.ang); cap = cos(prev.ang);
  const IpmCam cc = dt_ipm_camera(cur.cam[0], cur.cam[1], cur.cam[2], &cur.cam[3], sac, cac, W, H);
  const IpmCam cp = dt_ipm_camera(prev.cam[0], prev.cam[1], prev.cam[2], &prev.cam[3], sap, cap, W, H);
  const double Yc[9] = {sac, 0.0, cac, 0.0, 1.0, 0.0, -cac, 0.0, sac}, Yp[9] = {sap, 0.0, cap, 0.0, 1.0, 0.0, -cap, 0.0, sap};
  const double Rc[9] = {1.0, 0.0, 0.0, 0.0, cc.cth, -cc.sth, 0.0, cc.sth, cc.cth}, Rp[9] = {1.0, 0.0, 0.0, 0.0, cp.cth, -cp.sth, 0.0, cp.sth, cp.cth};
  dt_flow_mul33(Rc, Yc, false, f.Vc);
  dt_flow_mul33(Rp, Yp, false, f.Vp);
  // D - I: the yaw by da = ang_p - ang_c, Yp Yc^T = [[cos da, 0, -sin da], [0, 1, 0], [sin da, 0, cos da]]
  const double da = prev.ang - cur.ang, hs = sin(0.5 * da), g = -2.0 * hs * hs, s = sin(da);
  const double G[9] = {g, 0.0, -s, 0.0, 0.0, 0.0, s, 0.0, g};
  double T1[9], T2[9];
  dt_flow_mul33(Rp, G, false, T1);
  dt_flow_mul33(T1, Rc, true, T2);
  // Rx(dp), dp = pitch_p - pitch_c
  const double dp = prev.cam[1] - cur.cam[1], hp = sin(0.5 * dp), gp = -2.0 * hp * hp, sp = sin(dp);
  const double Rx[9] = {1.0, 0.0, 0.0, 0.0, 1.0 + gp, -sp, 0.0, sp, 1.0 + gp};
  for (int i = 0; i < 9; ++i) f.M[i] = Rx[i] + T2[i];
  // d = Cc - Cp, term by term: the agent's positions, the noise, the 0.066 m offsets along each state's heading, the heights
  f.d[0] = (cur.x - prev.x) + (cur.cam[3] - prev.cam[3]) + DT_IPM_FORWARD_DIST * (cac - cap);
  f.d[1] = (cur.cam[4] - prev.cam[4]) + (cur.cam[0] - prev.cam[0]);
  f.d[2] = (cur.z - prev.z) + (cur.cam[5] - prev.cam[5]) - DT_IPM_FORWARD_DIST * (sac - sap);
  f.Cc[0] = cur.x + cur.cam[3] + DT_IPM_FORWARD_DIST * cac; f.Cc[1] = cc.cy; f.Cc[2] = cur.z + cur.cam[5] - DT_IPM_FORWARD_DIST * sac;
  double t[3];
  dt_flow_mul3(f.Vp, f.d, t);
  dt_flow_round(f.M, t, rec.fix);
  rec.txc = (float)cc.tx; rec.tyc = (float)cc.ty; rec.txp = (float)cp.tx; rec.typ = (float)cp.ty;
}

// The pair of dynamic slot k: the object's centre (x, height, z) and y_rot (degrees) at both times; static_y: the instance's own height
// cancels (k_obj_setup adds it to both), so the heights here are DTSIM_FIELD_OBJ_Y's.
DT_IPM_HD inline void dt_flow_object(const FlowFrame& f, const double cur[4], const double prev[4], FlowXf& out) {
  const double dth = (prev[3] - cur[3]) * (3.141592653589793 / 180.0), hs = sin(0.5 * dth), g = -2.0 * hs * hs, s = sin(dth);
  const double G[9] = {g, 0.0, s, 0.0, 0.0, 0.0, -s, 0.0, g};          // Ro - I
  double T1[9], T2[9], M[9], r[3], gr[3], d[3], t[3];
  dt_flow_mul33(f.Vp, G, false, T1);
  dt_flow_mul33(T1, f.Vc, true, T2);
  for (int i = 0; i < 9; ++i) M[i] = f.M[i] + T2[i];
  for (int i = 0; i < 3; ++i) r[i] = f.Cc[i] - cur[i];
  dt_flow_mul3(G, r, gr);
  for (int i = 0; i < 3; ++i) d[i] = f.d[i] + gr[i] + (prev[i] - cur[i]);
  dt_flow_mul3(f.Vp, d, t);
  dt_flow_round(M, t, out);
}

// The whole record of one env.  per_env: the handle renders per-env cameras (DTSIM_F_DOMAIN_RAND) -- else both states take the shared
// camera, whatever their camera floats hold.  cur_episode / cur_map: the current state's.
DT_IPM_HD inline void dt_flow_record(const FlowMark& m, const FlowState& cur_in, int cur_episode, int cur_map, bool per_env, int W, int H,
                                     FlowRec& rec) {
  FlowState cur = cur_in, prev;
  prev.x = m.x; prev.z = m.z; prev.ang = m.ang;
  for (int k = 0; k < 6; ++k) prev.cam[k] = (double)m.cam[k];
  if (!per_env) { dt_flow_shared_camera(cur.cam); dt_flow_shared_camera(prev.cam); }
  for (int k = 0; k < 8; ++k)
    for (int c = 0; c < 4; ++c) prev.ob[k][c] = m.ob[k][c];
  FlowFrame f;
  dt_flow_static(cur, prev, W, H, rec, f);
  for (int k = 0; k < 8; ++k) dt_flow_object(f, cur.ob[k], prev.ob[k], rec.dyn[k]);
  rec.valid = (m.has != 0 && m.episode == cur_episode && m.map_id == cur_map) ? 1 : 0;
  rec.pad[0] = rec.pad[1] = rec.pad[2] = 0;
}
