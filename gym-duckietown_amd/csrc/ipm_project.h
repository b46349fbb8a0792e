// ipm_project.h -- the ground projection of dtsim_ipm (the quantity: include/dtsim.h), stated once for the device kernels (render_views.hip
// k_ipm_table, k_ipm_env) and for host programs: floor cell -> source pixel of the env's camera frame, in float64.  Plain C++ without a HIP
// header, so a host program can include it (tests/test_ipm_model_host.py compiles it with g++ under the sanitizers).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DT_IPM_HD __host__ __device__
#else
#define DT_IPM_HD
#endif

#define DT_IPM_NEAR 0.04              // the near plane (oracle/raster.py NEAR)
#define DT_IPM_FORWARD_DIST 0.066     // CAMERA_FORWARD_DIST: the camera centre sits this far ahead of the axle

// One plumb-bob calibration as the projection reads it: K (fx, fy, u0, v0), D (k1, k2, p1, p2, k3) and the inverse of new_K, row-major.
struct IpmCal { double fx, fy, u0, v0, k1, k2, p1, p2, k3, ir[9]; };

// The camera of one env in the AGENT's frame (the pose's position cancels: a cell is given in that frame).  nf, nr: the camera noise along
// the agent's forward d = (cos a, -sin a) and right r = (sin a, cos a); cy: the centre's height above the tile plane; the pitch's sine and
// cosine; the half-extents of the image plane at depth 1.
struct IpmCam { double nf, nr, cy, sth, cth, tx, ty; };

// pitch and fov_y in radians, noise = (x, y, z) in world axes, sa / ca = sin / cos of the agent's angle
DT_IPM_HD inline IpmCam dt_ipm_camera(double cam_height, double pitch, double fov_y, const double noise[3], double sa, double ca, int W, int H) {
  IpmCam c;
  c.nf = noise[0] * ca - noise[2] * sa;
  c.nr = noise[0] * sa + noise[2] * ca;
  c.cy = noise[1] + cam_height;
  c.sth = sin(pitch); c.cth = cos(pitch);
  c.ty = tan(fov_y / 2);
  c.tx = c.ty * ((double)W / (double)H);
  return c;
}
// default_cam()'s: 0.108 m, 19.15 degrees, 75 degrees, no noise -- rigid in the agent's frame, whatever its angle
DT_IPM_HD inline IpmCam dt_ipm_shared_camera(int W, int H) {
  const double none[3] = {0.0, 0.0, 0.0};
  return dt_ipm_camera(0.108, 19.15 * (3.141592653589793 / 180.0), 75.0 * (3.141592653589793 / 180.0), none, 0.0, 1.0, W, H);
}

// K [9], D [5], new_K [9] (row-major, as OpenCV's) -> the record; false when a value is not finite or new_K has no inverse
inline bool dt_ipm_pack_cal(IpmCal& c, const double* K, const double* D, const double* nk) {
  for (int i = 0; i < 9; ++i) if (!isfinite(K[i]) || !isfinite(nk[i])) return false;
  for (int i = 0; i < 5; ++i) if (!isfinite(D[i])) return false;
  c.fx = K[0]; c.fy = K[4]; c.u0 = K[2]; c.v0 = K[5];
  c.k1 = D[0]; c.k2 = D[1]; c.p1 = D[2]; c.p2 = D[3]; c.k3 = D[4];
  const double c00 = nk[4] * nk[8] - nk[5] * nk[7], c01 = nk[5] * nk[6] - nk[3] * nk[8], c02 = nk[3] * nk[7] - nk[4] * nk[6];
  const double det = nk[0] * c00 + nk[1] * c01 + nk[2] * c02;
  if (!isfinite(det) || det == 0.0) return false;
  const double id = 1.0 / det;
  c.ir[0] = c00 * id; c.ir[1] = (nk[2] * nk[7] - nk[1] * nk[8]) * id; c.ir[2] = (nk[1] * nk[5] - nk[2] * nk[4]) * id;
  c.ir[3] = c01 * id; c.ir[4] = (nk[0] * nk[8] - nk[2] * nk[6]) * id; c.ir[5] = (nk[2] * nk[3] - nk[0] * nk[5]) * id;
  c.ir[6] = c02 * id; c.ir[7] = (nk[1] * nk[6] - nk[0] * nk[7]) * id; c.ir[8] = (nk[0] * nk[4] - nk[1] * nk[3]) * id;
  for (int i = 0; i < 9; ++i) if (!isfinite(c.ir[i])) return false;
  return true;
}

// where cell (i, j) lies in the agent's frame, in metres: f ahead, s to the right (dtsim_bev's cell geometry)
DT_IPM_HD inline void dt_ipm_cell(int i, int j, int oh, int ow, double cell, int rows_behind, double& f, double& s) {
  f = ((double)(oh - rows_behind - i) - 0.5) * cell;
  s = (((double)j + 0.5) - 0.5 * (double)ow) * cell;
}

// Step 3 of the quantity, the calibration's forward model, stated once for dt_ipm_source and for dtsim_flow (render_views.hip k_flow):
// dtsim/distortion.py rectify_maps -- cv::initUndistortRectifyMap's arithmetic -- at the real-valued index coordinates (px, py) of the
// rectified image gives the index coordinates (xd, yd) of the distorted one, plus `off` (0.5: what dt_ipm_source rounds down to a pixel; the
// sum is written here so that its kernels keep the instructions they had before the function existed -- tools/isa_compare.py).
DT_IPM_HD inline void dt_ipm_forward(const IpmCal& cal, double px, double py, double off, double& xd, double& yd) {
  const double _x = py * cal.ir[1] + cal.ir[2] + px * cal.ir[0];
  const double _y = py * cal.ir[4] + cal.ir[5] + px * cal.ir[3];
  const double _w = py * cal.ir[7] + cal.ir[8] + px * cal.ir[6];
  const double iw = 1.0 / _w;
  const double x = _x * iw, y = _y * iw;
  const double x2 = x * x, y2 = y * y, r2 = x2 + y2, _2xy = 2.0 * x * y;
  const double kr = 1.0 + ((cal.k3 * r2 + cal.k2) * r2 + cal.k1) * r2;
  const double xu = x * kr + cal.p1 * _2xy + cal.p2 * (r2 + 2.0 * x2);
  const double yu = y * kr + cal.p1 * (r2 + 2.0 * y2) + cal.p2 * _2xy;
  xd = cal.fx * xu + cal.u0 + off;
  yd = cal.fy * yu + cal.v0 + off;
}

// Steps 1 to 4 of the quantity: the source pixel r * W + c of the floor point f ahead and s to the right of the agent, or -1 where the
// cell is invalid.  cal: the env's calibration (the frames are fisheye), or null (rectilinear).  Every comparison is written so that a
// NaN fails it, and no value is converted to an integer before it is known to lie inside the frame.
DT_IPM_HD inline int32_t dt_ipm_source(const IpmCam& c, const IpmCal* cal, int W, int H, double f, double s) {
  // eye coordinates (oracle/raster.py Camera.to_eye) of P - C, C = pos + noise + (0.066 d, cam_height): along the agent's right,
  // up and backward axes first, then pitched
  const double xla = s - c.nr, yla = -c.cy, zla = -(f - DT_IPM_FORWARD_DIST - c.nf);
  const double xe = xla, ye = yla * c.cth - zla * c.sth, ze = yla * c.sth + zla * c.cth;
  const double w = -ze;
  if (!(w >= DT_IPM_NEAR)) return -1;
  const double u = (xe / w / c.tx + 1.0) * 0.5 * (double)W, v = (1.0 - ye / w / c.ty) * 0.5 * (double)H;
  double pc = u, pr = v;               // what is rounded down to the source pixel's column and row
  if (cal) {
    if (!(u >= 0.0 && u < (double)W && v >= 0.0 && v < (double)H)) return -1;
    dt_ipm_forward(*cal, u - 0.5, v - 0.5, 0.5, pc, pr);
  }
  if (!(pc >= 0.0 && pc < (double)W && pr >= 0.0 && pr < (double)H)) return -1;
  return (int32_t)pr * W + (int32_t)pc;  // (both are >= 0: the conversion rounds down)
}
