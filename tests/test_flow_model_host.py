"""CPU: the model of dtsim_flow (tests/flow_model.py) against a plain per-pixel loop; the DERIVATION of the tolerances tests/test_gpu_flow.py
holds the device to, with the constants it reads written beside it; the share of sure pixels; csrc/flow_transform.h -- the per-env
transform k_flow_setup compiles -- as a program of its own under the sanitizers; the ABI.

THE TOLERANCES.  The device is compared with a CANDIDATE of the model (flow_model.py) within
    plane-sure pixels:  4 E_PLANE + RHO, and `valid` must agree -- no cap
    everywhere else:    4 E_OBJ[case] + RHO on all but the case's cap of ALL pixels (fp.ORACLE_MESH.gt1 with meshes, fp.ORACLE_PLANE.gt1 without)
E_PLANE: the largest |delta flow| (px) between the oracle's map and its map from the float32-rounded poses scaled by 1 + 2e-7, over the
plane-sure pixels of every case.  E_OBJ[case]: over the other pixels of that comparison, the smallest bound that leaves at most a quarter
of the case's cap of all pixels beyond it (the worst env of the case).  The factor 4 is the depth row's, for the depth row's reason: it
covers the device's float32 ray set-up against the oracle's float64 (depth_model.INV_DEPTH_TOL).
RHO = 2 R ulp32(max(W, H)): R = 15 is the number of float32 roundings between the eye-space hit and a pixel coordinate in k_flow as
written, counted beside the lines they count (render_views.hip: 3 + 3 for the x and w of M X + t, 4 for the previous point's projection, 4
for the current one's, 1 for the difference; the forward model is float64 and adds none), each at most one ulp of a coordinate below
max(W, H).  R <= 32, so the projection stays float32."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import depth_model as dm
import flow_model as fm
import ipm_model as im
from dtsim import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gym-duckietown_amd", "csrc")

# ---- the constants (test_the_recorded_bounds_are_the_derived_ones recomputes them; profiles/flow_parity.txt lists them per case) ----------
E_PLANE = 2.124e-04                                # px ("planes_dr-backward": points a few cm in front of the previous camera)
E_OBJ = {"planes-forward": 3.598e-05, "planes-rotate": 2.580e-05, "planes-backward": 1.126e-04, "planes-tile": 1.887e-05,
         "planes_dr-forward": 3.577e-05, "planes_dr-rotate": 2.579e-05, "planes_dr-backward": 1.076e-04, "planes_dr-tile": 1.940e-05,
         "pedestrians-still": 1.328e-04, "pedestrians-forward": 1.284e-04, "town-forward": 1.730e-05, "town_odd-rotate": 6.632e-06}
R_ROUNDINGS = 15
assert R_ROUNDINGS <= 32


def ulp32(x):
    return float(np.spacing(np.float32(x)))


def rho(W, H):
    return 2 * R_ROUNDINGS * ulp32(max(W, H))


def tolerances(name):
    """(plane tolerance, tolerance elsewhere, cap) of a case, in px."""
    c = fm.case_of(name)
    return 4 * E_PLANE + rho(c.W, c.H), 4 * E_OBJ[name] + rho(c.W, c.H), c.cap


def derive(name):
    """(largest plane-sure nudge difference, E_obj, smallest share of sure pixels, per-env rows) of a case, on the oracle alone."""
    c = fm.case_of(name)
    plane, e_obj, sure, rows = 0.0, 0.0, 1.0, []
    for e in range(len(c.states)):
        s = fm.nudge_stats(name, e)
        rest = np.sort(np.where(s["plane"], 0.0, s["err"]).ravel())[::-1]
        eo = float(rest[int(math.floor(c.cap / 4 * rest.size))])        # at most cap / 4 of ALL pixels lie beyond it
        plane, e_obj, sure = max(plane, s["plane_max"]), max(e_obj, eo), min(sure, s["sure"])
        rows.append(f"{name:20s} env {e}  {c.W:3d} x {c.H:3d}  plane-sure {s['n_plane']:5d} px max {s['plane_max']:.3e}  E_obj {eo:.3e}  sure {s['sure']:.3f}  "
                    f"valid {s['valid']:.2f}  |flow| up to {s['flow_max']:.1f} px")
    return plane, e_obj, sure, rows


def parity_report():
    """The text of profiles/flow_parity.txt."""
    lines = ["dtsim_flow: the tolerances of tests/test_gpu_flow.py, derived by tests/test_flow_model_host.py (python -c 'import test_flow_model_host as t; print(t.parity_report())')",
             "oracle-side model (tests/flow_model.py) against itself from the float32-rounded poses scaled by 1 + 2e-7; px", ""]
    worst = 0.0
    for name in fm.CASES:
        plane, _, _, rows = derive(name)
        worst = max(worst, plane)
        lines += rows
    lines += ["", f"E_PLANE {worst:.3e}", f"R = {R_ROUNDINGS}: RHO = {rho(160, 120):.3e} at 160 x 120, {rho(90, 62):.3e} at 90 x 62"]
    lines += [f"{n:20s} tolerance plane-sure {tolerances(n)[0]:.3e}  elsewhere {tolerances(n)[1]:.3e}  cap {tolerances(n)[2]:.1e}" for n in fm.CASES]
    return "\n".join(lines)


@pytest.mark.parametrize("name", list(fm.CASES))
def test_the_recorded_bounds_are_the_derived_ones(name):
    """The constants above state what the oracle gives, to the digits written (the plane bound: no case exceeds it, and the worst states it),
    and at least 80 % of every env's pixels are sure."""
    plane, e_obj, sure, _ = derive(name)
    assert plane <= E_PLANE * (1 + 1e-3), (name, plane)
    if name == "planes_dr-backward":
        assert plane >= E_PLANE * (1 - 1e-3), (name, plane)
    assert abs(e_obj - E_OBJ[name]) <= 1e-3 * E_OBJ[name], (name, e_obj)
    assert sure >= 0.80, (name, sure)


def test_the_cases_cover_what_they_are_named_for():
    """"backward" takes points behind the previous near plane and past its image border; "tile" crosses a tile border; the pedestrians move."""
    r = fm.run("planes-backward", 0)
    hit = np.isfinite(dm.host_buffers("planes", 0)[0])
    assert (hit & ~r.valid).sum() > 1000
    ts = dm.scene_of("planes").m.tile_size
    moved = 0
    for (x, z, a, *_r) in fm.case_of("planes-tile").states:
        px, pz, _ = fm.prev_pose(x, z, a, "tile")
        moved += (math.floor(px / ts), math.floor(pz / ts)) != (math.floor(x / ts), math.floor(z / ts))
    assert moved >= 1
    cur, prev = fm.host_objects("pedestrians-forward", 1)
    assert max(float(np.abs(np.asarray(a["pos"]) - np.asarray(b["pos"])).max()) for a, b in zip(cur, prev)) > 1e-3


@pytest.mark.parametrize("name,e,fisheye", [("planes_dr-backward", 2, False), ("pedestrians-forward", 1, True)])
def test_the_model_against_a_plain_loop(name, e, fisheye):
    cal = im.nominal_cal() if fisheye else None
    exp = fm.expected(name, e, None, cal)
    flow, valid = fm.expected_loop(name, e, cal)
    assert np.array_equal(valid, exp.valid)
    assert np.abs(flow - exp.flow).max() <= 1e-9
    assert valid.mean() > 0.3 and np.abs(flow).max() > 5.0


def test_a_candidate_set_holds_its_own_members_and_refuses_others():
    name = "pedestrians-forward"
    exp = fm.expected(name, 1)
    tp, to, cap = tolerances(name)
    own = np.moveaxis(exp.flow, -1, 0).astype(np.float32)
    fm.hold(exp, own, exp.valid.astype(np.uint8), tp, to, cap, name)
    off = own.copy()
    off[0][exp.plane & exp.valid] += 0.01
    with pytest.raises(AssertionError):
        fm.hold(exp, off, exp.valid.astype(np.uint8), tp, to, cap, name)
    flipped = exp.valid.astype(np.uint8)
    y, x = np.argwhere(exp.plane & exp.valid)[0]
    flipped[y, x] = 0
    zero = own.copy()
    zero[:, y, x] = 0
    with pytest.raises(AssertionError):
        fm.hold(exp, zero, flipped, tp, to, cap, name)


# ---- csrc/flow_transform.h as a host program -----------------------------------------------------------------------------------------------
PROGRAM = r"""
#include <stdio.h>
#include <string.h>
#include "flow_transform.h"
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %d: %s\n", __LINE__, #c); return 1; } } while (0)
static bool identity(const FlowXf& x) {
  for (int i = 0; i < 9; ++i) if (x.M[i] != (i % 4 == 0 ? 1.f : 0.f)) return false;
  return x.t[0] == 0.f && x.t[1] == 0.f && x.t[2] == 0.f;
}
static void print(const FlowXf& x) {
  for (float v : x.M) printf("%.9g ", v);
  for (float v : x.t) printf("%.9g ", v);
  printf("\n");
}
// input: W H per_env; cur: x z ang cam[6] ob0[4]; prev: the same
int main(int argc, char** argv) {
  CHECK(argc == 2);
  FILE* fi = fopen(argv[1], "r");
  CHECK(fi);
  int W, H, per_env;
  CHECK(fscanf(fi, "%d %d %d", &W, &H, &per_env) == 3);
  FlowState cur;
  FlowMark m;
  memset(&cur, 0, sizeof cur); memset(&m, 0, sizeof m);
  CHECK(fscanf(fi, "%lf %lf %lf", &cur.x, &cur.z, &cur.ang) == 3);
  for (double& v : cur.cam) CHECK(fscanf(fi, "%lf", &v) == 1);
  for (double& v : cur.ob[0]) CHECK(fscanf(fi, "%lf", &v) == 1);
  CHECK(fscanf(fi, "%lf %lf %lf", &m.x, &m.z, &m.ang) == 3);
  for (float& v : m.cam) CHECK(fscanf(fi, "%f", &v) == 1);
  for (double& v : m.ob[0]) CHECK(fscanf(fi, "%lf", &v) == 1);
  fclose(fi);
  m.has = 1; m.episode = 3; m.map_id = 1;
  FlowRec r;
  dt_flow_record(m, cur, 3, 1, per_env != 0, W, H, r);
  CHECK(r.valid == 1);
  print(r.fix); print(r.dyn[0]);
  printf("%.9g %.9g %.9g %.9g\n", r.txc, r.tyc, r.txp, r.typ);
  // slots nothing moved in take the static pair, bit for bit
  for (int k = 1; k < 8; ++k) CHECK(memcmp(&r.dyn[k], &r.fix, sizeof(FlowXf)) == 0);
  // a mark of another episode, of another map, or none
  dt_flow_record(m, cur, 4, 1, per_env != 0, W, H, r); CHECK(r.valid == 0);
  dt_flow_record(m, cur, 3, 0, per_env != 0, W, H, r); CHECK(r.valid == 0);
  m.has = 0; dt_flow_record(m, cur, 3, 1, per_env != 0, W, H, r); CHECK(r.valid == 0);
  m.has = 1;
  // zero motion: the identity in every bit, at headings far outside (-pi, pi], per-env and shared camera, with objects in every slot
  const double angs[] = {40.5, -7.5, 0.3, 0.0};
  for (double a : angs)
    for (int pe = 0; pe < 2; ++pe) {
      FlowState s = cur;
      s.ang = a;
      for (int k = 0; k < 8; ++k) { s.ob[k][0] = 1.1 + 0.37 * k; s.ob[k][1] = 0.01 * k; s.ob[k][2] = 2.3 - 0.21 * k; s.ob[k][3] = 77.7 * k - 200.0; }
      FlowMark z;
      memset(&z, 0, sizeof z);
      z.x = s.x; z.z = s.z; z.ang = s.ang; z.has = 1;
      for (int k = 0; k < 6; ++k) { z.cam[k] = (float)s.cam[k]; s.cam[k] = (double)z.cam[k]; }
      for (int k = 0; k < 8; ++k) for (int c = 0; c < 4; ++c) z.ob[k][c] = s.ob[k][c];
      dt_flow_record(z, s, 0, 0, pe != 0, W, H, r);
      CHECK(r.valid == 1 && identity(r.fix) && r.txc == r.txp && r.tyc == r.typ);
      for (int k = 0; k < 8; ++k) CHECK(identity(r.dyn[k]));
      // the robot still, one duckie walking: the static pair stays the identity, only that slot moves
      z.ob[2][0] -= 0.05; z.ob[2][3] += 12.0;
      dt_flow_record(z, s, 0, 0, pe != 0, W, H, r);
      CHECK(identity(r.fix) && !identity(r.dyn[2]) && identity(r.dyn[1]) && identity(r.dyn[3]));
    }
  return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("flow_host")
    (d / "flow_host.cpp").write_text(PROGRAM)
    exe = d / "flow_host"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                           str(d / "flow_host.cpp"), "-o", str(exe)])
    return d, exe


@pytest.mark.parametrize("per_env", [False, True])
def test_the_transform_header_under_sanitizers_against_the_oracles_cameras(program, per_env):
    """csrc/flow_transform.h in a program of its own, built with AddressSanitizer and UndefinedBehaviorSanitizer and run as a child process:
    M E + t takes the oracle camera's eye coordinates of a world point to the previous camera's, for a static point and for a point of a
    moved object, within float32 rounding; the zero-motion identities hold exactly (checked inside the program, at theta = 40.5 and -7.5);
    it exits clean."""
    from oracle import raster
    d, exe = program
    W, H = 160, 120
    camf = [float(np.float32(v)) for v in (0.1134, 0.3501, 1.2543, 0.003, -0.002, 0.004)]
    camp = [float(np.float32(v)) for v in (0.1034, 0.3301, 1.3543, -0.001, 0.002, 0.001)]
    cur, prev = (1.9, 1.5, 40.5), (1.93, 1.46, 40.38)
    ob_c, ob_p = (2.3, 0.02, 1.2, 35.0), (2.25, 0.0, 1.31, -20.0)
    words = [W, H, int(per_env), *cur, *camf, *ob_c, *prev, *camp, *ob_p]
    (d / f"in{int(per_env)}.txt").write_text(" ".join(repr(v) for v in words))
    r = subprocess.run([str(exe), str(d / f"in{int(per_env)}.txt")], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    rows = [np.array(l.split(), np.float64) for l in r.stdout.strip().split("\n")]

    def cam(pose, c):
        kw = dict(cam_height=c[0], cam_angle_deg=math.degrees(c[1]), cam_fov_y_deg=math.degrees(c[2]), camera_noise=c[3:], domain_rand=True) if per_env else {}
        return raster.Camera((pose[0], 0.0, pose[1]), pose[2], width=W, height=H, **kw)
    cc, cp = cam(cur, camf), cam(prev, camp)
    assert np.allclose(rows[2], [cc.tx, cc.ty, cp.tx, cp.ty], rtol=2e-7, atol=0)
    P = np.array([[2.0, 0.0, 1.0], [2.4, 0.05, 1.3], [1.5, -0.008, 2.5], [30.0, 0.0, -20.0]])
    for row, Pp in ((rows[0], P), (rows[1], np.asarray(ob_p[:3]) + (P - np.asarray(ob_c[:3])) @ (fm._ry(ob_p[3]) @ fm._ry(ob_c[3]).T).T)):
        M, t = row[:9].reshape(3, 3), row[9:]
        got, want = cc.to_eye(P) @ M.T + t, cp.to_eye(Pp)
        assert np.abs(got - want).max() <= 4e-7 * max(1.0, float(np.abs(want).max())), (per_env, got, want)


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------

def test_abi_declares_the_entry_points_and_states_the_quantity():
    hdr = open(os.path.join(ROOT, "include", "dtsim.h")).read()
    assert re.search(r"^int dtsim_flow_mark\(dtsim_t\* h, const uint8_t\* mask\);", hdr, re.M)
    assert re.search(r"^int dtsim_flow\(dtsim_t\* h, float\* flow, uint8_t\* valid, int oh, int ow, uint32_t flags\);", hdr, re.M)
    assert re.search(r"^int dtsim_flow_masked\(dtsim_t\* h, float\* flow, uint8_t\* valid, int oh, int ow, uint32_t flags, const uint8_t\* mask\);", hdr, re.M)
    lib_names = ("dtsim_flow_mark", "dtsim_flow", "dtsim_flow_masked")
    assert all(n in _ffi.EXPORTS for n in lib_names)
    assert re.search(r"#define DTSIM_ABI_VERSION 12\b", hdr) and _ffi.ABI_VERSION == 12
    for words in ("flow = A(proj_prev(P_prev)) - A(proj_cur(P))", "prev_frame[p + flow] is what cur_frame[p] shows", "w_prev >= 0.04", "exactly 0.0",
                  "approximate INVERSE table", "dtsim_set_maps and dtsim_set_assets drop all marks"):
        assert words in hdr, words


@pytest.mark.parametrize("kw,word", [
    (dict(flow_valid=True), "flow_shape"),
    (dict(flow_shape=64), "flow_shape"),
    (dict(flow_shape=(7, 160)), "divide"),
    (dict(flow_shape=(120, 160), motion_blur=True, action_mode="wheels"), "motion_blur"),
    (dict(flow_shape=(120, 160), camera_rand=True, distortion=True), "camera_rand"),
    (dict(flow_shape=(120, 160), camera_rand=True, distortion=True, camera_rand_maps=True), "camera_rand"),
    (dict(flow_shape=(120, 160), undistort=True, distortion=True), "undistort"),
])
def test_the_vector_env_refuses_bad_arguments_before_it_touches_a_device(kw, word):
    from dtsim.vecenv import DuckietownVecEnv
    with pytest.raises(ValueError, match=word):
        DuckietownVecEnv("small_loop", 4, **kw)
