"""The expected ground projection of dtsim_ipm (include/dtsim.h), from the oracle's side alone, and the inputs the IPM tests share.

The quantity, steps 1 to 4, in float64 numpy: cell (i, j) stands for the point P = (x, z) + f d + s r on the tile plane y = 0 -- dtsim_bev's
cell geometry --; P goes through `oracle.raster.Camera` (to_eye, then overlay_lines' projection: u = (x_eye / w / tx + 1) W / 2,
v = (1 - y_eye / w / ty) H / 2, w = -z_eye); on rectilinear frames the source pixel is (floor v, floor u); on fisheye frames `forward`, a
real-valued restatement of dtsim/distortion.py rectify_maps, is evaluated at the index coordinates (u - 0.5, v - 0.5) and gives (xd, yd),
the source pixel is (floor(yd + 0.5), floor(xd + 0.5)).  Valid iff w >= 0.04, with a fisheye (u, v) inside [0, W) x [0, H), and the
source pixel inside the frame.  `src` is r W + c, or -1 where the cell is invalid: (valid, src) in one number.

The CANDIDATE SET of a cell: every src it takes when (xd, yd), (u, v) and w move by up to DELTA = 1e-6 px (w: DELTA_W = 1e-9 m) -- across
a pixel border, an image border or the near plane.  A cell is SURE when its set has one member: there the device must agree exactly;
elsewhere it must name a member of the set.

DELTA is derived, not chosen.  Both sides compute in float64 from the same inputs: the float64 pose and the float32-valued camera parameters
of DTSIM_FIELD_CAMERA, promoted.  About 50 roundings lie between those inputs and the compared coordinate, each at most one ulp of a value
below 1024 px, 1.1e-13: at most 1e-11 px together (the divisions by w >= 0.04 and by tx, ty >= 0.1 are part of the count: their results
are the coordinates themselves).  The device takes sin / cos / tan from ocml, numpy from glibc; both are within a few ulp, the same order.
DELTA leaves four orders of magnitude on top of that, and a pixel is six orders wider still.  DELTA_W likewise: w is below 100 m, an ulp
1.4e-14 m."""
import itertools
import math
from typing import NamedTuple, Optional

import numpy as np

from dtsim import distortion as pdist
from oracle import raster

DELTA, DELTA_W = 1e-6, 1e-9
assert 50 * 2.0 ** -43 * 1e4 <= DELTA          # 50 ulps of a coordinate below 1024 px, and four orders of magnitude

# (oh, ow, cell, rows_behind): 64 x 64; neither size a multiple of four, and a centre column that projects exactly onto u = W / 2 (the tie
# the candidate rule exists for); one cell; the agent inside the window; the whole window behind it (every cell invalid)
SHAPES = ((64, 64, 0.02, 0), (37, 53, 0.013, 0), (1, 1, 0.02, 0), (128, 96, 0.01, 32), (16, 24, 0.02, 16))
# x, z (metres), theta: on the road; negative coordinates; theta beyond 2 pi; theta negative beyond -2 pi
POSES = ((1.0, 0.9, 0.3), (-0.3, -0.2, -0.7), (1.9, 1.5, 40.5), (2.0, 1.1, -7.5))


class EnvCamera(NamedTuple):
    """The per-env camera as DTSIM_FIELD_CAMERA holds it: float32-valued height, pitch (rad), fov_y (rad), noise (x, y, z)."""
    height: float
    pitch: float
    fov_y: float
    noise: tuple


class Cal(NamedTuple):
    K: np.ndarray
    D: np.ndarray
    new_K: np.ndarray


def nominal_cal() -> Cal:
    return Cal(pdist.CAMERA_MATRIX.copy(), pdist.DIST_COEFS.copy(), pdist.optimal_new_camera_matrix())


def make_cal(K, D) -> Cal:
    K, D = np.asarray(K, np.float64), np.asarray(D, np.float64).reshape(-1)
    return Cal(K, D, pdist.optimal_new_camera_matrix(K, D))       # new_K for 640 x 480 at any camera size, as the reference computes it


def oracle_camera(pose, W, H, cam: Optional[EnvCamera] = None):
    x, z, th = pose
    if cam is None:
        return raster.Camera((x, 0.0, z), th, width=W, height=H)
    return raster.Camera((x, 0.0, z), th, cam_height=float(cam.height), cam_angle_deg=math.degrees(float(cam.pitch)),
                         cam_fov_y_deg=math.degrees(float(cam.fov_y)), camera_noise=tuple(float(v) for v in cam.noise), domain_rand=True,
                         width=W, height=H)


def cell_points(pose, shape):
    """P [oh, ow, 3] of the cells (y = 0): dtsim_bev's geometry in float64."""
    oh, ow, cell, rb = shape
    x, z, th = pose
    d, r = (math.cos(th), -math.sin(th)), (math.sin(th), math.cos(th))
    f = ((oh - rb - np.arange(oh, dtype=np.float64)) - 0.5)[:, None] * cell
    s = ((np.arange(ow, dtype=np.float64) + 0.5) - 0.5 * ow)[None, :] * cell
    return np.stack([x + f * d[0] + s * r[0], np.zeros((oh, ow)), z + f * d[1] + s * r[1]], axis=-1)


def project(cam, P):
    """(w, u, v) of world points through the oracle's camera: Camera.to_eye, then overlay_lines' projection."""
    pe = cam.to_eye(P)
    w = -pe[..., 2]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        u = (pe[..., 0] / w / cam.tx + 1) * 0.5 * cam.W
        v = (1 - pe[..., 1] / w / cam.ty) * 0.5 * cam.H
    return w, u, v


def forward(cal: Cal, x, y):
    """rectify_maps at real-valued index coordinates (x = column, y = row), float64, not rounded to float32: the distorted-image
    coordinates (xd, yd) that rectified index (x, y) samples."""
    k1, k2, p1, p2, k3 = np.asarray(cal.D, np.float64)[:5]
    K = cal.K
    fx, fy, u0, v0 = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    ir = np.linalg.inv(cal.new_K)
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    _x = y * ir[0, 1] + ir[0, 2] + x * ir[0, 0]
    _y = y * ir[1, 1] + ir[1, 2] + x * ir[1, 0]
    _w = y * ir[2, 1] + ir[2, 2] + x * ir[2, 0]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        w = 1.0 / _w
        x, y = _x * w, _y * w
        x2, y2 = x * x, y * y
        r2, _2xy = x2 + y2, 2 * x * y
        kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
        xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2)
        yd = y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy
        return fx * xd + u0, fy * yd + v0


def decide(w, u, v, pc, pr, W, H, fisheye):
    """src of cells whose depth is w, rectilinear coordinates (u, v) and rounded-down source coordinates (pc, pr): step 4."""
    with np.errstate(invalid="ignore"):
        ok = w >= raster.NEAR
        if fisheye:
            ok = ok & (u >= 0) & (u < W) & (v >= 0) & (v < H)
        ok = ok & (pc >= 0) & (pc < W) & (pr >= 0) & (pr < H)
    c = np.floor(np.where(ok, pc, 0.0)).astype(np.int64)
    r = np.floor(np.where(ok, pr, 0.0)).astype(np.int64)
    return np.where(ok, r * W + c, -1).astype(np.int32)


class Expected(NamedTuple):
    src: np.ndarray         # [oh, ow] int32, -1 = invalid
    sure: np.ndarray        # [oh, ow] bool
    cands: dict             # (i, j) -> frozenset of src, for the cells that are not sure
    w: np.ndarray
    u: np.ndarray
    v: np.ndarray

    @property
    def valid(self):
        return self.src >= 0


def _near_int(a):
    with np.errstate(invalid="ignore"):
        return np.abs(a - np.rint(a)) <= DELTA


def expected(pose, shape, W, H, cam: Optional[EnvCamera] = None, cal: Optional[Cal] = None) -> Expected:
    oc = oracle_camera(pose, W, H, cam)
    w, u, v = project(oc, cell_points(pose, shape))
    fisheye = cal is not None
    if fisheye:
        xd, yd = forward(cal, u - 0.5, v - 0.5)
        pc, pr = xd + 0.5, yd + 0.5
    else:
        pc, pr = u, v
    src = decide(w, u, v, pc, pr, W, H, fisheye)
    # the cells a move of DELTA can change: w at the near plane, a rounded coordinate at an integer (pixel and frame borders alike), (u, v)
    # at the image border (integers too)
    touch = (np.abs(w - raster.NEAR) <= DELTA_W) | _near_int(pc) | _near_int(pr)
    if fisheye:
        touch |= _near_int(u) | _near_int(v)
    cands = {}
    idx = np.argwhere(touch)
    if len(idx):
        ii, jj = idx[:, 0], idx[:, 1]
        seen = [set() for _ in idx]
        steps = (-1.0, 0.0, 1.0)
        # rectilinear: the rounded coordinates ARE (u, v) and move with them; fisheye: (xd, yd) move on their own
        for dw, du, dv, dc, dr in itertools.product(steps, steps, steps, steps if fisheye else (None,), steps if fisheye else (None,)):
            dc, dr = (du if dc is None else dc), (dv if dr is None else dr)
            got = decide(w[ii, jj] + dw * DELTA_W, u[ii, jj] + du * DELTA, v[ii, jj] + dv * DELTA, pc[ii, jj] + dc * DELTA,
                         pr[ii, jj] + dr * DELTA, W, H, fisheye)
            for k, g in enumerate(got):
                seen[k].add(int(g))
        for k, (i, j) in enumerate(idx):
            if len(seen[k]) > 1:
                cands[int(i), int(j)] = frozenset(seen[k])
    sure = np.ones(src.shape, bool)
    for i, j in cands:
        sure[i, j] = False
    return Expected(src, sure, cands, w, u, v)


def hold(exp: Expected, got_src):
    """The device's src of one env against the model: equal on sure cells, a member of the candidate set elsewhere.  Returns the number of
    unsure cells that took another member than the model's own."""
    got_src = np.asarray(got_src)
    assert got_src.shape == exp.src.shape and got_src.dtype == np.int32
    bad = (got_src != exp.src) & exp.sure
    assert not bad.any(), (int(bad.sum()), [(int(i), int(j), int(got_src[i, j]), int(exp.src[i, j])) for i, j in np.argwhere(bad)[:5]])
    other = 0
    for (i, j), c in exp.cands.items():
        assert int(got_src[i, j]) in c, (i, j, int(got_src[i, j]), sorted(c))
        other += int(got_src[i, j]) != int(exp.src[i, j])
    return other


def expected_loop(pose, shape, W, H, cam: Optional[EnvCamera] = None, cal: Optional[Cal] = None):
    """The same quantity cell by cell in plain Python floats, written out from the issue's statement without numpy or the oracle's classes:
    src [oh, ow]."""
    oh, ow, cell, rb = shape
    x, z, th = pose
    sa, ca = math.sin(th), math.cos(th)
    if cam is None:
        height, pitch, fov, noise = 0.108, math.radians(19.15), math.radians(75.0), (0.0, 0.0, 0.0)
    else:
        height, pitch, fov, noise = float(cam.height), float(cam.pitch), float(cam.fov_y), tuple(float(n) for n in cam.noise)
    C = (x + noise[0] + 0.066 * ca, 0.0 + noise[1] + height, z + noise[2] - 0.066 * sa)
    sth, cth = math.sin(pitch), math.cos(pitch)
    ty = math.tan(fov / 2)
    tx = ty * W / H
    if cal is not None:
        ir = np.linalg.inv(cal.new_K).tolist()
        k1, k2, p1, p2, k3 = (float(q) for q in np.asarray(cal.D).reshape(-1)[:5])
        fx, fy, u0, v0 = float(cal.K[0, 0]), float(cal.K[1, 1]), float(cal.K[0, 2]), float(cal.K[1, 2])
    out = np.full((oh, ow), -1, np.int32)
    for i in range(oh):
        for j in range(ow):
            f, s = (oh - rb - i - 0.5) * cell, (j + 0.5 - ow / 2) * cell
            P = (x + f * ca + s * sa, 0.0, z - f * sa + s * ca)
            rel = (P[0] - C[0], P[1] - C[1], P[2] - C[2])
            xla, yla, zla = rel[0] * sa + rel[2] * ca, rel[1], -(rel[0] * ca - rel[2] * sa)
            xe, ye, ze = xla, yla * cth - zla * sth, yla * sth + zla * cth
            w = -ze
            if not w >= 0.04:
                continue
            u, v = (xe / w / tx + 1) * W / 2, (1 - ye / w / ty) * H / 2
            if cal is None:
                pc, pr = u, v
            else:
                if not (0 <= u < W and 0 <= v < H):
                    continue
                a, b = u - 0.5, v - 0.5
                _x, _y, _w = ir[0][0] * a + ir[0][1] * b + ir[0][2], ir[1][0] * a + ir[1][1] * b + ir[1][2], ir[2][0] * a + ir[2][1] * b + ir[2][2]
                nx, ny = _x / _w, _y / _w
                r2 = nx * nx + ny * ny
                kr = 1 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
                xd = nx * kr + 2 * p1 * nx * ny + p2 * (r2 + 2 * nx * nx)
                yd = ny * kr + p1 * (r2 + 2 * ny * ny) + 2 * p2 * nx * ny
                pc, pr = fx * xd + u0 + 0.5, fy * yd + v0 + 0.5
            if 0 <= pc < W and 0 <= pr < H:
                out[i, j] = math.floor(pr) * W + math.floor(pc)
    return out
