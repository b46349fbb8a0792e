"""`-m gpu`: dtsim_ipm (k_ipm_table + k_ipm_gather, k_ipm_env) against the model of tests/ipm_model.py -- the ground-projected camera image,
its validity flags and its source-pixel indices for N = 130 envs (two full chunks of 64 and a tail of 2) with a 160 x 120 camera, and one
case at 640 x 480 with N = 3.  `src` is EQUAL to the model's on the model's sure cells and a member of the cell's candidate set elsewhere:
no capped share, one wrong pixel anywhere fails.  `valid` is src >= 0.  The image is held to `src` exactly: on frames bound to a tensor
whose pixels encode (env, row, column) uniquely, and on really rendered frames.

Measured on an MI355X: profiles/ipm_parity.txt."""
import ctypes as C
import itertools

import numpy as np
import pytest

import ipm_model as im
from dtsim import BatchedSimulator, _ffi
from dtsim import distortion as pdist

pytestmark = pytest.mark.gpu
N, W, H = 130, 160, 120
SENTINEL = 201
KINDS = {
    "shared_rect": dict(distortion=False, domain_rand=False),
    "shared_fish": dict(distortion=True, domain_rand=False),
    "dr_rect": dict(distortion=False, domain_rand=True),
    "dr_fish": dict(distortion=True, domain_rand=True),
    "camera_rand": dict(distortion=True, domain_rand=False, camera_rand=True, camera_rand_pool=5),
    "big_fish": dict(distortion=True, domain_rand=False, camera_width=640, camera_height=480, num_envs=3),
}
# every shape on the four kinds of k_ipm_gather and k_ipm_env; two on the others (640 x 480: the 64 x 64 map and the one no multiple of 4)
SHAPES_OF = {k: im.SHAPES for k in ("shared_rect", "shared_fish", "dr_rect", "dr_fish")}
SHAPES_OF.update(camera_rand=(im.SHAPES[1], im.SHAPES[3]), big_fish=im.SHAPES[:2])


def pose_of(e):
    return im.POSES[(e % 64) % len(im.POSES)]


def make_sim(kind):
    kw = dict(camera_width=W, camera_height=H, num_envs=N, seed=3, max_steps=10 ** 6)
    kw.update(KINDS[kind])
    n = kw.pop("num_envs")
    sim = BatchedSimulator("small_loop", n, **kw)
    pos, ang, cam = sim.read(_ffi.FIELD_POS), sim.read(_ffi.FIELD_ANGLE), sim.read(_ffi.FIELD_CAMERA)
    for e in range(n):
        x, z, a = pose_of(e)
        pos[e], ang[e] = (x, 0.0, z), a
    if kind.startswith("dr"):
        cam[64:128] = cam[0:64]                              # envs e, e + 64 and e + 128 are one state
        cam[128:] = cam[0:n - 128]
    sim.write(_ffi.FIELD_POS, pos)
    sim.write(_ffi.FIELD_ANGLE, ang)
    sim.write(_ffi.FIELD_CAMERA, cam)
    return sim


def encoded_frames(n, w, h):
    """[n, h, w, 3] uint8 on the device: the three bytes of pixel (e, r, c) spell e * h * w + r * w + c + 1, little-endian (0: no pixel)."""
    import torch
    assert n * w * h + 1 < 1 << 24
    code = torch.arange(1, n * w * h + 1, dtype=torch.int32, device="cuda").view(n, h, w)
    fr = torch.stack([(code >> s) & 255 for s in (0, 8, 16)], dim=-1).to(torch.uint8).contiguous()
    torch.cuda.synchronize()
    return fr


def decode(img, chw):
    a = img.astype(np.int64)
    return a[:, 0] + (a[:, 1] << 8) + (a[:, 2] << 16) if chw else a[..., 0] + (a[..., 1] << 8) + (a[..., 2] << 16)


class Rig:
    def __init__(self, kind):
        self.kind, self.sim = kind, make_sim(kind)
        sim = self.sim
        self.n, self.w, self.h = sim.num_envs, sim.camera_width, sim.camera_height
        self.code = encoded_frames(self.n, self.w, self.h)
        sim.bind_frames(self.code.data_ptr())
        self.per_env = kind.startswith("dr") or kind == "camera_rand"
        self.cam = sim.read(_ffi.FIELD_CAMERA)
        assert self.cam.dtype == np.float32 and self.cam.shape == (self.n, 6)
        self.cals = None
        if KINDS[kind]["distortion"]:
            cc = sim.camera_calibrations
            if cc is None:
                self.cals, self.env_cal = [im.nominal_cal()], np.zeros(self.n, np.int32)
            else:
                self.cals, self.env_cal = [im.Cal(cc[0][i], cc[1][i], cc[2][i]) for i in range(len(cc[0]))], cc[3]
        self._models = {}

    def model(self, e, shape):
        cam = im.EnvCamera(*self.cam[e, :3], tuple(self.cam[e, 3:])) if self.per_env else None
        ci = None if self.cals is None else int(self.env_cal[e])
        key = (shape, (e % 64) % len(im.POSES) if cam is None else e, ci)
        if key not in self._models:
            self._models[key] = im.expected(pose_of(e), shape, self.w, self.h, cam, None if ci is None else self.cals[ci])
        return self._models[key]

    def run(self, shape, chw=True, img=True, valid=True, index=True, mask=None, fill=None):
        """One call with outputs of its own; returns (img, valid, src) as numpy (None where not asked for)."""
        import torch
        oh, ow, cell, rb = shape
        mk = lambda shp, dt: torch.full(shp, SENTINEL if fill is None else fill, dtype=dt, device="cuda")
        o = mk((self.n, 3, oh, ow) if chw else (self.n, oh, ow, 3), torch.uint8)
        v = mk((self.n, oh, ow), torch.uint8) if valid else None
        s = mk((self.n, oh, ow), torch.int32) if index else None
        torch.cuda.synchronize()
        if img:
            self.sim.ipm(oh, ow, cell, rb, chw=chw, out=o, mask=mask, valid_out=v, index_out=s)
        else:                                                # (the method always fills an image: the other subsets through the library)
            flags = _ffi.IPM_CHW if chw else 0
            mp = None if mask is None else C.c_void_p(mask.data_ptr())
            ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
            _ffi.check(self.sim._lib, self.sim._lib.dtsim_ipm(self.sim._h, None, ptr(v), ptr(s), oh, ow, cell, rb, flags, mp))
        self.sim.sync()
        return tuple(None if t is None else t.cpu().numpy() for t in (o if img else None, v, s))


_RIGS = {}


@pytest.fixture(scope="module")
def rigs():
    def get(kind):
        if kind not in _RIGS:
            _RIGS[kind] = Rig(kind)
        return _RIGS[kind]
    yield get
    for r in _RIGS.values():
        r.sim.close()
    _RIGS.clear()


CASES = [(k, s) for k in KINDS for s in SHAPES_OF[k]]


@pytest.mark.parametrize("kind,shape", CASES, ids=[f"{k}-{s[0]}x{s[1]}" for k, s in CASES])
def test_src_valid_and_image_against_the_model(rigs, kind, shape):
    """src: equal to the model on sure cells, a member of the candidate set elsewhere, for every env; valid = (src >= 0); the image of
    encoded frames decodes to (env, src) exactly, CHW and HWC, and is zero where the cell is invalid."""
    rig = rigs(kind)
    img, valid, src = rig.run(shape)
    other = unsure = n_valid = 0
    for e in range(rig.n):
        exp = rig.model(e, shape)
        other += im.hold(exp, src[e])
        unsure += int((~exp.sure).sum())
        n_valid += int(exp.valid.sum())
    print(f"ipm parity {kind} {shape}: {src.size} cells, {n_valid / src.size:.4f} valid, {1 - unsure / src.size:.6f} sure, {other} took another member")
    assert np.array_equal(valid, (src >= 0).astype(np.uint8))
    if kind == "camera_rand":                                # each env is held to its OWN calibration: the pool's differ where it matters
        assert len(rig.cals) == 5 and len({rig.model(e, shape).src.tobytes() for e in range(5)}) == 5
    hw = rig.w * rig.h
    want = np.where(src >= 0, np.arange(rig.n, dtype=np.int64)[:, None, None] * hw + src + 1, 0)
    assert np.array_equal(decode(img, True), want)
    img_hwc, _, src2 = rig.run(shape, chw=False)
    assert np.array_equal(src2, src) and np.array_equal(decode(img_hwc, False), want)


@pytest.mark.parametrize("kind", ["shared_rect", "shared_fish", "dr_fish", "camera_rand"])
def test_image_of_rendered_frames_is_the_frame_at_src(rigs, kind):
    """On really rendered frames in the handle's own buffer: img[e, :, i, j] == frames[e].reshape(-1, 3)[src[e, i, j]], zero where invalid."""
    rig = rigs(kind)
    sim = rig.sim
    try:
        sim.bind_frames(None)
        sim.render()
        frames = sim.frames_host().reshape(rig.n, -1, 3)
        assert frames.std() > 10                             # a scene, not a blank batch
        for shape, chw in ((im.SHAPES[0], True), (im.SHAPES[1], False)):
            img, valid, src = rig.run(shape, chw=chw)
            px = img.transpose(0, 2, 3, 1) if chw else img
            want = np.where((src >= 0)[..., None], frames[np.arange(rig.n)[:, None, None], np.maximum(src, 0)], 0)
            assert np.array_equal(px, want)
            assert valid.any() and not valid.all()
    finally:
        sim.bind_frames(rig.code.data_ptr())


@pytest.mark.parametrize("kind", ["shared_fish", "dr_rect"])
def test_one_state_gives_the_same_bytes(rigs, kind):
    """Envs e, e + 64 and e + 128 of one state; a second call; every subset of the three outputs; a call after a masked render: all
    byte-identical (the image against its own env's code)."""
    import torch
    rig = rigs(kind)
    sim = rig.sim
    for shape in (im.SHAPES[1], im.SHAPES[3]):
        img, valid, src = rig.run(shape)
        for e in range(rig.n - 64):
            assert src[e].tobytes() == src[e + 64].tobytes() and valid[e].tobytes() == valid[e + 64].tobytes(), e
        again = rig.run(shape)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (img, valid, src)))
        for use in itertools.product((False, True), repeat=3):
            if not any(use):
                continue
            got = rig.run(shape, img=use[0], valid=use[1], index=use[2])
            for g, full in zip(got, (img, valid, src)):
                assert g is None or g.tobytes() == full.tobytes(), use
        mask = torch.zeros(rig.n, dtype=torch.uint8, device="cuda")
        mask[::3] = 1
        torch.cuda.synchronize()
        sim.bind_frames(None)
        sim.render(mask=mask)
        sim.bind_frames(rig.code.data_ptr())
        after = rig.run(shape)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(after, (img, valid, src)))


@pytest.mark.parametrize("kind", ["shared_rect", "dr_fish"])
def test_masked_call_leaves_unselected_rows(rigs, kind):
    import torch
    rig = rigs(kind)
    mask = torch.zeros(rig.n, dtype=torch.bool, device="cuda")
    mask[[0, 5, 63, 64, 129]] = True
    torch.cuda.synchronize()
    sel = mask.cpu().numpy()
    for shape, chw in ((im.SHAPES[0], True), (im.SHAPES[1], False)):
        full = rig.run(shape, chw=chw)
        got = rig.run(shape, chw=chw, mask=mask)
        for g, f in zip(got, full):
            assert np.array_equal(g[sel], f[sel])
            assert (g[~sel] == SENTINEL).all()


def test_user_calibration_changes_src_and_the_cached_table_is_rebuilt():
    """The shared camera's table is cached on its key: a new shape, cell, rows_behind or calibration rebuilds it, and going back gives the
    first bytes again.  A user calibration through set_camera_calibrations is held to the model with that calibration."""
    sim = BatchedSimulator("small_loop", 4, camera_width=W, camera_height=H, distortion=True, domain_rand=False, seed=3, max_steps=10 ** 6)
    try:
        import torch
        pose = (1.0, 0.9, 0.3)
        pos, ang = sim.read(_ffi.FIELD_POS), sim.read(_ffi.FIELD_ANGLE)
        pos[:], ang[:] = (pose[0], 0.0, pose[1]), pose[2]
        sim.write(_ffi.FIELD_POS, pos)
        sim.write(_ffi.FIELD_ANGLE, ang)

        def src_of(shape):
            s = torch.full((4, shape[0], shape[1]), -7, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            sim.ipm(*shape, index_out=s)
            sim.sync()
            return s.cpu().numpy()

        a, b = im.SHAPES[0], (64, 64, 0.021, 0)
        first = src_of(a)
        im.hold(im.expected(pose, a, W, H, None, im.nominal_cal()), first[0])
        other = src_of(b)                                    # same sizes, another cell: the table must not be reused
        im.hold(im.expected(pose, b, W, H, None, im.nominal_cal()), other[3])
        assert other.tobytes() != first.tobytes()
        im.hold(im.expected(pose, (64, 64, 0.02, 5), W, H, None, im.nominal_cal()), src_of((64, 64, 0.02, 5))[1])
        assert src_of(a).tobytes() == first.tobytes()
        Ks, Ds = pdist.sample_calibrations(1, 11)
        sim.set_camera_calibrations(Ks, Ds, np.zeros(4, np.int32))
        user = src_of(a)
        im.hold(im.expected(pose, a, W, H, None, im.make_cal(Ks[0], Ds[0])), user[2])
        assert (user != first).mean() > 0.05                 # a 5 % change of the calibration moves the source pixels
        # a failed setter leaves the calibrations in force
        dp = C.POINTER(C.c_double)
        K = np.ascontiguousarray(Ks, np.float64)
        D = np.ascontiguousarray(Ds, np.float64)
        nk = np.ascontiguousarray(im.make_cal(Ks[0], Ds[0]).new_K[None], np.float64)
        bad_nk = np.zeros((1, 3, 3))
        bad_env = np.array([0, 0, 1, 0], np.int32)
        p = lambda x: x.ctypes.data_as(dp)
        lib, h = sim._lib, sim._h
        for args in ((1, p(K), p(D), p(bad_nk), None), (1, p(K), None, p(nk), None), (-1, p(K), p(D), p(nk), None),
                     (0, p(K), None, None, None), (2, p(K), p(D), p(nk), None),
                     (1, p(K), p(D), p(nk), bad_env.ctypes.data_as(C.POINTER(C.c_int32)))):
            assert lib.dtsim_set_ipm_calibrations(h, *args) == _ffi.E_INVALID, args[0]
            assert src_of(a).tobytes() == user.tobytes()
        Dn = D.copy()
        Dn[0, 1] = np.nan
        assert lib.dtsim_set_ipm_calibrations(h, 1, p(K), p(Dn), p(nk), None) == _ffi.E_INVALID
        assert src_of(a).tobytes() == user.tobytes()
        # uninstalled: the rectilinear projection
        assert lib.dtsim_set_ipm_calibrations(h, 0, None, None, None, None) == 0
        im.hold(im.expected(pose, a, W, H, None, None), src_of(a)[0])
    finally:
        sim.close()


def test_bad_arguments_are_refused_and_leave_the_last_result(rigs):
    import torch
    rig = rigs("shared_rect")
    sim = rig.sim
    oh, ow, cell, rb = im.SHAPES[0]
    out = torch.full((N, 3, oh, ow), SENTINEL, dtype=torch.uint8, device="cuda")
    val = torch.full((N, oh, ow), SENTINEL, dtype=torch.uint8, device="cuda")
    idx = torch.full((N, oh, ow), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    sim.ipm(oh, ow, cell, rb, out=out, valid_out=val, index_out=idx)
    sim.sync()
    keep = [t.clone() for t in (out, val, idx)]
    torch.cuda.synchronize()
    bad_mask = torch.ones(N + 1, dtype=torch.uint8, device="cuda")
    for kw in (dict(height=0), dict(height=1025), dict(width=0), dict(width=1025), dict(width=64.5), dict(cell=0.0), dict(cell=-0.02),
               dict(cell=float("nan")), dict(cell=float("inf")), dict(rows_behind=-1), dict(rows_behind=oh + 1), dict(rows_behind=1.5),
               dict(mask=bad_mask), dict(mask=np.ones(N, np.uint8)), dict(valid_out=idx), dict(index_out=val), dict(out=val),
               dict(valid_out=val[:, :, :32]), dict(chw=False)):
        args = dict(height=oh, width=ow, cell=cell, rows_behind=rb, out=out, valid_out=val, index_out=idx)
        args.update(kw)
        with pytest.raises(ValueError):
            sim.ipm(**args)
    with pytest.raises(ValueError):
        sim.ipm(oh, ow, cell, rb, out=out, valid_out=out.view(torch.uint8)[:, 0], index_out=idx)
    lib, h = sim._lib, sim._h
    po, pv, pi = (C.c_void_p(t.data_ptr()) for t in (out, val, idx))
    for args in ((None, None, None, oh, ow, cell, rb, 1, None), (po, po, pi, oh, ow, cell, rb, 1, None), (po, pv, pv, oh, ow, cell, rb, 1, None),
                 (po, pv, po, oh, ow, cell, rb, 1, None), (po, pv, pi, oh, ow, cell, rb, 2, None), (po, pv, pi, oh, ow, cell, rb, 0x80000001, None),
                 (po, pv, pi, 0, ow, cell, rb, 1, None), (po, pv, pi, oh, 1025, cell, rb, 1, None), (po, pv, pi, oh, ow, 0.0, rb, 1, None),
                 (po, pv, pi, oh, ow, float("nan"), rb, 1, None), (po, pv, pi, oh, ow, float("inf"), rb, 1, None),
                 (po, pv, pi, oh, ow, cell, -1, 1, None), (po, pv, pi, oh, ow, cell, oh + 1, 1, None)):
        assert lib.dtsim_ipm(h, *args) == _ffi.E_INVALID, args[3:8]
    assert lib.dtsim_ipm(None, po, pv, pi, oh, ow, cell, rb, 1, None) == _ffi.E_INVALID
    sim.sync()
    torch.cuda.synchronize()
    for t, k in zip((out, val, idx), keep):
        assert torch.equal(t, k)


def test_state_errors():
    """DTSIM_E_STATE before the first reset; ValueError for render=False and undistort=True before the library is called."""
    sim = BatchedSimulator("small_loop", 2, camera_width=W, camera_height=H, distortion=False, domain_rand=False, seed=3, do_reset=False)
    try:
        import torch
        out = torch.zeros((2, 3, 8, 8), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert sim._lib.dtsim_ipm(sim._h, C.c_void_p(out.data_ptr()), None, None, 8, 8, 0.02, 0, 1, None) == _ffi.E_STATE
        sim.reset()
        sim.ipm(8, 8, out=out)
        sim.sync()
    finally:
        sim.close()
    sim = BatchedSimulator("small_loop", 2, render=False, domain_rand=False, seed=3)
    try:
        with pytest.raises(ValueError, match="render"):
            sim.ipm(8, 8)
        assert sim._lib.dtsim_ipm(sim._h, C.c_void_p(64), None, None, 8, 8, 0.02, 0, 1, None) == _ffi.E_STATE
        assert sim._lib.dtsim_set_ipm_calibrations(sim._h, 0, None, None, None, None) == _ffi.E_STATE
    finally:
        sim.close()
    sim = BatchedSimulator("small_loop", 2, camera_width=W, camera_height=H, distortion=True, undistort=True, domain_rand=False, seed=3)
    try:
        with pytest.raises(ValueError, match="undistort"):
            sim.ipm(8, 8)
    finally:
        sim.close()
