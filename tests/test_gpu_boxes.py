"""`-m gpu`: dtsim_boxes (k_boxes) -- one box and pixel count per id and env of an [N, h, w] uint8 id map -- against the numpy model
(instance_model.box_model, held to a plain loop by tests/test_instance_model_host.py), EXACTLY: integer minima, maxima and sums.

Synthetic maps at the places the kernel can go wrong: a 16-byte chunk that spans two or more rows (widths 1, 5, 17, 90: no multiple of 16,
three of them none of 4), env bases at every alignment (51- and 5-byte envs; views 1, 2 and 3 bytes into a larger buffer), fewer bytes than
lanes, one byte, an id only in the last byte, ids above 64, more than one workgroup (N = 3, 130).  Then the device's own instance maps of
the crowd and the walking duckies: exactly their numpy reduction, and consistent with the oracle's map id by id."""
import ctypes as C

import numpy as np
import pytest

import crowd_scenes as cs
import instance_model as im
from dtsim import BatchedSimulator, _ffi, assets

pytestmark = pytest.mark.gpu
SHAPES = ((1, 1), (1, 5), (3, 17), (5, 64), (62, 90), (120, 160))
NS = (1, 3, 130)
SENTINEL = -7


@pytest.fixture(autouse=True)
def crowd_map(monkeypatch):
    monkeypatch.setitem(assets.MAPS, "crowd", cs.crowd_map())


@pytest.fixture(scope="module")
def sims():
    """One small simulator per batch size (dtsim_boxes takes the batch size from the handle and nothing else)."""
    made = {}

    def get(n):
        if n not in made:
            made[n] = BatchedSimulator("small_loop", n, camera_width=64, camera_height=48, distortion=False, domain_rand=False, seed=1)
        return made[n]
    yield get
    for s in made.values():
        s.close()


def contents(n, h, w, rng):
    """name -> [n, h, w] uint8 maps."""
    out = {"zero": np.zeros((n, h, w), np.uint8), "one id": np.full((n, h, w), 37, np.uint8)}
    if h * w >= im.MAX_OBJECTS:                      # each id 1 .. 64 in exactly one pixel, (0, 0) and (h - 1, w - 1) among them; per env another placing
        m = np.zeros((n, h * w), np.uint8)
        for e in range(n):
            at = np.concatenate([[0, h * w - 1], 1 + rng.permutation(h * w - 2)[:im.MAX_OBJECTS - 2]])
            m[e, at] = rng.permutation(im.MAX_OBJECTS) + 1
        out["one pixel each"] = m.reshape(n, h, w)
    last = np.zeros((n, h, w), np.uint8)
    last[:, -1, -1] = 64                              # an id only in the last byte
    out["last byte"] = last
    for p in (0.02, 0.3, 1.0):                        # random bytes 0 .. 255 (three quarters of them above 64) at several densities
        out[f"random {p}"] = (rng.integers(0, 256, (n, h, w)) * (rng.random((n, h, w)) < p)).astype(np.uint8)
    out["runs"] = np.repeat(rng.integers(0, 9, (n, h, (w + 4) // 5)), 5, axis=2)[:, :, :w].astype(np.uint8)     # runs of five pixels, cut by the row ends
    return out


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("shape", SHAPES)
def test_boxes_match_the_numpy_model_exactly(shape, n, sims):
    import torch
    sim = sims(n)
    h, w = shape
    rng = np.random.default_rng(1000 * h + w + n)
    for name, m in contents(n, h, w, rng).items():
        assert m.shape == (n, h, w)
        want = im.box_model(m)
        t = torch.from_numpy(m).cuda()
        torch.cuda.synchronize()
        got = sim.boxes(t)
        sim.sync()
        assert got.shape == (n, im.MAX_OBJECTS, 5) and got.dtype == torch.int32
        a = got.cpu().numpy().copy()
        assert np.array_equal(a, want), (shape, n, name, np.argwhere(a != want)[:6].tolist())
        sim.boxes(t)
        sim.sync()
        assert got.cpu().numpy().tobytes() == a.tobytes()                         # a second call: the same bytes
    if h * w >= im.MAX_OBJECTS:
        one = im.box_model(contents(1, h, w, np.random.default_rng(0))["one pixel each"])[0]
        assert (one[:, 4] == 1).all() and ((one[:, 2] - one[:, 0]) * (one[:, 3] - one[:, 1]) == 1).all()


@pytest.mark.parametrize("shape", [(3, 17), (5, 64), (62, 90)])
def test_unaligned_bases_give_the_aligned_result(shape, sims):
    """inst as a view starting 1, 2 and 3 (and 13, 15) bytes into a larger buffer, out as a view 1, 2 and 3 ints into one: the aligned run's
    bytes, and not one int around `out` touched."""
    import torch
    n = 3
    sim = sims(n)
    h, w = shape
    rng = np.random.default_rng(7)
    m = (rng.integers(0, 80, (n, h, w)) * (rng.random((n, h, w)) < 0.4)).astype(np.uint8)
    m[:, -1, -1] = 64
    m[:, 0, 0] = 1
    want = im.box_model(m)
    t = torch.from_numpy(m).cuda()
    torch.cuda.synchronize()
    ref = sim.boxes(t)
    sim.sync()
    assert np.array_equal(ref.cpu().numpy(), want)
    size = n * h * w
    for off in (1, 2, 3, 13, 15):
        buf = torch.zeros(size + 32, dtype=torch.uint8, device="cuda")
        view = buf[off:off + size].view(n, h, w)
        view.copy_(torch.from_numpy(m))
        buf[:off] = 200; buf[off + size:] = 9                                     # ids around the map: never read as part of it
        obuf = torch.full((n * im.MAX_OBJECTS * 5 + 8,), SENTINEL, dtype=torch.int32, device="cuda")
        oo = off % 4 if off % 4 else 2
        out = obuf[oo:oo + n * im.MAX_OBJECTS * 5].view(n, im.MAX_OBJECTS, 5)
        torch.cuda.synchronize()
        assert view.data_ptr() % 16 == (buf.data_ptr() + off) % 16 and view.is_contiguous()
        assert sim.boxes(view, out=out) is out
        sim.sync()
        assert np.array_equal(out.cpu().numpy(), want), (shape, off)
        assert bool((obuf[:oo] == SENTINEL).all()) and bool((obuf[oo + n * im.MAX_OBJECTS * 5:] == SENTINEL).all())


def test_mask_keeps_the_other_rows_and_invalid_arguments_write_nothing(sims):
    import torch
    n = 130
    sim = sims(n)
    h, w = 62, 90
    rng = np.random.default_rng(3)
    m = (rng.integers(0, 70, (n, h, w)) * (rng.random((n, h, w)) < 0.5)).astype(np.uint8)
    want = im.box_model(m)
    t = torch.from_numpy(m).cuda()
    sel = torch.zeros(n, dtype=torch.uint8, device="cuda")
    pick = [0, 5, 63, 64, 129]
    sel[pick] = 1
    out = torch.full((n, im.MAX_OBJECTS, 5), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert sim.boxes(t, out=out, mask=sel) is out
    sim.sync()
    got = out.cpu().numpy()
    keep = np.ones(n, bool)
    keep[pick] = False
    assert (got[keep] == SENTINEL).all() and np.array_equal(got[pick], want[pick])
    # invalid arguments: DTSIM_E_INVALID, nothing launched, nothing written
    out.fill_(SENTINEL)
    torch.cuda.synchronize()
    lib, hd = sim._lib, sim._h
    ip, op, mp = C.c_void_p(t.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(sel.data_ptr())
    assert lib.dtsim_boxes(None, ip, h, w, op, 0, None) == _ffi.E_INVALID
    assert lib.dtsim_boxes(hd, None, h, w, op, 0, None) == _ffi.E_INVALID
    assert lib.dtsim_boxes(hd, ip, h, w, None, 0, mp) == _ffi.E_INVALID
    assert lib.dtsim_boxes(hd, ip, 0, w, op, 0, None) == _ffi.E_INVALID and lib.dtsim_boxes(hd, ip, h, -1, op, 0, mp) == _ffi.E_INVALID
    assert lib.dtsim_boxes(hd, ip, h, w, op, 1, None) == _ffi.E_INVALID
    assert lib.dtsim_boxes(hd, ip, 65536, 65536, op, 0, None) == _ffi.E_INVALID                  # the product does not fit an int32
    for bad in (dict(inst=t.float()), dict(inst=t[:3]), dict(inst=t[:, :, ::2]), dict(inst=t[0]), dict(inst=m), dict(inst=t, out=out[:4]),
                dict(inst=t, out=out.float()), dict(inst=t, mask=sel.cpu()), dict(inst=t, mask=sel[:5])):
        with pytest.raises(ValueError):
            sim.boxes(**bad)
    sim.sync()
    assert bool((out == SENTINEL).all())
    assert lib.dtsim_boxes(hd, ip, h, w, op, 0, None) == _ffi.OK                                 # (and the valid call, through the C-ABI)
    sim.sync()
    assert np.array_equal(out.cpu().numpy(), want)


@pytest.mark.parametrize("name,kind", [("crowd_far", None), ("crowd_far", "fisheye"), ("pedestrians", None), ("pedestrians", "undistort")])
def test_boxes_of_the_device_instance_maps(name, kind):
    """boxes(instances()) is exactly the numpy reduction of the device's own map, full size and 60 x 80; and against the oracle, for every id:
    the box contains the bounding box of the SURE pixels of that id, and n lies between their count and the count of the expected pixels of
    the id plus all unsure pixels."""
    c = im.CASES[name]
    sim = im.make_sim(name, kind=kind)
    sim.render()
    inst = sim.instances()
    boxes = sim.boxes(inst)
    sim.sync()
    m, b = inst.cpu().numpy(), boxes.cpu().numpy().copy()
    assert np.array_equal(b, im.box_model(m)), (name, kind)
    seen = 0
    for e in range(c.n_envs):
        want, sure = im.expected(name, e, kind)
        im.check_boxes_against_oracle(b[e], want, sure, (name, kind, e))
        seen += int((b[e][:, 4] > 0).sum())
        print(f"{name} {kind} env {e}: {int((b[e][:, 4] > 0).sum())} objects in view, largest {int(b[e][:, 4].max())} px")
    assert seen >= (40 if name == "crowd_far" else 6)
    small = sim.instances(60, 80)
    bs = sim.boxes(small)
    sim.sync()
    assert np.array_equal(bs.cpu().numpy(), im.box_model(small.cpu().numpy()))
    sim.close()
