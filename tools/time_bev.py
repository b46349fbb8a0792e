"""Time of the bird's-eye pass (dtsim_bev, k_bev) in ONE process, against two yardsticks that are not the code under test: a device-to-device
copy of the same output bytes, and dtsim_labels (k_labels) at 120 x 160 on the same handle.  Device events around REPS back-to-back calls on
the handle's stream, after a warm-up, the calls alternating over ROUNDS rounds per shape (128 x 128 at 0.02 m, 64 x 64 at 0.04 m); the median
round and the spread (min .. max) of each.  The expectation to confirm or refute: without objects the pass costs about as much as the copy
and well below k_labels; with objects its cost follows the rectangles that survive the window cull (counted here on the host from
object_footprints(), by the kernel's own rule: the bounding circle plus one cell meets the window).
N=4096 W=160 H=120 by default; MAPS=small_loop,loop_pedestrians,crowd (crowd: the 64-object map of tests/crowd_scenes.py); STEPS zero-action
steps first on the maps with walkers, so that the duckies have walked."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gym-duckietown_amd"), os.path.join(ROOT, "tests"), ROOT]
import numpy as np
import torch
from dtsim import BatchedSimulator, _ffi, assets
from timing import alternating_rounds, median_spread

N = int(os.environ.get("N", "4096"))
MAPS = os.environ.get("MAPS", "small_loop,loop_pedestrians,crowd").split(",")
W, H = int(os.environ.get("W", "160")), int(os.environ.get("H", "120"))
REPS = int(os.environ.get("REPS", "20"))
ROUNDS = int(os.environ.get("ROUNDS", "5"))
STEPS = int(os.environ.get("STEPS", "40"))
SHAPES = ((128, 128, 0.02, 0), (64, 64, 0.04, 0))


def survivors(sim, oh, ow, cell, rb):
    """Mean number of rectangles per env that k_bev's cull keeps."""
    corners, drawn = sim.object_footprints()
    pos, th = sim.read(_ffi.FIELD_POS), sim.read(_ffi.FIELD_ANGLE)
    d = corners - pos[:, [0, 2]][:, None, None, :]
    c, s = np.cos(th)[:, None, None], np.sin(th)[:, None, None]
    f, r = (d[..., 0] * c - d[..., 1] * s) / cell, (d[..., 0] * s + d[..., 1] * c) / cell          # [N, K, 4]
    uf, us, vf, vs = (f[..., 1] - f[..., 0]) / 2, (r[..., 1] - r[..., 0]) / 2, (f[..., 3] - f[..., 0]) / 2, (r[..., 3] - r[..., 0]) / 2
    cf, cs = f[..., 0] + uf + vf, r[..., 0] + us + vs
    rad = np.sqrt(np.maximum((uf + vf) ** 2 + (us + vs) ** 2, (uf - vf) ** 2 + (us - vs) ** 2)) + 1
    df = np.maximum(np.maximum(-rb - cf, cf - (oh - rb)), 0)
    ds = np.maximum(np.abs(cs) - ow / 2, 0)
    keep = drawn & (df * df + ds * ds <= rad * rad)
    return float(keep.sum(1).mean()), float(drawn.sum(1).mean())


for MAP in MAPS:
    if MAP == "crowd":
        import crowd_scenes as cs
        assets.MAPS["crowd"] = cs.crowd_map()
    stream = torch.cuda.Stream()
    sim = BatchedSimulator(MAP, N, camera_width=W, camera_height=H, distortion=False, domain_rand=False, seed=0, device_reset=True,
                           stream=stream.cuda_stream, max_steps=10 ** 6)
    if STEPS and any(not o.static for o in sim.maps[0].objects):
        sim.step(np.zeros((STEPS, N, 2), np.float32), n_steps=STEPS)
    sim.render()
    lab = torch.empty((N, 120, 160), dtype=torch.uint8, device="cuda")
    sim.labels(120, 160, out=lab)                               # (installs the default tables outside the timed calls)
    print(f"bird's-eye pass: {MAP} N={N}, {len(sim.maps[0].objects)} objects in the map, {ROUNDS} alternating rounds of {REPS} calls per figure")
    for (oh, ow, cell, rb) in SHAPES:
        out = torch.empty((N, oh, ow), dtype=torch.uint8, device="cuda")
        ids = torch.empty_like(out)
        copy = torch.empty_like(out)
        calls = {"bev (classes)": lambda: sim.bev(oh, ow, cell=cell, rows_behind=rb, out=out),
                 "bev (classes + ids)": lambda: sim.bev(oh, ow, cell=cell, rows_behind=rb, out=out, instances_out=ids),
                 "copy of the map (d2d)": lambda: copy.copy_(out),
                 "labels 120 x 160": lambda: sim.labels(120, 160, out=lab)}
        ms = alternating_rounds(stream, calls, REPS, ROUNDS)
        med = {k: median_spread(v)[0] for k, v in ms.items()}
        kept, drawn = survivors(sim, oh, ow, cell, rb)
        for k, v in ms.items():
            print(f"  {oh:3d} x {ow:3d} at {cell:.2f} m  {k:22s}: median {med[k]:7.3f} ms per call (of {ROUNDS}: {min(v):.3f} .. {max(v):.3f})")
        print(f"  {oh:3d} x {ow:3d} at {cell:.2f} m  map {N * oh * ow / 1e6:.1f} MB; rectangles per env after the cull: mean {kept:.2f} of {drawn:.2f} drawn; "
              f"bev / copy = {med['bev (classes)'] / med['copy of the map (d2d)']:.2f}, bev / labels = {med['bev (classes)'] / med['labels 120 x 160']:.2f}, "
              f"ids beside the classes: + {med['bev (classes + ids)'] - med['bev (classes)']:.3f} ms")
    sim.close()
