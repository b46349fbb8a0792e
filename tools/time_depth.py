"""Time of the depth pass alone (dtsim_depth: k_depth) on one rendered batch: device events around REPS back-to-back calls on the handle's
stream, after a warm-up, per output size and dtype; bytes written / time.  N=4096 MAP=small_loop W=640 H=480 FISHEYE=1 by default;
MAP=loop_pedestrians for the triangle loop (STEPS zero-action steps first, so that the duckies have walked)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-duckietown_amd"))
import numpy as np
import torch
from dtsim import BatchedSimulator
from timing import alternating_rounds, median_spread

N = int(os.environ.get("N", "4096"))
MAP = os.environ.get("MAP", "small_loop")
W, H = int(os.environ.get("W", "640")), int(os.environ.get("H", "480"))
FISHEYE = os.environ.get("FISHEYE", "1") == "1"
DR = os.environ.get("DOMAIN_RAND", "0") == "1"
REPS = int(os.environ.get("REPS", "20"))
STEPS = int(os.environ.get("STEPS", "0"))

stream = torch.cuda.Stream()
sim = BatchedSimulator(MAP, N, camera_width=W, camera_height=H, distortion=FISHEYE, domain_rand=DR, seed=0, device_reset=True,
                       stream=stream.cuda_stream, max_steps=10 ** 6)
if STEPS:
    sim.step(np.zeros((STEPS, N, 2), np.float32), n_steps=STEPS)
sim.render()
print(f"depth pass alone: {MAP} N={N} {W} x {H}{' fisheye' if FISHEYE else ''}{' domain_rand' if DR else ''}, raster {sim.render_pipeline}, {REPS} calls per figure")
for (h, w) in ((H // 4, W // 4), (H, W)):
    for dtype, item in (("float32", 4), ("float16", 2)):
        out = torch.empty((N, h, w), dtype=getattr(torch, dtype), device="cuda")
        # (three rounds: the spread)
        m, lo, hi = median_spread(alternating_rounds(stream, {"depth": lambda: sim.depth(h, w, dtype=dtype, out=out)}, REPS, 3)["depth"])
        by = N * h * w * item
        print(f"  {h:3d} x {w:3d} {dtype}: {m:7.3f} ms per call (of three: {lo:.3f} .. {hi:.3f}), {by / 1e6:7.1f} MB written, {by / m / 1e9:6.3f} TB/s, "
              f"{N * h * w / m / 1e6:7.1f} G pixels/s")
sim.close()
