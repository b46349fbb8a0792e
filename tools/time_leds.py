"""Time of the LED post-pass alone (dtsim_draw_leds: one k_overlay_leds launch per env that has spheres) on one rendered batch: device events
around REPS back-to-back calls on the handle's stream, after a warm-up; each call uploads the sphere list and draws SPHERES spheres into every
env's frame, so the figure is per call of N launches.  N=64 MAP=small_loop W=640 H=480 FISHEYE=1 by default; MAP=loop_pedestrians for the
triangle loop under the spheres (STEPS zero-action steps first, so that the duckies have walked).  The spheres stand 0.15 .. 0.6 m in front of
each robot, 1 .. 4 cm in radius: over the road, and on loop_pedestrians over whatever duckie stands there."""
import math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-duckietown_amd"))
import numpy as np
import torch
from dtsim import BatchedSimulator, _ffi
from timing import alternating_rounds, median_spread

N = int(os.environ.get("N", "64"))
MAP = os.environ.get("MAP", "small_loop")
W, H = int(os.environ.get("W", "640")), int(os.environ.get("H", "480"))
FISHEYE = os.environ.get("FISHEYE", "1") == "1"
REPS = int(os.environ.get("REPS", "10"))
STEPS = int(os.environ.get("STEPS", "0"))
SPHERES = int(os.environ.get("SPHERES", "10"))

stream = torch.cuda.Stream()
sim = BatchedSimulator(MAP, N, camera_width=W, camera_height=H, distortion=FISHEYE, domain_rand=False, seed=0, device_reset=True,
                       stream=stream.cuda_stream, max_steps=10 ** 6)
if STEPS:
    sim.step(np.zeros((STEPS, N, 2), np.float32), n_steps=STEPS)
sim.render()
pos, ang = sim.read(_ffi.FIELD_POS), sim.read(_ffi.FIELD_ANGLE)
rng = np.random.default_rng(7)
rows = []
for e in range(N):
    d = np.array([math.cos(ang[e]), 0.0, -math.sin(ang[e])])
    r = np.array([math.sin(ang[e]), 0.0, math.cos(ang[e])])
    for _ in range(SPHERES):
        c = pos[e] + d * rng.uniform(0.15, 0.6) + r * rng.uniform(-0.15, 0.15) + np.array([0.0, rng.uniform(0.02, 0.1), 0.0])
        rows.append([*c, rng.uniform(0.01, 0.04), *rng.uniform(0.2, 1.0, 3), 0.2])
spheres, idx = np.asarray(rows, np.float32), np.repeat(np.arange(N), SPHERES)
print(f"LED pass alone: {MAP} N={N} {W} x {H}{' fisheye' if FISHEYE else ''}, raster {sim.render_pipeline}, {SPHERES} spheres per env, {REPS} calls per figure")
m, lo, hi = median_spread(alternating_rounds(stream, {"leds": lambda: sim.draw_leds(spheres, idx)}, REPS, 5)["leds"])
print(f"  {H:3d} x {W:3d} k_overlay_leds x {N}: median {m:7.3f} ms per call (of 5: {lo:.3f} .. {hi:.3f}), {m / N * 1e3:7.1f} us per env")
sim.close()
