"""Time of the fused camera-map launch WITHOUT flow (dtsim_camera_maps with depth, labels and instances: k_camera_maps<false, CAL>) on one
rendered batch, under the single fisheye table (CAL = false) and under camera_rand's per-env tables (CAMERA_RAND=1: CAL = true).
tools/time_camera_maps.py times the launch with flow.  Device events around REPS back-to-back calls on
the handle's stream, after a warm-up, over ROUNDS rounds; the median round and the spread (min .. max).
N=4096 MAP=small_loop W=640 H=480, maps at H / 4 x W / 4; MAP=loop_pedestrians for the triangle loop (STEPS zero-action steps first)."""
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
CAMERA_RAND = os.environ.get("CAMERA_RAND", "0") == "1"
REPS = int(os.environ.get("REPS", "20"))
ROUNDS = int(os.environ.get("ROUNDS", "5"))
STEPS = int(os.environ.get("STEPS", "8"))

stream = torch.cuda.Stream()
sim = BatchedSimulator(MAP, N, camera_width=W, camera_height=H, distortion=True, camera_rand=CAMERA_RAND, domain_rand=False, seed=0,
                       device_reset=True, stream=stream.cuda_stream, max_steps=10 ** 6)
if STEPS:
    sim.step(np.zeros((STEPS, N, 2), np.float32), n_steps=STEPS)
sim.render()
h, w = H // 4, W // 4
f = dict(depth=torch.empty((N, h, w), dtype=torch.float32, device="cuda"), labels=torch.empty((N, h, w), dtype=torch.uint8, device="cuda"),
         instances=torch.empty((N, h, w), dtype=torch.uint8, device="cuda"))
name = f"k_camera_maps, depth + labels + instances{', per-env tables' if CAMERA_RAND else ''}"
print(f"fused camera maps without flow: {MAP} N={N} {W} x {H} fisheye{' camera_rand' if CAMERA_RAND else ''} -> {h} x {w}, {ROUNDS} rounds of {REPS} calls")
ms = alternating_rounds(stream, {name: lambda: sim.camera_maps(h, w, **f)}, REPS, ROUNDS)
for k, v in ms.items():
    med, lo, hi = median_spread(v)
    print(f"  {k:60s}: median {med:7.3f} ms per call (of {ROUNDS}: {lo:.3f} .. {hi:.3f})")
sim.close()
