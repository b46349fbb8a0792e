"""Time of the label pass alone (dtsim_labels: k_labels) against the depth pass (dtsim_depth: k_depth, float32) on one rendered batch, in
ONE process: device events around REPS back-to-back calls on the handle's stream, after a warm-up, the two kernels alternating over ROUNDS
rounds per output size; the median round and the spread (min .. max) of each.  N=4096 MAP=small_loop W=640 H=480 FISHEYE=1 by default;
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
ROUNDS = int(os.environ.get("ROUNDS", "5"))
STEPS = int(os.environ.get("STEPS", "0"))

stream = torch.cuda.Stream()
sim = BatchedSimulator(MAP, N, camera_width=W, camera_height=H, distortion=FISHEYE, domain_rand=DR, seed=0, device_reset=True,
                       stream=stream.cuda_stream, max_steps=10 ** 6)
if STEPS:
    sim.step(np.zeros((STEPS, N, 2), np.float32), n_steps=STEPS)
sim.render()
print(f"label pass against depth pass: {MAP} N={N} {W} x {H}{' fisheye' if FISHEYE else ''}{' domain_rand' if DR else ''}, raster {sim.render_pipeline}, "
      f"{ROUNDS} alternating rounds of {REPS} calls per figure")
for (h, w) in ((H // 4, W // 4), (H, W)):
    lab = torch.empty((N, h, w), dtype=torch.uint8, device="cuda")
    dep = torch.empty((N, h, w), dtype=torch.float32, device="cuda")
    calls = {"k_labels uint8": lambda: sim.labels(h, w, out=lab), "k_depth float32": lambda: sim.depth(h, w, out=dep)}
    ms = alternating_rounds(stream, calls, REPS, ROUNDS)
    med = {k: median_spread(v)[0] for k, v in ms.items()}
    for k, v in ms.items():
        by = N * h * w * (1 if "labels" in k else 4)
        print(f"  {h:3d} x {w:3d} {k:16s}: median {med[k]:7.3f} ms per call (of {ROUNDS}: {min(v):.3f} .. {max(v):.3f}), {by / 1e6:7.1f} MB written, "
              f"{N * h * w / med[k] / 1e6:7.1f} G pixels/s")
    print(f"  {h:3d} x {w:3d} k_labels / k_depth = {med['k_labels uint8'] / med['k_depth float32']:.3f}")
ids, cnt = torch.unique(lab, return_counts=True)
print("  classes of the full map: " + " ".join(f"{int(i)}:{int(c)}" for i, c in zip(ids.cpu(), cnt.cpu())))
sim.close()
