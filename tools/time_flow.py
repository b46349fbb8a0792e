"""Time of the flow pass alone (dtsim_flow: k_flow_setup + k_flow) against the instance pass (dtsim_instances without labels:
k_labels<false, true>, the same four classifications per pixel) on one rendered batch with one mark, in ONE process: device events around
REPS back-to-back calls on the handle's stream, after a warm-up, the two alternating over ROUNDS rounds per output size; the median round
and the spread (min .. max) of each.  N=4096 MAP=small_loop W=640 H=480 FISHEYE=1 by default; MAP=loop_pedestrians for the triangle loop
and the per-object pairs (STEPS zero-action steps before the mark and MOVE driven ones after it -- the robot starts at rest and its first updates move
nothing --, so that the duckies have walked and the picture moved)."""
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
STEPS = int(os.environ.get("STEPS", "8"))
MOVE = int(os.environ.get("MOVE", "8"))

stream = torch.cuda.Stream()
sim = BatchedSimulator(MAP, N, camera_width=W, camera_height=H, distortion=FISHEYE, domain_rand=DR, seed=0, device_reset=True,
                       stream=stream.cuda_stream, max_steps=10 ** 6)
if STEPS:
    sim.step(np.zeros((STEPS, N, 2), np.float32), n_steps=STEPS)
sim.flow_mark()
act = np.tile(np.array([0.4, 0.2], np.float32), (MOVE, N, 1))
sim.step(act, n_steps=MOVE)
sim.render()
print(f"flow pass against instance pass: {MAP} N={N} {W} x {H}{' fisheye' if FISHEYE else ''}{' domain_rand' if DR else ''}, raster {sim.render_pipeline}, "
      f"{ROUNDS} alternating rounds of {REPS} calls per figure")
for (h, w) in ((H // 4, W // 4), (H, W)):
    flo = torch.empty((N, 2, h, w), dtype=torch.float32, device="cuda")
    val = torch.empty((N, h, w), dtype=torch.uint8, device="cuda")
    ins = torch.empty((N, h, w), dtype=torch.uint8, device="cuda")
    calls = {"k_flow + valid": lambda: sim.flow(h, w, out=flo, valid_out=val), "k_labels<false, true>": lambda: sim.instances(h, w, out=ins)}
    ms = alternating_rounds(stream, calls, REPS, ROUNDS)
    med = {k: median_spread(v)[0] for k, v in ms.items()}
    for k, v in ms.items():
        by = N * h * w * (9 if "flow" in k else 1)
        print(f"  {h:3d} x {w:3d} {k:22s}: median {med[k]:7.3f} ms per call (of {ROUNDS}: {min(v):.3f} .. {max(v):.3f}), {by / 1e6:7.1f} MB written, "
              f"{N * h * w / med[k] / 1e6:7.1f} G pixels/s")
    print(f"  {h:3d} x {w:3d} k_flow / k_labels<false, true> = {med['k_flow + valid'] / med['k_labels<false, true>']:.3f}")
sim.sync()
print(f"  full map: {float(val.float().mean()):.3f} of the pixels valid, median |flow| of them {float(flo.abs().amax(dim=1)[val != 0].median()):.2f} px, "
      f"largest {float(flo.abs().max()):.1f} px")
sim.close()
