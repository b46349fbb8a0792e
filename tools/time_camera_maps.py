"""Time of the fused camera-map launch (dtsim_camera_maps with depth, labels, instances, flow and flags: k_flow_setup + k_camera_maps) against
the three single launches it stands for -- dtsim_depth (k_depth), dtsim_instances with a label map (k_labels<true, true>) and dtsim_flow
(k_flow_setup + k_flow) -- on one rendered batch with one mark, in ONE process: device events around REPS back-to-back calls on the handle's
stream, after a warm-up, the four alternating over ROUNDS rounds; the median round and the spread (min .. max) of each, the sum of the
three single launches round by round, and whether the fused launch is faster than that sum by more than the spread of the run.
N=4096 MAP=small_loop W=640 H=480 FISHEYE=1, maps at H / 4 x W / 4 by default; MAP=loop_pedestrians for the triangle loop (STEPS zero-action
steps before the mark and MOVE driven ones after it, as tools/time_flow.py, so that the duckies have walked and the picture moved)."""
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
REPS = int(os.environ.get("REPS", "20"))
ROUNDS = int(os.environ.get("ROUNDS", "5"))
STEPS = int(os.environ.get("STEPS", "8"))
MOVE = int(os.environ.get("MOVE", "8"))
DIV = int(os.environ.get("DIV", "4"))

stream = torch.cuda.Stream()
sim = BatchedSimulator(MAP, N, camera_width=W, camera_height=H, distortion=FISHEYE, domain_rand=False, seed=0, device_reset=True,
                       stream=stream.cuda_stream, max_steps=10 ** 6)
if STEPS:
    sim.step(np.zeros((STEPS, N, 2), np.float32), n_steps=STEPS)
sim.flow_mark()
sim.step(np.tile(np.array([0.4, 0.2], np.float32), (MOVE, N, 1)), n_steps=MOVE)
sim.render()
h, w = H // DIV, W // DIV
print(f"fused camera maps against the three single launches: {MAP} N={N} {W} x {H}{' fisheye' if FISHEYE else ''} -> {h} x {w}, raster "
      f"{sim.render_pipeline}, {ROUNDS} alternating rounds of {REPS} calls per figure")


def bufs():
    return dict(depth=torch.empty((N, h, w), dtype=torch.float32, device="cuda"), labels=torch.empty((N, h, w), dtype=torch.uint8, device="cuda"),
                instances=torch.empty((N, h, w), dtype=torch.uint8, device="cuda"), flow=torch.empty((N, 2, h, w), dtype=torch.float32, device="cuda"),
                flow_valid=torch.empty((N, h, w), dtype=torch.uint8, device="cuda"))


f, s = bufs(), bufs()
calls = {"k_camera_maps, all outputs": lambda: sim.camera_maps(h, w, **f),
         "k_depth": lambda: sim.depth(h, w, out=s["depth"]),
         "k_labels<true, true>": lambda: sim.instances(h, w, out=s["instances"], labels_out=s["labels"]),
         "k_flow + valid": lambda: sim.flow(h, w, out=s["flow"], valid_out=s["flow_valid"])}
ms = alternating_rounds(stream, calls, REPS, ROUNDS)
for k, v in ms.items():
    med, lo, hi = median_spread(v)
    print(f"  {k:28s}: median {med:7.3f} ms per call (of {ROUNDS}: {lo:.3f} .. {hi:.3f})")
fused = ms["k_camera_maps, all outputs"]
three = [sum(ms[k][r] for k in list(calls)[1:]) for r in range(ROUNDS)]
fm, fl, fh = median_spread(fused)
tm, tl, th = median_spread(three)
spread = max(fh - fl, th - tl)
print(f"  three single launches together: median {tm:7.3f} ms (of {ROUNDS}: {tl:.3f} .. {th:.3f}); fused / three = {fm / tm:.3f}, "
      f"fused / k_flow = {fm / median_spread(ms['k_flow + valid'])[0]:.3f}")
print(f"  saved {tm - fm:.3f} ms per step of maps; spread of the run {spread:.3f} ms; faster by more than the spread: {tm - fm > spread} "
      f"(worst round of fused {fh:.3f} against best round of the three {tl:.3f})")
sim.sync()
differ = {k: int((f[k] != s[k]).sum()) for k in f}
print(f"  elements that differ from the single passes' (every pass reads the render pass's box stream: 0 everywhere): {differ}")
sim.close()
