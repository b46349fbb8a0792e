"""Time of the instance pass and the box reduction on one rendered batch, in ONE process: dtsim_labels (k_labels<true, false>),
dtsim_instances alone (k_labels<false, true>), dtsim_instances with a label map beside it (k_labels<true, true>: the fused launch) and
dtsim_boxes (k_boxes), with a device-to-device copy of the instance map's bytes as the yardstick for k_boxes (it reads those bytes once).
Device events around REPS back-to-back calls on the handle's stream, after a warm-up, the calls alternating over ROUNDS rounds per output
size; the median round and the spread (min .. max) of each.  The claim the fused launch has to earn: fused < labels + instances of the same
run by more than the run's spread -- the last line of each size states both sides.
N=4096 MAP=small_loop W=640 H=480 FISHEYE=1 by default; MAP=loop_pedestrians for the triangle loop (STEPS zero-action steps first, so that
the duckies have walked)."""
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
print(f"instance pass and boxes: {MAP} N={N} {W} x {H}{' fisheye' if FISHEYE else ''}{' domain_rand' if DR else ''}, raster {sim.render_pipeline}, "
      f"{ROUNDS} alternating rounds of {REPS} calls per figure")
for (h, w) in ((H // 4, W // 4), (H, W)):
    lab = torch.empty((N, h, w), dtype=torch.uint8, device="cuda")
    inst = torch.empty((N, h, w), dtype=torch.uint8, device="cuda")
    copy = torch.empty_like(inst)
    box = torch.empty((N, 64, 5), dtype=torch.int32, device="cuda")
    sim.labels(h, w, out=lab)                                 # (installs the default tables outside the timed calls)
    sim.instances(h, w, out=inst)
    calls = {"labels": lambda: sim.labels(h, w, out=lab), "instances": lambda: sim.instances(h, w, out=inst),
             "instances(labels_out=)": lambda: sim.instances(h, w, out=inst, labels_out=lab), "boxes": lambda: sim.boxes(inst, out=box),
             "copy of the map (d2d)": lambda: copy.copy_(inst)}
    ms = alternating_rounds(stream, calls, REPS, ROUNDS)
    med = {k: median_spread(v)[0] for k, v in ms.items()}
    for k, v in ms.items():
        print(f"  {h:3d} x {w:3d} {k:24s}: median {med[k]:7.3f} ms per call (of {ROUNDS}: {min(v):.3f} .. {max(v):.3f}), map {N * h * w / 1e6:7.1f} MB, "
              f"{N * h * w / med[k] / 1e6:7.1f} G pixels/s")
    two = med["labels"] + med["instances"]
    spread = max(max(v) - min(v) for k, v in ms.items() if k in ("labels", "instances", "instances(labels_out=)"))
    print(f"  {h:3d} x {w:3d} fused {med['instances(labels_out=)']:.3f} ms against labels + instances {two:.3f} ms: saves {two - med['instances(labels_out=)']:.3f} ms "
          f"(largest spread of the three: {spread:.3f} ms); boxes / copy = {med['boxes'] / med['copy of the map (d2d)']:.2f}")
torch.cuda.synchronize()
ids = torch.unique(inst)
n = box[:, :, 4]
print(f"  ids in the full map: {len(ids) - int(ids[0] == 0)}; objects in view per env: mean {float((n > 0).sum(1).float().mean()):.2f}, "
      f"object pixels per env: mean {float(n.sum(1).float().mean()):.0f}")
sim.close()
