"""Time of the ground-projection pass (dtsim_ipm) in ONE process: the shared camera's gather (k_ipm_gather through the cached table), the
per-env projection (k_ipm_env, on a second handle with domain randomisation: a camera per env), and two yardsticks that are not the
code under test -- a device-to-device copy of the output's bytes, and dtsim_bev (k_bev) at the same shape on the same handle.  Device events
around REPS back-to-back calls on the handles' stream, after a warm-up, the calls alternating over ROUNDS rounds; the median round and the
spread (min .. max) of each.  The expectation to confirm or refute: the gather is bound by its scattered 3-byte frame reads, not by
arithmetic, so it costs a small multiple of the copy and does not depend on the fisheye; k_ipm_env pays the float64 projection per cell and
env on top.
N=4096 W=640 H=480 DISTORTION=1 by default; SHAPES as oh,ow,cell;... (128,128,0.02;64,64,0.04)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gym-duckietown_amd"), os.path.join(ROOT, "tests"), ROOT]
import torch
from dtsim import BatchedSimulator
from timing import alternating_rounds, median_spread

N = int(os.environ.get("N", "4096"))
W, H = int(os.environ.get("W", "640")), int(os.environ.get("H", "480"))
DIST = os.environ.get("DISTORTION", "1") == "1"
REPS = int(os.environ.get("REPS", "20"))
ROUNDS = int(os.environ.get("ROUNDS", "5"))
SHAPES = [(int(a), int(b), float(c)) for a, b, c in (s.split(",") for s in os.environ.get("SHAPES", "128,128,0.02;64,64,0.04").split(";"))]

stream = torch.cuda.Stream()
kw = dict(camera_width=W, camera_height=H, distortion=DIST, seed=0, device_reset=True, stream=stream.cuda_stream, max_steps=10 ** 6)
shared = BatchedSimulator("small_loop", N, domain_rand=False, **kw)
shared.render()
per_env = BatchedSimulator("small_loop", N, domain_rand=True, **kw)         # a camera per env: k_ipm_env
per_env.bind_frames(shared.frames_device().__cuda_array_interface__["data"][0])    # one frame batch for both: no second batch is read
lab = shared.bev(8, 8)                                                      # (installs the default tables outside the timed calls)
print(f"ground projection: small_loop N={N}, {W} x {H}{' + fisheye' if DIST else ''}, {ROUNDS} alternating rounds of {REPS} calls per figure")
for (oh, ow, cell) in SHAPES:
    for chw in (True, False):
        out = torch.empty((N, 3, oh, ow) if chw else (N, oh, ow, 3), dtype=torch.uint8, device="cuda")
        out2, copy = torch.empty_like(out), torch.empty_like(out)
        val = torch.empty((N, oh, ow), dtype=torch.uint8, device="cuda")
        idx = torch.empty((N, oh, ow), dtype=torch.int32, device="cuda")
        bev = torch.empty((N, oh, ow), dtype=torch.uint8, device="cuda")
        calls = {"ipm gather (image)": lambda: shared.ipm(oh, ow, cell=cell, chw=chw, out=out),
                 "ipm gather (image + valid + index)": lambda: shared.ipm(oh, ow, cell=cell, chw=chw, out=out, valid_out=val, index_out=idx),
                 "ipm per env (image)": lambda: per_env.ipm(oh, ow, cell=cell, chw=chw, out=out2),
                 "copy of the image (d2d)": lambda: copy.copy_(out),
                 "bev (classes)": lambda: shared.bev(oh, ow, cell=cell, out=bev)}
        ms = alternating_rounds(stream, calls, REPS, ROUNDS)
        med = {k: median_spread(v)[0] for k, v in ms.items()}
        tag = f"{oh:3d} x {ow:3d} at {cell:.2f} m {'CHW' if chw else 'HWC'}"
        for k, v in ms.items():
            print(f"  {tag}  {k:36s}: median {med[k]:7.3f} ms per call (of {ROUNDS}: {min(v):.3f} .. {max(v):.3f})")
        print(f"  {tag}  image {N * oh * ow * 3 / 1e6:.1f} MB; gather / copy = {med['ipm gather (image)'] / med['copy of the image (d2d)']:.2f}, "
              f"gather / bev = {med['ipm gather (image)'] / med['bev (classes)']:.2f}, per env / gather = "
              f"{med['ipm per env (image)'] / med['ipm gather (image)']:.2f}")
shared.close()
per_env.close()
