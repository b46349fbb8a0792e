"""camera_rand cost: ms per step (dtsim_step + dtsim_render) at N envs, 640x480 + fisheye, loop_only_duckies, domain_rand off,
camera_rand off and on with pools of P calibrations; and the host build time of the remap tables.

    python tools/time_camera_rand.py [--n 4096] [--pools 1,64,4096] [--steps 20]

k_remap_cal's own time comes from a kernel trace of the same run (rocprofv3 --kernel-trace --stats -- python tools/time_camera_rand.py
--pools 64); its bytes: the scratch frame read and the frame write (3 B a pixel each) plus the table (4 B a pixel, once per calibration
when the tables stay in the Infinity Cache)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-duckietown_amd"))
import numpy as np
import torch

from dtsim import BatchedSimulator
from dtsim import distortion as pdist

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4096)
ap.add_argument("--pools", default="1,64,4096")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--skip-off", action="store_true")
args = ap.parse_args()
N, W, H = args.n, 640, 480


def run(pool):
    t0 = time.perf_counter()
    sim = BatchedSimulator("loop_only_duckies", N, camera_width=W, camera_height=H, domain_rand=False, distortion=True,
                           camera_rand=pool is not None, camera_rand_pool=pool, seed=0, max_steps=100000, device_reset=True)
    setup = time.perf_counter() - t0
    acts = np.random.default_rng(0).uniform(0.2, 0.7, (N, 2)).astype(np.float32)
    a = torch.as_tensor(acts, device="cuda")
    torch.cuda.synchronize()
    for _ in range(5):
        sim.step(a)
        sim.render()
    sim.sync()
    t = time.perf_counter()
    for _ in range(args.steps):
        sim.step(a)
        sim.render()
    sim.sync()
    ms = (time.perf_counter() - t) / args.steps * 1e3
    print(f"N={N} {W}x{H} fisheye, camera_rand {'off' if pool is None else f'on, P={pool}'}: {ms:.3f} ms per step "
          f"(construction {setup:.1f} s)", flush=True)
    sim.close()
    torch.cuda.empty_cache()


if not args.skip_off:
    run(None)
for p in [int(v) for v in args.pools.split(",") if v]:
    K, D = pdist.sample_calibrations(p, seed=0)
    t = time.perf_counter()
    pdist.build_src_index(K, D, W, H)
    print(f"table build, P={p} at {W}x{H}: {time.perf_counter() - t:.2f} s", flush=True)
    run(p)
