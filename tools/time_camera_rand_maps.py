"""Cost of the camera post-passes under per-env distortion tables (DTSIM_MAP_ENV_TABLES: k_depth<F16, true>, k_labels<LAB, INST, true>)
against the single-table passes, on ONE handle and one set of states; and the DuckietownVecEnv step under camera_rand with the map options
on against off.

    python tools/time_camera_rand_maps.py [--n 4096] [--pool 64] [--reps 10] [--rounds 5] [--env-steps 20] [--skip-env]

Per round the handle takes the nominal table for every env (dtsim_set_distortion_lut: the folded fisheye, flags 0), is rendered, and each
pass is timed; then the per-env tables (dtsim_set_distortion_luts), a render, and each pass under the flag -- the two alternate in one
process, device events around `reps` back-to-back calls on the handle's stream; the median and spread of the rounds.  640 x 480, the 120 x 160
and the full-size maps."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-duckietown_amd"))
import numpy as np
import torch

from dtsim import BatchedSimulator, DuckietownVecEnv, _ffi
from dtsim import distortion as pdist
from timing import median_spread

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4096)
ap.add_argument("--pool", type=int, default=64)
ap.add_argument("--map", default="loop_pedestrians")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--env-steps", type=int, default=20)
ap.add_argument("--skip-env", action="store_true")
ap.add_argument("--skip-passes", action="store_true")
args = ap.parse_args()
N, W, H = args.n, 640, 480
SIZES = ((H // 4, W // 4), (H, W))


def timed(stream, f, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    for _ in range(reps):
        f()
    t1.record(stream)
    t1.synchronize()
    return t0.elapsed_time(t1) / reps


def passes():
    stream = torch.cuda.Stream()
    sim = BatchedSimulator(args.map, N, camera_width=W, camera_height=H, domain_rand=False, distortion=True, camera_rand=True,
                           camera_rand_pool=args.pool, seed=0, max_steps=10 ** 6, device_reset=True, stream=stream.cuda_stream)
    sim._need_label_assets()
    lib, h = sim._lib, sim._h
    rmx, rmy = pdist.distortion_maps(W, H)
    fp = C.POINTER(C.c_float)
    print(f"passes alone: {args.map} N={N} {W} x {H}, camera_rand with {args.pool} calibrations, {args.reps} calls per figure, {args.rounds} rounds, "
          f"single table (nominal, flags 0) and per-env tables (DTSIM_MAP_ENV_TABLES) alternating on one handle", flush=True)
    bufs = {s: (torch.empty((N, *s), dtype=torch.float32, device="cuda"), torch.empty((N, *s), dtype=torch.uint8, device="cuda"),
                torch.empty((N, *s), dtype=torch.uint8, device="cuda")) for s in SIZES}
    ms = {}

    def calls(s, flags):
        d, l, i = (C.c_void_p(t.data_ptr()) for t in bufs[s])
        return {"depth f32": lambda: _ffi.check(lib, lib.dtsim_depth(h, d, s[0], s[1], flags)),
                "depth f16": lambda: _ffi.check(lib, lib.dtsim_depth(h, d, s[0], s[1], flags | _ffi.DEPTH_F16)),
                "labels": lambda: _ffi.check(lib, lib.dtsim_labels(h, l, s[0], s[1], flags)),
                "instances": lambda: _ffi.check(lib, lib.dtsim_instances(h, i, None, s[0], s[1], flags)),
                "instances+labels": lambda: _ffi.check(lib, lib.dtsim_instances(h, i, l, s[0], s[1], flags))}

    with torch.cuda.stream(stream):
        for r in range(args.rounds + 1):                     # round 0: the warm-up, not counted
            for kind in ("single", "per-env"):
                if kind == "single":
                    _ffi.check(lib, lib.dtsim_set_distortion_lut(h, rmx.ctypes.data_as(fp), rmy.ctypes.data_as(fp)))
                else:
                    sim._install_calibrations()
                sim.render()
                for s in SIZES:
                    for name, f in calls(s, 0 if kind == "single" else _ffi.MAP_ENV_TABLES).items():
                        t = timed(stream, f, 3 if r == 0 else args.reps)
                        if r:
                            ms.setdefault((s, name, kind), []).append(t)
    for s in SIZES:
        for name in ("depth f32", "depth f16", "labels", "instances", "instances+labels"):
            a, b = median_spread(ms[(s, name, "single")]), median_spread(ms[(s, name, "per-env")])
            print(f"  {s[0]:3d} x {s[1]:3d} {name:17s} single {a[0]:8.3f} ms ({a[1]:.3f} .. {a[2]:.3f})   per-env {b[0]:8.3f} ms ({b[1]:.3f} .. {b[2]:.3f})   "
                  f"ratio {b[0] / a[0]:.3f}", flush=True)
    sim.close()
    torch.cuda.empty_cache()


def env_step():
    kw = dict(camera_rand=True, distortion=True, domain_rand=False, camera_width=W, camera_height=H, camera_rand_pool=args.pool, seed=0,
              obs_shape=(120, 160))
    shape = (H // 4, W // 4)
    envs = {"off": DuckietownVecEnv(args.map, N, **kw),
            "on": DuckietownVecEnv(args.map, N, depth_shape=shape, label_shape=shape, instance_shape=shape, boxes=True, camera_rand_maps=True, **kw)}
    a = torch.as_tensor(np.random.default_rng(0).uniform(0.2, 0.7, (N, 2)).astype(np.float32), device="cuda")
    ms = {k: [] for k in envs}
    for r in range(args.rounds + 1):
        for k, env in envs.items():
            if r == 0:
                env.reset()
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(3 if r == 0 else args.env_steps):
                env.step(a)
            torch.cuda.synchronize()
            if r:
                ms[k].append((time.perf_counter() - t) / args.env_steps * 1e3)
    a_, b_ = median_spread(ms["off"]), median_spread(ms["on"])
    print(f"DuckietownVecEnv step: {args.map} N={N} {W} x {H} camera_rand, obs 120 x 160, {args.env_steps} steps per figure, {args.rounds} rounds alternating: "
          f"without map options {a_[0]:.3f} ms ({a_[1]:.3f} .. {a_[2]:.3f}); with depth, labels, instances 120 x 160 and boxes {b_[0]:.3f} ms "
          f"({b_[1]:.3f} .. {b_[2]:.3f}); ratio {b_[0] / a_[0]:.3f}", flush=True)
    for env in envs.values():
        env.close()


if not args.skip_passes:
    passes()
if not args.skip_env:
    env_step()
