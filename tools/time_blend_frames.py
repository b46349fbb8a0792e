"""k_blend_frames alone (BatchedSimulator.blend_frames) beside a device-to-device copy of the same byte count, in one process.
N envs (default 4096) at 640 x 480: the reference's window of four frame batches into a fifth -- 5 x N x 921 600 bytes per launch -- against
torch's copy_ of 2.5 frame batches (hipMemcpyAsync device to device: the same bytes read + written).  ROUNDS alternating rounds of REPS
launches each, host clock around a device synchronise; the median round is reported, with uint8 and float32 (8 frame batches of traffic) out."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-duckietown_amd"))
import torch
from dtsim import BatchedSimulator
N = int(os.environ.get("N", "4096"))
REPS = int(os.environ.get("REPS", "20"))
ROUNDS = int(os.environ.get("ROUNDS", "5"))
W, H = 640, 480
WEIGHTS = (80, 15, 4, 1)

sim = BatchedSimulator("small_loop", N, camera_width=W, camera_height=H, domain_rand=False, seed=0)
batch = N * H * W * 3
frames = [torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, device="cuda") for _ in WEIGHTS]
out_u8 = torch.empty_like(frames[0])
out_f32 = torch.empty((N, H, W, 3), dtype=torch.float32, device="cuda")
src = torch.randint(0, 256, (batch * 5 // 2,), dtype=torch.uint8, device="cuda")
dst = torch.empty_like(src)
torch.cuda.synchronize()


def blend(out):
    for _ in range(REPS):
        sim.blend_frames(out, frames, WEIGHTS)
    sim.sync()


def copy():
    for _ in range(REPS):
        dst.copy_(src)
    torch.cuda.synchronize()


cases = [("k_blend_frames<uint8, 4>", lambda: blend(out_u8), 5 * batch), ("k_blend_frames<float, 4>", lambda: blend(out_f32), 8 * batch),
         ("device-to-device copy", copy, 2 * src.numel())]
ms = {name: [] for name, _, _ in cases}
for _, fn, _ in cases:
    fn()                                                   # warm-up
for r in range(ROUNDS):
    for name, fn, _ in (cases if r % 2 == 0 else cases[::-1]):
        t = time.perf_counter()
        fn()
        ms[name].append((time.perf_counter() - t) / REPS * 1e3)
for name, _, nbytes in cases:
    s = sorted(ms[name])
    med = s[len(s) // 2]
    print(f"N={N} {name:28s} {nbytes / 1e9:6.2f} GB per launch: median {med:.3f} ms (min {s[0]:.3f}, max {s[-1]:.3f}; {ROUNDS} rounds of {REPS}) "
          f"-> {nbytes / med / 1e9:.2f} TB/s")
sim.close()
