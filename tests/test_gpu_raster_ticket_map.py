"""GPU: k_raster_v3's workgroup map with a ticketed suffix (csrc/raster_map.h, raster_wg / raster_claim_* in raster_common.h) writes every frame
tile of every env once, whoever claims the item.

The frame batch is filled with a sentinel; a full pass (the static prefix, the claimed suffix, stealing between the XCDs' lists) must then
equal, byte for byte, the masked pass with an all-ones mask over a batch filled with the sentinel again -- that pass goes through the SUB
instantiation's linear map, which has no tickets -- and a second full pass.  No tolerance: equality only.

Shapes: 160 x 120 (2 x 15 raster tiles: groups of 15) and 128 x 88 (1 x 11 tiles: a short last group), fisheye; N = 72 (two chunks, one
partial: two lists of one chunk, six empty) and N = 584 (10 chunks: five lists of two chunks and three empty ones, whose workgroups can
only steal); the mesh-object instantiation with k_resolve_obj's items behind it, and the per-env light."""
import numpy as np
import pytest

from dtsim import BatchedSimulator

pytestmark = pytest.mark.gpu

# (map, BatchedSimulator kwargs, render_pipeline, (W, H), N)
CASES = {
    "160x120-72": ("small_loop", {}, "k_raster_v3", (160, 120), 72),
    "160x120-584": ("small_loop", {}, "k_raster_v3", (160, 120), 584),
    "128x88-72": ("small_loop", {}, "k_raster_v3", (128, 88), 72),
    "128x88-584": ("small_loop", {}, "k_raster_v3", (128, 88), 584),
    "objects-128x88-584": ("loop_only_duckies", {}, "k_raster_v3", (128, 88), 584),
    "light-160x120-584": ("small_loop", dict(light_capture=True), "k_raster_v3+light", (160, 120), 584),
}


@pytest.mark.parametrize("case", list(CASES))
def test_full_pass_equals_the_masked_pass_over_all_envs(case):
    import torch
    map_name, kw, want, (W, H), N = CASES[case]
    sim = BatchedSimulator(map_name, N, camera_width=W, camera_height=H, distortion=True, domain_rand=False, seed=N + W, max_steps=100000,
                           action_mode="vel_steer", device_reset=True, do_reset=False, **kw)
    try:
        sim.reset()
        sim.step(np.random.default_rng(N).uniform(0.2, 0.9, (3, N, 2)).astype(np.float32), n_steps=3)
        dev = torch.device(f"cuda:{sim.device_index}")
        frames = torch.as_tensor(sim.frames_device(), device=dev).view(N, H * W * 3)
        sentinel = torch.randint(0, 256, (N, H * W * 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(N)).to(dev)
        ones = torch.ones(N, dtype=torch.bool, device=dev)

        def render(mask=None):
            sim.sync()
            frames.copy_(sentinel)
            torch.cuda.synchronize(dev)                # (the library's stream does not wait for torch's)
            sim.render(mask=mask)
            assert sim.render_pipeline == want, (case, sim.render_pipeline)
            sim.sync()
            return frames.clone()

        full = render()
        masked = render(ones)
        again = render()

        def envs(a, b):
            return torch.nonzero((a != b).any(dim=1)).flatten()[:8].tolist()

        # a tile of an env that no workgroup rendered keeps its sentinel in the full pass and not in the masked one
        assert torch.equal(full, masked), (case, "the full pass differs from the masked pass over all envs", envs(full, masked))
        assert torch.equal(full, again), (case, "the second full pass differs", envs(full, again))
        assert not bool((full == sentinel).all(dim=1).any()), (case, "a frame is still its sentinel")
        assert float(full.float().std()) > 10.0         # views, not a constant
    finally:
        sim.close()
