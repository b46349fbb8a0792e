"""GPU parity AT the BASELINE.json configurations themselves (not at reduced sizes / with parts switched off):

  C3  configs[2]: small_loop, 4096 envs, 640x480 + fisheye -- >= 64 envs of the 4096-env batch, stratified over the
      render order (one per (tile under the camera, heading quadrant) bin of k_env_sort: the first and the last of the
      order, every XCD slice), rendered by the oracle DIRECTLY (no transitive small batch);
  C4  configs[3]: loop_pedestrians, domain randomisation + fisheye, 640x480, after 260 steps (duckies mid-walk);
  C5  configs[4]: MultiMap, both *_only_duckies maps alternating per env slot, 640x480 + fisheye, shared camera:
      k_raster_v3<OBJ> + k_resolve_obj over more than one env chunk.

  C4 / C5 at N = 4096 (round 4): the same two configurations at the batch size the bench lines are quoted on -- 32 (C4) and 16 (C5)
      envs of the 4096-env batch picked like the C3 test (first / last env, both sides of 32-env chunk borders, the middle of
      every XCD's eighth of the chunks, the tail chunk), each rendered by the oracle directly.

Reference: simulator.py:1707-1951 (_render_img), objects.py:384-431 (DuckieObj.step), envs/multimap_env.py:44-49.
Thresholds ("Tolerances"; tests/frame_parity.py): ORACLE_PLANE for plane-only scenes; ORACLE_MESH for scenes with mesh objects
(silhouette pixels of the meshes flip coverage where float32 edge functions meet the oracle's float64 ones).  The oracle is
oracle/raster.py in its "pixel" lighting mode.
"""
import numpy as np
import pytest

from dtsim import BatchedSimulator, _ffi
from dtsim import distortion as pdist
from frame_parity import ORACLE_MESH, ORACLE_PLANE, compare_envs, frames_of, scene, stratified_picks

pytestmark = pytest.mark.gpu
W, H = 640, 480


def test_c3_full_size_batch_matches_oracle_directly():
    N = 4096
    sim = BatchedSimulator("small_loop", N, camera_width=W, camera_height=H, distortion=True, domain_rand=False, seed=5,
                           action_mode="vel_steer")
    acts = np.random.default_rng(0).uniform(-1, 1, (12, N, 2)).astype(np.float32)
    sim.step(acts, n_steps=12)
    sim.render()
    sim.sync()
    pos, ang = sim.read(_ffi.FIELD_POS), sim.read(_ffi.FIELD_ANGLE)
    # the sort key of k_env_sort (render_setup.hip): tile under the camera centre and heading quadrant
    ts = 0.585
    cx, cz = pos[:, 0] + 0.066 * np.cos(ang), pos[:, 2] - 0.066 * np.sin(ang)
    ti, tj = np.clip(np.floor(cx / ts), 0, 31).astype(int), np.clip(np.floor(cz / ts), 0, 31).astype(int)
    quad = np.floor(ang * (2.0 / np.pi) + 0.5).astype(int) & 3
    key = (((tj << 5) | ti) << 2) | quad
    picks = []
    for k in np.unique(key):                               # one env per bin: first, last and every slice of the order
        picks.append(int(np.nonzero(key == k)[0][0]))
    rng = np.random.default_rng(1)
    rpos = sim.read(_ffi.FIELD_RENDER_POS)                 # the order the pass actually ran in: bins as recomputed above, ties broken on the device
    assert sorted(rpos.tolist()) == list(range(N))
    env_at = np.argsort(rpos)
    assert (np.diff(key[env_at]) >= 0).mean() > 0.98       # sorted by the key (the device bins in float32: an env on a bin border may move)
    picks += [int(env_at[0]), int(env_at[-1]), 0, N - 1, int(env_at[31]), int(env_at[32]), int(env_at[63]), int(env_at[64])]
    picks += [int(env_at[i]) for i in range(N // 16, N, N // 8)]    # the middle of each XCD's eighth of the order
    while len(set(picks)) < 64:
        picks.append(int(rng.integers(N)))
    picks = sorted(set(picks))
    assert len(picks) >= 64
    worst, _ = compare_envs(sim, frames_of(sim, picks), picks, scene("small_loop"), pdist.distortion_maps(W, H), ORACLE_PLANE, dr=False, mode="pixel")
    print("C3 4096-env batch, %d envs against the oracle: worst" % len(picks), worst)
    sim.close()


def test_c4_config_matches_oracle():
    """loop_pedestrians + domain randomisation + fisheye at 640x480 after the duckies started walking."""
    N, steps = 4, 260
    sim = BatchedSimulator("loop_pedestrians", N, camera_width=W, camera_height=H, distortion=True, domain_rand=True,
                           seed=31, max_steps=100000)
    sim.step(np.zeros((steps, N, 2), np.float32), n_steps=steps)
    assert sim.read(_ffi.FIELD_OBJ_ACTIVE).any()           # somebody is walking
    sim.render()
    frames = sim.frames_host()
    _, n_obj_px = compare_envs(sim, frames, range(N), scene("loop_pedestrians"), pdist.distortion_maps(W, H), ORACLE_MESH, dr=True, mode="pixel",
                               count_objects=N)
    assert n_obj_px > 200, n_obj_px
    sim.close()


def test_c5_config_matches_oracle():
    """MultiMap: two maps alternating per env slot, shared camera, fisheye, more than one env chunk."""
    N = 72
    names = ["loop_only_duckies", "small_loop_only_duckies"]
    sim = BatchedSimulator(names, N, camera_width=W, camera_height=H, distortion=True, domain_rand=False, seed=17,
                           map_cycle=True, max_steps=100000)
    # multimap_env.py:44-49: every slot starts on map index 1 and moves on at each of ITS resets: restart the even slots
    # once more, so that the two maps alternate over the batch as they do in a running MultiMap-v0 job
    sim.reset(mask=(np.arange(N) % 2 == 0))
    acts = np.random.default_rng(4).uniform(0.1, 0.6, (6, N, 2)).astype(np.float32)
    sim.step(acts, n_steps=6)
    sim.render()
    frames = sim.frames_host()
    mid = sim.read(_ffi.FIELD_MAP_ID)
    assert set(np.unique(mid)) == {0, 1} and mid[0] != mid[1]
    scenes = [scene(n) for n in names]
    envs = [0, 1, 30, 31, 32, 33, 63, 64, 71]              # both maps, chunk borders (64 envs per chunk; 32 before round 6), the tail chunk
    _, n_obj_px = compare_envs(sim, frames[envs], envs, lambda e: scenes[int(mid[e])], pdist.distortion_maps(W, H), ORACLE_MESH, dr=False,
                               mode="pixel", count_objects=len(envs))
    assert n_obj_px > 200, n_obj_px
    sim.close()


def test_c4_full_size_batch_matches_oracle_directly():
    """C4 at the size its bench line is quoted on: 4096 envs of loop_pedestrians with domain randomisation and fisheye after 260
    steps; k_raster_v3dr + k_resolve + k_resolve_obj over 128 chunks, every XCD slice, the persistent work lists wrapped many times."""
    N, steps = 4096, 260
    sim = BatchedSimulator("loop_pedestrians", N, camera_width=W, camera_height=H, distortion=True, domain_rand=True,
                           seed=31, max_steps=100000)
    for _ in range(steps // 52):                           # 260 steps, 52 per launch
        sim.step(np.zeros((52, N, 2), np.float32), n_steps=52)
    assert sim.read(_ffi.FIELD_OBJ_ACTIVE).any()
    sim.render()
    sim.sync()
    picks = stratified_picks(sim, N, 32, 2)
    assert len(picks) >= 32
    worst, n_obj_px = compare_envs(sim, frames_of(sim, picks), picks, scene("loop_pedestrians"), pdist.distortion_maps(W, H), ORACLE_MESH, dr=True,
                                   mode="pixel", count_objects=6)
    assert n_obj_px > 200, n_obj_px
    print("C4 4096-env batch, %d envs against the oracle: worst" % len(picks), worst)
    sim.close()


def test_c5_full_size_batch_matches_oracle_directly():
    """C5's per-GPU share at the size its bench line is quoted on: 4096 envs over both *_only_duckies maps (MultiMap slot
    alternation), shared camera, fisheye: k_raster_v3<OBJ> + k_resolve_obj."""
    N = 4096
    names = ["loop_only_duckies", "small_loop_only_duckies"]
    sim = BatchedSimulator(names, N, camera_width=W, camera_height=H, distortion=True, domain_rand=False, seed=17,
                           map_cycle=True, max_steps=100000)
    sim.reset(mask=(np.arange(N) % 2 == 0))                # multimap_env.py:44-49 (see test_c5_config_matches_oracle)
    acts = np.random.default_rng(4).uniform(0.1, 0.6, (6, N, 2)).astype(np.float32)
    sim.step(acts, n_steps=6)
    sim.render()
    sim.sync()
    mid = sim.read(_ffi.FIELD_MAP_ID)
    assert set(np.unique(mid)) == {0, 1}
    picks = stratified_picks(sim, N, 16, 3)
    assert len(picks) >= 16 and {int(mid[e]) for e in picks} == {0, 1}
    scenes = [scene(n) for n in names]
    worst, _ = compare_envs(sim, frames_of(sim, picks), picks, lambda e: scenes[int(mid[e])], pdist.distortion_maps(W, H), ORACLE_MESH, dr=False,
                            mode="pixel")
    print("C5 4096-env batch, %d envs against the oracle: worst" % len(picks), worst)
    sim.close()


@pytest.mark.parametrize("cfg", ["c5", "c4"])
def test_two_handles_render_one_state_to_the_same_bytes(cfg):
    """Two fresh handles built from one seeded state render the same frames, bit for bit, on the mesh-object paths: 1024 envs =
    16 chunks in the sorted render order, k_raster_v3<OBJ> + k_resolve_obj for C5, k_raster_v3dr<OBJ> + k_resolve_dr + k_resolve_obj
    for C4 (the envs reach the raster and the persistent exact-path wavefronts in an order that differs from launch to launch)."""
    N = 1024
    kw = dict(c5=dict(maps=["loop_only_duckies", "small_loop_only_duckies"], dr=False, extra=dict(map_cycle=True)),
              c4=dict(maps="loop_pedestrians", dr=True, extra={}))[cfg]
    out = []
    for _ in range(2):
        sim = BatchedSimulator(kw["maps"], N, camera_width=W, camera_height=H, distortion=True, domain_rand=kw["dr"], seed=5, max_steps=100000,
                               **kw["extra"])
        acts = np.random.default_rng(9).uniform(0.2, 0.9, (4, N, 2)).astype(np.float32)
        sim.step(acts, n_steps=4)
        sim.render()
        out.append(sim.frames_host().copy())
        sim.close()
    assert out[0].std() > 10.0
    assert np.array_equal(out[0], out[1])
