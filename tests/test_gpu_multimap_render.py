"""GPU: every raster of dt_raster_pipe (csrc/render.hip) past two resident maps and at the grid limits of k_raster_v3 / k_raster_v3dr.

The sets, poses and the N = 130 batch of tests/multimap_scenes.py (tests/test_multimap_scenes_host.py shows what they reach), at 160 x 120,
each through the shared camera, domain randomisation and light_capture -- and the sets that stay on the v3 kernels through
DTSIM_RASTER_OLD=1 as well.  Every case sits behind an assert of sim.render_pipeline against the dispatch restated in
multimap_scenes.expected_pipeline.  Then:

  a. at most six envs against the oracle in the mode of the pass (ORACLE_PLANE for object-free sets, ORACLE_MESH for the others);
  b. EVERY env against the frame of the same state on a handle that holds its map alone: byte for byte where both handles take the same
     raster, within frame_parity.Q_VS_V3 where the set fell to k_raster_q and the one-map handle did not -- and on T2's 0.585 m map, whose
     MSAA margin moves with q_per_m, the larger of the resident maps';
  c. replicas, a second pass and a masked pass over the envs of the highest map id: the same bytes;
  d. depth() and labels() of S4, S5 and L4 against the one-map handles', byte for byte.

A map id the LDS tile table mixes up (the column offset of k_cam_setup's EnvQ.tab3, the mi * V3_MAP_COLS stride of v3_fill_tile_table) reads
another map's entries of the same table: nothing faults, the frames are wrong.  Both mutants were run: v3_fill_tile_table with (mi & 1) fails
a. and b. at map id 2 of S3, S4, P4 and L4 (frame mean 0.4 - 26 against 0.03); k_cam_setup with (map_id & 1) fails a. and b. at map id 2 of P4
and L4 -- S3 and S4 cannot see it, their maps 2 / 3 repeat the tiles of maps 0 / 1.

Measured on the MI355X (worst over the sets, beyond +-1 / beyond +-2 / mean): k_raster_v3 5.2e-5 / 0 / 0.0044, +light 1.0e-4 / 0 / 0.0041,
k_raster_q 5.2e-5 / 0 / 0.0044, +light 1.0e-4 / 0 / 0.0041, k_raster_env 0 / 0 / 0.0009; k_raster_v3dr 3.1e-4 / 3.1e-4 / 0.0025 (the 24 x 16 map;
the small maps 0 / 0 / 0.0009) -- 3.3e-3 / 2.5e-3 / 0.058 before k_resolve_dr wrapped the pixel centre (test_frames_match_the_oracle's
docstring).  No pixel differs in either Q_VS_V3 comparison; byte identity with the one-map handles holds under light_capture and domain randomisation
-- which is why it cannot see a fault both handles share.  158 tests, 13 s.

Five maps under domain randomisation render through the generic per-env raster (k_raster_env, llvmpipe's texture filter), the one-map
handles through k_raster_v3dr (the byte-weight filter): the two filters round apart by 1/255 on 38.5 % of a frame's pixels at worst (measured;
5.2e-5 of them by 2, none by more), which is no case for Q_VS_V3's 0.2 % -- a bound for two rasters with ONE filter.  Those frames are held to
the oracle in their own mode, and byte for byte to the one-map handles created under DTSIM_RASTER_OLD=1, which take the generic raster too."""
import functools
import os
from typing import NamedTuple, Optional

import numpy as np
import pytest

import frame_parity as fp
import multimap_scenes as ms
from dtsim import BatchedSimulator, _ffi
from util import oracle_mode

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
CASES = [(s, m, False, False) for s in ms.SETS for m in ms.MODES] + [(s, "shared", False, True) for s in ms.V3_SETS] + [("L4", "shared", True, False)]
IDS = [f"{s}-{m}{'-fisheye' if f else ''}{'-old' if o else ''}" for s, m, f, o in CASES]
DEPTH_SETS = ("S4", "S5", "L4")
STRIDES = ((1, 1), (2, 2))


@pytest.fixture(autouse=True)
def maps(monkeypatch):
    ms.patch_maps(monkeypatch)


@pytest.fixture(scope="module", autouse=True)
def drop_the_frames_afterwards():
    """run() and alone() keep every case's frames for the tests of this file: let go of them when the file is through."""
    yield
    run.cache_clear()
    alone.cache_clear()


def make_sim(names, n, mode, fisheye, old):
    """A simulator over `names` of n envs in `mode`; old: created under DTSIM_RASTER_OLD=1 (read at dtsim_create)."""
    before = os.environ.get("DTSIM_RASTER_OLD")
    os.environ["DTSIM_RASTER_OLD"] = "1" if old else "0"
    try:
        return BatchedSimulator(names, n, camera_width=ms.W, camera_height=ms.H, distortion=fisheye, domain_rand=(mode == "dr"),
                                light_capture=(mode == "light"), seed=1, max_steps=100000, do_reset=False)
    finally:
        if before is None:
            del os.environ["DTSIM_RASTER_OLD"]
        else:
            os.environ["DTSIM_RASTER_OLD"] = before


def load(sim, states):
    sim.reset(states=states)
    sim.init_states = states


def host(sim, t):
    sim.sync()
    return t.cpu().numpy().copy()


def maps_of(sim):
    """{(sy, sx): (depth [N, h, w] float32, labels [N, h, w] uint8)} of the pass that just ran."""
    return {(sy, sx): (host(sim, sim.depth(ms.H // sy, ms.W // sx)), host(sim, sim.labels(ms.H // sy, ms.W // sx))) for sy, sx in STRIDES}


class Run(NamedTuple):
    pipe: str
    frames: np.ndarray                   # [N, H, W, 3] of the first pass
    again_differ: list                   # envs whose frame of the second pass is not the first's
    sel: np.ndarray                      # [N] bool: the envs of the highest map id, the mask of the masked pass
    masked_differ: list                  # selected envs whose frame of the masked pass is not the first pass's
    masked_rest: str                     # the other frames after the masked pass (buffer filled with SENTINEL before it): "sentinel", "rendered" or "other"
    masked_pipe: str
    oracle_mode: str                     # util.oracle_mode of the handle after the pass
    oracle: Optional[dict]               # worst gt1 / gt2 / mean over the picks, or None with `oracle_error` set
    oracle_error: Optional[str]
    maps: Optional[dict]                 # maps_of(), for DEPTH_SETS


def envs_that_differ(a, b):
    return [int(e) for e in np.flatnonzero((a != b).reshape(len(a), -1).any(axis=1))]


@functools.lru_cache(maxsize=None)
def run(set_name, mode, fisheye=False, old=False):
    """The set's batch through one handle, everything the tests below look at; once per process, read-only."""
    import torch
    names, mid = ms.SETS[set_name], ms.map_ids(set_name)
    sim = make_sim(names, ms.N, mode, fisheye, old)
    load(sim, ms.init_states(set_name, mode, fisheye))
    assert np.array_equal(sim.read(_ffi.FIELD_MAP_ID), mid)
    sim.render()
    pipe = sim.render_pipeline
    frames = sim.frames_host().copy()
    depth_maps = maps_of(sim) if set_name in DEPTH_SETS and mode != "light" and not (fisheye or old) else None
    omode = oracle_mode(sim)
    oracle, err = None, None
    if pipe == ms.expected_pipeline(set_name, mode == "dr", mode == "light", old):      # (else the dispatch test fails, and that is the finding)
        picks = ms.picks(set_name, mode)
        scenes = [ms.scene(n) for n in names]
        try:
            oracle, _ = fp.compare_envs(sim, frames[picks], picks, lambda e: scenes[int(mid[e])], ms.rmap(fisheye), ms.tolerance(set_name), dr=(mode == "dr"),
                                        mode=ms.oracle_mode_of(pipe), colors=sim.read(_ffi.FIELD_COLORS) if mode == "light" else None)
        except AssertionError as e:
            err = str(e)
    sim.render()
    again_differ = envs_that_differ(frames, sim.frames_host())
    sel = mid == len(names) - 1
    dev = torch.as_tensor(sim.frames_device(), device=f"cuda:{sim.device_index}")
    sim.sync()
    dev.fill_(SENTINEL)
    dm = torch.as_tensor(sel, device=f"cuda:{sim.device_index}")
    torch.cuda.synchronize()                               # (the library's stream does not wait for torch's)
    sim.render(mask=dm)
    masked, masked_pipe = sim.frames_host(), sim.render_pipeline
    sim.close()
    masked_differ = [e for e in envs_that_differ(frames, masked) if sel[e]]
    rest = "sentinel" if (masked[~sel] == SENTINEL).all() else "rendered" if np.array_equal(masked[~sel], frames[~sel]) else "other"
    frames.setflags(write=False)
    return Run(pipe, frames, again_differ, sel, masked_differ, rest, masked_pipe, omode, oracle, err, depth_maps)


@functools.lru_cache(maxsize=None)
def alone(map_name, mode, fisheye=False, old=False):
    """(pipeline, frames [N_POSES, H, W, 3], maps_of()) of the eight poses of `map_name` on a handle that holds that map alone."""
    sim = make_sim(map_name, ms.N_POSES, mode, fisheye, old)
    st = (_ffi.InitState * ms.N_POSES)()
    for k in range(ms.N_POSES):
        st[k] = ms.init_state(map_name, k, mode)
    load(sim, st)
    sim.render()
    out = sim.render_pipeline, sim.frames_host().copy(), (maps_of(sim) if mode != "light" else None)
    sim.close()
    out[1].setflags(write=False)
    return out


def differing(a, b):
    return int((a != b).any(axis=-1).sum())


@pytest.mark.parametrize("set_name,mode,fisheye,old", CASES, ids=IDS)
def test_the_raster_of_the_pass_is_the_table_s(set_name, mode, fisheye, old):
    r = run(set_name, mode, fisheye, old)
    want = ms.expected_pipeline(set_name, mode == "dr", mode == "light", old)
    assert r.pipe == want and r.masked_pipe == want, (r.pipe, r.masked_pipe, want)
    if not old:                                            # the issue's table, spelled out
        v3 = set_name in ms.V3_SETS
        assert want == {"shared": "k_raster_v3" if v3 else "k_raster_q", "dr": "k_raster_v3dr" if v3 else "k_raster_env",
                        "light": "k_raster_v3+light" if v3 else "k_raster_q+light"}[mode]
    assert r.oracle_mode == ms.oracle_mode_of(want), (r.oracle_mode, want)     # util.oracle_mode names the filter of that raster
    assert r.frames.std() > 10.0


@pytest.mark.parametrize("set_name,mode,fisheye,old", CASES, ids=IDS)
def test_frames_match_the_oracle(set_name, mode, fisheye, old):
    """The "dr" cases of the 24 x 16 map are what found that k_resolve_dr clamped the pixel centre of an exact-path entry into the padded grid.  On
    pose 3 -- from the last tile along the last column, the far border of the grid 9.2 m away -- one sample of a pixel of the row under the
    horizon still hits tile row 0 (8.4 m away) while the pixel CENTRE lands 13 m away, 8 tiles past the border and 4 past the DT_QRING ring; GL,
    the oracle and the generic raster shade that sample with the tile's texture coordinates extrapolated to the centre (GL_REPEAT wraps them),
    the clamp put the ring's border cell there: 80 of the row's 160 pixels off, 43 of them by 28 - 37 (frame: 3.3e-3 / 2.5e-3 / 0.058 against
    ORACLE_PLANE's 1e-3 / 5e-4 / 0.02; the nudged oracle: 5.2e-5 / 5.2e-5 / 0.0033; k_raster_env on the 25 x 16 and 24 x 17 maps: 0 / 0 / 0.0009).
    Since the centre is wrapped by whole tiles (dr_centre_wrap): 3.1e-4 / 3.1e-4 / 0.0025 at worst.  It takes a tile edge more than about 8 m from
    the camera: no library map is that long.  k_raster_v3's exact path keeps the clamp (14 pixels of that row by up to 29 on the shared camera,
    where the oracle's own headroom does not allow the comparison)."""
    r = run(set_name, mode, fisheye, old)
    assert r.pipe == ms.expected_pipeline(set_name, mode == "dr", mode == "light", old)
    if r.oracle_error is not None:
        pytest.fail(r.oracle_error)
    print(f"multimap {set_name} {mode}{' fisheye' if fisheye else ''}{' old' if old else ''} ({r.pipe}, {'ORACLE_MESH' if ms.has_objects(set_name) else 'ORACLE_PLANE'}): "
          f"envs {ms.picks(set_name, mode)} worst beyond +-1 {r.oracle['gt1']:.2e} beyond +-2 {r.oracle['gt2']:.2e} mean {r.oracle['mean']:.4f}")


@pytest.mark.parametrize("set_name,mode,fisheye,old", CASES, ids=IDS)
def test_every_env_renders_as_on_a_handle_that_holds_its_map_alone(set_name, mode, fisheye, old):
    """(A one-map set against its one-map handle: the same raster over 130 envs and over 8.  Lw and Lh have no v3 one-map handle to be held to --
    their map alone is past the grid limit too -- so their tile-filled far views on the shared camera meet k_raster_q only; L1 under
    DTSIM_RASTER_OLD=1 is held to k_raster_v3 on the same map.)"""
    r = run(set_name, mode, fisheye, old)
    assert r.pipe == ms.expected_pipeline(set_name, mode == "dr", mode == "light", old)
    names, mid = ms.SETS[set_name], ms.map_ids(set_name)
    # the one-map handle on the SAME raster: created under DTSIM_RASTER_OLD=1 where the set left the v3 kernels
    same_old = old or set_name not in ms.V3_SETS
    worst = (0.0, 0.0, 0)
    pose = ms.pose_of(mode, fisheye)
    for e in range(ms.N):
        name, k = names[mid[e]], int(pose[e])
        pipe1, frames1, _ = alone(name, mode, fisheye, same_old)
        assert pipe1 == r.pipe, (name, pipe1, r.pipe)
        moved = set_name == "T2" and name == "small_loop"                       # q_per_m is mm_t47's: the margin that picks the exact-path pixels moves
        if moved:
            worst = max(worst, fp.assert_pair(r.frames[e], frames1[k], fp.Q_VS_V3, (set_name, mode, "env", e, name, "pose", k)))
        else:
            assert np.array_equal(r.frames[e], frames1[k]), (set_name, mode, "env", e, "map id", int(mid[e]), name, "pose", k, differing(r.frames[e], frames1[k]))
        if same_old and mode != "dr" and set_name not in ("Lw", "Lh"):     # k_raster_q over the set against k_raster_v3 on the one-map handle
            pipe3, frames3, _ = alone(name, mode, fisheye, False)
            assert pipe3.startswith("k_raster_v3"), pipe3
            worst = max(worst, fp.assert_pair(r.frames[e], frames3[k], fp.Q_VS_V3, (set_name, mode, "env", e, name, "pose", k, "against k_raster_v3")))
    if worst != (0.0, 0.0, 0):
        print(f"multimap {set_name} {mode}{' old' if old else ''}: worst pair (differ, beyond 1, max) {worst[0]:.2e} {worst[1]:.2e} {worst[2]}")


@pytest.mark.parametrize("set_name,mode,fisheye,old", CASES, ids=IDS)
def test_replicas_a_second_pass_and_a_masked_pass_give_the_same_bytes(set_name, mode, fisheye, old):
    r = run(set_name, mode, fisheye, old)
    reps = ms.replicas(set_name)
    assert len(reps) >= 13
    bad = [(a, b, differing(r.frames[a], r.frames[b])) for a, b in reps if not np.array_equal(r.frames[a], r.frames[b])]
    assert not bad, bad[:8]
    assert not r.again_differ, r.again_differ[:8]
    sel = r.sel
    assert sel.sum() >= 66 and (~sel).sum() >= (1 if len(ms.SETS[set_name]) > 1 else 0)
    assert not r.masked_differ, r.masked_differ[:8]
    # the masked quad-record passes never write the other frames; the generic fallback re-renders unchanged state to the same bytes
    assert r.masked_rest == ("sentinel" if r.pipe.startswith(("k_raster_v3", "k_raster_q")) or sel.all() else "rendered"), r.masked_rest


@pytest.mark.parametrize("mode", ["shared", "dr"])
@pytest.mark.parametrize("set_name", DEPTH_SETS)
def test_depth_and_labels_equal_the_one_map_handles(set_name, mode):
    r = run(set_name, mode)
    names, mid = ms.SETS[set_name], ms.map_ids(set_name)
    same_old = set_name not in ms.V3_SETS
    for stride in STRIDES:
        depth, labels = r.maps[stride]
        assert depth.dtype == np.float32 and labels.dtype == np.uint8 and depth.shape == labels.shape == (ms.N, ms.H // stride[0], ms.W // stride[1])
        assert np.array_equal(labels == 1, np.isinf(depth))                     # sky exactly where the depth is inf
        assert np.isinf(depth).any() and (labels > 2).any()
        for e in range(ms.N):
            d1, l1 = alone(names[mid[e]], mode, False, same_old)[2][stride]
            k = int(ms.pose_of(mode)[e])
            assert depth[e].tobytes() == d1[k].tobytes(), (set_name, mode, stride, "depth", "env", e, "map id", int(mid[e]), int((depth[e] != d1[k]).sum()))
            assert labels[e].tobytes() == l1[k].tobytes(), (set_name, mode, stride, "labels", "env", e, "map id", int(mid[e]), int((labels[e] != l1[k]).sum()))
