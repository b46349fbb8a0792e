"""GPU: the mesh-object path -- k_obj_setup -> the <OBJ> raster -> k_resolve_obj -- in crowds and close-ups, against the oracle object by object.

The views of tests/crowd_scenes.py (tests/test_crowd_scenes_host.py shows what they reach: all 64 objects live, dozens of boxes in one raster
tile, heavy regions, units of more than 128 entries, every border cut, triangles across the near plane, hidden and moved objects), one env per
view, through every pipeline that carries objects; frame_parity.compare_objects holds the whole frame to ORACLE_MESH, every object with a countable
interior to 5 % + 2 of its interior pixels, and the pixels away from the objects to ORACLE_PLANE's beyond-2 share.  Then, without the oracle:
replicas over several chunks, two maps in one chunk, and the same bytes twice.

Measured worst figures per case: DESIGN.md section 4 (no interior pixel of any object beyond +-2 in any case).  Case "q" is what found that
k_raster_q marked EVERY object-box pixel as a plane edge, so that k_resolve_obj shaded the plane pixels inside the boxes again with the exact
path's filter (+-1 on a quarter of their channel values against the byte-weight filter of the pixels around them): frame mean 0.0300 in "inside"
before the raster told the two apart, 0.0073 since."""
import functools

import numpy as np
import pytest

import crowd_scenes as cs
import frame_parity as fp
from dtsim import BatchedSimulator, assets
from oracle import raster
from util import oracle_mode

pytestmark = pytest.mark.gpu

# case -> (width, height, fisheye, domain randomisation, DTSIM_RASTER_OLD, the raster of the pass)
CASES = {
    "v3": (320, 240, True, False, None, "k_raster_v3"),
    "v3_plain": (160, 120, False, False, None, "k_raster_v3"),        # every silhouette pixel weighs four times as much
    "v3dr": (320, 240, True, True, None, "k_raster_v3dr"),
    "q": (160, 120, True, False, "1", "k_raster_q"),
    "generic": (162, 120, False, False, None, "k_raster"),            # a width that is no multiple of 4
}
SEGMENT = (160, 120, False, False, None, "k_raster_env")


@pytest.fixture
def maps(monkeypatch):
    """The two maps as fixtures of the asset library, so that one simulator can hold both by name."""
    monkeypatch.setitem(assets.MAPS, "crowd", cs.crowd_map())
    monkeypatch.setitem(assets.MAPS, "empty", cs.map_data("empty"))


def make_sim(cfg, views, names="crowd", map_ids=None):
    """A simulator of `cfg` with env e at views[e] on map names[map_ids[e]]; the crowd envs carry their view's object state."""
    W, H, fisheye, dr, _, _ = cfg
    sim = BatchedSimulator(names, len(views), camera_width=W, camera_height=H, distortion=fisheye, domain_rand=dr, seed=1, max_steps=100000,
                           do_reset=False)
    st = cs.init_states(views, dr, map_ids)
    sim.reset(states=st)
    sim.init_states = st
    on_crowd = [v if (map_ids is None or sim.map_names[int(map_ids[e])] == "crowd") else None for e, v in enumerate(views)]
    cs.write_env_state(sim, on_crowd)
    return sim


def rendered(sim, pipe, **kw):
    sim.render(**kw)
    out = sim.frames_host().copy()
    assert sim.render_pipeline == pipe, sim.render_pipeline
    return out


@functools.lru_cache(maxsize=None)
def case_frames(case):
    """(frames [4, H, W, 3] of the four views, the oracle mode of the pass) of `case`, rendered once per process: read-only.  (The "q" case is
    created under DTSIM_RASTER_OLD=1: its test sets it.)"""
    cfg = CASES[case]
    sim = make_sim(cfg, cs.VIEWS)
    frames = rendered(sim, cfg[5])
    mode = oracle_mode(sim)
    for e, view in enumerate(cs.VIEWS):              # the device holds exactly the state the cached oracle frames were rendered from
        dev, want = fp.obj_states(sim, e, cs.scene()), cs.obj_states(view)
        assert all(np.array_equal(a["pos"], b["pos"]) and a["y_rot"] == b["y_rot"] and a["visible"] == b["visible"] for a, b in zip(dev, want)), (case, view)
        cam, ref = fp.camera(sim, e, cfg[0], cfg[1], cfg[3]), cs.camera(view, cfg[0], cfg[1], cfg[3])
        assert np.array_equal(cam.C, ref.C) and (cam.sa, cam.ca, cam.sth, cam.ty) == (ref.sa, ref.ca, ref.sth, ref.ty), (case, view)
    sim.close()
    frames.setflags(write=False)
    return frames, mode


def report(case, results):
    """One line per case: the figures DESIGN.md section 4 / PARITY.md record."""
    worst = max(results, key=lambda r: r["obj_share"])
    print(f"crowd {case}: objects judged {sum(r['judged'] for r in results)} ({' + '.join(str(r['judged']) for r in results)}), worst per-object share "
          f"{worst['obj_share']:.4f} (object, beyond +-2, interior) = {worst['obj_worst']}, outside the objects {max(r['outside'] for r in results)} px, "
          f"frame beyond +-1 {max(r['frame']['gt1'] for r in results):.2e} beyond +-2 {max(r['frame']['gt2'] for r in results):.2e} "
          f"mean {max(r['frame']['mean'] for r in results):.4f}")


@pytest.mark.parametrize("case", list(CASES))
def test_crowd_views_match_the_oracle_object_by_object(case, maps, monkeypatch):
    W, H, fisheye, dr, old, _ = CASES[case]
    if old:
        monkeypatch.setenv("DTSIM_RASTER_OLD", old)
    frames, mode = case_frames(case)
    assert mode == {"v3": "pixel", "v3_plain": "pixel", "v3dr": "pixel-dr", "q": "pixel", "generic": "pixel-gl"}[case]
    results = []
    for e, view in enumerate(cs.VIEWS):
        ref, ids = cs.oracle_view(view, mode, W, H, fisheye, dr)
        results.append(fp.compare_objects(frames[e], ref, ids, fp.ORACLE_OBJECTS, ctx=(case, f"env {e}", view)))
    report(case, results)
    assert all(r["judged"] >= 1 for r in results)                    # every view has a countable object at this size too


def test_crowd_segment_views_match_the_oracle_object_by_object(maps):
    """`render(segment=True)` through the generic raster: unlit flat-coloured meshes on magenta, against raster.segment_view."""
    W, H, fisheye, dr, _, pipe = SEGMENT
    sim = make_sim(SEGMENT, cs.VIEWS)
    frames = rendered(sim, pipe, segment=True)
    seg_tex, rgb = sim.segment_assets()
    seg_by_kind = {kd: seg_tex[i] for i, kd in enumerate(sim.texture_kinds)}
    cols = {mk: rgb[i] for i, mk in enumerate(sim._mesh_order)}
    results = []
    for e, view in enumerate(cs.VIEWS):
        cam, sc = raster.segment_view(cs.camera(view, W, H), cs.scene(), seg_by_kind, cols)
        ref, ids = raster.render_obs(cam, sc, "pixel", None, obj_states=fp.obj_states(sim, e, cs.scene()), return_ids=True)
        results.append(fp.compare_objects(frames[e], ref, np.stack(ids), fp.ORACLE_OBJECTS, ctx=("segment", f"env {e}", view)))
    sim.close()
    report("generic (segment)", results)


@pytest.mark.parametrize("case", ["v3", "v3dr"])
def test_replicas_over_three_chunks_render_the_views_bytes(case, maps):
    """N = 130: two 64-env chunks and a tail of two, env e a replica of view e % 4 -- many heavy work items at once, both ends of the item list, the
    chunk tail.  Every frame must be its view's frame of the N = 4 run."""
    N = 130
    cfg = CASES[case]
    want, _ = case_frames(case)
    sim = make_sim(cfg, [cs.VIEWS[e % 4] for e in range(N)])
    got = rendered(sim, cfg[5])
    sim.close()
    differ = [e for e in range(N) if not np.array_equal(got[e], want[e % 4])]
    assert not differ, (case, differ[:16], [int((got[e] != want[e % 4]).any(axis=-1).sum()) for e in differ[:16]])


def test_two_maps_in_one_chunk_render_as_each_map_alone(maps):
    """["crowd", "empty"] at N = 8 with alternating map ids: 64 objects next to none inside one chunk, the object ranges per map.  The crowd envs
    must render as in the single-map run, the empty-map envs as a small_loop run of the same poses."""
    cfg = CASES["v3"]
    views = [cs.VIEWS[e // 2] for e in range(8)]
    sim = make_sim(cfg, views, ["crowd", "empty"], np.arange(8) % 2)
    got = rendered(sim, cfg[5])
    sim.close()
    crowd, _ = case_frames("v3")
    plain = make_sim(cfg, cs.VIEWS, "small_loop")
    bare = rendered(plain, cfg[5])
    plain.close()
    for e in range(8):
        want = crowd[e // 2] if e % 2 == 0 else bare[e // 2]
        assert np.array_equal(got[e], want), (e, views[e], int((got[e] != want).any(axis=-1).sum()))
    assert all((crowd[v] != bare[v]).any() for v in range(4))          # the objects are in every view: the two halves differ


def test_crowd_renders_to_the_same_bytes_twice(maps):
    cfg = CASES["v3"]
    sim = make_sim(cfg, cs.VIEWS)
    a = rendered(sim, cfg[5])
    b = rendered(sim, cfg[5])
    sim.close()
    assert np.array_equal(a, b), int((a != b).any(axis=-1).sum())
    assert np.array_equal(a, case_frames("v3")[0])
