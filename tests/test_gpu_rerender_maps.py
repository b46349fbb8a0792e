"""`-m gpu`: the maps of a handle that has rendered BEFORE -- dtsim_depth, dtsim_labels, dtsim_instances, dtsim_boxes, dtsim_camera_maps, their
masked forms and dtsim_draw_leds after a second render from another pose -- against the oracle of the CURRENT state, and byte for byte against
a fresh twin handle whose first and only render is that state.

Every test primes its handle: reset to the prime poses of tests/rerender_model.py, render(), the current poses by dtsim_write, render().  At
the current poses part of an object that was in full view leaves the frame or crosses the near plane, so the pass culls triangles whose
ScreenTri records still describe the first render; tests/test_rerender_model_host.py asserts that a reader going by those records would get
3 x the caps' worth of pixels wrong in every pair.  Tolerances and caps are read where tests/test_gpu_depth.py, test_gpu_labels.py and
test_gpu_instances.py read them.  The "parity" lines this file prints are the record of profiles/rerender_parity.txt."""
import functools

import numpy as np
import pytest

import camera_rand_maps_model as cm
import depth_model as dm
import frame_parity as fp
import instance_model as im
import label_model as lm
import rerender_model as rm
from dtsim import BatchedSimulator, DuckietownVecEnv, _ffi
from oracle import raster
from test_gpu_camera_maps import SENTINEL, fresh, host
from test_gpu_depth import TOL

pytestmark = pytest.mark.gpu
THREE = ("depth", "labels", "instances")
BOX_SENTINEL = -7
STRIDE = (2, 2)
KINDS = (None, "fisheye")


# ---- handles ---------------------------------------------------------------------------------------------------------------------------------------

def make(group, which, kind=None, **kw):
    """A handle of the group's map and size, env e at pair e's pose `which` (rerender_model.case)."""
    c = rm.case(group, which)
    args = dict(camera_width=c.W, camera_height=c.H, distortion=kind == "fisheye", domain_rand=False, seed=1, max_steps=10 ** 6, do_reset=False)
    args.update(kw)
    if c.asset_tree:
        args["asset_root"] = fp.ASSETS
    sim = BatchedSimulator(c.map_name, len(c.states), **args)
    sim.reset(states=dm.init_states(c))
    return sim


def move(sim, group, which="cur"):
    """The poses `which` by dtsim_write, as tests/test_gpu_flow.py's to_current moves a handle."""
    cur = dm.init_states(rm.case(group, which))
    sim.write(_ffi.FIELD_POS, np.array([list(st.pos) for st in cur], np.float64))
    sim.write(_ffi.FIELD_ANGLE, np.array([st.angle for st in cur], np.float64))


def primed(group, kind=None, history=("prime",), **kw):
    """A handle that rendered every pose of `history`, then stands at the current poses (not yet rendered there)."""
    sim = make(group, history[0], kind, **kw)
    sim.render()
    for which in history[1:]:
        move(sim, group, which)
        sim.render()
    move(sim, group)
    return sim


def twin_of(sim, group, kind=None, **kw):
    """A fresh handle holding `sim`'s state, byte for byte (DTSIM_FIELD_STATE_BLOB); nothing rendered yet."""
    tw = make(group, "cur", kind, **kw)
    blob = sim.read(_ffi.FIELD_STATE_BLOB)
    tw.write(_ffi.FIELD_STATE_BLOB, blob)
    assert np.array_equal(tw.read(_ffi.FIELD_STATE_BLOB), blob)
    return tw


def check_state(sim, group):
    """The device holds the state the oracle's maps of the current poses were made from."""
    c = rm.case(group)
    sc = dm.scene_of(c)
    pos, ang = sim.read(_ffi.FIELD_POS), sim.read(_ffi.FIELD_ANGLE)
    for e, (x, z, a, *_rest) in enumerate(c.states):
        assert (pos[e, 0], pos[e, 2], ang[e]) == (x, z, a), (group, e)
        for got, want in zip(fp.obj_states(sim, e, sc), dm.host_objects(c)[e]):
            assert np.allclose(got["pos"], want["pos"], rtol=0, atol=1e-9) and abs(got["y_rot"] - want["y_rot"]) <= 1e-7 and got["visible"] == want["visible"], (group, e)


def outputs(sim, h, w, dtype="float32", mask=None):
    """Every map of the last render at one size, on the host: depth, labels, instances by their single passes, boxes of that instance map, and
    fused_depth, fused_labels, fused_instances by one dtsim_camera_maps call; each written into a sentinel-filled tensor of the test's own."""
    import torch
    b, f = fresh(sim, h, w, THREE, dtype), fresh(sim, h, w, THREE, dtype)
    boxes = torch.full((sim.num_envs, _ffi.MAX_OBJECTS, 5), BOX_SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    sim.depth(h, w, dtype=dtype, out=b["depth"], mask=mask)
    sim.labels(h, w, out=b["labels"], mask=mask)
    sim.instances(h, w, out=b["instances"], mask=mask)
    sim.boxes(b["instances"], out=boxes, mask=mask)
    sim.camera_maps(h, w, depth_dtype=dtype, mask=mask, **f)
    out = host(sim, b)
    out["boxes"] = boxes.cpu().numpy().copy()
    out.update({"fused_" + k: v for k, v in host(sim, f).items()})
    return out


def all_outputs(sim, group):
    """outputs() at full size, at STRIDE and in float16, and the frames: {(size name, output): host array}."""
    c = rm.case(group)
    out = {("frames", "frames"): sim.frames_host().copy()}
    for tag, (h, w, dtype) in dict(full=(c.H, c.W, "float32"), strided=(c.H // STRIDE[0], c.W // STRIDE[1], "float32"), half=(c.H, c.W, "float16")).items():
        out.update({(tag, k): v for k, v in outputs(sim, h, w, dtype).items()})
    return out


def differing(a, b):
    """{key: number of differing elements} of two all_outputs() results, keys with a difference only."""
    assert set(a) == set(b)
    return {k: int((a[k] != b[k]).sum()) for k in a if a[k].tobytes() != b[k].tobytes()}


@functools.lru_cache(maxsize=None)
def runs(group, kind):
    """The three handles of one (group, source map), each rendered at the current poses once and read out: "primed" (one earlier render),
    "twin" (a fresh handle holding the primed one's state blob: its records of culled triangles were never written), "thrice" (three earlier
    renders from three poses).  Computed once per process; the tests below assert on it."""
    sim = primed(group, kind)
    check_state(sim, group)
    sim.render()
    tw = twin_of(sim, group, kind)
    tw.render()
    out = dict(primed=all_outputs(sim, group), twin=all_outputs(tw, group))
    sim.close(); tw.close()
    sim = primed(group, kind, history=(0, 1, "prime"))
    check_state(sim, group)
    sim.render()
    out["thrice"] = all_outputs(sim, group)
    sim.close()
    c = rm.case(group)
    for e, name in enumerate(rm.names(group)):             # the record: profiles/rerender_parity.txt
        w = rm.predicted(name, kind)
        d = {k: int((out["primed"][("full", k)][e] != out["twin"][("full", k)][e]).sum()) for k in THREE}
        print(f"parity {name} {kind}: {c.H} x {c.W}; predicted wrong: depth {int(w.depth.sum())}, labels {int(w.labels.sum())}, instances {int(w.instances.sum())}; "
              f"primed handle differing from its fresh twin: depth {d['depth']}, labels {d['labels']}, instances {d['instances']}")
    return out


# ---- a. against the oracle ------------------------------------------------------------------------------------------------------------------------

def hold_to_oracle(out, group, kind, who):
    """The full-size and strided maps of one all_outputs() result, single passes and fused, against the models of the current state."""
    c = rm.case(group)
    for e, name in enumerate(rm.names(group)):
        want_d = dm.min_depth(dm.host_buffers(c, e)[0])
        want_d = want_d if kind is None else dm.remap_nearest(want_d, dm.rmap(c.W, c.H, kind))
        want_l, sure_l = lm.expected(c, e, kind)
        want_i, sure_i = im.expected(c, e, kind)
        for tag, (sy, sx) in dict(full=(1, 1), strided=STRIDE).items():
            cut = lambda a: dm.strided(a, sy, sx)
            for pre in ("", "fused_"):
                ctx = (who, name, kind, tag, pre)
                rd = dm.compare(out[(tag, pre + "depth")][e], cut(want_d), TOL, c.cap, ctx)
                rl = lm.compare(out[(tag, pre + "labels")][e], cut(want_l), cut(sure_l), c.cap, ctx)
                ri = im.compare(out[(tag, pre + "instances")][e], cut(want_i), cut(sure_i), c.cap, ctx)
                if tag == "full" and not pre:
                    print(f"oracle {who} {name} {kind}: depth beyond tol {rd['n_beyond']} px (max within {rd['max_within']:.2e}), labels off {rl['n_off']} px, "
                          f"instances off {ri['n_off']} px")
            im.check_boxes_against_oracle(out[(tag, "boxes")][e], cut(want_i), cut(sure_i), (who, name, kind, tag))
            assert np.array_equal(out[(tag, "boxes")][e], im.box_model(out[(tag, "instances")][e])), (who, name, kind, tag)
        # float16: the rounded float32, bit for bit -- and so held to the oracle with it
        import torch
        for pre in ("", "fused_"):
            f32 = torch.from_numpy(out[("full", pre + "depth")][e])
            assert out[("half", pre + "depth")][e].tobytes() == f32.half().numpy().tobytes(), (who, name, kind, pre)
            assert out[("half", pre + "labels")][e].tobytes() == out[("full", pre + "labels")][e].tobytes()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("group", list(rm.GROUPS))
def test_the_maps_after_a_second_render_match_the_oracle(group, kind):
    """depth, labels, instances, boxes and the fused camera_maps of a primed handle, rectilinear and through the fisheye, at full size, at one
    stride and in float16: held to dm.compare, lm.compare, im.compare and im.check_boxes_against_oracle of the current state."""
    hold_to_oracle(runs(group, kind)["primed"], group, kind, "primed")


# ---- b. history independence ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("group", list(rm.GROUPS))
def test_a_primed_handle_gives_its_fresh_twins_bytes(group, kind):
    """The frames and every output of the primed handle equal, byte for byte, those of a fresh handle holding the same state blob; so do those
    of a handle primed three times from three poses; and the twin alone -- whose records of the culled triangles nobody ever wrote -- matches
    the oracle too."""
    r = runs(group, kind)
    assert not differing(r["primed"], r["twin"]), (group, kind, differing(r["primed"], r["twin"]))
    assert not differing(r["thrice"], r["twin"]), (group, kind, differing(r["thrice"], r["twin"]))
    hold_to_oracle(r["twin"], group, kind, "twin")
    for k in THREE:                                         # and one classification: the fused pass is the single passes
        for tag in ("full", "strided", "half"):
            assert r["twin"][(tag, k)].tobytes() == r["twin"][(tag, "fused_" + k)].tobytes(), (group, kind, tag, k)


# ---- c. the masked forms ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("group", ["town", "ped"])
def test_the_masked_forms_after_a_masked_second_render(group):
    """Prime all envs, move all envs, render(mask): the masked depth, labels, instances, boxes and camera_maps give the twin's bytes in the
    selected rows and leave the others their sentinel."""
    import torch
    c = rm.case(group)
    n = len(c.states)
    sim = primed(group)
    sel = torch.tensor([e % 2 == 0 for e in range(n)], dtype=torch.uint8, device="cuda")
    s = sel.cpu().numpy() != 0
    assert s.any() and not s.all()
    sim.render(mask=sel)
    got = outputs(sim, c.H, c.W, mask=sel)
    frames = sim.frames_host().copy()
    sim.close()
    want = runs(group, None)["twin"]
    assert frames[s].tobytes() == want[("frames", "frames")][s].tobytes()
    for k, a in got.items():
        w = want[("full", k)]
        sentinel = BOX_SENTINEL if k == "boxes" else SENTINEL[k.replace("fused_", "")]
        assert (a[~s] == sentinel).all(), (group, k)
        assert a[s].tobytes() == w[s].tobytes(), (group, k, int((a[s] != w[s]).sum()))


# ---- d. a drive -------------------------------------------------------------------------------------------------------------------------------------

class StaleWatch:
    """The model's eye on a handle that renders step after step: per env the passes so far (rerender_model.setup_pass on the read-back state)
    and, at each new pass, how many triangles are stale -- culled now, of an object still live, with a record of an earlier pass."""

    def __init__(self, scene, W, H, n):
        self.scene, self.W, self.H = scene, W, H
        self.hist = [[] for _ in range(n)]

    def look(self, sim):
        stale = 0
        pos, ang = sim.read(_ffi.FIELD_POS), sim.read(_ffi.FIELD_ANGLE)
        for e, hist in enumerate(self.hist):
            cam = raster.Camera(pos[e], float(ang[e]), width=self.W, height=self.H)          # (the shared camera: only its geometry is read)
            cur = rm.setup_pass(cam, self.scene, fp.obj_states(sim, e, self.scene), self.W, self.H)
            stale += sum(int((last >= 0).sum()) for last in rm.stale_triangles(hist, cur))
            hist.append(cur)
        return stale


# env e starts DRIVE_FROM m before object DRIVE_OBJ[group][e] of its map, on a heading of its own, looking DRIVE_TURN past it, and drives on with
# its fixed wheel pair: the object slides out of the frame's side and across the near plane while the handle renders every step
DRIVE_OBJ = dict(ped=(6, 0, 3, 1), town=(3, 2, 0, 3))
DRIVE_FROM, DRIVE_TURN, DRIVE_STEPS, DRIVE_MID = 0.22, (0.30, -0.25, 0.20, -0.35), 30, 15
DRIVE_WHEELS = ((1.0, 0.9), (0.8, 1.0), (1.0, 1.0), (0.9, 0.7))


def drive_states(group):
    g = rm.GROUPS[group]
    poses = [rm.on_line(group, k, DRIVE_FROM, a=0.2 + 0.7 * e, turn=DRIVE_TURN[e]) for e, k in enumerate(DRIVE_OBJ[group])]
    c = dm.Case(g.map_name, g.W, g.H, False, tuple(tuple(p) + dm.DEFAULT_CAM for p in poses), asset_tree=g.asset_tree, mesh=True)
    return c, dm.init_states(c)


def oracle_of_the_device(sim, e, sc, tables, W, H):
    """The expected maps of env e at the state read back from the device (fp.camera, fp.obj_states), by the models' rules on the oracle and
    its nudged self: dict(depth [H, W], labels (map, sure), instances (map, sure)) -- the sure masks as label_model.expected_with and
    instance_model.expected state them."""
    runs = []
    for nudge in (False, True):
        cam = fp.camera(sim, e, W, H, False)
        if nudge:
            pos = sim.read(_ffi.FIELD_POS)[e].astype(np.float32).astype(np.float64) * (1 + 2e-7)
            cam = fp.camera_of_state(sim.init_states[e], pos, float(np.float32(sim.read(_ffi.FIELD_ANGLE)[e])), W, H, False)
        depths, ids = dm.oracle_buffers(cam, sc, fp.obj_states(sim, e, sc))
        srf = dm.surfaces(cam, depths, ids)
        runs.append((depths, srf) + lm.sample_classes_of(cam, sc, tables, depths, srf))
    (d0, s0, c0, same0), (d1, s1, c1, same1) = runs
    agree = (s0 == s0[0]).all(axis=0) & (s1 == s1[0]).all(axis=0) & (s0[0] == s1[0])
    one = (c0 == c0[0]).all(axis=0) & (c1 == c1[0]).all(axis=0) & (c0[0] == c1[0])
    return dict(depth=dm.min_depth(d0), labels=(lm.labels_of(d0, c0).astype(np.uint8), agree & one & same0.all(axis=0) & same1.all(axis=0)),
                instances=(im.instances_of(d0, s0).astype(np.uint8), agree))


@pytest.mark.parametrize("group", ["ped", "town"])
def test_a_drive_past_an_object_gives_a_fresh_twins_bytes_at_every_step(group):
    """loop_pedestrians (its duckies walking) and test_town: four envs drive past an object for DRIVE_STEPS steps, a render and every map after
    each.  After each step the maps equal those of a twin restored from that step's state blob; at the last step and at a mid step depth, labels,
    instances (single passes and fused) and boxes are held to the oracle built from the read-back state (fp.camera, fp.obj_states).  First of all the model must see stale
    triangles at some step of the drive: otherwise it proves nothing."""
    c, states = drive_states(group)
    n, sc, tables = len(c.states), dm.scene_of(rm.case(group)), lm.host_tables(rm.case(group))
    kw = dict(camera_width=c.W, camera_height=c.H, distortion=False, domain_rand=False, seed=1, max_steps=10 ** 6, do_reset=False)
    if c.asset_tree:
        kw["asset_root"] = fp.ASSETS
    sim = BatchedSimulator(c.map_name, n, **kw)
    sim.reset(states=states)
    act = np.array(DRIVE_WHEELS, np.float32)
    watch = StaleWatch(sc, c.W, c.H, n)
    sim.render()
    stale, diffs, held, seen = [watch.look(sim)], [], 0, 0
    for t in range(1, DRIVE_STEPS + 1):
        sim.step(act)
        sim.render()
        got = outputs(sim, c.H, c.W)
        got["frames"] = sim.frames_host().copy()
        stale.append(watch.look(sim))
        tw = BatchedSimulator(c.map_name, n, **kw)         # a twin renders ONCE: every step has a new handle
        tw.reset(states=states)
        tw.write(_ffi.FIELD_STATE_BLOB, sim.read(_ffi.FIELD_STATE_BLOB))
        tw.render()
        want = outputs(tw, c.H, c.W)
        want["frames"] = tw.frames_host().copy()
        tw.close()
        diffs.append({k: int((got[k] != want[k]).sum()) for k in got if got[k].tobytes() != want[k].tobytes()})
        if t in (DRIVE_MID, DRIVE_STEPS):
            for e in range(n):
                want_o = oracle_of_the_device(sim, e, sc, tables, c.W, c.H)
                for pre in ("", "fused_"):
                    ctx = (group, t, e, pre)
                    dm.compare(got[pre + "depth"][e], want_o["depth"], TOL, c.cap, ctx)
                    lm.compare(got[pre + "labels"][e], *want_o["labels"], c.cap, ctx)
                    im.compare(got[pre + "instances"][e], *want_o["instances"], c.cap, ctx)
                im.check_boxes_against_oracle(got["boxes"][e], *want_o["instances"], (group, t, e))
                seen += int((want_o["instances"][0] > 0).sum())
                held += 1
    sim.close()
    print(f"parity drive {group}: stale triangles per step (model, read-back poses) {stale}; elements differing from the fresh twin per step "
          f"{[sum(d.values()) for d in diffs]}")
    assert max(stale) >= 8 and sum(s > 0 for s in stale) >= 2, stale          # the drive culls part of a live object, at more than one step
    assert not any(diffs), [(t + 1, d) for t, d in enumerate(diffs) if d]
    assert held == 2 * n and seen > 100, (held, seen)          # and the oracle's maps of those two steps show objects


# ---- e. per-env tables ------------------------------------------------------------------------------------------------------------------------------

def test_per_env_tables_a_primed_handle_gives_its_fresh_twins_bytes():
    """DTSIM_MAP_ENV_TABLES, two calibrations (camera_rand_maps_model's tables 0 and 5, envs alternating): k_depth<., true>, k_labels<., ., true>
    and the fused pass of a primed handle give a fresh twin's bytes."""
    group = "town"
    c = rm.case(group)
    cal = [0, cm.N_CAL - 1] * (len(c.states) // 2) + [0] * (len(c.states) % 2)
    assert (c.W, c.H) == (cm.W, cm.H)
    sim = make(group, "prime", "fisheye")
    cm.install(sim, cal)
    assert sim._env_tables_flag() == _ffi.MAP_ENV_TABLES
    sim.render()
    move(sim, group)
    sim.render()
    tw = twin_of(sim, group, "fisheye")
    cm.install(tw, cal)
    tw.render()
    a, b = all_outputs(sim, group), all_outputs(tw, group)
    sim.close(); tw.close()
    assert not differing(a, b), differing(a, b)
    assert a[("full", "depth")][0].tobytes() != runs(group, "fisheye")["twin"][("full", "depth")][0].tobytes()      # the tables took effect
    assert (a[("full", "instances")] > 0).any()


# ---- f. LEDs ----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("group", list(rm.GROUPS))
def test_draw_leds_after_a_second_render(group):
    """dtsim_draw_leds on a primed handle: first each pair's hidden sphere alone -- on the ray through the middle of the pixels a stale reader
    gets wrong, between the stale surface and the real one, so that such a reader hides it --, then, on a new render, that sphere with the usual
    set of tests/led_model.py.  Both times the frames equal the fresh twin's byte for byte and are held to raster.overlay_leds on the oracle's
    depth buffers within tests/test_gpu_leds.py's share of the touched pixels."""
    c = rm.case(group)
    names = rm.names(group)
    sim = primed(group)
    tw = twin_of(sim, group)
    lists = {"hidden": [rm.led_spheres(n)[:1] for n in names],
             "with the usual set": [rm.led_spheres(n) for n in names]}
    for what, sps in lists.items():
        idx = np.repeat(np.arange(len(names)), [len(s) for s in sps])
        frames = {}
        for who, h in (("primed", sim), ("twin", tw)):
            h.render()
            before = h.frames_host().copy()
            h.draw_leds(np.concatenate(sps), idx)
            frames[who] = (before, h.frames_host().copy())
        assert frames["primed"][0].tobytes() == frames["twin"][0].tobytes(), (group, what)
        n_diff = int((frames["primed"][1] != frames["twin"][1]).any(-1).sum())
        print(f"parity leds {group} {what}: pixels differing from the fresh twin after the pass {n_diff}")
        assert n_diff == 0, (group, what, n_diff)
        before, after = frames["primed"]
        for e, name in enumerate(names):
            want = raster.overlay_leds(before[e], dm.host_camera(c, e), list(dm.host_buffers(c, e)[0]), sps[e])
            touched = (want != before[e]).any(-1)
            bad = np.abs(after[e].astype(int) - want.astype(int)).max(-1) > 1
            print(f"leds {name} {what}: touched {int(touched.sum())} px, off by more than 1: {int(bad.sum())} (share {rm.led_share(touched.sum()):.1f})")
            assert touched.sum() >= (40 if what == "hidden" else 150), (name, what, int(touched.sum()))
            assert bad.sum() <= rm.led_share(touched.sum()), (name, what, int(bad.sum()), int(touched.sum()))
    sim.close(); tw.close()


# ---- g. the vector env ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("group", ["ped", "town"])
def test_the_vector_env_single_passes_are_the_fused_pass_through_a_drive(group):
    """DuckietownVecEnv with depth_shape, label_shape, instance_shape and boxes, and a second env with fused_maps=True, on one seed, put on (d)'s
    start poses and driven by (d)'s wheel pairs: the info maps are equal byte for byte at every step (the single passes read what the fused
    pass reads), and the model sees stale triangles on the way."""
    import torch
    c, states = drive_states(group)
    n, sc = len(c.states), dm.scene_of(rm.case(group))
    shape = (c.H // 2, c.W // 2)
    kw = dict(obs_shape=(24, 32), depth_shape=shape, label_shape=shape, instance_shape=shape, boxes=True, domain_rand=False, distortion=False,
              max_steps=10 ** 6, seed=4, action_mode="wheels", camera_width=c.W, camera_height=c.H)
    if c.asset_tree:
        kw["asset_root"] = fp.ASSETS
    A, B = DuckietownVecEnv(c.map_name, n, **kw), DuckietownVecEnv(c.map_name, n, fused_maps=True, **kw)
    A.reset(); B.reset()
    for env in (A, B):
        env.sim.write(_ffi.FIELD_POS, np.array([list(st.pos) for st in states], np.float64))
        env.sim.write(_ffi.FIELD_ANGLE, np.array([st.angle for st in states], np.float64))
    act = torch.tensor(DRIVE_WHEELS, dtype=torch.float32, device="cuda")
    watch = StaleWatch(sc, c.W, c.H, n)
    stale, diffs = [], []
    for t in range(DRIVE_STEPS + 1):
        _, _, _, ia = A.step(act)
        _, _, _, ib = B.step(act)
        torch.cuda.synchronize()
        A.sim.sync(); B.sim.sync()
        stale.append(watch.look(A.sim))
        diffs.append({k: int((ia[k] != ib[k]).sum()) for k in ("depth", "labels", "instances", "boxes")
                      if not torch.equal(ia[k].contiguous().view(torch.uint8), ib[k].contiguous().view(torch.uint8))})
        assert np.array_equal(A.sim.read(_ffi.FIELD_STATE_BLOB), B.sim.read(_ffi.FIELD_STATE_BLOB)), t
    seen = int((ia["instances"] > 0).sum())
    A.close(); B.close()
    print(f"parity vecenv {group}: stale triangles per step {stale}; elements differing between single and fused passes per step {[sum(d.values()) for d in diffs]}")
    assert max(stale) >= 8 and seen > 0, (stale, seen)
    assert not any(diffs), [(t, d) for t, d in enumerate(diffs) if d]
