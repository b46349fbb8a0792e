"""The conditions tests/test_gpu_rerender_maps.py rests on, asserted on the host (tests/rerender_model.py): every (prime pose, current pose) pair
would show a reader of stale ScreenTri records far more wrong pixels than the comparisons' caps forgive -- so that an unfixed kernel cannot hide
under them --, while the oracle itself stays as steady at the current poses as at the poses of dm.CASES, so that no tolerance has to move.
They are conditions, not measurements: a pair that misses one is replaced in rerender_model.PAIRS, never excused here."""
import numpy as np
import pytest

import depth_model as dm
import instance_model as im
import label_model as lm
import rerender_model as rm
from oracle import raster

KINDS = (None, "fisheye")


def test_the_pairs_stay_out_of_the_models_case_tables():
    import flow_model as fm
    cases = {rm.case(g, w) for g in rm.GROUPS for w in ("prime", "cur", 0, 1)}
    for table in (dm.CASES, lm.CASES):
        assert not cases & set(table.values())
    assert not cases & {c.dm_case for c in im.CASES.values()}
    assert not cases & {fm.case_of(n) for n in fm.CASES}
    assert set(rm.GROUPS) == {p.group for p in rm.PAIRS.values()}
    assert any(rm.GROUPS[p.group].map_name == "loop_pedestrians" for p in rm.PAIRS.values())       # a walking-duckie map is among them
    assert any((rm.GROUPS[p.group].W, rm.GROUPS[p.group].H) == (90, 62) for p in rm.PAIRS.values())  # and the odd size


def test_the_setup_model_culls_as_the_oracle_draws():
    """The model's float32 survive rule against the same rule stated in float64 on the oracle's own projection (raster.render_rectilinear's
    w, sx, sy), at every pose of every group: every vertex w > NEAR, area not 0, the box padded by DT_TRI_PAD meeting the frame.  The two agree
    on EVERY triangle that does not sit on a threshold (a w within 1e-5 of NEAR, a box edge within 1e-3 px of the frame's, an area under 1e-6
    px^2), those are few, and an object is live exactly when one of its triangles survives: the frustum cull never takes a survivor away."""
    checked = on_edge = 0
    for g in rm.GROUPS:
        for which in ("prime", "cur", 0, 1):
            c = rm.case(g, which)
            sc = dm.scene_of(c)
            for e in range(len(c.states)):
                cam = dm.host_camera(c, e)
                ps = rm.passes(g, which)[e]
                assert len(ps) == len(sc.m.objects)
                for (Vw, *_rest, k) in raster._object_instances(sc, dm.host_objects(c)[e]):
                    Pe = cam.to_eye(Vw)
                    w = -Pe[..., 2]
                    with np.errstate(divide="ignore", invalid="ignore"):
                        sx = (Pe[..., 0] / w / cam.tx + 1) * 0.5 * c.W
                        sy = (1 - Pe[..., 1] / w / cam.ty) * 0.5 * c.H
                        area = (sx[:, 1] - sx[:, 0]) * (sy[:, 2] - sy[:, 0]) - (sx[:, 2] - sx[:, 0]) * (sy[:, 1] - sy[:, 0])
                    near = (w > raster.NEAR).all(axis=1)
                    box = np.stack([sx.min(axis=1) - 0.5, sx.max(axis=1) + 0.5, sy.min(axis=1) - 0.5, sy.max(axis=1) + 0.5], axis=1)
                    with np.errstate(invalid="ignore"):
                        meets = ~((box[:, 1] < 0) | (box[:, 0] > c.W) | (box[:, 3] < 0) | (box[:, 2] > c.H))
                        edge = (np.abs(w - raster.NEAR).min(axis=1) < 1e-5) | (near & (np.abs(area) < 1e-6)) | (near & (
                            (np.abs(box[:, 1]) < 1e-3) | (np.abs(box[:, 0] - c.W) < 1e-3) | (np.abs(box[:, 3]) < 1e-3) | (np.abs(box[:, 2] - c.H) < 1e-3)))
                        want = near & (area != 0) & meets
                    assert np.array_equal(ps[k].ok[~edge], want[~edge]), (g, which, e, k, np.flatnonzero(ps[k].ok != want))
                    assert ps[k].live == bool(ps[k].ok.any()) and (ps[k].live or not want[~edge].any()), (g, which, e, k)
                    checked += int((~edge).sum()); on_edge += int(edge.sum())
    print(f"{checked} triangles agree, {on_edge} sit on a threshold")
    assert checked > 5000 and on_edge <= 0.01 * checked, (checked, on_edge)
    # an object out of view is not live: nothing of it is ever tested
    assert sum(not o.live for o in rm.passes("town", "cur")[0]) >= 2


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(rm.PAIRS))
def test_a_stale_reader_cannot_hide_under_the_caps(name, kind):
    p = rm.PAIRS[name]
    g = rm.GROUPS[p.group]
    w = rm.predicted(name, kind)
    print(f"{name} {kind}: stale {w.stale} / {w.tris} triangles; predicted wrong pixels: depth {int(w.depth.sum())}, labels {int(w.labels.sum())}, "
          f"instances {int(w.instances.sum())}")
    assert 0 < w.stale < w.tris
    assert w.depth.sum() >= 3 * dm.CAP_MESH * g.H * g.W, (name, kind, int(w.depth.sum()))
    assert w.labels.sum() >= 20 and w.instances.sum() >= 20, (name, kind)
    # more earlier passes change nothing of the condition: the record that stands is the last survivor's
    w3 = rm.predicted(name, kind, (0, 1, "prime"))
    assert w3.depth.sum() >= 3 * dm.CAP_MESH * g.H * g.W and w3.stale >= w.stale


@pytest.mark.parametrize("name", list(rm.PAIRS))
def test_the_oracle_is_steady_at_the_current_poses(name):
    """The oracle against its nudged self at the pair's current pose: inside the tolerance and caps tests/test_gpu_depth.py,
    test_gpu_labels.py and test_gpu_instances.py read, every sure pixel exact."""
    p = rm.PAIRS[name]
    e, c = rm.env_of(name), rm.case(p.group)
    r = dm.nudge_stats(c, e, dm.INV_DEPTH_TOL)
    rl, ri = lm.nudge_share(c, e), im.nudge_share(c, e)
    print(f"{name}: oracle vs nudged oracle: depth beyond {r['beyond']:.2e}, labels off {rl['n_off']} px, instances off {ri['n_off']} px (cap {c.cap:.1e})")
    assert c.cap == dm.CAP_MESH
    assert r["beyond"] <= dm.CAP_MESH
    assert rl["off"] <= c.cap and rl["sure_off"] == 0
    assert ri["off"] <= c.cap and ri["sure_off"] == 0
    for kind in KINDS:                               # and the expected maps hold what the wrong pixels are counted against
        assert lm.expected(c, e, kind)[1].mean() > 0.8 and im.expected(c, e, kind)[1].mean() > 0.8


@pytest.mark.parametrize("name", list(rm.PAIRS))
def test_the_hidden_sphere_is_worth_three_shares(name):
    """dtsim_draw_leds: the sphere placed between the stale surface and the real one loses, under a stale reader, three times the pixels
    tests/test_gpu_leds.py's share (0.04 x touched + 4) forgives -- of the call that draws IT ALONE, which is why
    tests/test_gpu_rerender_maps.py draws it alone first and with the usual set of tests/led_model.py after.  Beside that set no single
    sphere can be worth three shares: at these close poses the set touches 1000 to 6300 pixels (a sphere through an object 12 cm away fills a
    quarter of the frame), three shares of that are 130 to 770 pixels, and the whole stale region of "bot_left" is 503 (printed below)."""
    sphere, (y, x) = rm.hidden_sphere(name)
    p = rm.PAIRS[name]
    e, c = rm.env_of(name), rm.case(p.group)
    hidden, shown = rm.hidden_pixels(name, sphere)
    black = np.zeros((c.H, c.W, 3), np.uint8)
    touched = raster.overlay_leds(black, dm.host_camera(c, e), list(dm.host_buffers(c, e)[0]), rm.led_spheres(name)).any(-1)
    print(f"{name}: hidden sphere r = {sphere[3]:.4f} m at pixel ({y}, {x}): {int(hidden.sum())} of its {int(shown.sum())} pixels hidden, share "
          f"{rm.led_share(shown.sum()):.1f}; with the usual set the spheres touch {int(touched.sum())}, share {rm.led_share(touched.sum()):.1f}")
    assert shown[y, x] and np.array_equal(sphere, rm.led_spheres(name)[0])
    assert hidden.sum() >= 3 * rm.led_share(shown.sum()), (name, int(hidden.sum()), int(shown.sum()))
