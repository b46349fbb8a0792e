"""GPU: DuckietownVecEnv(camera_rand=True, camera_rand_maps=True, distortion=True, depth_shape=..., label_shape=..., instance_shape=...,
boxes=True) -- every env's maps go through its own distortion table.  obs, reward, done and the other info entries are bit-identical to the same env built without the
map options; every info[...] map, and with final_obs=True every final_ twin on the rows of the envs that finished, is byte for byte what the
literal call sequence gives on a second BatchedSimulator driven by hand (render -> depth -> instances with the label map -> boxes, before
and after reset_done); motion_blur with a map option still raises ValueError, and so does camera_rand without camera_rand_maps.
160 x 120 cameras, N = 72 (a full chunk of the passes' env loop and a tail), max_steps = 3: every env finishes."""
import pytest

from dtsim import BatchedSimulator, DuckietownVecEnv, _ffi

pytestmark = pytest.mark.gpu

MAP, N, STEPS, MAX_STEPS = "loop_pedestrians", 72, 7, 3
SHAPE = (30, 40)
KW = dict(camera_rand=True, distortion=True, domain_rand=False, camera_width=160, camera_height=120, max_steps=MAX_STEPS)
MAPS = ("depth", "labels", "instances", "boxes")


@pytest.mark.parametrize("final", [True, False])
def test_the_maps_ride_with_the_observation_under_camera_rand(final):
    import torch
    A = DuckietownVecEnv(MAP, N, obs_shape=(24, 32), seed=4, depth_shape=SHAPE, label_shape=SHAPE, instance_shape=SHAPE, boxes=True,
                         final_obs=final, camera_rand_maps=True, **KW)
    B = DuckietownVecEnv(MAP, N, obs_shape=(24, 32), seed=4, final_obs=final, **KW)
    ref = BatchedSimulator(MAP, N, action_mode="vel_steer", seed=4, device_reset=True, auto_reset=False, do_reset=False, **KW)
    assert A.sim.camera_calibrations is not None and len(set(A.sim.camera_calibrations[3].tolist())) > 1       # a table per env
    new_keys = set(MAPS) | {"final_" + k for k in MAPS}
    lab = torch.zeros((N, *SHAPE), dtype=torch.uint8, device="cuda")

    def ref_pass():
        ref.render()
        d = ref.depth(*SHAPE)
        i = ref.instances(*SHAPE, labels_out=lab)             # the shapes agree: one launch fills both maps
        b = ref.boxes(i)
        ref.sync()
        return dict(depth=d.clone(), labels=lab.clone(), instances=i.clone(), boxes=b.clone())

    def same(x, y):
        return x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))

    oa, ob = A.reset(), B.reset()
    ref.reset()
    torch.cuda.synchronize()
    assert same(oa, ob) and all(getattr(B, k) is None for k in MAPS)
    first = ref_pass()
    for k in MAPS:
        assert same(getattr(A, k), first[k]), k                # the first frames' maps: env.depth, env.labels, ...
    assert A.depth.shape == (N, *SHAPE) and A.boxes.shape == (N, _ffi.MAX_OBJECTS, 5)
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    n_done, n_seen = torch.zeros(N, device="cuda"), int(first["instances"].any())
    for t in range(STEPS):
        a = torch.rand((N, 2), device="cuda", generator=g) * 2 - 1
        oa, ra, da, ia = A.step(a)
        ob, rb, db, ib = B.step(a)
        torch.cuda.synchronize()
        ref.step(a)                                          # by hand: step -> render -> passes -> reset_done -> render -> passes
        before = ref_pass()
        ref_done = torch.as_tensor(ref.field_device(_ffi.FIELD_DONE), device="cuda").to(torch.bool).clone()
        ref.reset_done()
        after = ref_pass()
        # everything the env without the map options returns: bit-identical
        assert same(oa, ob) and same(ra, rb) and same(da, db) and torch.equal(da, ref_done), t
        assert set(ia) - new_keys == set(ib) and not (set(ib) & new_keys), (sorted(ia), sorted(ib))
        for key in ib:
            if key == "final_obs":
                assert same(ia[key][da], ib[key][db]), (t, key)
            else:
                assert same(ia[key], ib[key]), (t, key)
        for k in MAPS:
            assert ia[k] is getattr(A, k)                    # one persistent tensor
            assert same(ia[k], after[k]), (t, k)             # byte for byte, the restarted envs' first frames included
            assert same(after[k][~da], before[k][~da]), (t, k)
            if final:
                assert ia["final_" + k].shape == ia[k].shape and same(ia["final_" + k][da], before[k][da]), (t, k, int(da.sum()))
            else:
                assert "final_" + k not in ia
        n_seen += int(after["instances"].any())
        n_done += da.float()
    assert float(n_done.min()) >= 2                          # every env finished at least twice
    assert n_seen > 0                                        # a duckie was in view at some step
    for e in (A, B):
        e.close()
    ref.close()


@pytest.mark.parametrize("kw", [dict(depth_shape=SHAPE), dict(label_shape=SHAPE), dict(instance_shape=SHAPE, boxes=True)])
def test_motion_blur_with_a_map_option_still_raises(kw):
    with pytest.raises(ValueError, match="motion_blur"):
        DuckietownVecEnv(MAP, 4, obs_shape=(24, 32), motion_blur=True, action_mode="wheels", camera_rand_maps=True, **kw, **KW)
    with pytest.raises(ValueError, match="camera_rand_maps"):
        DuckietownVecEnv(MAP, 4, obs_shape=(24, 32), **kw, **KW)                   # the opt-in left out: refused as before
