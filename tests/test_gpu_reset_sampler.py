"""GPU: the device-side reset sampler (csrc/physics.hip sample_init and the `rs` branches of apply_init / duckie_step, on
csrc/philox_rng.h) against tests/reset_sampler_model.py -- the device's own Philox stream restated in numpy -- and, for the spawn pose,
against the oracle's acceptance test over the model's candidates.

What is exact: every sampled field that does not pass through log / cos (camera, colours, wheel distance, episode, visibility, tile
choice, every spawn candidate, object wait / wiggle / follower parameters, map ids).  What has a bound: the Box-Muller normal (trim ->
war / wal, a duckie's |vel|), where ocml's log and cos meet glibc's: |delta| <= scale * 1e-13 (both sides take the same correctly rounded
sqrt and the same IEEE product 2 pi u2; with k ulps of error in log and cos each, |delta z| <= (k + 2) * 2^-53 * 8.6, about 6e-15 at
k = 4: the bound leaves a factor of 16, and is twelve orders below the spread).

An env is judged SURE when the oracle's verdict on every candidate up to the accepted one is the same on the pose as drawn and on the
pose scaled by 1 + 1e-9; tests/test_reset_sampler_model_host.py caps the unsure envs at 1 % (there are none).  The cases, the judged env
subset and the oracle's verdicts are computed here without the device and shared with that file.

Two departures from the plain reading of the plan, both forced by the C ABI: dtsim_set_reset_sampler refuses accept_start_angle_deg = 0,
so the sampler that accepts nothing carries the smallest positive double (it would take a lane angle of exactly 0 degrees); and
DTSIM_LUTS_CAMERA_RAND needs a rendering handle, so the camera_rand case alone is created with render=True (it never renders)."""
import copy
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import reset_sampler_model as RM
from dtsim import BatchedSimulator, _ffi, assets, maps as dmaps
from test_gpu_step_lanes import N_LANES_1, N_LANES_2, N_LANES_4, SIZES
from test_state_fields_host import ARRAYS, expected_offsets

pytestmark = pytest.mark.gpu

SEED = (0x5EED << 32) + 20240611                       # above 2^32: the key's high word is in play
NORMAL_TOL = 1e-13                                      # times the scale of the normal (module docstring)
PHYSICS_TOL = 1e-9                                      # tests/test_gpu_physics.py FLOAT_TOL
UNSURE_SCALE = 1.0 + 1e-9
TINY_ACCEPT = 5e-324                                    # the smallest positive double: accepts a lane angle of exactly 0 only


# ---------------------------------------------------------------- cases, shared with the host test (no device below this line until the tests)
def map_data(key):
    if key == "junctions_optional":                     # as test_reset_tile_and_pose_branches_match_oracle[optional]
        from util import junction_map
        md = junction_map()
        md["tiles"] = [[("grass" if c == "empty" else c) for c in row] for row in md["tiles"]]
        return md
    if key == "small_loop_start_pose":
        md = assets.get_map("small_loop")
        md["start_tile"], md["start_pose"] = [1, 2], [[0.35, 0.0, 0.29], 1.5707]
        return md
    return assets.get_map(key)


@functools.lru_cache(maxsize=None)
def map_tables(key):
    return dmaps.interpret_map(map_data(key), key, {"duckie": assets.get_mesh("duckie"), "*": assets.get_mesh("*")})


# (map, N, accept_start_angle_deg, max_attempts judged by the oracle)
POSE_CASES = [(m, n, 60.0) for m in ("small_loop", "loop_pedestrians", "junctions_optional") for n in SIZES] + [("small_loop", N_LANES_4, 4.0)]
POSE_IDS = [f"{m}-N{n}-accept{a:g}" for m, n, a in POSE_CASES]
POSE_EPISODES = (1, 2)
EXHAUST_CASE = ("small_loop", N_LANES_4, TINY_ACCEPT)
EXHAUST_JUDGED = (0, N_LANES_4 - 1)                     # the oracle walks all 5000 candidates of these two; the device test holds all 33 to the fallback
DRAW_CASES = [("dr", n) for n in SIZES] + [("no_dr", N_LANES_4), ("camera_rand", N_LANES_4)]


def judged_envs(N):
    """0 .. 32, the last 33, and 16 on each side of 8192 where the batch reaches it"""
    s = set(range(33)) | set(range(N - 33, N))
    if N > 8192:
        s |= set(range(8192 - 16, min(N, 8192 + 16)))
    return np.array(sorted(s))


def oracle_accepts(o, x, z, a, accept):
    """the spawn loop's acceptance test (simulator.py:692-738) on one pose"""
    from oracle import sim as osim
    pos = np.array([x, 0.0, z])
    if o._inconvenient_spawn(pos) or not o._valid_pose(pos, a, safety_factor=1.3):
        return False
    try:
        lp = o.get_lane_pos2(pos, a)
    except osim.NotInLane:
        return False
    return bool(-accept < lp[2] < accept)


@functools.lru_cache(maxsize=None)
def judged(map_key, N, accept, envs=None, episodes=POSE_EPISODES):
    """Per episode, for the judged envs of the case: the model's reset (`res`), and from the oracle's acceptance test over the model's
    candidates -- with the model's visibility on the oracle's objects -- `first` (the index of the first accepted candidate, -1: none in
    max_attempts), `pose` (x, z, angle of it, or the fallback) and `unsure` (a verdict up to `first` changes under the 1 + 1e-9 scaling)."""
    from oracle import sim as osim
    from util import EXT
    mt = map_tables(map_key)
    cfg = RM.SamplerCfg.for_map(mt, domain_rand=True, accept_start_angle_deg=accept)
    env = judged_envs(N) if envs is None else np.array(envs)
    o = osim.OracleSim(copy.deepcopy(map_data(map_key)), EXT, domain_rand=True, do_reset=False)
    out = {}
    for ep in episodes:
        res = RM.sample_reset(SEED, env, ep, mt, cfg)
        first, unsure = np.full(env.size, -1), np.zeros(env.size, bool)
        pose = np.tile(np.array(RM.FALLBACK_POSE), (env.size, 1))
        CH = 64
        for k0 in range(0, cfg.max_attempts, CH):
            rows = np.flatnonzero(first < 0)
            if rows.size == 0:
                break
            cand = res["candidates"](k0, min(k0 + CH, cfg.max_attempts))
            for r in rows:
                for ob, v in zip(o.map.objects, res["visible"][r]):
                    ob.visible = bool(v)
                for k, (x, z, a) in enumerate(cand[r]):
                    ok = oracle_accepts(o, x, z, a, accept)
                    unsure[r] |= ok != oracle_accepts(o, x * UNSURE_SCALE, z * UNSURE_SCALE, a * UNSURE_SCALE, accept)
                    if ok:
                        first[r], pose[r] = k0 + k, (x, z, a)
                        break
        out[ep] = SimpleNamespace(env=env, res=res, first=first, pose=pose, unsure=unsure, oracle=o)
    return out


# ---------------------------------------------------------------- the device
def make_sim(map_key, N, *, dr=True, accept=60.0, seed=SEED, **kw):
    kw.setdefault("render", False)
    return BatchedSimulator(map_key, N, map_data=map_data(map_key), domain_rand=dr, seed=seed, device_reset=True, accept_start_angle_deg=accept, **kw)


def bytes_of(a):
    a = np.ascontiguousarray(a)
    return a.reshape(a.shape[0], -1).view(np.uint8)


def first_bad(a, b):
    bad = (bytes_of(a) != bytes_of(b)).any(axis=1)
    return int(np.flatnonzero(bad)[0]) if bad.any() else None


def blob_array(sim, name):
    """array `name` of DTSIM_FIELD_STATE_BLOB as [planes, N], through the ARRAYS table"""
    N = sim.num_envs
    off, total = expected_offsets(N)
    blob = sim.read(_ffi.FIELD_STATE_BLOB)
    assert blob.size == total
    dt, planes = next((d, p) for n, d, p in ARRAYS if n == name)
    return blob[off[name]:off[name] + N * planes * np.dtype(dt).itemsize].view(dt).reshape(planes, N)


def read_draws(sim):
    d = {f: sim.read(getattr(_ffi, "FIELD_" + f)) for f in ("CAMERA", "COLORS", "WHEEL_DIST", "EPISODE", "OBJ_VISIBLE", "POS", "ANGLE")}
    d["war"], d["wal"] = blob_array(sim, "war")[0].copy(), blob_array(sim, "wal")[0].copy()
    return d


def assert_draws(dev, model, episode, envs=None, who=""):
    """the sampled fields of the device (read_draws) against sample_reset's for the rows `envs` (None: all); returns the largest
    |device - model| of war / wal, to be held to NORMAL_TOL by the caller's assertion here"""
    sel = slice(None) if envs is None else envs
    n_obj = model["visible"].shape[1]
    for name, got, want in (("cam", dev["CAMERA"][sel], model["cam"]), ("colors", dev["COLORS"][sel], model["colors"]),
                            ("wheel_dist", dev["WHEEL_DIST"][sel], model["wheel_dist"]),
                            ("visible", dev["OBJ_VISIBLE"][sel][:, :n_obj], model["visible"])):
        assert got.dtype == want.dtype, (name, got.dtype, want.dtype)
        bad = first_bad(got, want)
        assert bad is None, (who, name, "first env row", bad, got[bad], want[bad])
    assert (dev["OBJ_VISIBLE"][sel][:, n_obj:] == 1).all()
    assert (np.broadcast_to(dev["EPISODE"][sel], model["trim"].shape) == episode).all(), who
    err = max(np.abs(dev["war"][sel] - model["war"]).max(), np.abs(dev["wal"][sel] - model["wal"]).max())
    assert err <= 15.0 * 0.02 * NORMAL_TOL, (who, "war / wal", err)       # war = 15 (1 + trim), trim ~ N(0, 0.02)
    return err


@functools.lru_cache(maxsize=None)
def draw_run(kind, N):
    """three full resets and one masked reset: the sampled fields after each, [(episode per env, mask, fields)]"""
    kw = {"dr": dict(dr=True), "no_dr": dict(dr=False), "camera_rand": dict(dr=False, camera_rand=True, distortion=True, render=True,
                                                                            camera_width=160, camera_height=120)}[kind]
    sim = make_sim("small_loop", N, dynamics_rand=True, **kw)
    assert bool(sim.camera_rand_on) == (kind == "camera_rand")
    cfg = RM.SamplerCfg.from_ffi(sim._sampler)
    assert cfg == RM.SamplerCfg.for_map(sim.maps[0], domain_rand=kw["dr"], dynamics_rand=True, accept_start_angle_deg=60.0), "install_reset_sampler's rule"
    out = [(1, None, read_draws(sim))]
    for ep in (2, 3):
        sim.reset()
        out.append((ep, None, read_draws(sim)))
    mask = (np.arange(N) % 3 != 1)
    mask[-1] = True
    sim.reset(mask)
    out.append((4, mask, read_draws(sim)))
    sim.close()
    return SimpleNamespace(runs=out, cfg=cfg, camera_rand=kind == "camera_rand")


@pytest.mark.parametrize("kind,N", DRAW_CASES, ids=[f"{k}-N{n}" for k, n in DRAW_CASES])
def test_draws_match_the_model_on_every_env(kind, N):
    run = draw_run(kind, N)
    mt, env, worst = map_tables("small_loop"), np.arange(N), 0.0
    prev = None
    for ep, mask, dev in run.runs:
        if mask is None:
            model = RM.sample_reset(SEED, env, ep, mt, run.cfg, run.camera_rand)
            worst = max(worst, assert_draws(dev, model, ep, who=f"{kind} N={N} episode {ep}"))
        else:
            model = RM.sample_reset(SEED, env[mask], ep, mt, run.cfg, run.camera_rand)
            worst = max(worst, assert_draws(dev, model, ep, np.flatnonzero(mask), who=f"{kind} N={N} masked episode {ep}"))
            for f in dev:                                   # the others keep episode 3's values
                assert first_bad(dev[f][~mask], prev[f][~mask]) is None, f
        prev = dev
    print(f"{kind} N={N}: max |war, wal - model| {worst:.3e} (bound {15.0 * 0.02 * NORMAL_TOL:.1e}); as trim: {worst / 15.0:.3e}")
    if kind == "no_dr":                                     # nothing perturbed, the camera unscaled, the noise still drawn
        dev = run.runs[0][2]
        assert (dev["WHEEL_DIST"] == 0.102).all() and (dev["COLORS"][:, 12:16] == [0, 3, 0, 1]).all() and dev["CAMERA"][:, 3:].any()
    if kind == "camera_rand":                               # the camera scaled without domain randomisation, its noise zeroed
        dev = run.runs[0][2]
        assert not dev["CAMERA"][:, 3:].any() and len(np.unique(dev["CAMERA"][:, 0])) > N // 2 and (dev["WHEEL_DIST"] == 0.102).all()


def test_lane_count_and_batch_position_change_no_draw():
    """env e < 33 with seed s: identical sampled fields (the spawn pose included) at 4, 2 and 1 lanes per env"""
    ref = draw_run("dr", N_LANES_4).runs
    for N in (N_LANES_2, N_LANES_1):
        for (ep, _, a), (_, _, b) in zip(ref, draw_run("dr", N).runs):
            for f in a:
                assert first_bad(a[f][:33], b[f][:33]) is None, (N, ep, f, first_bad(a[f][:33], b[f][:33]))     # (the masked reset takes the same envs below 33)


@pytest.mark.parametrize("map_key,N,accept", POSE_CASES, ids=POSE_IDS)
def test_pose_is_the_first_candidate_the_oracle_accepts(map_key, N, accept):
    J = judged(map_key, N, accept)
    sim = make_sim(map_key, N, accept=accept)
    n_unsure = 0
    lane_err = 0.0
    for ep in POSE_EPISODES:
        j = J[ep]
        if ep > 1:
            sim.reset()
        cen = sim.read(_ffi.FIELD_OBJ_CENTER)[j.env]       # the objects the spawn test looked at: nothing has stepped, so the oracle's own
        dyn = [ob for ob in j.oracle.map.objects if not ob.static]
        for d, ob in enumerate(dyn):
            assert (cen[:, d, 0] == ob.pos[0]).all() and (cen[:, d, 1] == ob.pos[2]).all(), (ep, d)
        dev = read_draws(sim)
        assert_draws(dev, j.res, ep, j.env, who=f"{map_key} N={N} episode {ep}")
        got = np.stack([dev["POS"][j.env, 0], dev["POS"][j.env, 2], dev["ANGLE"][j.env]], axis=1)
        assert (dev["POS"][:, 1] == 0).all()
        tile, lane, in_lane = sim.read(_ffi.FIELD_TILE)[j.env], sim.read(_ffi.FIELD_LANE)[j.env], sim.read(_ffi.FIELD_IN_LANE)[j.env]
        deep = int(j.first.max()) + 1
        cand = j.res["candidates"](0, deep)
        for r, e in enumerate(j.env):
            member = np.flatnonzero((bytes_of(cand[r]) == bytes_of(got[r:r + 1])).all(axis=1))
            assert member.size, (ep, int(e), "the device's pose is none of the model's candidates", got[r])
            if j.unsure[r]:
                n_unsure += 1
                continue
            assert member[0] == j.first[r], (ep, int(e), "device took candidate", int(member[0]), "the oracle accepts", int(j.first[r]))
            pos = np.array([got[r, 0], 0.0, got[r, 1]])
            assert tuple(tile[r]) == tuple(j.oracle.map.get_grid_coords(pos)) and in_lane[r] == 1
            lp = j.oracle.get_lane_pos2(pos, got[r, 2])
            lane_err = max(lane_err, np.abs(lane[r] - np.array(lp)).max())
    sim.close()
    print(f"{map_key} N={N} accept {accept:g}: {len(J[1].env)} envs x {len(POSE_EPISODES)} episodes judged, unsure {n_unsure}, "
          f"deepest accepted attempt {max(int(J[ep].first.max()) for ep in POSE_EPISODES) + 1}, max |lane - oracle| {lane_err:.3e}")
    assert lane_err <= PHYSICS_TOL


def test_exhausted_attempts_fall_back_with_the_draws_intact():
    """a sampler that accepts nothing: every env at the fallback pose (1, 0, 1), angle 1.0 (simulator.py:732-736), after all 5000 attempts"""
    map_key, N, accept = EXHAUST_CASE
    sim = make_sim(map_key, N)
    sim._sampler.accept_start_angle_deg = accept
    _ffi.check(sim._lib, sim._lib.dtsim_set_reset_sampler(sim._h, C.byref(sim._sampler)))
    sim.reset()
    dev = read_draws(sim)
    cfg = RM.SamplerCfg.from_ffi(sim._sampler)
    assert cfg.accept_start_angle_deg == accept and cfg.max_attempts == 5000
    assert_draws(dev, RM.sample_reset(SEED, np.arange(N), 2, sim.maps[0], cfg), 2, who="exhausted")
    assert (dev["POS"] == [1.0, 0.0, 1.0]).all() and (dev["ANGLE"] == 1.0).all()
    sim.close()


def test_start_pose_map_spawns_there_with_the_draws_intact():
    """simulator.py:679-688 on the device sampler (tests/test_gpu_device_reset.py's check), plus the draws: no spawn loop runs"""
    N = N_LANES_4
    sim = make_sim("small_loop_start_pose", N)
    mt = sim.maps[0]
    cfg = RM.SamplerCfg.from_ffi(sim._sampler)
    assert cfg.start_tile == (1, 2) and cfg.start_pose == (0.35, 0.29, 1.5707)
    for ep in (1, 2):
        if ep > 1:
            sim.reset()
        dev = read_draws(sim)
        model = RM.sample_reset(SEED, np.arange(N), ep, mt, cfg)
        assert_draws(dev, model, ep, who="start_pose")
        assert np.allclose(dev["POS"], [1 * 0.585 + 0.35, 0.0, 2 * 0.585 + 0.29], atol=1e-12) and np.allclose(dev["ANGLE"], 1.5707)
        assert np.array_equal(dev["POS"][:, [0, 2]], model["fixed_pose"][:, :2]) and np.array_equal(dev["ANGLE"], model["fixed_pose"][:, 2])
    sim.close()


@pytest.mark.parametrize("N", SIZES)
def test_auto_reset_in_k_step_equals_reset_after_step(N):
    """k_step<true, L>'s auto reset against k_reset: handle A restarts at the top of steps 2, 3 and 4 of one fused launch (max_steps = 1),
    handle B steps, then resets the done envs from the host.  Same state, byte for byte: a reset depends on (seed, env, episode) only."""
    kw = dict(dynamics_rand=True, max_steps=1, action_mode="vel_steer")
    acts = np.random.default_rng(5).uniform(-1, 1, (4, N, 2)).astype(np.float32)
    a = make_sim("small_loop", N, auto_reset=True, **kw)
    b = make_sim("small_loop", N, **kw)
    assert first_bad(a.read(_ffi.FIELD_STATE_BLOB)[None], b.read(_ffi.FIELD_STATE_BLOB)[None]) is None
    a.step(acts, n_steps=4)
    for t in range(4):
        if t:
            done = b.read(_ffi.FIELD_DONE)
            assert done.all()
            b.reset(done)
        b.step(acts[t])
    ba, bb = a.read(_ffi.FIELD_STATE_BLOB), b.read(_ffi.FIELD_STATE_BLOB)
    assert (a.read(_ffi.FIELD_EPISODE) == 4).all() and (b.read(_ffi.FIELD_EPISODE) == 4).all()
    if not np.array_equal(ba, bb):
        off, _ = expected_offsets(N)
        first = int(np.flatnonzero(ba != bb)[0])
        name = [n for n, _, _ in ARRAYS if off[n] <= first][-1]
        raise AssertionError(f"N={N}: the state blobs differ first at byte {first}, in array {name}")
    a.close(); b.close()


def test_reset_done_restarts_exactly_the_done_envs():
    N = N_LANES_4
    sim = make_sim("small_loop", N, dynamics_rand=True, max_steps=10**6)
    T = 60
    acts = np.zeros((T, N, 2), np.float32)
    acts[:, ::2] = 1.0                                      # every other env drives straight on until it leaves the road; the rest stand still
    sim.step(acts, n_steps=T)
    done = sim.read(_ffi.FIELD_DONE).astype(bool)
    assert done.any() and not done[1::2].any(), done
    before = read_draws(sim)
    sim.reset_done()
    dev = read_draws(sim)
    assert np.array_equal(dev["EPISODE"], 1 + done.astype(np.int32)) and not sim.read(_ffi.FIELD_DONE).any()
    cfg = RM.SamplerCfg.from_ffi(sim._sampler)
    assert_draws(dev, RM.sample_reset(SEED, np.flatnonzero(done), 2, sim.maps[0], cfg), 2, np.flatnonzero(done), who="reset_done")
    assert (sim.read(_ffi.FIELD_STEP_COUNT) == np.where(done, 0, T)).all()
    for f in dev:
        assert first_bad(dev[f][~done], before[f][~done]) is None, f
    j = judged("small_loop", N, 60.0, envs=tuple(np.flatnonzero(done).tolist()), episodes=(2,))[2]
    sure = ~j.unsure
    got = np.stack([dev["POS"][done, 0], dev["POS"][done, 2], dev["ANGLE"][done]], axis=1)
    assert first_bad(got[sure], j.pose[sure]) is None
    sim.close()


def test_walking_duckies_draw_the_models_streams():
    """DuckieObj under domain randomisation: the creation draws, and the redraw of the first finish_walk of every duckie that ends a
    walk within T steps, at the step_count where FIELD_OBJ_ACTIVE dropped"""
    N, T = N_LANES_4, 700
    sim = make_sim("loop_pedestrians", N, max_steps=10**6)
    mt, env = sim.maps[0], np.arange(N)
    slots = [o.dyn_slot for o in mt.objects if o.dyn_kind == 1]
    assert len(slots) == 8
    par = sim.read(_ffi.FIELD_OBJ_PARAMS)
    worst = 0.0
    for d in slots:
        vel, wait, wiggle, _ = RM.create_duckie(SEED, env, 1, d, True)
        assert np.array_equal(par[:, d, 1], wait) and np.array_equal(par[:, d, 2], wiggle), d
        worst = max(worst, np.abs(par[:, d, 0] - vel).max())
    assert worst <= 0.005 * NORMAL_TOL, worst
    zero = np.zeros((N, 2), np.float32)
    active = sim.read(_ffi.FIELD_OBJ_ACTIVE).astype(bool)
    assert not active.any()
    seen, worst_walk, n_walks = np.zeros((N, 8), bool), 0.0, 0
    for t in range(1, T + 1):
        sim.step(zero)
        now = sim.read(_ffi.FIELD_OBJ_ACTIVE).astype(bool)
        drop = active & ~now & ~seen
        if drop.any():
            p1 = sim.read(_ffi.FIELD_OBJ_PARAMS)
            for d in np.flatnonzero(drop.any(axis=0)):
                e = np.flatnonzero(drop[:, d])
                vel, wait, _ = RM.finish_walk(SEED, e, 1, int(d), t, par[e, d, 0])
                assert np.array_equal(p1[e, d, 1], wait), (t, d, e)
                assert (p1[e, d, 0] < 0).all()               # the first walk went forward
                worst_walk = max(worst_walk, np.abs(p1[e, d, 0] - vel).max())
                n_walks += e.size
            seen |= drop
        active = now
    assert (sim.read(_ffi.FIELD_STEP_COUNT) == T).all()
    print(f"duckies: creation max |vel - model| {worst:.3e}, {n_walks} first walks ended, max |vel - model| {worst_walk:.3e} (bound {0.005 * NORMAL_TOL:.1e})")
    assert n_walks > N and worst_walk <= 0.005 * NORMAL_TOL
    sim.close()


def test_follower_duckiebots_draw_the_models_stream():
    N = N_LANES_4
    sim = make_sim("loop_dyn_duckiebots", N)
    mt = sim.maps[0]
    bots = [o for o in mt.objects if o.dyn_kind == 2]
    assert len(bots) == 4
    par, ext = sim.read(_ffi.FIELD_OBJ_PARAMS), sim.read(_ffi.FIELD_OBJ_EXTRA)
    for o in bots:
        p, x, _ = RM.create_duckiebot(SEED, np.arange(N), 1, o.dyn_slot, gain=o.wait_time, trim=o.wiggle)
        assert first_bad(par[:, o.dyn_slot], p) is None and first_bad(ext[:, o.dyn_slot], x) is None, o.dyn_slot
    sim.close()


def test_random_maps_follow_the_map_stream():
    N = N_LANES_4
    names = ["loop_only_duckies", "small_loop_only_duckies"]
    sim = BatchedSimulator(names, N, render=False, domain_rand=False, seed=SEED, device_reset=True, map_random=True)
    seen = set()
    for ep in (1, 2, 3):
        if ep > 1:
            sim.reset()
        want, _ = RM.next_map(SEED, np.arange(N), ep, len(names))
        got = sim.read(_ffi.FIELD_MAP_ID)
        assert np.array_equal(got, want), (ep, got, want)
        seen |= set(got.tolist())
    assert seen == {0, 1}
    sim.close()
