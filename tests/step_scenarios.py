"""Deterministic k_step scenarios shared by tests/test_step_scenarios_host.py (the oracle alone: do the inputs reach what
they are meant to reach?) and tests/test_gpu_step_lanes.py (the device against the oracle at every lane count).

A scenario is P = 32 probe envs with explicit starts (no reset() sampling) and seeded actions.  The GPU tests run it at batch
sizes N = 1 (mod 32), where env e is a replica of probe e % 32, so the oracle's record of the 32 probes -- computed once per
(scenario, action mode, frame_skip) and cached -- is the reference for every batch size.

  "mixed"   all five fixture maps in one simulator, probe p on map p % 5: adjacent lane groups of one wavefront have different
            object counts (0/0, 4/0, 8/0, 0/8 and 3/4 static/dynamic), blob offsets and DynInit rows.
  "cluster" one map (small_loop tiles) with 5 static and 3 walking duckies -- an odd tail for 2 and for 4 lanes per env.  The static
            ones stand on both sides of the lane along z = 1.3 tiles, each 0.25 tiles (0.146 m) from its centre line: further than
            the robot's half width plus the duckie's (0.075 m + 0.036 m), nearer than the two safety radii (0.162 m + 0.066 m), so a
            robot on the centre line has up to five negative proximity scores at once and no collision.

The walking duckies' initial wait (8 s = 240 updates in the reference) is shortened to DUCKIE_WAIT on both sides -- the oracle
object's attribute, DTSIM_FIELD_OBJ_PARAMS on the device -- so that they walk, and one finishes its walk, within the run.
"""
import copy
import ctypes as C
import functools
import math
from types import SimpleNamespace

import numpy as np

from dtsim import _ffi, assets
from oracle import sim as osim
from util import EXT

P = 32                      # probe envs
T = 150                     # steps
DUCKIE_WAIT = 0.5           # s: 15 updates of 1/30 s, then the duckies walk one tile in 30 updates
PARAMS = (("wheels", 1), ("vel_steer", 3))          # (action mode, frame_skip)
SCENARIOS = ("mixed", "cluster")
MIXED_MAPS = ("small_loop", "small_loop_only_duckies", "loop_only_duckies", "loop_pedestrians", "loop_dyn_duckiebots")
MIXED_COUNTS = ((0, 0), (4, 0), (8, 0), (0, 8), (3, 4))      # (n_static, n_dyn) of MIXED_MAPS; dtsim_set_maps takes all five

CLUSTER_STATIC = [((2.40, 1.05), 20), ((2.50, 1.55), 110), ((2.56, 1.05), 200), ((2.66, 1.55), 290), ((2.45, 1.55), 75)]
CLUSTER_WALKERS = [((1.05, 2.45), 0), ((3.95, 2.55), 180), ((2.5, 3.05), 270)]      # each crosses both lanes of its straight tile


def cluster_map():
    md = assets.get_map("small_loop")
    md["objects"] = [dict(kind="duckie", pos=list(p), rotate=r, height=0.06, static=True) for p, r in CLUSTER_STATIC] + \
                    [dict(kind="duckie", pos=list(p), rotate=r, height=0.06, static=False) for p, r in CLUSTER_WALKERS]
    return md


def map_datas(scenario):
    """[(name, MapFormat1 dict)] of the scenario's maps, in map_id order."""
    if scenario == "mixed":
        return [(n, assets.get_map(n)) for n in MIXED_MAPS]
    return [("cluster", cluster_map())]


# ---- probe starts: (tile i, tile j, curve of the tile, curve parameter t, speed factor).  The pose is the point of the lane's
# centre line at t, heading along its tangent; the speed factor scales the probe's actions (the slow ones outlive the run).
# Probe p of "mixed" is on map p % 5.
MIXED_STARTS = [
    # small_loop             small_loop_only_duckies  loop_only_duckies        loop_pedestrians         loop_dyn_duckiebots
    (2, 1, 0, 0.5, 1.0),     (1, 2, 1, 0.1, 0.3),     (1, 2, 0, 0.5, 0.3),     (1, 4, 1, 0.5, 0.3),     (5, 1, 1, 0.9, 0.05),
    (1, 2, 0, 0.5, 1.0),     (2, 3, 0, 0.1, 1.0),     (1, 2, 0, 0.5, 0.05),    (1, 5, 1, 0.1, 0.05),    (4, 1, 0, 0.5, 0.3),
    (1, 1, 0, 0.1, 0.05),    (2, 3, 1, 0.5, 0.05),    (2, 1, 0, 0.9, 0.05),    (6, 2, 1, 0.1, 0.05),    (5, 1, 1, 0.5, 0.3),
    (3, 3, 1, 0.5, 0.05),    (3, 2, 0, 0.1, 0.3),     (6, 2, 0, 0.5, 0.3),     (2, 1, 0, 0.9, 0.3),     (5, 1, 0, 0.1, 0.3),
    (2, 3, 1, 0.1, 0.05),    (1, 3, 0, 0.9, 1.0),     (4, 4, 0, 0.5, 0.05),    (1, 1, 0, 0.1, 0.05),    (4, 4, 0, 0.1, 0.05),
    (3, 2, 0, 0.5, 0.05),    (1, 1, 0, 0.5, 0.05),    (1, 5, 1, 0.9, 1.0),     (6, 2, 1, 0.1, 0.3),     (6, 1, 1, 0.5, 1.0),
    (1, 3, 0, 0.9, 0.05),    (3, 1, 0, 0.9, 0.3),
]
CLUSTER_STARTS = [
    # before / inside / past the cluster on the lane it flanks (tile (2, 1), curve 1, driving towards -x) and on the lane it blocks
    (2, 1, 1, 0.5, 0.05),    (2, 1, 1, 0.1, 0.3),     (2, 1, 1, 0.1, 1.0),     (2, 1, 1, 0.9, 0.05),    (2, 1, 0, 0.1, 0.3),
    (1, 1, 0, 0.5, 0.3),     (3, 1, 1, 0.9, 0.3),     (3, 1, 1, 0.9, 1.0),
    # a short drive before a walking duckie's crossing
    (1, 2, 0, 0.1, 1.0),     (3, 2, 1, 0.1, 1.0),     (2, 3, 0, 0.1, 1.0),     (1, 2, 1, 0.5, 0.3),
    # anywhere valid
    (1, 3, 0, 0.5, 1.0),     (3, 3, 0, 0.5, 1.0),     (2, 1, 1, 0.1, 0.05),    (2, 1, 0, 0.1, 0.05),    (2, 1, 1, 0.5, 0.3),
    (2, 1, 1, 0.5, 1.0),     (2, 1, 1, 0.9, 1.0),     (1, 1, 1, 0.9, 0.05),    (3, 1, 0, 0.1, 0.05),    (2, 3, 1, 0.5, 1.0),
    (3, 2, 0, 0.5, 0.3),     (1, 2, 0, 0.9, 0.05),    (3, 3, 1, 0.9, 0.05),    (1, 1, 0, 0.9, 0.3),     (2, 1, 0, 0.1, 1.0),
    (1, 3, 1, 0.1, 0.05),    (2, 3, 0, 0.9, 0.05),    (3, 2, 1, 0.9, 0.05),    (1, 1, 0, 0.5, 1.0),     (2, 1, 1, 0.3, 0.1),
]


def probe_map(scenario, p):
    return p % len(MIXED_MAPS) if scenario == "mixed" else 0


def lane_pose(omap, i, j, curve, t):
    """(x, z, angle) on the centre line of `curve` of tile (i, j) at parameter t, heading along the tangent."""
    cps = omap.get_tile(i, j)["curves"][curve]
    pt, tg = osim.bezier_point(cps, t), osim.bezier_tangent(cps, t)
    return float(pt[0]), float(pt[2]), float(math.atan2(-tg[2], tg[0]))


@functools.lru_cache(maxsize=None)
def starts(scenario):
    """[P] of (map_id, x, z, angle, speed factor)."""
    table = MIXED_STARTS if scenario == "mixed" else CLUSTER_STARTS
    assert len(table) == P
    omaps = [osim.OracleMap(md, EXT) for _, md in map_datas(scenario)]
    out = []
    for p, (i, j, c, t, speed) in enumerate(table):
        mid = probe_map(scenario, p)
        out.append((mid,) + lane_pose(omaps[mid], i, j, c, t) + (float(speed),))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def actions(scenario, mode):
    """float32 [T, P, 2], seeded: mostly forward (one step in 25 backs up), a little random steering, scaled per probe."""
    return shape_actions(np.array([s[4] for s in starts(scenario)]), mode)


def shape_actions(speed, mode):
    rng = np.random.default_rng(20240)
    fwd = rng.uniform(0.35, 0.65, (T, P))
    turn = rng.uniform(-0.06, 0.06, (T, P))
    fwd = np.where(rng.uniform(size=(T, P)) < 0.04, -0.2, fwd)
    fwd, turn = fwd * speed, turn * speed
    a = np.stack([fwd - turn, fwd + turn] if mode == "wheels" else [fwd, 8.0 * turn], axis=-1)
    return np.ascontiguousarray(a, np.float32)


def tiled_actions(scenario, mode, N):
    """[T, N, 2]: env e gets the actions of probe e % P."""
    return np.ascontiguousarray(actions(scenario, mode)[:, np.arange(N) % P])


def make_oracles(scenario, frame_skip, max_steps=1500):
    """One OracleSim per probe at its start, walking duckies' wait shortened."""
    datas = map_datas(scenario)
    out = []
    for mid, x, z, ang, _ in starts(scenario):
        o = osim.OracleSim(copy.deepcopy(datas[mid][1]), EXT, do_reset=False, frame_skip=frame_skip, max_steps=max_steps)
        o.wheel_dist = osim.WHEEL_DIST                      # what reset() sets without domain randomisation
        o.set_pose([x, 0.0, z], ang)
        for ob in o.map.objects:
            if not ob.static and ob.kind == "duckie":
                ob.pedestrian_wait_time = DUCKIE_WAIT
        out.append(o)
    return out


def dyn_objects(o):
    """The oracle's dynamic objects in the order of the device's dynamic slots."""
    return [ob for ob in o.map.objects if not ob.static]


def contributing(o):
    """How many objects have a negative proximity score at the oracle's current pose (proximity_penalty2's terms)."""
    pos = osim.actual_center(o.cur_pos, o.cur_angle)
    n = 0
    if len(o.map.collidable_centers):
        d = np.linalg.norm(o.map.collidable_centers - pos, axis=1)
        n += int(np.count_nonzero(d - osim.AGENT_SAFETY_RAD - o.map.collidable_safety_radii < 0))
    return n + sum(1 for ob in o.map.objects if ob.proximity(pos, osim.AGENT_SAFETY_RAD) < 0)


def end_causes(o):
    """Why _valid_pose rejects the oracle's current pose: a subset of {"road", "static", "walker", "walker_moved", "follower"}."""
    pos, ang = osim.actual_center(o.cur_pos, o.cur_angle), o.cur_angle
    f_vec, r_vec = osim.get_dir_vec(ang), osim.get_right_vec(ang)
    pts = [pos, pos - 0.5 * osim.ROBOT_WIDTH * r_vec, pos + 0.5 * osim.ROBOT_WIDTH * r_vec, pos + 0.5 * osim.ROBOT_LENGTH * f_vec]
    out = set()
    if not all(o._drivable_pos(q) for q in pts):
        out.add("road")
    corners = osim.get_agent_corners(pos, ang)
    norm = osim.generate_norm(corners)
    m = o.map
    if len(m.collidable_corners) and osim.intersects(corners, m.collidable_corners, norm, m.collidable_norms):
        out.add("static")
    for ob in m.objects:
        if ob.check_collision(corners, norm):
            if ob.kind == "duckiebot":
                out.add("follower")
            else:
                out.add("walker")
                if not np.array_equal(ob.center, ob.start) or ob.vel < 0:      # it has left its first start point
                    out.add("walker_moved")
    return out


@functools.lru_cache(maxsize=None)
def oracle_record(scenario, mode, frame_skip):
    """The oracle's per-step record of the P probes: arrays [T, P, ...]; rows after a probe's episode ended (stepped[t, p] False)
    are not meaningful.  Computed once per process and shared: treat it as read-only."""
    oracles = make_oracles(scenario, frame_skip)
    acts = actions(scenario, mode)
    D = _ffi.MAX_DYNAMIC
    r = SimpleNamespace(
        stepped=np.zeros((T, P), bool), done=np.zeros((T, P), bool), code=np.zeros((T, P), np.uint8),
        tile=np.zeros((T, P, 2), np.int32), in_lane=np.zeros((T, P), bool), step_count=np.zeros((T, P), np.int32),
        pos=np.zeros((T, P, 3)), angle=np.zeros((T, P)), reward=np.zeros((T, P)), prox=np.zeros((T, P)),
        lane=np.zeros((T, P, 4)), speed=np.zeros((T, P)),
        obj_center=np.zeros((T, P, D, 2)), obj_active=np.zeros((T, P, D), bool), obj_yrot=np.zeros((T, P, D)),
        contributing=np.zeros((T, P), np.int32),
        map_id=np.array([s[0] for s in starts(scenario)]),
        dyn_kind=[[ob.kind for ob in dyn_objects(o)] for o in oracles],
        causes=[set() for _ in range(P)],             # why the episode ended (empty: alive at T, or max_steps)
        reversed=np.zeros(P, bool),                   # a walking duckie finished its walk and turned round
        follower_moved=np.zeros(P),                   # largest displacement of a follower, m
    )
    bot_start = [[np.copy(ob.pos) for ob in dyn_objects(o)] for o in oracles]
    alive = np.ones(P, bool)
    for t in range(T):
        for p, o in enumerate(oracles):
            if not alive[p]:
                continue
            a = acts[t, p].astype(np.float64)
            rew, d, c = o.step_vel_steer(a) if mode == "vel_steer" else o.step(a)
            inf = o.info()
            r.stepped[t, p], r.done[t, p], r.code[t, p] = True, d, c
            r.tile[t, p], r.in_lane[t, p], r.step_count[t, p] = inf["tile"], inf["in_lane"], inf["step_count"]
            r.pos[t, p], r.angle[t, p], r.reward[t, p], r.prox[t, p] = inf["pos"], inf["angle"], rew, inf["prox"]
            r.lane[t, p], r.speed[t, p] = inf["lane"], inf["speed"]
            r.contributing[t, p] = contributing(o)
            for k, ob in enumerate(dyn_objects(o)):
                if ob.kind == "duckiebot":
                    r.obj_center[t, p, k] = np.asarray(ob.pos, float)[[0, 2]]
                    r.follower_moved[p] = max(r.follower_moved[p], float(np.linalg.norm(ob.pos - bot_start[p][k])))
                else:
                    r.obj_center[t, p, k] = np.asarray(ob.center, float)[[0, 2]]
                    r.obj_active[t, p, k] = ob.pedestrian_active
                    r.reversed[p] = r.reversed[p] or ob.vel < 0
                r.obj_yrot[t, p, k] = ob.y_rot
            if d:
                alive[p] = False
                if c == osim.DONE_INVALID_POSE:
                    r.causes[p] = end_causes(o)
    r.alive_at_end = alive
    return r


# ---- the device side --------------------------------------------------------------------------------------------------------
def init_states(scenario, N, order=None):
    """(_ffi.InitState * N): env e starts where probe order[e % P] does (order: a permutation of range(P), default the identity)."""
    probes = (_ffi.InitState * P)()
    for p, (mid, x, z, ang, _) in enumerate(starts(scenario)):
        st = probes[p]
        st.pos[:] = [x, 0.0, z]
        st.angle, st.map_id, st.wheel_dist = ang, mid, osim.WHEEL_DIST
        st.cam_height, st.cam_angle_deg, st.cam_fov_y_deg = osim.CAMERA_FLOOR_DIST, osim.CAMERA_ANGLE, float(osim.CAMERA_FOV_Y)
    out = (_ffi.InitState * N)()
    sz = C.sizeof(_ffi.InitState)
    for e in range(N):
        p = e % P if order is None else int(order[e % P])
        C.memmove(C.byref(out, e * sz), C.byref(probes, p * sz), sz)
    return out


def make_sim(scenario, N, mode, frame_skip, **kw):
    """A BatchedSimulator of the scenario at its starts (host-fed reset), walking duckies' wait shortened."""
    from dtsim import BatchedSimulator
    datas = map_datas(scenario)
    if scenario == "mixed":
        sim = BatchedSimulator([n for n, _ in datas], N, render=False, domain_rand=False, do_reset=False, action_mode=mode,
                               frame_skip=frame_skip, **kw)
    else:
        sim = BatchedSimulator(datas[0][0], N, map_data=copy.deepcopy(datas[0][1]), render=False, domain_rand=False, do_reset=False,
                               action_mode=mode, frame_skip=frame_skip, **kw)
    sim.reset(states=init_states(scenario, N))
    par = sim.read(_ffi.FIELD_OBJ_PARAMS)                     # [N, MAX_DYNAMIC, (vel, wait_time, wiggle)]
    mids = np.array([s[0] for s in starts(scenario)])[np.arange(N) % P]
    for mid, (_, md) in enumerate(datas):
        kinds = [d["kind"] for d in md["objects"] if not d.get("static", True)]
        for k, kind in enumerate(kinds):
            if kind == "duckie":
                par[mids == mid, k, 1] = DUCKIE_WAIT
    sim.write(_ffi.FIELD_OBJ_PARAMS, par)
    return sim
