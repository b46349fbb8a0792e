"""`not gpu`: pin the oracle against the reference's OWN code.  The reference's answers to the queries of the first tests of this file
are recorded by oracle/make_golden.py (`python -m oracle.make_golden pins`, through oracle/refstub.py) in tests/golden/ref_pins.npz, inputs
included; the tests after them read the reference's source or GL call stream live and are skipped where /root/reference does not exist."""
import copy
import os

import numpy as np
import pytest

from dtsim import assets
from oracle import refstub, sim as osim
from oracle.fixtures import start_tile_cases
from oracle.make_golden import ENV_KW, MOVING, SEGMENT_NAMES, SEGMENT_PATHS
from util import EXT, junction_map

needs_ref = pytest.mark.skipif(not refstub.available(), reason="reference tree not present")
PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_pins.npz")


@pytest.fixture(scope="module")
def pins():
    with np.load(PINS) as d:
        return {k: d[k] for k in d.files}


def _ref(map_name, dr=False, seed=None, md=None):
    from oracle.make_golden import ref_sim
    return ref_sim(map_name, dr, seed, md)


def _lane(o, pos, a):
    """The oracle's lane pose as the recorded row: NaN x 4 where the reference raised NotInLane."""
    try:
        return [float(v) for v in o.get_lane_pos2(pos, a)]
    except osim.NotInLane:
        return [np.nan] * 4


def _check_queries(pins, key, o):
    """Valid pose, collision, proximity and lane pose of the oracle against the reference's answers to the same recorded poses."""
    for q, (pos, a) in enumerate(zip(pins[key + "_pos"], pins[key + "_angle"])):
        assert pins[key + "_valid"][q] == o._valid_pose(pos, a), (key, q)
        assert pins[key + "_collision"][q] == o._collision(osim.get_agent_corners(pos, a)), (key, q)
        assert pins[key + "_prox"][q] == o.proximity_penalty2(pos, a), (key, q)
        assert np.array_equal(pins[key + "_lane"][q], _lane(o, pos, a), equal_nan=True), (key, q)


@pytest.mark.parametrize("m", ["small_loop_only_duckies", "loop_only_duckies"])
def test_fresh_random_poses(m, pins):
    o = osim.OracleSim(assets.get_map(m), EXT, do_reset=False)
    assert len(pins[f"fresh_{m}_pos"]) == 800
    _check_queries(pins, f"fresh_{m}", o)


@pytest.mark.parametrize("dr", [False, True])
def test_reset_streams(dr, pins):
    k = f"resets_dr{int(dr)}"
    q = 0
    for seed in (11, 12, 13):
        o = osim.OracleSim(assets.get_map("loop_only_duckies"), EXT, domain_rand=dr, seed=seed, do_reset=False)
        for _ in range(3):
            o.reset()
            assert np.array_equal(pins[k + "_pos"][q], o.cur_pos) and pins[k + "_angle"][q] == o.cur_angle
            assert np.array_equal(pins[k + "_ground"][q], o.ground_color)
            q += 1


def test_reference_fill_holes_equals_oracle_and_product(pins):
    from dtsim import distortion as pd
    from oracle import distortion as od
    rx, ry = pins["fill_rx"], pins["fill_ry"]
    mapx, mapy = od.rectify_maps(160, 120)
    ox, oy = od.invert_map(mapx.copy(), mapy.copy())
    px, py = pd.distortion_maps(160, 120)
    assert np.array_equal(rx, ox) and np.array_equal(ry, oy)
    assert np.array_equal(rx, px) and np.array_equal(ry, py)


def test_segmentation_rules_equal_the_reference(pins):
    """graphics.py:59-67 should_segment_out and objmesh.py:260-266 gen_segmentation_color (a closure inside
    ObjMesh.__init__, observed through the colour it hands to load_texture) against dtsim/assets.py."""
    for p, want in zip(SEGMENT_PATHS, pins["segment_out"], strict=True):
        assert assets.should_segment_out(p) == want, p
    for k, name in enumerate(SEGMENT_NAMES):                  # untextured chunk -> the black_tile hack with the name's colour
        assert pins["segment_flag"][k] and pins["segment_texture"][k] == "black_tile.png"
        assert list(pins["segment_color"][k]) == assets.gen_segmentation_color(name), name
    assert len(pins["segment_color"]) == len(SEGMENT_NAMES)


def test_every_tile_kind_and_orientation_against_the_reference(pins):
    """Curves, drivable flags, lane pose, valid pose, collision and proximity on a map holding every drivable tile kind
    in every orientation -- the loop fixtures only have straights and curves."""
    md = junction_map()
    o = osim.OracleSim(copy.deepcopy(md), EXT, do_reset=False)
    # curve tables: same control points, tile by tile
    q, c0 = 0, 0
    for j in range(o.map.grid_height):
        for i in range(o.map.grid_width):
            ot = o.map.get_tile(i, j)
            if not pins["tiles_present"][q]:
                assert ot is None
                q += 1
                continue
            assert pins["tiles_drivable"][q] == ot["drivable"] and pins["tiles_kind"][q] == ot["kind"] and pins["tiles_angle"][q] == ot["angle"]
            if ot["drivable"]:
                n = int(pins["tiles_n_curves"][q])
                assert np.array_equal(pins["tiles_curves"][c0:c0 + n], np.asarray(ot["curves"])), (i, j, ot["kind"], ot["angle"])
                c0 += n
            q += 1
    assert q == len(pins["tiles_present"]) and c0 == len(pins["tiles_curves"])
    _check_queries(pins, "junctions", o)
    for q, (pos, a) in enumerate(zip(pins["junctions_pos"], pins["junctions_angle"])):
        assert pins["junctions_drivable"][q] == o._drivable_pos(pos)
        ocp, oct = o.closest_curve_point(pos, a)
        assert pins["junctions_has_cp"][q] == (ocp is not None)
        if ocp is not None:
            assert np.array_equal(pins["junctions_cp"][q], np.concatenate([ocp, oct]))
    assert (~np.isnan(pins["junctions_lane"][:, 0])).sum() > 1000


@needs_ref
def test_wrappers_equal_the_reference():
    """src/gym_duckietown/wrappers.py run through the stub loader: the action wrappers' arithmetic, the observation
    transpose, and the calibration constants UndistortWrapper / Distortion carry (cv2 itself is absent: the remaps stay
    restatements)."""
    import gym_duckietown.wrappers as mine
    from dtsim import distortion as pdist
    ns = refstub.load()
    ref = ns.wrappers

    class Env:
        wheel_dist = 0.1093
        distortion = True
        undistort = False
        observation_space = None
        action_space = None

        @property
        def unwrapped(self):
            return self

    rng = np.random.default_rng(4)
    for a in range(3):
        assert list(ref.DiscreteWrapper(Env()).action(a)) == list(mine.DiscreteWrapper(Env()).action(a))
    for kw in ({}, dict(gain=1.3, trim=0.07, radius=0.03, k=25.0, limit=0.8)):
        r, m = ref.SteeringToWheelVelWrapper(Env(), **kw), mine.SteeringToWheelVelWrapper(Env(), **kw)
        for _ in range(200):
            act = rng.uniform(-1.5, 1.5, 2)
            assert np.array_equal(np.asarray(r.action(act), dtype=np.float64), np.asarray(m.action(act), dtype=np.float64))
    obs = rng.integers(0, 256, (6, 8, 3), dtype=np.uint8)
    po = ref.PyTorchObsWrapper.__new__(ref.PyTorchObsWrapper)
    assert np.array_equal(po.observation(obs), mine.PyTorchObsWrapper.observation(None, obs))
    e = Env()
    u = ref.UndistortWrapper(e)
    assert e.undistort is True
    assert np.array_equal(u.camera_matrix, mine.UndistortWrapper.K) and np.array_equal(u.camera_matrix, pdist.CAMERA_MATRIX)
    assert np.array_equal(np.ravel(u.distortion_coefs), mine.UndistortWrapper.D) and np.array_equal(np.ravel(u.distortion_coefs), pdist.DIST_COEFS)
    assert np.array_equal(u.projection_matrix, mine.UndistortWrapper.P) and np.array_equal(u.projection_matrix[:, :3], pdist.UNDISTORT_P)
    ns.distortion.cv2.getOptimalNewCameraMatrix = lambda **kw: (None, None)      # cv2 is a stub here
    d = ns.distortion.Distortion()
    assert np.array_equal(d.camera_matrix, pdist.CAMERA_MATRIX) and np.array_equal(np.ravel(d.distortion_coefs), pdist.DIST_COEFS)
    assert (d.W, d.H) == (640, 480)


def test_duckietown_env_kinematics_equal_the_reference(pins):
    """envs/duckietown_env.py:36-61: (vel, steering) -> [left, right] duty handed to Simulator.step, and the
    `DuckietownEnv` info block; against the oracle's wheels_from_vel_steer (which the HIP k_step is checked against)."""
    acts, vels = pins["env_action"].reshape(len(ENV_KW), -1, 2), pins["env_vels"].reshape(len(ENV_KW), -1, 2)
    assert acts.shape[1] == 300
    for kw, a_k, v_k in zip(ENV_KW, acts, vels):
        o = osim.OracleSim(assets.get_map("small_loop"), EXT, do_reset=False, **kw)
        o.wheel_dist = 0.102 * 1.04
        for act, want in zip(a_k, v_k):
            assert np.array_equal(want, np.asarray(o.wheels_from_vel_steer(act), dtype=np.float64))
    assert set(pins["env_info_keys"]) == {"k", "gain", "train", "radius", "omega_r", "omega_l"}


@pytest.mark.parametrize("dr", [False, True])
def test_reset_start_tile_branches(dr, pins):
    """reset()'s tile / pose selection branches (simulator.py:659-688): `user_tile_start`, the map's `start_tile`,
    the map's `start_pose`; optional objects' visibility draw (:648-656) on the junction map."""
    for c, (md, kw) in enumerate(start_tile_cases(assets.get_map("loop_only_duckies"), junction_map())):
        k = f"start_dr{int(dr)}_{c}"
        o = osim.OracleSim(copy.deepcopy(md), EXT, domain_rand=dr, seed=3, do_reset=False, **kw)
        for q in range(3):
            o.reset()
            assert np.array_equal(pins[k + "_pos"][q], o.cur_pos) and pins[k + "_angle"][q] == o.cur_angle
            assert list(pins[k + "_visible"][q]) == [bool(ob.visible) for ob in o.map.objects]


@pytest.mark.parametrize("m,steps", list(MOVING.items()))
def test_collision_and_proximity_against_moving_objects(m, steps, pins):
    """_collision (static batch + every object's check_collision with its *stored* obj_norm, simulator.py:1473-1492,
    objects.py:152-160, 272-281, 373-382), proximity_penalty2 and _inconvenient_spawn while DuckieObj pedestrians are
    mid-walk / DuckiebotObj followers have driven away from their spawn."""
    o = osim.OracleSim(copy.deepcopy(assets.get_map(m)), EXT, do_reset=False)
    t = 0
    for t_end in steps:
        while t < t_end:
            for ob in o.map.objects:
                if ob.kind == "duckiebot" and not ob.static:
                    ob.step_duckiebot(1 / 30, o.closest_curve_point)
                elif not ob.static:
                    ob.step(1 / 30)
            t += 1
        key = f"moving_{m}_{t_end}"
        ref_pos = pins[key + "_obj_pos"]
        assert len(ref_pos) == len(o.map.objects)
        for rp, oo in zip(ref_pos, o.map.objects):
            assert np.array_equal(rp, np.asarray(oo.pos, float))
        assert pins[key + "_obj_static"].sum() < len(ref_pos)          # some objects moved
        _check_queries(pins, key, o)
        for q, pos in enumerate(pins[key + "_pos"]):
            assert pins[key + "_inconvenient"][q] == o._inconvenient_spawn(pos)
        assert pins[key + "_collision"].sum() > 30


@needs_ref
def test_dr_constants_match_the_reference():
    """The distribution table tests/test_gpu_device_reset.py checks the device sampler against IS the reference's:
    randomization/config/default_dr.json, randomizer.py DEFAULT_CONFIG, and the camera / wheel constants of simulator.py."""
    import ast, json, os, re
    import test_gpu_device_reset as T
    root = "/root/reference/src/gym_duckietown"
    with open(os.path.join(root, "randomization/config/default_dr.json")) as f:
        assert json.load(f) == T.DR_CONFIG
    src = open(os.path.join(root, "randomization/randomizer.py")).read()
    m = re.search(r"DEFAULT_CONFIG = (\{.*?\n\})", src, re.S)
    assert ast.literal_eval(m.group(1)) == T.DR_CONFIG
    sim = open(os.path.join(root, "simulator.py")).read()
    for name, val in (("CAMERA_FLOOR_DIST", T.CAMERA_FLOOR_DIST), ("CAMERA_ANGLE", T.CAMERA_ANGLE), ("CAMERA_FOV_Y", T.CAMERA_FOV_Y),
                      ("WHEEL_DIST", T.WHEEL_DIST)):
        mm = re.search(rf"^{name} = ([0-9.]+)", sim, re.M)
        assert mm and float(mm.group(1)) == val, name
    # the perturbation scales and base colours used in the device test (simulator.py:551-597)
    for frag in ("self._perturb(self.color_sky)", "self._perturb(WALL_COLOR)", "self._perturb([0.15, 0.15, 0.15], 0.4)",
                 "self._perturb([0.9, 0.9, 0.9], 0.4)", "self._perturb(ambient, 0.3)", "self._perturb(diffuse, 0.99)",
                 "self._perturb(np.array(self.color_ground), 0.3)", "self._perturb(WHEEL_DIST)", "DIM = 0.5",
                 "WALL_COLOR = np.array([0.64, 0.71, 0.28])", "BLUE_SKY = np.array([0.45, 0.82, 1])"):
        assert frag in sim, frag
    obj = open(os.path.join(root, "objects.py")).read()
    for frag in ("self.follow_dist = np.random.uniform(0.3, 0.4)", "self.velocity = np.random.uniform(0.05, 0.15)",
                 "self.gain = gain + np.random.uniform(-0.3, 0.3)", "self.trim = trim + np.random.uniform(-0.1, 0.1) + 2",
                 "self.radius = radius + 0.0002 * np.random.uniform(-1, 1)", "self.wheel_dist = wheel_dist + 0.01 * np.random.uniform(-1, 1)",
                 "self.robot_width = robot_width + 0.01 * np.random.uniform(-1, 1)",
                 "self.robot_length = robot_length + 0.01 * np.random.uniform(-1, 1)"):
        assert frag in obj, frag


@needs_ref
def test_led_spheres_are_the_reference_s_draw_calls():
    """enable_leds: WorldObj.render_mesh (objects.py:68-121) run UNMODIFIED with recording GL mocks -- the translate of every LED, the
    glColor4f before each gluSphere and the sphere radii -- against the table oracle/raster.py (and gym_duckietown/simulator.py) state the
    spheres from: positions in the dict's order, DuckiebotObj.leds_color for a follower, blue for any other duckiebot-kind object, a
    1 cm sphere at alpha 1 and a halo of mean(colour) x 4 cm at alpha 0.2."""
    from oracle import raster
    r, ns = _ref("loop_dyn_duckiebots", False, 1)
    gl, glu = ns.objects.gl, ns.objects.gluSphere
    bot = [o for o in r.objects if o.kind == "duckiebot"][0]
    blue = copy.copy([o for o in r.objects if o.kind == "duckie"][0])
    blue.kind = "duckiebot"                              # a static WorldObj of kind duckiebot: not a DuckiebotObj
    for obj, colours in ((bot, raster.LED_FOLLOWER), (blue, raster.LED_STATIC)):
        gl.reset_mock(); glu.reset_mock()
        obj.render_mesh(segment=False, enable_leds=True)
        tr = [tuple(float(v) for v in c.args) for c in gl.glTranslatef.call_args_list]
        assert tr == [tuple(p) for p in raster.LED_POSITIONS]
        cols = [tuple(float(v) for v in c.args) for c in gl.glColor4f.call_args_list]
        radii = [float(c.args[1]) for c in glu.call_args_list]
        assert all(c.args[2:] == (10, 10) for c in glu.call_args_list)
        assert len(cols) == 15 and len(radii) == 10       # per LED: sphere colour, halo colour, reset to white
        for k, col in enumerate(colours):
            assert cols[3 * k] == (*col, 1.0) and cols[3 * k + 1] == (*col, 0.2) and cols[3 * k + 2] == (1.0, 1.0, 1.0, 1.0)
            assert radii[2 * k] == 0.01 and abs(radii[2 * k + 1] - float(np.mean(col)) * 0.04) < 1e-15
        assert gl.glBlendFunc.call_args_list[0].args == (gl.GL_SRC_ALPHA, gl.GL_ONE)
    gl.reset_mock(); glu.reset_mock()
    bot.render_mesh(segment=False, enable_leds=False)
    assert not glu.called                                 # off by default
    duck = [o for o in r.objects if o.kind == "duckie"][0]
    duck.render_mesh(segment=False, enable_leds=True)
    assert not glu.called                                 # duckiebot-kind objects only


@needs_ref
def test_curve_overlay_segments_are_the_reference_s_draw_calls():
    """draw_curve: _render_img (simulator.py:1853-1904) run UNMODIFIED with draw_curve on against a recording gl mock -- the colour and the 20
    vertices of every line strip bezier_draw (graphics.py:336-349) emits, in order -- against gym_duckietown.simulator.curve_overlay_segments
    (what the facade hands to dtsim_draw_lines).  Bit-identical, including the reference's quirk: the "heading" the red curve is chosen by is
    the tile's orientation index (the tile loop rebinds `angle`), not the agent's."""
    from unittest.mock import MagicMock
    from gym_duckietown.simulator import curve_overlay_segments
    W, H = 640, 480
    for m, seed in (("loop_only_duckies", 3), ("small_loop_only_duckies", 4)):
        r, ns = _ref(m, False, seed)
        r.reset()
        gl = ns.simulator.gl
        assert ns.graphics.gl is gl
        r.graphics = True
        r.shadow_window = MagicMock(); r.draw_curve = True; r.enable_leds = False; r.draw_bbox = False
        r.road_vlist, r.ground_vlist, r.tri_vlist = MagicMock(), MagicMock(), MagicMock()
        gl.reset_mock()
        with pytest.raises(TypeError):                   # glReadPixels wants a ctypes pointer type: every draw call has been issued by then
            r._render_img(W, H, MagicMock(), MagicMock(), np.zeros((H, W, 3), np.uint8), top_down=False, segment=False)
        want, col, pts = [], None, None
        for c in gl.mock_calls:
            if c[0] == "glBegin" and c.args == (gl.GL_LINE_STRIP,):
                pts = []
            elif c[0] == "glColor3f" and pts is not None and not pts:
                col = tuple(float(v) for v in c.args)
            elif c[0] == "glVertex3f" and pts is not None:
                pts.append(tuple(float(v) for v in c.args))
            elif c[0] == "glEnd" and pts is not None:
                assert len(pts) == 20 and col in ((1.0, 0.0, 0.0), (0.0, 0.0, 1.0))
                want += [[*p0, *p1, *col] for p0, p1 in zip(pts[:-1], pts[1:])]
                pts = None
        got = np.asarray(curve_overlay_segments(r.grid, r.grid_width, r.grid_height), dtype=np.float64)
        n_curves = sum(len(t["curves"]) for t in r.grid if t is not None and t["drivable"])
        assert got.shape == (19 * n_curves, 9) == (len(want), 9)
        assert np.array_equal(got, np.asarray(want, dtype=np.float64))


def _gl_floats(gl, kind):
    """Arguments of the (GLfloat * n)(...) constructions recorded on the gl mock, in call order (kind: the mock call name)."""
    return [tuple(float(v) for v in c.args) for c in gl.mock_calls if c[0] == kind]


@needs_ref
@pytest.mark.parametrize("dr", [False, True])
def test_frame_gl_arguments_are_the_oracle_s_camera_and_scene(dr):
    """(Written when GL was believed absent; since round 6 the frames themselves are pinned on real GL, tests/test_gl_golden.py -- this test stays because
    it LOCALISES a failure.)  Every ARGUMENT the reference hands to GL can be read: reset() (simulator.py:565-584) and
    _render_img (:1707-1951) run UNMODIFIED against a recording gl mock -- projection, model-view, clear colour, light, ground quad, per-tile
    and per-object transforms -- and are compared with what oracle/raster.py renders from (Camera, Scene): what is left unpinned of the
    raster is what fixed-function GL does with these numbers, not which numbers it is given."""
    import math
    from unittest.mock import MagicMock
    from oracle import raster
    seed, W, H = 7, 640, 480
    r, ns = _ref("small_loop_only_duckies", dr, seed)
    o = osim.OracleSim(assets.get_map("small_loop_only_duckies"), EXT, domain_rand=dr, seed=seed, do_reset=False)
    gl = ns.simulator.gl
    gl.reset_mock()
    r.reset(); o.reset()
    assert np.array_equal(r.cur_pos, o.cur_pos) and r.cur_angle == o.cur_angle
    # ---- reset(): the light (position, ambient, diffuse, specular), simulator.py:565-584
    lf = _gl_floats(gl, "GLfloat.__mul__()")
    assert lf[0][:len(o.light_pos)] == tuple(float(v) for v in o.light_pos)      # (a 3-vector under domain randomisation: w is whatever GLfloat * 4 zero-fills = directional)
    assert lf[1] == tuple(float(v) for v in o.light_ambient) and lf[2] == tuple(float(v) for v in o.light_diffuse) and lf[3] == (0.0, 0.0, 0.0, 1.0)
    # the vertex lists (simulator.py:386-526): the tile quad grid with its texture coordinates, the ground quad
    saved_vl, rec_vl = ns.simulator.pyglet.graphics.vertex_list, MagicMock()
    ns.simulator.pyglet.graphics.vertex_list = rec_vl    # (other tests of this file install their own stand-in on the shared pyglet mock)
    try:
        type(r)._init_vlists(r)                          # (refstub's instances carry a no-op in its place: call the class's own)
    finally:
        ns.simulator.pyglet.graphics.vertex_list = saved_vl
    (n_road, road_v, road_t, _, _), (n_gnd, gnd_v) = [c.args for c in rec_vl.call_args_list]
    road_v, road_t = np.asarray(road_v[1]).reshape(-1, 3), np.asarray(road_t[1]).reshape(-1, 2)
    gnd_v = np.asarray(gnd_v[1], dtype=np.float64).reshape(4, 3)
    # ---- one frame
    r.graphics = True
    r.shadow_window = MagicMock(); r.draw_bbox = False; r.draw_curve = False; r.enable_leds = False
    r.road_vlist, r.ground_vlist, r.tri_vlist = MagicMock(), MagicMock(), MagicMock()
    gl.reset_mock()
    with pytest.raises(TypeError):                       # glReadPixels wants a ctypes pointer type: every draw call has been issued by then
        r._render_img(W, H, MagicMock(), MagicMock(), np.zeros((H, W, 3), np.uint8), top_down=False, segment=False)
    calls = gl.mock_calls
    by = lambda name: [c for c in calls if c[0] == name]
    f1 = lambda v: float(np.ravel(v)[0])                   # (the randomiser's draws are 1-element arrays)
    cam = raster.Camera(o.cur_pos, o.cur_angle, cam_height=f1(o.cam_height), cam_angle_deg=f1(o.cam_angle[0]), cam_fov_y_deg=f1(o.cam_fov_y),
                        camera_noise=list(o.randomization_settings["camera_noise"]) if dr else (0, 0, 0), domain_rand=dr,
                        horizon_color=list(o.horizon_color), ground_color=list(o.ground_color), light_pos=list(o.light_pos),
                        light_ambient=list(o.light_ambient), light_diffuse=list(o.light_diffuse), width=W, height=H)
    assert _gl_floats(gl, "GLfloat.__mul__()")[0] == (0.3, 0.3, 0.3, 1.0)                      # GL_LIGHT_MODEL_AMBIENT: Camera.base = 0.3 + light ambient
    assert np.allclose(cam.base, 0.3 + np.asarray(lf[1][:3]), atol=0, rtol=0) and np.array_equal(cam.dif, np.asarray(lf[2][:3]))
    cc = [float(v) for v in by("glClearColor")[0].args]
    assert np.array_equal(cam.horizon, np.asarray(cc[:3]) * 255.0)
    fov, aspect, near, far = by("gluPerspective")[0].args
    assert float(np.ravel(fov)[0]) == float(np.ravel(o.cam_fov_y)[0]) and aspect == W / float(H) and (near, far) == (raster.NEAR, raster.FAR)
    assert cam.ty == math.tan(math.radians(float(np.ravel(fov)[0])) / 2) and cam.tx == cam.ty * aspect
    i_mv = max(i for i, c in enumerate(calls) if c[0] == "gluLookAt")
    rots = [c.args for c in calls[:i_mv] if c[0] == "glRotatef"][-3:]
    assert [float(np.ravel(a[0])[0]) for a in rots] == [float(np.ravel(v)[0]) for v in o.cam_angle] and [tuple(a[1:]) for a in rots] == [(1, 0, 0), (0, 1, 0), (0, 0, 1)]
    assert [c.args for c in calls[:i_mv] if c[0] == "glTranslatef"][-1] == (0, 0, raster.CAMERA_FORWARD_DIST)
    la = [f1(v) for v in calls[i_mv].args]
    eye, tgt, up = np.asarray(la[0:3]), np.asarray(la[3:6]), la[6:9]
    d = np.array([math.cos(o.cur_angle), 0.0, -math.sin(o.cur_angle)])
    assert up == [0.0, 1.0, 0.0] and np.allclose(tgt - eye, d, atol=1e-15)
    # model-view = Rx(cam_angle) T(0, 0, forward) LookAt(eye, eye + dir): the eye of the composite sits `forward` ahead of the look-at eye, pitched down
    assert np.allclose(cam.C, eye + raster.CAMERA_FORWARD_DIST * d, atol=1e-15)
    assert cam.sth == math.sin(math.radians(f1(rots[0][0]))) and cam.cth == math.cos(math.radians(f1(rots[0][0])))
    # ---- ground quad: colour, scale and vertices (simulator.py:1806-1812)
    i_g = next(i for i, c in enumerate(calls) if c[0] == "glScalef")
    assert calls[i_g].args == (50, 0.01, 50) and [float(v) for v in calls[i_g - 2].args] == [float(v) for v in o.ground_color]
    assert np.array_equal(cam.ground, np.asarray(o.ground_color, dtype=np.float64)[:3] * 255.0)
    g = gnd_v * np.array([50, 0.01, 50])
    assert raster.GROUND_HALF == 50.0 and set(np.abs(g[:, 0])) == {50.0} and set(np.abs(g[:, 2])) == {50.0} and np.allclose(g[:, 1], raster.GROUND_Y, atol=1e-18)
    # ---- tiles (simulator.py:1853-1884): translate to the tile centre, rotate angle * 90 + 180 about y, the 7 x 7 quad grid with uv = (pu, 1 - pv)
    scene = raster.Scene(o.map, {}, {})
    ts = o.map.tile_size
    tile_calls = [(calls[i + 1].args, calls[i + 2].args) for i, c in enumerate(calls) if c[0] == "glPushMatrix" and calls[i + 2][0] == "glRotatef" and calls[i + 3][0] == "glBindTexture"]
    tiles = [(i, j) for i in range(o.map.grid_width) for j in range(o.map.grid_height) if o.map.grid[j * o.map.grid_width + i] is not None]
    assert len(tile_calls) == len(tiles) == int(scene.present.sum())
    pts = np.random.default_rng(0).uniform(0.02, 0.98, (40, 2))
    for (tr, rot), (i, j) in zip(tile_calls, tiles):
        ang = o.map.grid[j * o.map.grid_width + i]["angle"]
        assert tuple(float(v) for v in tr) == ((i + 0.5) * ts, 0.0, (j + 0.5) * ts) and rot == (ang * 90 + 180, 0, 1, 0)
        th = math.radians(rot[0])
        for fx, fz in pts:                                 # world point of the tile -> the quad's local frame (inverse of glRotatef about y) -> its texture coordinate
            dx, dz = (fx - 0.5) * ts, (fz - 0.5) * ts
            x, z = dx * math.cos(th) - dz * math.sin(th), dx * math.sin(th) + dz * math.cos(th)
            u_ref, v_ref = x / ts + 0.5, 1.0 - (z / ts + 0.5)                                    # get_point: tu = pu, tv = 1 - pv, linear over the grid
            u, v = raster._tile_uv(np.int64(ang), np.float64(fx), np.float64(fz))
            assert abs(float(u) - u_ref) < 1e-12 and abs(float(v) - v_ref) < 1e-12
    assert np.allclose(road_v[:, 1], 0.0) and np.allclose(road_t[:, 0], road_v[:, 0] / ts + 0.5) and np.allclose(road_t[:, 1], 1.0 - (road_v[:, 2] / ts + 0.5))
    assert n_road == 4 * 49 and n_gnd == 4
    # ---- objects (objects.py:123-148): translate(pos) scale(s) rotate(x_rot = 0, y_rot, z_rot = 0), glColor4f(obj colour)
    obj_calls = [(calls[i + 1].args, calls[i + 2].args, calls[i + 4].args) for i, c in enumerate(calls)
                 if c[0] == "glPushMatrix" and calls[i + 2][0] == "glScalef" and calls[i + 2].args != (50, 0.01, 50)]
    vis = [ob for ob in o.map.objects if ob.visible]
    assert len(obj_calls) == len(vis) > 0
    for (tr, sc, ry), ob in zip(obj_calls, vis):
        assert np.array_equal(np.asarray(tr, dtype=np.float64), np.asarray(ob.pos, dtype=np.float64))
        assert float(sc[0]) == float(sc[1]) == float(sc[2]) == float(ob.scale) and float(ry[0]) == float(ob.y_rot) and tuple(ry[1:]) == (0, 1, 0)


@needs_ref
@pytest.mark.parametrize("mode", ["top_down", "bbox"])
def test_window_views_gl_arguments_are_the_facade_s_viewer_camera(mode):
    """render(mode="top_down") and draw_bbox: the reference's model-view for those views (simulator.py:1776-1778, 1786-1798), read from the
    recording gl mock, against gym_duckietown.simulator.viewer_camera (the parameters the facade gives this backend's camera model) -- and,
    for draw_bbox, the line loops it draws (objects.py:131-139, simulator.py:1910-1918) against the collision rectangles the facade outlines."""
    import math
    from unittest.mock import MagicMock
    from gym_duckietown.simulator import viewer_camera
    from oracle import raster
    W, H = 800, 600
    r, ns = _ref("small_loop_only_duckies", False, 9)
    o = osim.OracleSim(assets.get_map("small_loop_only_duckies"), EXT, domain_rand=False, seed=9, do_reset=False)
    gl = ns.simulator.gl
    r.reset(); o.reset()
    r.graphics = True
    r.shadow_window = MagicMock(); r.draw_curve = False; r.enable_leds = False; r.draw_bbox = mode == "bbox"
    r.road_vlist, r.ground_vlist, r.tri_vlist, r.mesh = MagicMock(), MagicMock(), MagicMock(), MagicMock()
    gl.reset_mock()
    with pytest.raises(TypeError):
        r._render_img(W, H, MagicMock(), MagicMock(), np.zeros((H, W, 3), np.uint8), top_down=mode == "top_down", segment=False)
    calls = gl.mock_calls
    i_la = max(i for i, c in enumerate(calls) if c[0] == "gluLookAt")
    la = [float(np.ravel(v)[0]) for v in calls[i_la].args]
    eye, tgt = np.asarray(la[0:3]), np.asarray(la[3:6])
    i_mv = max(i for i, c in enumerate(calls[:i_la]) if c[0] == "glLoadIdentity")
    pre = [c for c in calls[i_mv:i_la] if c[0] in ("glRotatef", "glTranslatef")]
    fov = float(np.ravel(o.cam_fov_y)[0])
    vp, va, vh, vdeg = viewer_camera(mode == "top_down", mode == "bbox", o.cur_pos, o.cur_angle, o.map.grid_width, o.map.grid_height, o.map.tile_size, fov)
    cam = raster.Camera(vp, va, cam_height=vh, cam_angle_deg=vdeg, cam_fov_y_deg=fov, width=W, height=H)
    if mode == "top_down":
        assert pre == []                                                       # no pitch, no forward offset: the look-at alone
        assert np.allclose(cam.C, eye, atol=1e-12)
        fwd = (tgt - eye) / np.linalg.norm(tgt - eye)                          # the view direction of the look-at = the camera's pitched forward axis
        mine = np.array([cam.ca * cam.cth, -cam.sth, -cam.sa * cam.cth])
        assert np.allclose(mine, fwd, atol=1e-12)
        # the agent's own mesh in this view (simulator.py:1920-1927): translate(cur_pos) scale(1) rotate(cur_angle in degrees about y), drawn unscaled
        i_m = max(i for i, c in enumerate(calls) if c[0] == "glScalef")
        assert calls[i_m].args == (1, 1, 1) and np.array_equal(np.asarray(calls[i_m - 1].args, dtype=np.float64), np.asarray(o.cur_pos, dtype=np.float64))
        assert float(calls[i_m + 1].args[0]) == o.cur_angle * 180 / np.pi and tuple(calls[i_m + 1].args[1:]) == (0, 1, 0) and r.mesh.render.called
    else:
        assert [(c[0], c.args) for c in pre] == [("glRotatef", (90, 1, 0, 0))]
        assert np.allclose(cam.C, eye, atol=1e-15) and abs(eye[1] - (o.cur_pos[1] + 0.8)) < 1e-15
        assert abs(cam.sth - 1.0) < 1e-15 and abs(cam.cth) < 1e-15             # looking straight down
        d = np.array([math.cos(o.cur_angle), 0.0, -math.sin(o.cur_angle)])
        assert np.allclose(tgt - eye, d, atol=1e-15)
        # the line loops: every visible object's obj_corners, then the agent's, at y = 0.01 (the objects draw through objects.gl)
        all_v = [tuple(float(v) for v in c.args) for c in calls if c[0] == "glVertex3f"]           # (objects.gl is the same mock: one sequence)
        vis = [ob for ob in o.map.objects if ob.visible]
        assert len(all_v) == 4 * len(vis) + 4
        obj_v = all_v[:-4]
        for k, ob in enumerate(vis):
            c = np.asarray(ob.obj_corners, dtype=np.float64)
            c = c.T if c.shape == (2, 4) else c.reshape(4, 2)
            assert obj_v[4 * k:4 * k + 4] == [(float(c[i, 0]), 0.01, float(c[i, 1])) for i in range(4)]
        ag = all_v[-4:]
        # the agent's rectangle uses `angle` as the tile loop left it (simulator.py:1862 rebinds the name): the last tile's orientation index as radians
        from gym_duckietown.simulator import agent_bbox_angle
        a_box = agent_bbox_angle(o.map.grid, o.map.grid_width, o.map.grid_height, o.cur_angle)
        assert a_box in (0.0, 1.0, 2.0, 3.0)
        want = osim.get_agent_corners(o.cur_pos, a_box)
        assert ag == [(float(want[i, 0]), 0.01, float(want[i, 1])) for i in range(4)]


@needs_ref
def test_segment_view_gl_state_is_the_oracle_s_segment_view():
    """_render_img(segment=True) (simulator.py:1730-1737, 1753, 1808, 1815) under the recording gl mock: lighting, LIGHT0 and COLOR_MATERIAL
    disabled, the colour buffer cleared to and the ground quad drawn in (255, 0, 255), no distractor triangles, the objects rendered with
    segment=True -- what raster.segment_view turns a (camera, scene) into: base 1 / diffuse 0 (fragment = texture x vertex colour), magenta."""
    from unittest.mock import MagicMock
    from oracle import raster
    W, H = 160, 120
    r, ns = _ref("small_loop_only_duckies", False, 11)
    r.reset()
    gl = ns.simulator.gl
    r.graphics = True
    r.shadow_window = MagicMock(); r.draw_curve = False; r.enable_leds = False; r.draw_bbox = False
    r.road_vlist, r.ground_vlist, r.tri_vlist = MagicMock(), MagicMock(), MagicMock()
    for ob in r.objects:
        ob.render = MagicMock()
    gl.reset_mock()
    with pytest.raises(TypeError):
        r._render_img(W, H, MagicMock(), MagicMock(), np.zeros((H, W, 3), np.uint8), top_down=False, segment=True)
    calls = gl.mock_calls
    dis = [c.args[0] for c in calls if c[0] == "glDisable"]
    assert gl.GL_LIGHT0 in dis and gl.GL_LIGHTING in dis and gl.GL_COLOR_MATERIAL in dis
    en = [c.args[0] for c in calls if c[0] == "glEnable"]
    assert gl.GL_LIGHTING not in en and gl.GL_LIGHT0 not in en and gl.GL_COLOR_MATERIAL not in en
    assert [float(v) for v in [c for c in calls if c[0] == "glClearColor"][0].args] == [255.0, 0.0, 255.0, 1.0]
    i_g = next(i for i, c in enumerate(calls) if c[0] == "glScalef")
    assert [float(v) for v in calls[i_g - 2].args] == [255.0, 0.0, 255.0]
    assert not r.tri_vlist.draw.called                                       # "if not segment": no distractors
    assert all(ob.render.call_args.kwargs["segment"] is True for ob in r.objects)
    cam = raster.Camera(r.cur_pos, r.cur_angle, width=W, height=H)
    c2, _ = raster.segment_view(cam, raster.Scene(osim.OracleMap(assets.get_map("small_loop_only_duckies"), EXT), {}, {}), {}, {})
    assert np.array_equal(c2.base, np.ones(3)) and np.array_equal(c2.dif, np.zeros(3))
    assert np.array_equal(c2.horizon, [255.0, 0.0, 255.0]) and np.array_equal(c2.ground, [255.0, 0.0, 255.0])   # (clamped to 1.0 = 255 by the colour buffer)
