"""BatchedSimulator: N Duckietown envs on one MI355X behind libdtsim.so.

Vector counterpart of the reference's Simulator / DuckietownEnv (simulator.py:188,
envs/duckietown_env.py:9): same constructor keywords, same reset/step semantics per
env, batched over env index.  All per-step work happens in the HIP library; this class
only owns host-side set-up (assets, map tables, reset RNG order) and marshals arrays.
"""
from __future__ import annotations

import ctypes as C
import math
from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence, Union

import numpy as np

from . import _ffi, assets, maps, reset as R
from . import distortion as dist_mod


class DeviceArray:
    """Zero-copy view of library-owned device memory (`__cuda_array_interface__`, v2):
    `torch.as_tensor(arr, device="cuda")` wraps it without a copy."""

    def __init__(self, ptr: int, shape, typestr: str, owner):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False),
                                         "version": 2, "strides": None}
        self._owner = owner


def load_scene(library, map_names, datas, transform_uses_width=False, render=True):
    """Host prep of the maps `datas` (MapFormat1 dicts named map_names) against `library`: what scene_ffi takes, as attributes --
    meshes, mesh_order, texture_kinds, textures, mesh_tex_base, light_tex, maps."""
    use_lib = library if library.root else None
    meshes: Dict[str, assets.MeshData] = {"duckie": assets.get_mesh("duckie"), "*": assets.get_mesh("*")}
    first = [maps.interpret_map(d, n, meshes, transform_uses_width, library=use_lib) for d, n in zip(datas, map_names)]
    mesh_order = list(meshes)                      # "duckie", "*", then every object mesh the library loaded
    tex_kinds: List[str] = []
    for mt in first:
        for kd in mt.texture_kinds:
            if kd not in tex_kinds:
                tex_kinds.append(kd)
    tile_tex = [library.tile_texture(kd) for kd in tex_kinds]
    if tile_tex:                                   # the raster needs one size for all tile textures
        side = max(max(t.shape[0], t.shape[1]) for t in tile_tex)
        tile_tex = [assets.to_pow2(t, side) if t.shape[:2] != (side, side) else t for t in tile_tex]
    textures = list(tile_tex)
    mesh_tex_base: Dict[str, int] = {}             # mesh key -> index of its first texture
    for mk in mesh_order:
        mesh_tex_base[mk] = len(textures)
        textures.extend(meshes[mk].textures)
    light_tex = (-1, -1)                           # traffic-light cards (only when a map has lights and the tree has cards)
    if any(o.light_freq > 0 for mt in first for o in mt.objects):
        cards = library.light_cards()
        if cards is not None:
            light_tex = (len(textures), len(textures) + 1)
            textures.extend(cards)
    tex_ids = {kd: i for i, kd in enumerate(tex_kinds)} if render else None
    map_tables = [maps.interpret_map(d, n, meshes, transform_uses_width, texture_ids=tex_ids, library=use_lib)
                  for d, n in zip(datas, map_names)]
    return SimpleNamespace(meshes=meshes, mesh_order=mesh_order, texture_kinds=tex_kinds, textures=textures, mesh_tex_base=mesh_tex_base,
                           light_tex=light_tex, maps=map_tables)


def scene_ffi(sc, render=True):
    """The arguments of dtsim_set_assets and dtsim_set_maps for load_scene's `sc`: (Texture array, Mesh array, Map array, keep).  The
    ctypes arrays borrow numpy arrays: `keep` and `sc` must outlive their use.  render=False: no assets (null arrays), and maps that
    name no mesh or light texture."""
    textures, meshes, mesh_order, mesh_tex_base = sc.textures, sc.meshes, sc.mesh_order, sc.mesh_tex_base
    keep = []
    tarr = marr = None
    if render:
        tarr = (_ffi.Texture * max(len(textures), 1))()
        for i, t in enumerate(textures):
            tarr[i].width, tarr[i].height = t.shape[1], t.shape[0]
            tarr[i].rgba = t.ctypes.data_as(C.POINTER(C.c_uint8))
        marr = (_ffi.Mesh * len(mesh_order))()
        for i, mk in enumerate(mesh_order):
            m = meshes[mk]
            marr[i].n_tris = m.n_tris
            marr[i].verts = m.verts.ctypes.data_as(C.POINTER(C.c_float))
            marr[i].normals = m.normals.ctypes.data_as(C.POINTER(C.c_float))
            marr[i].colors = m.colors.ctypes.data_as(C.POINTER(C.c_float))
            if m.textures:
                gt = np.where(m.tri_tex >= 0, m.tri_tex + mesh_tex_base[mk], -1).astype(np.int32)
                keep.append(gt)
                marr[i].uvs = m.uvs.ctypes.data_as(C.POINTER(C.c_float))
                marr[i].tri_tex = gt.ctypes.data_as(C.POINTER(C.c_int32))
    mesh_ids = {mk: i for i, mk in enumerate(mesh_order)} if render else {}
    farr = (_ffi.Map * len(sc.maps))()
    for i, mt in enumerate(sc.maps):
        farr[i] = mt.to_ffi(mesh_ids, sc.light_tex if render else (-1, -1))
    return tarr, marr, farr, keep


class BatchedSimulator:
    def __init__(self, map_name: Union[str, Sequence[str]] = "small_loop", num_envs: int = 1, *,
                 max_steps: int = 1500, domain_rand: bool = True, frame_rate: float = 30, frame_skip: int = 1,
                 camera_width: int = 640, camera_height: int = 480, robot_speed: float = 1.20,
                 accept_start_angle_deg: float = 60, user_tile_start=None, seed: Optional[int] = None,
                 distortion: bool = False, dynamics_rand: bool = False, camera_rand: bool = False,
                 num_tris_distractors: int = 12, color_ground=(0.15, 0.15, 0.15), color_sky=R.BLUE_SKY,
                 # DuckietownEnv (envs/duckietown_env.py:15)
                 action_mode: str = "wheels", gain=1.0, trim=0.0, radius=0.0318, k=27.0, limit=1.0,
                 # batched / device options
                 render: bool = True, auto_reset: bool = False, delay_steps: Optional[int] = None, device: int = 0,
                 stream: Optional[int] = None, profile: bool = False, actions_f64: bool = False,
                 map_cycle: bool = False, map_random: bool = False, transform_uses_width: bool = False,
                 map_data: Optional[dict] = None,
                 asset_root: Optional[str] = None, style: str = "photos", device_reset: bool = False,
                 undistort: bool = False, per_env_camera: bool = False, light_capture: bool = False,
                 camera_rand_pool: Optional[int] = None, do_reset: bool = True):
        self._lib = _ffi.load()
        self._h = C.c_void_p()
        self._device = int(device)
        self.num_envs = int(num_envs)
        self.max_steps, self.domain_rand = max_steps, bool(domain_rand)
        self.frame_rate, self.frame_skip = frame_rate, int(frame_skip)
        self.delta_time = 1.0 / frame_rate
        if delay_steps is None:
            # the DB18 model's actuation delay is 0.15 s of simulated time (simulator.py:745-755, get_DB18_nominal(delay=0.15)):
            # the smallest k with k * delta_time >= 0.15 -- 5 steps at the default 30 Hz
            delay_steps = int(math.ceil(0.15 * frame_rate - 1e-9))
        if not 0 <= int(delay_steps) <= _ffi.MAX_DELAY:
            raise ValueError(f"delay_steps {delay_steps} (0.15 s at frame_rate {frame_rate}) outside [0, {_ffi.MAX_DELAY}] (DTSIM_MAX_DELAY)")
        self.delay_steps = int(delay_steps)
        self.camera_width, self.camera_height = int(camera_width), int(camera_height)
        self.robot_speed = robot_speed
        self.accept_start_angle_deg = accept_start_angle_deg
        self.user_tile_start = user_tile_start
        self.distortion = bool(distortion)
        self.dynamics_rand, self.camera_rand = bool(dynamics_rand), bool(camera_rand)
        self.num_tris_distractors = num_tris_distractors
        self.color_ground, self.color_sky = color_ground, list(color_sky)
        self.action_mode = action_mode
        self.render_enabled = bool(render)
        self.auto_reset = bool(auto_reset)
        self.actions_f64 = bool(actions_f64)
        self.map_cycle = bool(map_cycle)
        self.map_random = bool(map_random)     # randomize_maps_on_reset: a uniformly drawn map, reloaded, at every reset
        self.seed_value = seed
        self._bufs = {}                         # the methods' own result buffers, by method name (_result)
        self._have_label_assets = False         # set_label_assets() has run (_need_label_assets)
        self._mesh_class = None                 # its mesh table (object_classes())

        flags = 0
        flags |= _ffi.F_RENDER if render else 0
        flags |= _ffi.F_DISTORTION if (render and distortion) else 0
        # per_env_camera: render through the per-env camera / light path (the device flag of domain randomisation) while the reset draws stay
        # those of domain_rand=False -- for callers that write a per-env light or camera themselves (the gym facade's GL light capture)
        self.per_env_camera = bool(per_env_camera)
        if self.per_env_camera and not domain_rand and (device_reset or auto_reset):
            # the device sampler (physics.hip sample_init) always draws a camera_noise, and the per-env render path applies it: with
            # domain_rand off the frames after a device-side reset would be jittered while the reference's are not
            raise ValueError("per_env_camera with domain_rand=False needs host-side resets (device_reset / auto_reset draw a camera noise "
                             "that this render path would apply)")
        # camera_rand with the fisheye (simulator.py:352-358): a calibration per env -- the frames are gathered through per-env remap
        # tables (dtsim_set_distortion_luts) -- and reset() scales camera height / angle / fov_y even without domain_rand (:611-614),
        # so the frames go through the per-env camera path.  Without distortion camera_rand keeps its reset-only effect.
        self.camera_rand_on = bool(camera_rand and distortion and render)
        if self.camera_rand_on and light_capture:
            raise ValueError("camera_rand with light_capture is not supported (the per-env fisheye renders through the per-env camera path)")
        flags |= _ffi.F_DOMAIN_RAND if (domain_rand or per_env_camera or self.camera_rand_on) else 0
        flags |= _ffi.F_AUTO_RESET if auto_reset else 0
        # light_capture (DTSIM_F_LIGHT_CAPTURE): device-side resets take the new episode's light through the camera of the pose the previous
        # episode ended at, as GL does with reset()'s glLightfv (simulator.py:565-584).  With domain_rand=False the shared-camera render then
        # lights each env with its own light (ABI v12: the LIGHT instantiations of the quad rasters).
        self.light_capture = bool(light_capture)
        flags |= _ffi.F_LIGHT_CAPTURE if self.light_capture else 0
        flags |= _ffi.F_ACTIONS_F64 if actions_f64 else 0
        flags |= _ffi.F_PROFILE if profile else 0
        cfg = _ffi.Config()
        cfg.struct_size = C.sizeof(_ffi.Config)
        cfg.flags, cfg.num_envs, cfg.device = flags, self.num_envs, int(device)
        cfg.cam_width, cfg.cam_height = self.camera_width, self.camera_height
        cfg.frame_skip, cfg.max_steps, cfg.delay_steps = self.frame_skip, int(max_steps), int(delay_steps)
        cfg.action_mode = {"wheels": _ffi.ACTION_WHEELS, "vel_steer": _ffi.ACTION_VEL_STEER}[action_mode]
        cfg.delta_time, cfg.robot_speed = self.delta_time, float(robot_speed)
        cfg.gain, cfg.trim, cfg.radius, cfg.k, cfg.limit = float(gain), float(trim), float(radius), float(k), float(limit)
        cfg.stream = C.c_void_p(stream) if stream else None
        _ffi.check(self._lib, self._lib.dtsim_create(C.byref(cfg), C.byref(self._h)))

        # ---- maps + assets (one-time host prep)
        # Assets come from `asset_root` (or $DTSIM_ASSET_ROOT: a duckietown-world style data tree with
        # MapFormat1 YAML maps, tiles-processed/<style>/<kind>/texture.* and <kind>.obj/.mtl meshes)
        # with the deterministic fixtures of dtsim/assets.py as the fallback.
        self.state_version = 0
        self.library = assets.AssetLibrary(asset_root, style)
        names = [map_name] if isinstance(map_name, str) else list(map_name)
        datas = [map_data] if (map_data is not None) else [self.library.map_data(n) for n in names]
        self.map_names = [assets.map_basename(n) for n in names]
        self.map_datas, self._ctor_map_names = datas, names
        sc = load_scene(self.library, self.map_names, datas, transform_uses_width, render)
        self.meshes, self._mesh_order, self.texture_kinds, self.textures = sc.meshes, sc.mesh_order, sc.texture_kinds, sc.textures
        self.light_tex, self.maps = sc.light_tex, sc.maps
        self._have_segment_assets = False
        tarr, marr, farr, self._scene_keep = scene_ffi(sc, render)
        if render:
            _ffi.check(self._lib, self._lib.dtsim_set_assets(self._h, tarr, len(self.textures), marr, len(sc.mesh_order)))
        _ffi.check(self._lib, self._lib.dtsim_set_maps(self._h, farr, len(self.maps)))
        self.undistort = bool(undistort and distortion)
        self._skip_distort = False
        self._cal = None
        if self.camera_rand_on and not self.undistort:
            P = min(self.num_envs, 64) if camera_rand_pool is None else int(camera_rand_pool)
            if not 1 <= P <= self.num_envs:
                raise ValueError(f"camera_rand_pool {camera_rand_pool}: need 1 <= pool <= num_envs ({self.num_envs})")
            K, D = dist_mod.sample_calibrations(P, seed)
            self.set_camera_calibrations(K, D, np.arange(self.num_envs) % P)
        elif render and distortion:
            # undistort=True: UndistortWrapper(env) -- the simulator's fisheye is skipped (env.undistort, simulator.py:1969)
            # and the wrapper's rectify map is the per-pixel source map instead (wrappers.py:209-227)
            rmx, rmy = (dist_mod.undistort_wrapper_maps if self.undistort else dist_mod.distortion_maps)(
                self.camera_width, self.camera_height)
            self.rmapx, self.rmapy = rmx, rmy
            _ffi.check(self._lib, self._lib.dtsim_set_distortion_lut(
                self._h, rmx.ctypes.data_as(C.POINTER(C.c_float)), rmy.ctypes.data_as(C.POINTER(C.c_float))))
            if self.camera_rand_on:
                # undistort=True with camera_rand: no per-env tables (the wrapper skips the simulator's fisheye), but the device reset
                # sampler still scales the camera and zeroes its noise (the per-env camera path would apply a drawn one)
                _ffi.check(self._lib, self._lib.dtsim_set_distortion_luts(self._h, 0, None, None, _ffi.LUTS_CAMERA_RAND))
            self._install_ipm_calibrations()                 # ipm() projects through the nominal calibration

        # ---- per-env host reset state (RNG order lives on the host; reset.py)
        self.env_state = [R.EnvResetState(None if seed is None else seed + e) for e in range(self.num_envs)]
        self.env_map = np.zeros(self.num_envs, np.int32)
        self.init_states = (_ffi.InitState * self.num_envs)()
        self._have_reset = False
        self.device_reset = bool(device_reset)
        if self.device_reset:
            self.install_reset_sampler()
        if do_reset:
            self.reset()

    # ------------------------------------------------------------------ reset --
    def install_reset_sampler(self, seed: Optional[int] = None):
        """Device-side reset sampling (dtsim_reset_sampler): reset() and auto-reset then draw DR values and
        spawn poses on the GPU (the reference's distributions and acceptance test, Philox stream) instead
        of on the host in numpy's RNG order."""
        rs = _ffi.ResetSampler()
        sv = self.seed_value if seed is None else seed
        rs.seed = int(sv if sv is not None else np.random.SeedSequence().entropy) & 0xFFFFFFFFFFFFFFFF
        rs.domain_rand, rs.dynamics_rand = int(self.domain_rand), int(self.dynamics_rand)
        rs.map_cycle = 2 if self.map_random else int(self.map_cycle and len(self.maps) > 1)
        rs.max_attempts = R.MAX_SPAWN_ATTEMPTS
        rs.accept_start_angle_deg = float(self.accept_start_angle_deg)
        rs.color_sky[:] = [float(v) for v in self.color_sky]
        rs.color_ground[:] = [float(v) for v in self.color_ground]
        for m in range(_ffi.MAX_MAPS):
            tile = (-1, -1)
            if m < len(self.maps):
                if self.user_tile_start:
                    tile = tuple(int(v) for v in self.user_tile_start)
                elif self.maps[m].start_tile is not None:
                    tile = tuple(int(v) for v in self.maps[m].start_tile)
            rs.start_tile[m][0], rs.start_tile[m][1] = tile
            sp = self.maps[m].start_pose if m < len(self.maps) else None
            rs.has_start_pose[m] = 0 if sp is None else 1
            if sp is not None:                          # [[x, y, z], angle] relative to the start tile (simulator.py:679-688)
                rs.start_pose[m][0], rs.start_pose[m][1], rs.start_pose[m][2] = float(sp[0][0]), float(sp[0][2]), float(sp[1])
        _ffi.check(self._lib, self._lib.dtsim_set_reset_sampler(self._h, C.byref(rs)))
        self._sampler = rs

    def _map_for_reset(self, e: int) -> int:
        if self.map_random:                    # simulator.py:541-544: np_random.choice(map_names), the first draw of reset()
            return int(self.env_state[e].np_random.integers(0, len(self.maps)))
        if len(self.maps) == 1:
            return 0
        if not self.map_cycle:
            return e % len(self.maps)          # fixed assignment
        es = self.env_state[e]
        es.map_slot = (es.map_slot + 1) % len(self.maps)   # envs/multimap_env.py:46 (first reset -> 1)
        return es.map_slot

    def sample_states(self, envs: Sequence[int]) -> None:
        """Simulator.reset() for the given envs: fills self.init_states[e] (host draws in
        the reference order; geometry on the device via dtsim_query)."""
        envs = [int(e) for e in envs]
        pend = {}
        vis_all = None
        for e in envs:
            mi = self._map_for_reset(e)
            mt = self.maps[mi]
            st, tile, visible = R.draw_prefix(
                self.env_state[e], mt, domain_rand=self.domain_rand, camera_rand=self.camera_rand,
                dynamics_rand=self.dynamics_rand, color_sky=self.color_sky, color_ground=self.color_ground,
                num_tris_distractors=self.num_tris_distractors, n_visible_draw=(), user_tile_start=self.user_tile_start)
            st.map_id = mi | (_ffi.MAP_RELOAD if self.map_random else 0)
            if (self.per_env_camera or self.camera_rand_on) and not self.domain_rand:
                st.camera_noise[:] = [0.0, 0.0, 0.0]             # drawn, but only applied under domain_rand (simulator.py:1768-1769)
            self.init_states[e] = st
            self.env_state[e].spawn_attempts = 0
            if mt.start_pose is not None:                       # simulator.py:679-688
                i, j = tile
                sp = mt.start_pose
                st.pos[:] = [i * mt.tile_size + sp[0][0], 0.0, j * mt.tile_size + sp[0][2]]
                st.angle = float(sp[1])
                self.init_states[e] = st
            else:
                pend[e] = (mt, tile, visible)
        if not pend:
            return
        # The device evaluates candidates against each env's *current* world; a map switch
        # or a first reset must create that world first: provisional reset at a dummy pose.
        need_world = [e for e in pend if (not self._have_reset) or self.map_random
                      or self.env_map[e] != (self.init_states[e].map_id & ~_ffi.MAP_RELOAD)]
        if need_world:
            mask = np.zeros(self.num_envs, np.uint8)
            for e in need_world:
                mask[e] = 1
                self.init_states[e].pos[:] = [0.0, 0.0, 0.0]
                self.init_states[e].angle = 0.0
            self._reset_device(mask)
            for e in need_world:                               # the objects are fresh now: the final reset must keep them
                self.init_states[e].map_id &= ~_ffi.MAP_RELOAD
        self._write_visibility({e: pend[e][2] for e in pend})
        active = dict(pend)
        while active:
            q_env, q_pose, spans = [], [], {}
            for e, (mt, tile, _) in active.items():
                blk = R.attempt_block(self.env_state[e], tile, mt.tile_size)
                spans[e] = (len(q_env), blk)
                q_env.extend([e] * len(blk))
                q_pose.append(blk)
            probes = self.query(np.array(q_env, np.int32), np.concatenate(q_pose, axis=0), safety_factor=1.3)
            nxt = {}
            for e, (off, blk) in spans.items():
                es = self.env_state[e]
                k = len(blk)
                M = self.accept_start_angle_deg
                p = probes[off:off + k]
                ok = (~p["inconvenient"].astype(bool)) & p["valid"].astype(bool) & p["in_lane"].astype(bool) \
                    & (-M < p["angle_deg"]) & (p["angle_deg"] < M)
                budget = R.MAX_SPAWN_ATTEMPTS - es.spawn_attempts
                idx = np.flatnonzero(ok[:budget])
                st = self.init_states[e]
                if idx.size:
                    a = int(idx[0])
                    R.commit_attempts(es, a + 1)
                    st.pos[:] = [float(blk[a, 0]), 0.0, float(blk[a, 1])]
                    st.angle = float(blk[a, 2])
                elif budget <= k:                              # simulator.py:732-736 fallback pose
                    R.commit_attempts(es, budget)
                    st.pos[:] = [1.0, 0.0, 1.0]
                    st.angle = 1.0
                else:
                    R.commit_attempts(es, k)
                    nxt[e] = active[e]
                self.init_states[e] = st
            active = nxt

    def _write_visibility(self, vis: Dict[int, List[bool]]):
        if all(all(v) for v in vis.values()) and not getattr(self, "_vis_dirty", False):
            return
        self._vis_dirty = True
        arr = self.read(_ffi.FIELD_OBJ_VISIBLE)
        for e, v in vis.items():
            arr[e, :] = 1
            arr[e, :len(v)] = np.asarray(v, np.uint8)
        self.write(_ffi.FIELD_OBJ_VISIBLE, arr)

    def _reset_device(self, mask: Optional[np.ndarray]):
        mp = mask.ctypes.data_as(C.POINTER(C.c_uint8)) if mask is not None else None
        _ffi.check(self._lib, self._lib.dtsim_reset(self._h, mp, self.init_states))
        sel = range(self.num_envs) if mask is None else np.flatnonzero(mask)
        for e in sel:
            self.env_map[e] = self.init_states[e].map_id & ~_ffi.MAP_RELOAD
        self._have_reset = True

    def reset(self, mask: Optional[np.ndarray] = None, states=None):
        """Simulator.reset() for the masked envs (None = all).  `states`: optional
        ctypes array / list of _ffi.InitState to use instead of sampling (parity mode)."""
        self.state_version += 1                       # any cached read-back of the state is stale now
        if not self._have_reset:
            mask = None                        # the first reset creates every env's world
        if self.device_reset and states is None:
            m = None if mask is None else np.ascontiguousarray(np.asarray(mask).astype(np.uint8))
            mp = m.ctypes.data_as(C.POINTER(C.c_uint8)) if m is not None else None
            _ffi.check(self._lib, self._lib.dtsim_reset(self._h, mp, None))
            self.env_map[:] = self.read(_ffi.FIELD_MAP_ID)
            self._have_reset = True
            return
        sel = list(range(self.num_envs)) if mask is None else [int(e) for e in np.flatnonzero(mask)]
        if states is not None:
            for e in sel:
                self.init_states[e] = states[e]
        else:
            self.sample_states(sel)
        m = None
        if mask is not None:
            m = np.ascontiguousarray(np.asarray(mask).astype(np.uint8))
        self._reset_device(m)

    def reset_done(self):
        """Restart (device sampler) every env whose done flag is set; asynchronous, no host round trip."""
        self.state_version += 1                       # any cached read-back of the state is stale now
        _ffi.check(self._lib, self._lib.dtsim_reset_done(self._h))

    def field_device(self, field: int) -> DeviceArray:
        """Zero-copy device view of one SoA field ([N, ...] as documented in include/dtsim.h)."""
        dt, shp = self._FIELD_SHAPES[field]
        if shp != ():
            raise ValueError("device views are offered for the scalar per-env fields (the state is SoA: [component][N])")
        ptr = self._lib.dtsim_field_devptr(self._h, field)
        if not ptr:
            raise ValueError(f"field {field} has no contiguous device view")
        ts = {"f8": "<f8", "u1": "|u1", "i4": "<i4"}[dt]
        return DeviceArray(ptr, (self.num_envs,), ts, self)

    def make_spawn_pool(self, n_pool: int):
        """Pre-sample `n_pool` spawn states (env e%N's RNG stream) for DTSIM_F_AUTO_RESET."""
        pool = (_ffi.InitState * n_pool)()
        saved = [(_ffi.InitState.from_buffer_copy(self.init_states[e])) for e in range(self.num_envs)]
        done = 0
        while done < n_pool:
            batch = min(self.num_envs, n_pool - done)
            self.sample_states(range(batch))
            for e in range(batch):
                pool[done + e] = self.init_states[e]
            done += batch
        for e in range(self.num_envs):
            self.init_states[e] = saved[e]
        _ffi.check(self._lib, self._lib.dtsim_set_spawn_pool(self._h, pool, n_pool))
        self._pool = pool
        return pool

    def skip_distort(self, flag: bool):
        """`env.undistort = True` (simulator.py:1968-1970, 2001; set by UndistortWrapper, wrappers.py:209): render_obs
        returns the rectilinear image, i.e. the per-pixel source map becomes the identity; False restores the fisheye."""
        flag = bool(flag) and self.distortion and self.render_enabled
        if flag == self._skip_distort:
            return
        self._skip_distort = flag
        fp = C.POINTER(C.c_float)
        if self._cal is not None and not flag:
            self._install_calibrations()
        elif flag:
            _ffi.check(self._lib, self._lib.dtsim_set_distortion_lut(self._h, fp(), fp()))
        else:
            _ffi.check(self._lib, self._lib.dtsim_set_distortion_lut(self._h, self.rmapx.ctypes.data_as(fp), self.rmapy.ctypes.data_as(fp)))
        self._install_ipm_calibrations()

    def set_camera_calibrations(self, K, D, env_cal):
        """Install calibrations for the fisheye (camera_rand): K [P,3,3], D [P,5] (plumb-bob k1, k2, p1, p2, k3 -- e.g. a real
        Duckiebot's measured calibration) and env_cal [N] in [0, P), the calibration of every env.  The remap tables
        (dtsim.distortion.build_src_index, bit-identical to the reference's construction) are built on the host, and every render
        then gathers each env's frame through its own table.  Needs distortion=True; not with undistort=True (the wrapper skips
        the simulator's fisheye), light_capture, or the overlays (draw_lines / draw_leds)."""
        if not (self.distortion and self.render_enabled):
            raise ValueError("set_camera_calibrations needs distortion=True (and render=True)")
        if self.undistort:
            raise ValueError("set_camera_calibrations with undistort=True: UndistortWrapper skips the simulator's fisheye")
        if self.light_capture:
            raise ValueError("set_camera_calibrations with light_capture is not supported")
        K = np.ascontiguousarray(np.asarray(K, np.float64))
        D = np.ascontiguousarray(np.asarray(D, np.float64))
        if K.ndim != 3 or K.shape[1:] != (3, 3) or D.shape != (K.shape[0], 5) or K.shape[0] < 1:
            raise ValueError(f"K [P,3,3] and D [P,5]: got {K.shape} and {D.shape}")
        env_cal = np.ascontiguousarray(np.asarray(env_cal), np.int32)
        if env_cal.shape != (self.num_envs,) or env_cal.min() < 0 or env_cal.max() >= K.shape[0]:
            raise ValueError(f"env_cal: need [{self.num_envs}] indices in [0, {K.shape[0]})")
        src = dist_mod.build_src_index(K, D, self.camera_width, self.camera_height)
        new_K = np.stack([dist_mod.optimal_new_camera_matrix(K[i], D[i]) for i in range(K.shape[0])])
        self._cal = (K, D, new_K, env_cal, src)
        if not self._skip_distort:
            self._install_calibrations()
        self._install_ipm_calibrations()

    def _install_calibrations(self):
        _, _, _, env_cal, src = self._cal
        ip = C.POINTER(C.c_int32)
        _ffi.check(self._lib, self._lib.dtsim_set_distortion_luts(self._h, int(src.shape[0]), src.ctypes.data_as(ip), env_cal.ctypes.data_as(ip),
                                                                  _ffi.LUTS_CAMERA_RAND if self.camera_rand_on else 0))

    @property
    def camera_calibrations(self):
        """(K [P,3,3], D [P,5], new_K [P,3,3], env_cal [N]) of the installed calibrations, or None."""
        return None if self._cal is None else tuple(a.copy() for a in self._cal[:4])

    # ------------------------------------------------------------------- step --
    def step(self, actions, n_steps: int = 1, flags: int = 0):
        """actions: [n_steps, N, 2] or [N, 2] (float32, or float64 with actions_f64);
        numpy array (host) or an object with __cuda_array_interface__ (device).
        flags: _ffi.STEP_ONE_UPDATE (one update_physics, no frame_skip) / _ffi.STEP_POSE_ONLY (`_update_pos`)."""
        self.state_version += 1                       # any cached read-back of the state is stale now
        if hasattr(actions, "__cuda_array_interface__"):
            ptr = actions.__cuda_array_interface__["data"][0]
            _ffi.check(self._lib, self._lib.dtsim_step_ex(self._h, C.c_void_p(ptr), int(n_steps), 1, int(flags)))
            return
        dt = np.float64 if self.actions_f64 else np.float32
        a = np.ascontiguousarray(np.asarray(actions, dtype=dt))
        if a.size != n_steps * self.num_envs * 2:
            raise ValueError(f"actions has {a.size} elements, expected {n_steps}*{self.num_envs}*2")
        _ffi.check(self._lib, self._lib.dtsim_step_ex(self._h, a.ctypes.data_as(C.c_void_p), int(n_steps), 0, int(flags)))

    def _mask_ptr(self, mask) -> int:
        """Device pointer of a per-env mask: a CUDA uint8 / bool tensor of shape [N] on the handle's device (contiguous), else ValueError."""
        import torch
        if not isinstance(mask, torch.Tensor) or mask.device.type != "cuda" or mask.device.index != self.device_index:
            raise ValueError(f"mask: need a CUDA tensor on cuda:{self.device_index}, got {type(mask).__name__}"
                             f"{' on ' + str(mask.device) if isinstance(mask, torch.Tensor) else ''}")
        if mask.dtype not in (torch.uint8, torch.bool) or tuple(mask.shape) != (self.num_envs,) or (self.num_envs > 1 and mask.stride(0) != 1):
            raise ValueError(f"mask: need a contiguous uint8 / bool tensor of shape ({self.num_envs},), got {mask.dtype} of shape {tuple(mask.shape)}")
        return mask.data_ptr()

    def _mask_arg(self, mask):
        """An optional per-env mask as the C argument: None, or the device pointer of a mask _mask_ptr accepts."""
        return None if mask is None else C.c_void_p(self._mask_ptr(mask))

    def _dev_tensor(self, t, who: str, lead: Optional[int] = None, shape=None, dtypes=None):
        """`t` if it is a contiguous CUDA tensor on the handle's device -- with leading dimension `lead`, of exactly `shape`, of one of
        `dtypes`, where given --, else ValueError."""
        import torch
        dev = torch.device("cuda", self.device_index)
        if not isinstance(t, torch.Tensor) or t.device != dev or not t.is_contiguous() \
                or (lead is not None and (t.dim() < 1 or t.shape[0] != lead)) or (shape is not None and tuple(t.shape) != tuple(shape)):
            raise ValueError(f"{who} must be a contiguous CUDA tensor on {dev}" + (f" with leading dimension {lead}" if lead is not None else "")
                             + (f" of shape {tuple(shape)}" if shape is not None else ""))
        if dtypes is not None and t.dtype not in dtypes:
            raise ValueError(f"{who} must be {' or '.join(str(d)[6:] for d in dtypes)}, got {t.dtype}")
        return t

    @staticmethod
    def _out_ptr(out, shape, typestr: str, item: int, who: str) -> int:
        """The data pointer of a device output: any object with __cuda_array_interface__ of exactly `shape` and `typestr` (`item` bytes per
        element), C-contiguous, else ValueError -- the kernels write exactly this layout from the pointer: anything else would be misread
        or overrun."""
        ai = getattr(out, "__cuda_array_interface__", None)
        if ai is None:
            raise ValueError(f"{who}: out needs __cuda_array_interface__ (a device array), got {type(out).__name__}")
        c_strides = tuple(int(np.prod(shape[i + 1:])) * item for i in range(len(shape)))
        strides = ai.get("strides")
        if tuple(ai["shape"]) != shape or ai["typestr"] != typestr or not (
                strides is None or all(s == c for s, c, n in zip(strides, c_strides, shape) if n > 1)):
            raise ValueError(f"{who}: out: need a C-contiguous {typestr} array of shape {shape}, got shape {tuple(ai['shape'])}, "
                             f"typestr {ai['typestr']!r}, strides {strides}")
        return ai["data"][0]

    _TYPESTR = {"float32": ("<f4", 4), "float16": ("<f2", 2), "uint8": ("|u1", 1), "int32": ("<i4", 4)}

    def _result(self, who: str, out, shape, dtype: str = "uint8"):
        """(out, its device pointer) of method `who`: `out` as _out_ptr accepts it or, for None, the method's own buffer -- allocated at first
        use and again when the shape or dtype asked for changes."""
        if out is None:
            import torch
            out = self._bufs.get(who)
            if out is None or tuple(out.shape) != shape or out.dtype != getattr(torch, dtype):
                # (empty: a fill would run on torch's stream, unordered against the handle's own, and race with the kernel's stores; a
                # first call that is masked leaves the other rows uninitialised)
                out = self._bufs[who] = torch.empty(shape, dtype=getattr(torch, dtype), device=f"cuda:{self.device_index}")
        return out, C.c_void_p(self._out_ptr(out, shape, *self._TYPESTR[dtype], who))

    def _map_size(self, who: str, noun: str, height, width):
        """(h, w) of a camera post-pass's map: the camera's size, or a divisor of it, else ValueError."""
        h = self.camera_height if height is None else int(height)
        w = self.camera_width if width is None else int(width)
        if h <= 0 or w <= 0 or self.camera_height % h or self.camera_width % w:
            raise ValueError(f"{who}: a {h} x {w} map of {self.camera_height} x {self.camera_width} frames -- each size must divide the camera's "
                             f"({noun} point-sampled, never filtered)")
        return h, w

    def _need_label_assets(self):
        """The default label tables, installed at the first use of a pass that reads them."""
        if not self._have_label_assets:
            self.set_label_assets()

    def _map_pass(self, fn, fn_masked, mp, *args):
        """fn(handle, *args), or with a mask fn_masked(handle, *args, mask): a pass whose masked form takes the mask last."""
        _ffi.check(self._lib, fn(self._h, *args) if mp is None else fn_masked(self._h, *args, mp))

    def _env_tables_flag(self) -> int:
        """DTSIM_MAP_ENV_TABLES exactly while per-env calibrations are active (camera_rand, set_camera_calibrations): depth(), labels() and
        instances() then read each env's own distortion table.  0 in every other configuration: its calls stay as they are."""
        return _ffi.MAP_ENV_TABLES if self._cal is not None and not self._skip_distort else 0

    def render(self, segment: bool = False, gl_filter: bool = False, mask=None):
        """render_obs() of every env into the frame batch; `segment=True` is the reference's segmentation render
        (simulator.py:1730-1737,1753,1808,1879).  `gl_filter=True` (DTSIM_RENDER_GL_FILTER): tile textures filtered with the arithmetic of the
        reference's renderer (Mesa llvmpipe's 8-bit GL_LINEAR) by the generic raster -- frames bit-identical to the reference's on 99.2 - 99.96 % of
        the pixels, 2 - 4 x slower than the quad-record kernels: for validation, not for throughput.
        `mask` (CUDA uint8 / bool tensor [N] on the handle's device; anything else raises ValueError before a launch): dtsim_render_masked --
        only the selected envs are rendered, the other frames keep their bytes (the generic pipelines re-render them unchanged)."""
        flags = _ffi.RENDER_GL_FILTER if gl_filter else 0
        mp = self._mask_arg(mask)
        if segment:
            if not self._have_segment_assets:
                self._install_segment_assets()
            flags |= _ffi.RENDER_SEGMENT
        if mp is None:
            _ffi.check(self._lib, self._lib.dtsim_render_ex(self._h, flags))
        else:
            _ffi.check(self._lib, self._lib.dtsim_render_masked(self._h, flags, mp))

    _PIPE_NAMES = {_ffi.PIPE_GENERIC: "k_raster", _ffi.PIPE_GENERIC_ENV: "k_raster_env", _ffi.PIPE_Q: "k_raster_q",
                   _ffi.PIPE_V3: "k_raster_v3", _ffi.PIPE_V3DR: "k_raster_v3dr"}

    @property
    def render_pipeline(self) -> Optional[str]:
        """The raster of the last render() (DTSIM_FIELD_RENDER_PIPE): "k_raster_v3", "k_raster_q", "k_raster" (the shared camera),
        "k_raster_env" (the generic raster through each env's camera record), "k_raster_v3dr" (domain randomisation); "+light" is appended when
        the shared camera lit each env with its own light (light_capture).  None before the first pass."""
        code = int(self.read(_ffi.FIELD_RENDER_PIPE)[0])
        if not code:
            return None
        name = self._PIPE_NAMES[code & (_ffi.PIPE_ENV_LIGHT - 1)]
        return name + ("+light" if code & _ffi.PIPE_ENV_LIGHT else "")

    def segment_assets(self):
        """(segmented textures mirroring self.textures, per-mesh flat colours [n_meshes,3]) -- host prep of the
        segmentation render: tile textures through load_texture(segment=True) (graphics.py:70-126, into black),
        mesh textures and meshes through gen_segmentation_color(mesh_name) (objmesh.py:255-292)."""
        import os
        lib = self.library
        seg_tex = []
        for i, kd in enumerate(self.texture_kinds):
            p = lib.tile_texture_file(kd) if lib.root else None
            hint = p if p else os.path.join("tiles-processed", lib.style, kd, "texture.png")
            seg_tex.append(assets.segment_texture(self.textures[i], hint))
        rgb = np.zeros((len(self._mesh_order), 3), np.uint8)
        k = len(self.texture_kinds)
        for mi, mk in enumerate(self._mesh_order):
            m = self.meshes[mk]
            col = assets.gen_segmentation_color(getattr(m, "seg_name", None) or (mk if len(mk) >= 3 else "object"))
            rgb[mi] = col
            for t in m.textures:                   # only ever sampled through the flat colour (st.tex = -1 on the device)
                seg_tex.append(assets.segment_texture(t, "mesh", col))
                k += 1
        while len(seg_tex) < len(self.textures):   # traffic-light cards: a segmented mesh has no switching card
            seg_tex.append(assets.segment_texture(self.textures[len(seg_tex)], "trafficlight"))
        return seg_tex, rgb

    def _install_segment_assets(self):
        seg_tex, rgb = self.segment_assets()
        tarr = (_ffi.Texture * max(len(seg_tex), 1))()
        for i, t in enumerate(seg_tex):
            tarr[i].width, tarr[i].height = t.shape[1], t.shape[0]
            tarr[i].rgba = t.ctypes.data_as(C.POINTER(C.c_uint8))
        _ffi.check(self._lib, self._lib.dtsim_set_segment_assets(
            self._h, tarr, len(seg_tex), rgb.ctypes.data_as(C.POINTER(C.c_uint8)), len(self._mesh_order)))
        self._have_segment_assets = True

    def frames_device(self) -> DeviceArray:
        ptr = self._lib.dtsim_frames_devptr(self._h)
        return DeviceArray(ptr, (self.num_envs, self.camera_height, self.camera_width, 3), "|u1", self)

    def draw_lines(self, lines, env_idx=None):
        """GL_LINE overlays (the reference's draw_curve / draw_bbox) as a post-pass on the frames of the last render():
        lines [n, 9] = world-space segment (ax, ay, az, bx, by, bz) + colour (r, g, b in 0..1); env_idx [n] (non-decreasing) or None =
        env 0.  dtsim_draw_lines (include/dtsim.h)."""
        self._overlay("draw_lines", self._lib.dtsim_draw_lines, lines, 9, "segment", env_idx)

    def _overlay(self, who: str, cfn, records, width: int, noun: str, env_idx):
        """The body of draw_lines / draw_leds: `records` as [n, width] float32 and env_idx [n] (or None) to the post-pass `cfn`."""
        if self._cal is not None and not self._skip_distort:
            raise ValueError(f"{who} with per-env camera calibrations (camera_rand) is not supported")
        a = np.ascontiguousarray(np.asarray(records, dtype=np.float32).reshape(-1, width))
        n = a.shape[0]
        if n == 0:
            return
        ip = None
        if env_idx is not None:
            ei = np.ascontiguousarray(np.asarray(env_idx, dtype=np.int32).reshape(-1))
            if ei.shape[0] != n:
                raise ValueError(f"{who}: env_idx needs one entry per {noun}")
            ip = ei.ctypes.data_as(C.POINTER(C.c_int32))
        _ffi.check(self._lib, cfn(self._h, a.ctypes.data_as(C.POINTER(C.c_float)), ip, int(n)))

    _LED_POS = ((0.1, 0.05, -0.05), (0.1, 0.05, 0.05), (0.1, 0.05, 0.0), (-0.1, 0.05, -0.05), (-0.1, 0.05, 0.05))   # glTranslatef(px, pz, py): front_left,
    # front_right, center, back_left, back_right in the dict's order (objects.py:74-80, 96)
    _LED_FOLLOWER = ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5), (0.0, 0.0, 0.2), (0.5, 0.0, 0.0), (0.5, 0.0, 0.0))           # DuckiebotObj.leds_color (objects.py:218-224)
    _LED_STATIC = ((0.0, 0.0, 1.0),) * 5                                                                             # a static duckiebot-kind WorldObj (objects.py:86-92)

    def led_spheres(self, envs=None):
        """The spheres WorldObj.render_mesh draws with enable_leds (objects.py:68-121) for the given envs (default: all), from the current object
        states: per visible object of kind "duckiebot" and LED, the 1 cm sphere at alpha 1 and the halo of radius mean(colour) x 4 cm at alpha 0.2,
        inside the object's translate / scale / rotate, in draw order.  Returns (spheres [n, 8] float32, env_idx [n] int32) for draw_leds()."""
        envs = range(self.num_envs) if envs is None else [int(e) for e in envs]
        vis_all, cen_all = self.read(_ffi.FIELD_OBJ_VISIBLE), self.read(_ffi.FIELD_OBJ_CENTER)
        yrot_all, cy_all = self.read(_ffi.FIELD_OBJ_YROT), self.read(_ffi.FIELD_OBJ_Y)
        out, idx = [], []
        for e in envs:
            for k, o in enumerate(self.maps[int(self.env_map[e])].objects):
                if o.kind != "duckiebot" or not vis_all[e][k]:
                    continue
                if o.dyn_slot >= 0:
                    pos = np.array([cen_all[e][o.dyn_slot, 0], cy_all[e][o.dyn_slot], cen_all[e][o.dyn_slot, 1]], dtype=np.float64)
                    th = math.radians(float(yrot_all[e][o.dyn_slot]))
                else:
                    pos, th = np.asarray(o.pos, dtype=np.float64), float(o.angle)
                c, s_ = math.cos(th), math.sin(th)
                for (lx, ly, lz), col in zip(self._LED_POS, self._LED_STATIC if o.static else self._LED_FOLLOWER):
                    col = np.clip(np.asarray(col, dtype=np.float64), 0.0, 1.0)
                    x, y, z = lx * o.scale, ly * o.scale, lz * o.scale
                    cw = np.array([x * c + z * s_, y, -x * s_ + z * c]) + pos         # glRotatef(y_rot, 0, 1, 0) (objects.py:140-146)
                    out.append([*cw, 0.01 * o.scale, *col, 1.0]); idx.append(e)
                    out.append([*cw, float(np.mean(col)) * 0.04 * o.scale, *col, 0.2]); idx.append(e)
        return np.asarray(out, dtype=np.float32).reshape(-1, 8), np.asarray(idx, dtype=np.int32)

    def draw_leds(self, spheres, env_idx=None):
        """The LED spheres of the reference's enable_leds (objects.py:68-121) as a post-pass on the frames of the last render(): spheres [n, 8] =
        world-space centre (x, y, z), radius, colour (r, g, b in 0..1), alpha, in draw order; env_idx [n] (non-decreasing) or None = env 0.
        dtsim_draw_leds (include/dtsim.h)."""
        self._overlay("draw_leds", self._lib.dtsim_draw_leds, spheres, 8, "sphere", env_idx)

    def bind_frames(self, devptr: Optional[int]):
        _ffi.check(self._lib, self._lib.dtsim_bind_frames(self._h, C.c_void_p(devptr) if devptr else None))

    def allgather_frames(self, nccl_comm: int, recv, send=None):
        """RCCL all-gather of this rank's frame batch (or of `send`, any object with __cuda_array_interface__, e.g. the
        observe() output) into `recv` ([n_ranks, ...] device memory), enqueued on the library's stream behind the last
        render: dtsim_allgather_frames (include/dtsim.h).  `nccl_comm`: the ncclComm_t as an integer (address)."""
        rp = recv.__cuda_array_interface__["data"][0]
        sp, sb = None, 0
        if send is not None:
            ai = send.__cuda_array_interface__
            sp = ai["data"][0]
            sb = int(np.prod(ai["shape"])) * np.dtype(ai["typestr"]).itemsize
        _ffi.check(self._lib, self._lib.dtsim_allgather_frames(self._h, C.c_void_p(nccl_comm), C.c_void_p(rp), C.c_void_p(sp), C.c_size_t(sb)))

    def observe(self, height: int, width: int, chw: bool = False, normalize: bool = False, out=None, interpolation: str = "pil_bilinear",
                mask=None):
        """Learner-side observation of the last rendered batch, on the device: PIL-exact bilinear resize
        (learning/utils/wrappers.py ResizeWrapper) or, with interpolation="cv_cubic", the cv2 INTER_CUBIC resize of the
        reference's own ResizeWrapper (src/gym_duckietown/wrappers.py:129-138); optional HWC->CHW (ImgWrapper) and /255
        float32 (NormalizeWrapper).  Returns a device array ([N,h,w,3] or [N,3,h,w]); `out` may be any object with
        __cuda_array_interface__ of that shape/dtype, C-contiguous (e.g. the send buffer of the frame all-gather); any other `out` raises
        ValueError before anything is launched.  `mask` (as render's): only the rows of the selected envs are written, the others keep
        their content."""
        from . import resample
        if interpolation not in ("pil_bilinear", "cv_cubic"):
            raise ValueError(f"interpolation {interpolation!r}: 'pil_bilinear' or 'cv_cubic'")
        mp = self._mask_arg(mask)
        h, w = int(height), int(width)
        shape = (self.num_envs, 3, h, w) if chw else (self.num_envs, h, w, 3)
        out, ptr = self._result("observe", out, shape, "float32" if normalize else "uint8")
        ip = C.POINTER(C.c_int32)
        flags = (_ffi.OBS_CHW if chw else 0) | (_ffi.OBS_F32 if normalize else 0)
        if interpolation == "cv_cubic":
            fx, tx = resample.cubic_coeffs(self.camera_width, w)
            fy, ty = resample.cubic_coeffs(self.camera_height, h)
            fx, tx, fy, ty = (np.ascontiguousarray(a, dtype=np.int32) for a in (fx, tx, fy, ty))
            tabs = (fx.ctypes.data_as(ip), tx.ctypes.data_as(ip), fy.ctypes.data_as(ip), ty.ctypes.data_as(ip))
            if mp is None:
                _ffi.check(self._lib, self._lib.dtsim_observe_cubic(self._h, ptr, h, w, flags, *tabs))
            else:
                _ffi.check(self._lib, self._lib.dtsim_observe_cubic_masked(self._h, ptr, h, w, flags, mp, *tabs))
            return out
        bx = kx = by = ky = None
        nkx = nky = 0
        if w != self.camera_width:
            b, k = resample.coeffs(self.camera_width, w)
            bx, kx, nkx = b.ctypes.data_as(ip), k.ctypes.data_as(ip), k.shape[1]
        if h != self.camera_height:
            b, k = resample.coeffs(self.camera_height, h)
            by, ky, nky = b.ctypes.data_as(ip), k.ctypes.data_as(ip), k.shape[1]
        if mp is None:
            _ffi.check(self._lib, self._lib.dtsim_observe(self._h, ptr, h, w, flags, bx, kx, nkx, by, ky, nky))
        else:
            _ffi.check(self._lib, self._lib.dtsim_observe_masked(self._h, ptr, h, w, flags, mp, bx, kx, nkx, by, ky, nky))
        return out

    _DEPTH_DTYPES = ("float32", "float16")

    def depth(self, height=None, width=None, dtype: str = "float32", out=None, mask=None):
        """The depth map of every env's camera frame, on the device (dtsim_depth, include/dtsim.h): [N, h, w], per pixel the smallest eye depth
        (distance along the optical axis) of the nearest opaque surface -- tiles, ground, mesh objects -- over the four MSAA samples of the
        frame's source pixel; +inf where all four see the sky, 0 in the fisheye's black border.  Needs a preceding render() of the current state.
        With per-env calibrations (camera_rand, set_camera_calibrations) the source pixel is the one the env's OWN table names -- the surface
        whose colour the frame shows there --, and so it is for labels() and instances().
        Default size: the camera's; a smaller (h, w) must divide it and is the slice full[:, sy // 2::sy, sx // 2::sx] (sy = H // h, sx = W // w),
        of which only those pixels are traced.  dtype "float32" or "float16".  `out` may be any C-contiguous object with
        __cuda_array_interface__ of that shape and dtype; `mask` as render()'s (after render(mask=m) pass the same m): only the selected envs'
        rows are written (the others keep their content; in the simulator's own buffer that is whatever an earlier call left).  A bad size, dtype, out or mask raises ValueError before anything is launched."""
        if dtype not in self._DEPTH_DTYPES:
            raise ValueError(f"depth: dtype {dtype!r}: 'float32' or 'float16'")
        h, w = self._map_size("depth", "depth is", height, width)
        mp = self._mask_arg(mask)
        out, ptr = self._result("depth", out, (self.num_envs, h, w), dtype)
        flags = (_ffi.DEPTH_F16 if dtype == "float16" else 0) | self._env_tables_flag()
        self._map_pass(self._lib.dtsim_depth, self._lib.dtsim_depth_masked, mp, ptr, h, w, flags)
        return out

    def label_assets(self):
        """(per-texture class maps mirroring self.textures -- [h, w] uint8 each, in the texture's row order --, per-mesh classes [n_meshes] uint8):
        the default tables of labels() (dtsim/labels.py).  Tile textures: FLOOR on the kinds without lane curves, else ROAD where
        segment_assets() blacked the texel out and a marking class by the stated rule elsewhere; the other textures (mesh materials,
        traffic-light cards), which no tile shows, are all 0; meshes by the kind's name."""
        from . import labels
        seg_tex, _ = self.segment_assets()
        texel = [labels.texel_classes(self.textures[i], seg_tex[i], kd) for i, kd in enumerate(self.texture_kinds)]
        texel += [np.zeros(t.shape[:2], np.uint8) for t in self.textures[len(texel):]]
        return texel, labels.mesh_classes(self._mesh_order)

    def set_label_assets(self, texel_class=None, mesh_class=None):
        """Install the tables of labels() (dtsim_set_label_assets): texel_class = one [h, w] uint8 array per entry of self.textures, of its
        size and row order; mesh_class = [n_meshes] uint8 in the order of the simulator's meshes.  None: the default of label_assets().  A
        table of the wrong count, size or type raises ValueError before the library is called; a failed call leaves the installed tables."""
        if texel_class is None or mesh_class is None:
            d_texel, d_mesh = self.label_assets()
            texel_class = d_texel if texel_class is None else texel_class
            mesh_class = d_mesh if mesh_class is None else mesh_class
        if len(texel_class) != len(self.textures):
            raise ValueError(f"set_label_assets: {len(texel_class)} texel class maps for {len(self.textures)} textures")
        tc = []
        for i, (a, t) in enumerate(zip(texel_class, self.textures)):
            a = np.asarray(a)
            if a.dtype != np.uint8 or a.shape != t.shape[:2]:
                raise ValueError(f"set_label_assets: texel_class[{i}] must be uint8 of shape {t.shape[:2]}, got {a.dtype} {a.shape}")
            tc.append(np.ascontiguousarray(a))
        mc = np.asarray(mesh_class)
        if mc.dtype != np.uint8 or mc.shape != (len(self._mesh_order),):
            raise ValueError(f"set_label_assets: mesh_class must be uint8 of shape ({len(self._mesh_order)},), got {mc.dtype} {mc.shape}")
        mc = np.ascontiguousarray(mc)
        u8p = C.POINTER(C.c_uint8)
        parr = (u8p * max(len(tc), 1))()
        for i, a in enumerate(tc):
            parr[i] = a.ctypes.data_as(u8p)
        _ffi.check(self._lib, self._lib.dtsim_set_label_assets(self._h, parr, len(tc), mc.ctypes.data_as(u8p), len(mc)))
        self._have_label_assets = True
        self._mesh_class = mc.copy()                                # (object_classes())

    def labels(self, height=None, width=None, out=None, mask=None):
        """The semantic label map of every env's camera frame, on the device (dtsim_labels, include/dtsim.h): [N, h, w] uint8, per pixel the
        class of the surface that sets depth()'s value there -- of the four MSAA samples of the frame's source pixel the nearest one (ties: the
        lowest index; sky only when all four are sky): 0 in the fisheye's black border, 1 sky, 2 the ground quad, for a tile the class of the
        nearest texel of its texture, for a mesh object the class of its mesh (the tables of set_label_assets(); the defaults, installed at
        the first call: dtsim/labels.py).  Never filtered.  Needs a preceding render() of the current state.  Size, `out` and `mask` as
        depth()'s; a bad size, out or mask raises ValueError before anything is launched."""
        h, w = self._map_size("labels", "labels are", height, width)
        mp = self._mask_arg(mask)
        out, ptr = self._result("labels", out, (self.num_envs, h, w))
        self._need_label_assets()
        self._map_pass(self._lib.dtsim_labels, self._lib.dtsim_labels_masked, mp, ptr, h, w, self._env_tables_flag())
        return out

    def instances(self, height=None, width=None, out=None, mask=None, labels_out=None):
        """The instance map of every env's camera frame, on the device (dtsim_instances, include/dtsim.h): [N, h, w] uint8, per pixel o + 1
        where the nearest of the four MSAA samples of the frame's source pixel (the one that sets depth()'s value; ties: the lowest index) shows
        mesh object o -- its index in self.maps[map_id[e]].objects, the column of the FIELD_OBJ_* fields -- and 0 on tiles, ground, sky and in
        the fisheye's black border.  A hidden object's id never appears.  `labels_out` ([N, h, w] uint8, as labels()'s out): the same launch
        also writes labels()'s bytes into it, from the same classification (the default tables are installed at first use, as labels()
        does); without it no table is needed.  Needs a preceding render() of the current state.  Size, `out` and `mask` as labels()'s; a bad
        size, out, labels_out or mask raises ValueError before anything is launched."""
        h, w = self._map_size("instances", "instance ids are", height, width)
        mp = self._mask_arg(mask)
        shape = (self.num_envs, h, w)
        out, ptr = self._result("instances", out, shape)
        lp = None
        if labels_out is not None:
            lp = C.c_void_p(self._out_ptr(labels_out, shape, "|u1", 1, "instances: labels_out"))
            if lp.value == ptr.value:
                raise ValueError("instances: labels_out and out are one buffer")
            self._need_label_assets()
        self._map_pass(self._lib.dtsim_instances, self._lib.dtsim_instances_masked, mp, ptr, lp, h, w, self._env_tables_flag())
        return out

    def boxes(self, inst, out=None, mask=None):
        """One 2-D box and pixel count per id and env of an id map, on the device (dtsim_boxes, include/dtsim.h): `inst` is any C-contiguous
        uint8 CUDA tensor [N, h, w] on the handle's device (instances()'s map, or any other); returns [N, MAX_OBJECTS, 5] torch.int32, row k =
        x0, y0, x1, y1, n of id k + 1 -- n pixels, tightly bounded by columns [x0, x1) and rows [y0, y1) of the map; all 0 when the id is
        absent.  Stateless and stream-ordered; `out` (such a tensor) and `mask` (as render()'s: the other envs' rows keep every byte) are
        checked before anything is launched (ValueError)."""
        import torch
        self._dev_tensor(inst, "boxes: inst", lead=self.num_envs, dtypes=(torch.uint8,))
        if inst.dim() != 3 or inst.shape[1] < 1 or inst.shape[2] < 1 or inst.shape[1] * inst.shape[2] >= 2 ** 31:
            raise ValueError(f"boxes: inst must be [N, h, w] with h, w >= 1 and h * w below 2^31, got shape {tuple(inst.shape)}")
        mp = self._mask_arg(mask)
        shape = (self.num_envs, _ffi.MAX_OBJECTS, 5)
        if out is None:
            out, _ = self._result("boxes", None, shape, "int32")
        else:
            self._dev_tensor(out, "boxes: out", shape=shape, dtypes=(torch.int32,))
        _ffi.check(self._lib, self._lib.dtsim_boxes(self._h, C.c_void_p(inst.data_ptr()), int(inst.shape[1]), int(inst.shape[2]),
                                                    C.c_void_p(out.data_ptr()), 0, mp))
        return out

    def bev(self, height: int, width: int, cell: float = 0.02, rows_behind: int = 0, out=None, mask=None, instances_out=None):
        """The egocentric bird's-eye label map of every env, on the device (dtsim_bev, include/dtsim.h): [N, height, width] uint8, cell
        (i, j) = the class at the world point f metres ahead of the agent and s to its right, f = (height - rows_behind - i - 0.5) * cell,
        s = (j + 0.5 - width / 2) * cell (row 0 the farthest ahead, column 0 the leftmost; the agent's pose, not the camera's): the class of
        the mesh of the lowest-indexed visible object whose collision rectangle (object_footprints()) holds the point, else of the nearest
        texel of the tile under it (the tables of set_label_assets(), the defaults installed at first use, as labels() does), else 2, the
        ground.  0 and 1 never occur; never filtered; the agent's own rectangle is not drawn.  `instances_out` ([N, height, width] uint8):
        the same launch also writes o + 1 where object o owns the cell and 0 elsewhere -- instances()'s ids.  Not a post-pass: it reads the
        current state and needs no render().  `out` as labels()'s, `mask` as render()'s (only the selected envs' rows are written).  A size
        outside 1 .. 1024, a cell that is not finite and positive, rows_behind outside 0 .. height, a bad out, instances_out or mask
        raise ValueError before the library is called."""
        try:
            h, w, rb, c = int(height), int(width), int(rows_behind), float(cell)
            whole = h == height and w == width and rb == rows_behind
        except (TypeError, ValueError):
            whole = False
        if not whole:
            raise ValueError(f"bev: height, width and rows_behind must be integers and cell a number, got {height!r}, {width!r}, {rows_behind!r}, {cell!r}")
        if not (1 <= h <= _ffi.BEV_MAX_SIDE and 1 <= w <= _ffi.BEV_MAX_SIDE):
            raise ValueError(f"bev: a {h} x {w} map: each size must be in 1 .. {_ffi.BEV_MAX_SIDE}")
        if not (math.isfinite(c) and c > 0.0):
            raise ValueError(f"bev: cell {cell!r}: metres per cell, finite and > 0")
        if not 0 <= rb <= h:
            raise ValueError(f"bev: rows_behind {rows_behind!r} outside 0 .. {h}")
        if not self.render_enabled:
            raise ValueError("bev: the simulator was built with render=False and holds no render tables")
        mp = self._mask_arg(mask)
        shape = (self.num_envs, h, w)
        out, ptr = self._result("bev", out, shape)
        ip = None
        if instances_out is not None:
            ip = C.c_void_p(self._out_ptr(instances_out, shape, "|u1", 1, "bev: instances_out"))
            if ip.value == ptr.value:
                raise ValueError("bev: instances_out and out are one buffer")
        self._need_label_assets()
        _ffi.check(self._lib, self._lib.dtsim_bev(self._h, ptr, ip, h, w, c, rb, 0, mp))
        return out

    def _install_ipm_calibrations(self):
        """The forward models ipm() projects through (dtsim_set_ipm_calibrations), kept in step with the frames' fisheye: the installed
        calibrations (camera_rand, set_camera_calibrations), else the nominal one when distortion=True, none while the frames are
        rectilinear (distortion=False, skip_distort) or show UndistortWrapper's view (undistort=True: ipm() refuses)."""
        if not self.render_enabled:
            return
        dp = C.POINTER(C.c_double)
        if not self.distortion or self.undistort or self._skip_distort:
            _ffi.check(self._lib, self._lib.dtsim_set_ipm_calibrations(self._h, 0, None, None, None, None))
            return
        if self._cal is not None:
            K, D, new_K, env_cal = self._cal[:4]
        else:
            K, D = dist_mod.CAMERA_MATRIX[None], dist_mod.DIST_COEFS[None]
            new_K, env_cal = dist_mod.optimal_new_camera_matrix()[None], None
        K, D, new_K = (np.ascontiguousarray(a, np.float64) for a in (K, D, new_K))
        ep = None if env_cal is None else env_cal.ctypes.data_as(C.POINTER(C.c_int32))
        _ffi.check(self._lib, self._lib.dtsim_set_ipm_calibrations(self._h, int(K.shape[0]), K.ctypes.data_as(dp), D.ctypes.data_as(dp),
                                                                   new_K.ctypes.data_as(dp), ep))

    def ipm(self, height: int, width: int, cell: float = 0.02, rows_behind: int = 0, chw: bool = True, out=None, mask=None, valid_out=None,
            index_out=None):
        """The ground-projected camera image of every env, on the device (dtsim_ipm, include/dtsim.h): Duckietown's ground projection
        (inverse perspective mapping) of the current frame batch in bev()'s cell geometry -- [N, 3, height, width] uint8, or
        [N, height, width, 3] with chw=False; cell (i, j) shows the frame pixel that the floor point of bev()'s cell (i, j) projects to
        through the env's own camera (height, pitch, fov and noise under domain_rand) and, with distortion=True, its calibration's forward
        model (the nominal one, or the env's own of camera_rand / set_camera_calibrations); 0, 0, 0 where the point is behind the near plane
        or outside the image.  Nearest pixel, never filtered; a flat-world projection: no occlusion, and what stands on the floor smears away
        from the camera.  `valid_out` ([N, height, width] uint8): 1 / 0 per cell; `index_out` ([N, height, width] int32): the source pixel
        r * W + c, or -1 -- `torch.gather` of any camera map through it ground-projects that map.  It reads the frames as they are: call
        render() first.  `out` as labels()'s, `mask` as render()'s (only the selected envs' rows are written).  Sizes, cell and rows_behind as
        bev()'s; a bad one, a bad out, valid_out, index_out or mask, render=False and undistort=True (the frames show UndistortWrapper's
        view, not the camera's) raise ValueError before the library is called."""
        try:
            h, w, rb, c = int(height), int(width), int(rows_behind), float(cell)
            whole = h == height and w == width and rb == rows_behind
        except (TypeError, ValueError):
            whole = False
        if not whole:
            raise ValueError(f"ipm: height, width and rows_behind must be integers and cell a number, got {height!r}, {width!r}, {rows_behind!r}, {cell!r}")
        if not (1 <= h <= _ffi.BEV_MAX_SIDE and 1 <= w <= _ffi.BEV_MAX_SIDE):
            raise ValueError(f"ipm: a {h} x {w} map: each size must be in 1 .. {_ffi.BEV_MAX_SIDE}")
        if not (math.isfinite(c) and c > 0.0):
            raise ValueError(f"ipm: cell {cell!r}: metres per cell, finite and > 0")
        if not 0 <= rb <= h:
            raise ValueError(f"ipm: rows_behind {rows_behind!r} outside 0 .. {h}")
        if not self.render_enabled:
            raise ValueError("ipm: the simulator was built with render=False and has no frames")
        if self.undistort:
            raise ValueError("ipm with undistort=True is not supported (the frames show UndistortWrapper's view, not the camera's)")
        mp = self._mask_arg(mask)
        shape = (self.num_envs, h, w)
        out, ptr = self._result("ipm", out, (self.num_envs, 3, h, w) if chw else (self.num_envs, h, w, 3))
        ptrs = [ptr.value]
        vp = ip = None
        if valid_out is not None:
            vp = C.c_void_p(self._out_ptr(valid_out, shape, "|u1", 1, "ipm: valid_out"))
            ptrs.append(vp.value)
        if index_out is not None:
            ip = C.c_void_p(self._out_ptr(index_out, shape, "<i4", 4, "ipm: index_out"))
            ptrs.append(ip.value)
        if len(set(ptrs)) != len(ptrs):
            raise ValueError("ipm: out, valid_out and index_out must be three buffers")
        _ffi.check(self._lib, self._lib.dtsim_ipm(self._h, ptr, vp, ip, h, w, c, rb, _ffi.IPM_CHW if chw else 0, mp))
        return out

    def flow_mark(self, mask=None):
        """Remember the current state of the selected envs (`mask` as render()'s; None: every env) as the "previous" state of flow()
        (dtsim_flow_mark, include/dtsim.h): pose, camera, episode, map and the dynamic objects' poses, read from the state itself -- no
        render() is needed.  The marks live in the handle, not in the state blob; set_maps / set_assets drop them."""
        _ffi.check(self._lib, self._lib.dtsim_flow_mark(self._h, self._mask_arg(mask)))

    def flow(self, height=None, width=None, out=None, mask=None, valid_out=None):
        """The optical-flow map of every env's camera frame since its flow_mark(), on the device (dtsim_flow, include/dtsim.h): [N, 2, h, w]
        float32, plane 0 = x (to the right), plane 1 = y (down), in CAMERA pixels whatever the map's size; previous minus current, so
        prev_frame[p + flow] is what cur_frame[p] shows.  Per pixel the surface point that sets depth()'s value there -- moved with its object
        if a mesh object owns it -- is projected through the marked state's camera and through the current one (with distortion=True both
        through the calibration's forward model, as ipm() does) and the difference taken; exactly 0.0 where nothing moved.  `valid_out`
        ([N, h, w] uint8): 1 where the flow is defined -- a surface with a source pixel, a mark of the env's current episode, the previous
        point in front of the near plane and inside the image --, else 0, and the flow there is 0, 0.  Needs a preceding render() of the
        current state.  Size, `out` and `mask` as depth()'s.  Per-env calibrations (camera_rand, set_camera_calibrations) and undistort=True
        raise ValueError, as does a bad size, out, valid_out or mask, before anything is launched."""
        h, w = self._map_size("flow", "flow is", height, width)
        if self.undistort:
            raise ValueError("flow with undistort=True is not supported (the frames show UndistortWrapper's view, not the camera's)")
        if self._cal is not None:
            raise ValueError("flow with per-env calibrations (camera_rand, set_camera_calibrations) is not supported")
        mp = self._mask_arg(mask)
        out, ptr = self._result("flow", out, (self.num_envs, 2, h, w), "float32")
        vp = None
        if valid_out is not None:
            vp = C.c_void_p(self._out_ptr(valid_out, (self.num_envs, h, w), "|u1", 1, "flow: valid_out"))
        self._map_pass(self._lib.dtsim_flow, self._lib.dtsim_flow_masked, mp, ptr, vp, h, w, 0)
        return out

    def camera_maps(self, height=None, width=None, *, depth=None, depth_dtype: str = "float32", labels=None, instances=None, flow=None,
                    flow_valid=None, mask=None):
        """depth(), labels(), instances() and flow() of ONE size from one launch (dtsim_camera_maps, include/dtsim.h): the pixel is classified
        once -- what each single pass pays for -- and every output that is on is taken from that one nearest sample, so they agree with each
        other pixel by pixel.  Each of `depth`, `labels`, `instances`, `flow`, `flow_valid` is None (off), True (the simulator's own persistent
        tensor: the one the single method returns without `out`) or a tensor to write into, checked as the single method checks its `out`;
        `flow_valid` needs `flow`.  Returns a dict of the outputs that are on.  `depth_dtype`, the size and `mask` as depth()'s; labels install
        the default tables at first use, as labels() does; flow refuses what flow() refuses (per-env calibrations, undistort=True) and needs a
        flow_mark() on this simulator first (an env without a mark of its episode gets zeros, as in flow()).  Needs a preceding render() of the
        current state.  Every output is its single method's, byte for byte.  A bad argument raises ValueError before anything is launched."""
        if depth_dtype not in self._DEPTH_DTYPES:
            raise ValueError(f"camera_maps: depth_dtype {depth_dtype!r}: 'float32' or 'float16'")
        h, w = self._map_size("camera_maps", "the maps are", height, width)
        asked = dict(depth=depth, labels=labels, instances=instances, flow=flow, flow_valid=flow_valid)
        if all(v is None or v is False for v in asked.values()):
            raise ValueError("camera_maps: no output asked for")
        on = {k: v for k, v in asked.items() if v is not None and v is not False}
        if "flow_valid" in on and "flow" not in on:
            raise ValueError("camera_maps: flow_valid needs flow")
        if "flow" in on:
            if self.undistort:
                raise ValueError("camera_maps: flow with undistort=True is not supported (the frames show UndistortWrapper's view, not the camera's)")
            if self._cal is not None:
                raise ValueError("camera_maps: flow with per-env calibrations (camera_rand, set_camera_calibrations) is not supported")
        mp = self._mask_arg(mask)
        n = self.num_envs
        kinds = {"depth": ((n, h, w), depth_dtype), "labels": ((n, h, w), "uint8"), "instances": ((n, h, w), "uint8"),
                 "flow": ((n, 2, h, w), "float32"), "flow_valid": ((n, h, w), "uint8")}
        res, arg, spans = {}, _ffi.CameraMapsOut(), []
        for name, v in on.items():
            shape, dtype = kinds[name]
            res[name], ptr = self._result(name, None if v is True else v, shape, dtype)
            setattr(arg, name, ptr.value)
            spans.append((ptr.value, ptr.value + int(np.prod(shape)) * self._TYPESTR[dtype][1], name))
        spans.sort()
        for (a0, a1, an), (b0, b1, bn) in zip(spans, spans[1:]):
            if b0 < a1:
                raise ValueError(f"camera_maps: {an} and {bn} overlap")
        if "labels" in on:
            self._need_label_assets()
        flags = (_ffi.DEPTH_F16 if "depth" in on and depth_dtype == "float16" else 0) | self._env_tables_flag()
        self._map_pass(self._lib.dtsim_camera_maps, self._lib.dtsim_camera_maps_masked, mp, C.byref(arg), h, w, flags)
        return res

    @staticmethod
    def _state_array_offset(name: str, n: int) -> int:
        """Byte offset of array `name` in the state blob of n envs (csrc/state_fields.h DT_STATE_ARRAYS: [planes][n] float64 arrays in slab
        order, each starting on the next multiple of 256 bytes) -- for the arrays up to ob_corners, which no public field shows."""
        order = [("pos_x", 1), ("pos_z", 1), ("angle", 1), ("q_x", 1), ("q_y", 1), ("q_c", 1), ("q_s", 1), ("vel_u", 1), ("vel_w", 1),
                 ("ring", _ffi.MAX_DELAY * 2), ("war", 1), ("wal", 1), ("wheel_dist", 1), ("timestamp", 1), ("speed", 1), ("reward", 1),
                 ("lane", 4), ("prox", 1), ("wheels", 2), ("ob_cx", _ffi.MAX_DYNAMIC), ("ob_cz", _ffi.MAX_DYNAMIC), ("ob_sx", _ffi.MAX_DYNAMIC),
                 ("ob_sz", _ffi.MAX_DYNAMIC), ("ob_corners", _ffi.MAX_DYNAMIC * 8)]
        off = 0
        for nm, planes in order:
            if nm == name:
                return off
            off += (n * planes * 8 + 255) & ~255
        raise KeyError(name)

    def object_footprints(self):
        """(corners [N, MAX_OBJECTS, 4, 2] float64, drawn [N, MAX_OBJECTS] bool), on the host, synchronous: the collision rectangle of
        object k of env e's map as four (x, z) corners in order -- a static object's as the map packed it (self.maps[map_id].objects[k]
        .corners), a dynamic one's (duckies, followers, the checkerboard) the env's current one from the state blob (ob_corners: what the
        physics collides with) -- and whether bev() draws it: visible (FIELD_OBJ_VISIBLE) and with a mesh.  Rows past a map's object count
        are zero / False.  What a user overlays on the bev() map."""
        n = self.num_envs
        corners = np.zeros((n, _ffi.MAX_OBJECTS, 4, 2), np.float64)
        drawn = np.zeros((n, _ffi.MAX_OBJECTS), bool)
        map_id = self.read(_ffi.FIELD_MAP_ID)
        vis = self.read(_ffi.FIELD_OBJ_VISIBLE) != 0
        blob = self.read(_ffi.FIELD_STATE_BLOB)
        off = self._state_array_offset("ob_corners", n)
        dyn = blob[off:off + 8 * _ffi.MAX_DYNAMIC * n * 8].view(np.float64).reshape(8, _ffi.MAX_DYNAMIC, n)      # [coordinate][slot][env]
        for m, mt in enumerate(self.maps):
            envs = np.nonzero(map_id == m)[0]
            if not len(envs):
                continue
            slot = 0
            for k, o in enumerate(mt.objects):
                if o.static or not o.dyn_kind:                  # (dtsim_object.dynamic == 0: no slot)
                    corners[envs, k] = np.asarray(o.corners, np.float64).reshape(4, 2)
                else:
                    corners[envs, k] = dyn[:, slot, envs].T.reshape(-1, 4, 2)
                    slot += 1
                drawn[envs, k] = vis[envs, k] & (self.render_enabled and o.mesh_kind in self._mesh_order)
        return corners, drawn

    def object_classes(self):
        """[n_maps, MAX_OBJECTS] uint8 (numpy): the class labels() gives each object slot of each resident map -- mesh_class[mesh of object k
        of map m] under the table installed through set_label_assets(), or the default one (label_assets()) while none is -- and 0 past a
        map's object count.  A detector's class target for row k of boxes() in env e is object_classes()[map_id[e], k]."""
        mc = self._mesh_class if self._mesh_class is not None else self.label_assets()[1]
        out = np.zeros((len(self.maps), _ffi.MAX_OBJECTS), np.uint8)
        for m, mp in enumerate(self.maps):
            for k, o in enumerate(mp.objects):
                out[m, k] = mc[self._mesh_order.index(o.mesh_kind)]
        return out

    def copy_rows(self, dst, src, mask):
        """dst[e] = src[e] for every env selected by `mask` (as render's), on the device, stream-ordered; the other rows of dst keep their
        content.  dst / src: CUDA tensors on the handle's device, C-contiguous, same shape and dtype, leading dimension N."""
        mp = self._mask_ptr(mask)
        for name, t in (("dst", dst), ("src", src)):
            self._dev_tensor(t, "copy_rows: " + name, lead=self.num_envs)
        if dst.shape != src.shape or dst.dtype != src.dtype:
            raise ValueError(f"copy_rows: dst {tuple(dst.shape)} {dst.dtype} and src {tuple(src.shape)} {src.dtype} differ")
        row = src[0].numel() * src.element_size() if self.num_envs else 0
        _ffi.check(self._lib, self._lib.dtsim_copy_rows(self._h, C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), C.c_size_t(row), C.c_void_p(mp)))
        return dst

    def push_observation(self, stack, obs, first=None, mask=None, grayscale: bool = False):
        """The observation history on the device (dtsim_obs_push, include/dtsim.h): push `obs` (uint8 [N, 3, h, w], what
        observe(chw=True) returns) into `stack` ([N, depth, C, h, w], uint8 or float32 = / 255, C = 1 with grayscale -- Pillow's convert("L") --
        else 3; slot 0 is the oldest), in place and stream-ordered.  For every env selected by `mask` (as render's; None = all): with
        first[e] set all `depth` slots become the new observation, else the slots move one down and the last takes it; the other envs' rows
        keep every byte.  `first`: a mask like `mask`, or None = no env starts anew.  Both tensors are contiguous CUDA tensors on the handle's
        device and must not overlap; anything else raises ValueError before a launch.  Returns `stack`."""
        import torch
        fp, mp = self._mask_arg(first), self._mask_arg(mask)
        for name, t in (("stack", stack), ("obs", obs)):
            self._dev_tensor(t, "push_observation: " + name)
        if obs.dtype != torch.uint8 or obs.dim() != 4 or obs.shape[0] != self.num_envs or obs.shape[1] != 3 or obs[0].numel() == 0:
            raise ValueError(f"push_observation: obs must be uint8 of shape ({self.num_envs}, 3, h, w), got {obs.dtype} {tuple(obs.shape)}")
        h, w = int(obs.shape[2]), int(obs.shape[3])
        c = 1 if grayscale else 3
        if stack.dtype not in (torch.uint8, torch.float32) or stack.dim() != 5 or (stack.shape[0], *stack.shape[2:]) != (self.num_envs, c, h, w) \
                or not 1 <= stack.shape[1] <= _ffi.OBS_MAX_DEPTH:
            raise ValueError(f"push_observation: stack must be uint8 / float32 of shape ({self.num_envs}, 1 .. {_ffi.OBS_MAX_DEPTH}, {c}, {h}, {w}), "
                             f"got {stack.dtype} {tuple(stack.shape)}")
        s0, o0 = stack.data_ptr(), obs.data_ptr()
        if s0 < o0 + obs.numel() and o0 < s0 + stack.numel() * stack.element_size():
            raise ValueError("push_observation: stack and obs overlap")
        flags = _ffi.OBS_CHW | (_ffi.OBS_F32 if stack.dtype == torch.float32 else 0) | (_ffi.OBS_GRAY if grayscale else 0)
        _ffi.check(self._lib, self._lib.dtsim_obs_push(self._h, C.c_void_p(s0), C.c_void_p(o0), int(stack.shape[1]), h, w, flags, fp, mp))
        return stack

    def blend_frames(self, out, frames, weights, mask=None):
        """The weighted sum of several frame batches on the device (dtsim_blend_frames, include/dtsim.h; the blend of the reference's
        MotionBlurWrapper): `frames` is a sequence of 1 .. 8 uint8 [N, H, W, 3] tensors (the handle's camera size), oldest first, `weights` as
        many integers in 0 .. 255 with the sum D in 1 .. 256.  `out` of the same shape takes sum(w[i] * frames[i]) / D: uint8, rounded half up
        (it may be one of `frames`), or float32, one IEEE division (it must not overlap a frame).  `mask` (as render's): only the rows of the
        selected envs are written.  All tensors are contiguous CUDA tensors on the handle's device; anything else raises ValueError before a
        launch.  Stream-ordered; returns `out`."""
        import torch
        mp = self._mask_arg(mask)
        shape = (self.num_envs, self.camera_height, self.camera_width, 3)
        frames = list(frames) if isinstance(frames, (list, tuple)) else None
        if not frames or len(frames) > _ffi.BLEND_MAX:
            raise ValueError(f"blend_frames: frames must be a sequence of 1 .. {_ffi.BLEND_MAX} tensors")
        for name, t in [("out", out)] + [(f"frames[{i}]", f) for i, f in enumerate(frames)]:
            self._dev_tensor(t, "blend_frames: " + name, shape=shape, dtypes=(torch.uint8, torch.float32) if name == "out" else (torch.uint8,))
        try:
            w = [int(v) for v in weights]
            exact = all(v == x for v, x in zip(w, weights))
        except (TypeError, ValueError):
            w, exact = [], False
        if not exact or len(w) != len(frames) or any(not 0 <= v <= 255 for v in w) or not 1 <= sum(w) <= 256:
            raise ValueError(f"blend_frames: weights must be {len(frames)} integers in 0 .. 255 with a sum in 1 .. 256, got {weights!r}")
        o0, o1 = out.data_ptr(), out.data_ptr() + out.numel() * out.element_size()
        for f in frames:                                    # (the blend is element-wise at equal index: a uint8 out may BE a frame, nothing else)
            if f.data_ptr() < o1 and o0 < f.data_ptr() + f.numel() and (out.dtype == torch.float32 or f.data_ptr() != o0):
                raise ValueError("blend_frames: out overlaps a frame (a uint8 out may be one of the frames, a float32 out none)")
        fp = (C.c_void_p * len(frames))(*[f.data_ptr() for f in frames])
        wp = (C.c_uint32 * len(w))(*w)
        _ffi.check(self._lib, self._lib.dtsim_blend_frames(self._h, C.c_void_p(out.data_ptr()), fp, wp, len(w),
                                                           _ffi.OBS_F32 if out.dtype == torch.float32 else 0, mp))
        return out

    def frames_host(self) -> np.ndarray:
        """Synchronous copy of the frame batch to the host (tests / N=1 facade)."""
        import torch
        self.sync()
        t = torch.as_tensor(self.frames_device(), device=f"cuda:{self.device_index}")
        return t.cpu().numpy()

    @property
    def device_index(self) -> int:
        return self._device

    # ----------------------------------------------------------------- fields --
    _FIELD_SHAPES = {
        _ffi.FIELD_POS: ("f8", (3,)), _ffi.FIELD_ANGLE: ("f8", ()), _ffi.FIELD_REWARD: ("f8", ()),
        _ffi.FIELD_DONE: ("u1", ()), _ffi.FIELD_DONE_CODE: ("u1", ()), _ffi.FIELD_STEP_COUNT: ("i4", ()),
        _ffi.FIELD_TILE: ("i4", (2,)), _ffi.FIELD_LANE: ("f8", (4,)), _ffi.FIELD_IN_LANE: ("u1", ()),
        _ffi.FIELD_PROX: ("f8", ()), _ffi.FIELD_SPEED: ("f8", ()), _ffi.FIELD_TIMESTAMP: ("f8", ()),
        _ffi.FIELD_WHEELS: ("f8", (2,)), _ffi.FIELD_MAP_ID: ("i4", ()),
        _ffi.FIELD_OBJ_CENTER: ("f8", (_ffi.MAX_DYNAMIC, 2)), _ffi.FIELD_OBJ_ACTIVE: ("u1", (_ffi.MAX_DYNAMIC,)),
        _ffi.FIELD_OBJ_YROT: ("f8", (_ffi.MAX_DYNAMIC,)), _ffi.FIELD_OBJ_PARAMS: ("f8", (_ffi.MAX_DYNAMIC, 3)),
        _ffi.FIELD_OBJ_VISIBLE: ("u1", (_ffi.MAX_OBJECTS,)), _ffi.FIELD_EPISODE: ("i4", ()),
        _ffi.FIELD_OBJ_LIGHT: ("u1", (_ffi.MAX_OBJECTS,)), _ffi.FIELD_OBJ_Y: ("f8", (_ffi.MAX_DYNAMIC,)),
        _ffi.FIELD_OBJ_EXTRA: ("f8", (_ffi.MAX_DYNAMIC, 5)), _ffi.FIELD_CAMERA: ("f4", (6,)), _ffi.FIELD_COLORS: ("f4", (16,)),
        _ffi.FIELD_WHEEL_DIST: ("f8", ()), _ffi.FIELD_RENDER_POS: ("i4", ()), _ffi.FIELD_RENDER_PIPE: ("i4", ()),
    }

    def read(self, field: int) -> np.ndarray:
        if field == _ffi.FIELD_STATE_BLOB:
            out = np.empty(self._lib.dtsim_state_bytes(self._h), np.uint8)
        else:
            dt, shp = self._FIELD_SHAPES[field]
            out = np.empty((self.num_envs,) + shp, dtype=dt)
        _ffi.check(self._lib, self._lib.dtsim_read(self._h, field, out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    def read_agent(self, env: int = 0) -> "_ffi.AgentInfo":
        """dtsim_read_agent: pose, speed, wheels, lane pose, proximity, reward / done of one env in one transfer."""
        out = _ffi.AgentInfo()
        _ffi.check(self._lib, self._lib.dtsim_read_agent(self._h, int(env), C.byref(out)))
        return out

    def write(self, field: int, arr: np.ndarray):
        self.state_version += 1                       # any cached read-back of the state is stale now
        if field == _ffi.FIELD_STATE_BLOB:
            a = np.ascontiguousarray(arr, np.uint8)
        else:
            dt, shp = self._FIELD_SHAPES[field]
            a = np.ascontiguousarray(np.asarray(arr, dtype=dt).reshape((self.num_envs,) + shp))
        _ffi.check(self._lib, self._lib.dtsim_write(self._h, field, a.ctypes.data_as(C.c_void_p), a.nbytes))

    def query(self, env_idx, poses, safety_factor: float = 1.0) -> np.ndarray:
        """Reference geometry queries at arbitrary poses [n,3] = (x, z, angle), evaluated
        on the device; returns a structured array mirroring dtsim_probe."""
        env_idx = np.ascontiguousarray(env_idx, np.int32)
        poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 3)
        n = poses.shape[0]
        out = np.zeros(n, dtype=_ffi.probe_dtype())
        if n:
            _ffi.check(self._lib, self._lib.dtsim_query(
                self._h, n, env_idx.ctypes.data_as(C.POINTER(C.c_int32)), poses.ctypes.data_as(C.POINTER(C.c_double)),
                float(safety_factor), C.cast(out.ctypes.data, C.POINTER(_ffi.Probe))))
        return out

    def sync(self):
        _ffi.check(self._lib, self._lib.dtsim_sync(self._h))

    @property
    def stream(self) -> int:
        return int(self._lib.dtsim_stream(self._h) or 0)

    def profile_read(self, kernel: int):
        n, ms = C.c_int(), C.c_double()
        _ffi.check(self._lib, self._lib.dtsim_profile_read(self._h, kernel, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    @property
    def state_bytes(self) -> int:
        return int(self._lib.dtsim_state_bytes(self._h))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.dtsim_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
