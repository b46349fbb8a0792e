"""A vectorised, device-resident env for learners: the gym.Env contract of the reference
(`reset() -> obs`, `step(a) -> obs, reward, done, info`), batched over N envs, with every tensor living in HBM.

    env = DuckietownVecEnv("small_loop", num_envs=4096, obs_shape=(120, 160))
    obs = env.reset()                                  # torch.float32 [N, 3, 120, 160] on the GPU
    obs, reward, done, info = env.step(actions)        # actions: torch / numpy [N, 2]

One step is: `dtsim_step` (kinematics, collisions, reward / done) -> reward and done are copied out ->
`dtsim_reset_done` restarts the finished episodes with the device-side sampler (the reference's reset
distributions and spawn test) -> `dtsim_render` -> `dtsim_observe` (the learners' ResizeWrapper /
ImgWrapper / NormalizeWrapper, bit-identical to PIL).  So, as with gym's vector envs, the observation returned
with `done[e] = True` is already the first observation of env e's next episode.  Everything is launched on one
HIP stream shared with torch and ordered against the caller's stream on the GPU: no host synchronisation in the loop.

Final observations (`final_obs=True`; gymnasium's `final_observation`, SB3's `terminal_observation`): the step renders and observes the
whole batch BEFORE the reset -- the frames the reference's step() returns --, keeps the rows of the finished envs in
`info["final_obs"]` (`dtsim_copy_rows`), restarts them and renders / observes only them again (`dtsim_render_masked`,
`dtsim_observe_masked`).  `info["final_obs"]` is one persistent device tensor shaped like `obs` (raw frames with obs_shape=None);
its rows where `info["final_obs_mask"]` (= done) is set hold the final observations, the other rows are unspecified.
Always: `info["truncated"]` = done with done_code DTSIM_DONE_MAX_STEPS (the time limit: bootstrap on V(final obs)),
`info["terminated"]` = the other finished envs (invalid pose).

Observation history (`frame_stack=K`, 1 .. 16, and / or `grayscale=True`; needs `obs_shape` and `chw=True`): `obs` is `[N, K * C, h, w]`, the
last K observations of every env, oldest first and channel-concatenated -- C = 3, or 1 in grey (Pillow's convert("L") of the resized frame);
float32 with `normalize=True`, uint8 without.  It is a view of one persistent `[N, K, C, h, w]` tensor the env keeps on the device
(`dtsim_obs_push`: one in-place kernel per step): as with the plain observations, the returned tensor is the env's own buffer and the next
step rewrites it -- clone what has to outlive the step.  The first observation of an episode fills all K slots (gym's FrameStack), so no frame of
the previous episode leaks into the next one's stack.  With `final_obs=True`, `info["final_obs"]` (same shape) holds for a finished env its
history ENDING WITH its final frame, and the returned `obs` of that env is its new episode's first frame, K times.
`frame_stack=1, grayscale=False` (the default) runs the plain path, call for call.

Motion blur (`motion_blur=True`, or a window of 2 .. 8 integer weights, oldest frame first; needs `action_mode="wheels"` and `frame_skip=1`):
the reference's MotionBlurWrapper (learning/utils/wrappers.py:8-36), its only model of a camera's exposure, taken literally.  The wrapper cuts
the env's delta_time in three, and per step clips the action to [-1, 1], does `render_obs(); update_physics(a)` three times, renders a fourth
frame and returns np.average of the four with the weights 0.8 / 0.15 / 0.04 / 0.01, the OLDEST frame weighted 0.8.  Here a window of L weights
(True = (80, 15, 4, 1)) builds the simulator with `frame_rate * (L - 1)` -- a frame_rate whose 0.15 s actuation delay exceeds DTSIM_MAX_DELAY
steps fails with BatchedSimulator's error --, and a step is L - 1 times `dtsim_step_ex(DTSIM_STEP_ONE_UPDATE)` (update_physics: the wheel pair
as given, which is why the env clips it) + a render into the next slot of a ring of L raw frame batches, then one `dtsim_blend_frames` of the
ring in age order: sum(w[i] * frame[i]) / sum(w) in exact integers.  The window's first frame is the last frame of the previous window (one
state renders to the same bytes every time), so a step costs L - 1 renders, not L.  Reward and done are those of the state after the last
sub-update; an env that leaves the road mid-window keeps being updated, as in the reference; `step_count` advances once per sub-update, so
`info["episode_steps"]` and `max_steps` count sub-updates.  `reset()` returns the plain frame (the reference's reset() is render_obs()), and
so is the first observation of a restarted env; `info["final_obs"]` is the blurred final observation, at no extra render.  `final_obs`,
`frame_stack`, `grayscale`, `obs_shape=None`, `normalize` and `chw` compose as without the blur.  Deviation: the reference returns the float64
average (its learners' imresize then rescales by the array's min and max); here the blend is rounded half up to uint8 and takes the PIL-exact
resize of every other frame -- `BatchedSimulator.blend_frames(out=float32)` gives the unrounded value.  Memory: L extra frame batches (15 GB for
the default window at N = 4096, 640 x 480).  `motion_blur=False` (the default) runs the paths above, call for call.

Auxiliary outputs (depth, labels, instances, boxes, flow, flow_valid, bev, bev_instances, ipm, ipm_valid; each off by default, and an option left off makes no new call).  What
they share, said once.  Output X is one persistent device tensor, `info["X"]`, of the state whose observation `obs` shows -- for an env
restarted in the step, the first state of its new episode.  `reset()` keeps returning `obs` alone: after it the output is `env.X`, the same
tensor (None while X is off).  With `final_obs=True`, `info["final_X"]` is a second persistent tensor whose rows where
`info["final_obs_mask"]` is set hold X of the final state (the other rows are unspecified).  The passes stand together after every observe,
in the order depth, labels, instances, boxes, flow, bev, ipm, masked where the observe is masked: full render -> observe -> passes ->
`dtsim_copy_rows` of each -> `dtsim_reset_done` -> masked render -> masked observe -> masked passes.  They compose with one another and with
`frame_stack`, `grayscale`, `obs_shape=None` and `domain_rand` (no output is ever stacked).  Depth, labels, instances and boxes are CAMERA
post-passes: point-sampled from the frame's source pixels, never filtered, so each size of their `(h, w)` must divide the camera's; and they
read one rendered state, so `motion_blur` (its observation shows the states of its window) raises ValueError.  Under `camera_rand` (a
distortion table per env) they are opt-in, `camera_rand_maps=True`: every env's maps then go through its OWN table (`DTSIM_MAP_ENV_TABLES`,
include/dtsim.h), pixel-aligned with its frame, and everything above composes as without `camera_rand`; without the option the combination
keeps raising ValueError, as it always has.  (Still out of scope there: the line and LED overlays, and the N = 1 gym facade.)

Depth (`depth_shape=(h, w)`; `depth_dtype` "float32" or "float16"): `info["depth"]` is the `[N, h, w]` depth map (`dtsim_depth`,
include/dtsim.h: smallest eye depth over the four MSAA samples of the frame's source pixel, +inf = sky, 0 = the fisheye's black border).

Labels (`label_shape=(h, w)`): `info["labels"]` is the `[N, h, w]` `torch.uint8` semantic label map (`dtsim_labels`, include/dtsim.h: per
pixel the class of the surface that sets the depth there -- 0 the fisheye's black border, 1 sky, 2 ground, tiles by the nearest texel's
class, mesh objects by their mesh's; the default classes: dtsim/labels.py).

Instances and boxes (`instance_shape=(h, w)`; `boxes=True` needs it): `info["instances"]` is the `[N, h, w]` `torch.uint8` instance map
(`dtsim_instances`, include/dtsim.h: per pixel o + 1 where the surface that sets the depth there is mesh object o of the env's own map --
the column of the `DTSIM_FIELD_OBJ_*` fields --, 0 on every other surface and in the fisheye's black border), and with `boxes=True`
`info["boxes"]` a `[N, 64, 5]` `torch.int32` tensor, row k = x0, y0, x1, y1, n of object k in that map's pixels (`dtsim_boxes`; all 0 for an
object not in view; its class: `sim.object_classes()[map_id, k]`).  With `label_shape == instance_shape` ONE `dtsim_instances` launch fills
both maps from one classification and `dtsim_labels` is not called.

Bird's-eye view (`bev_shape=(h, w)`, each 1 .. 1024; `bev_cell` metres per cell, `bev_rows_behind` of the h rows behind the agent;
`bev_instances=True` needs it): `info["bev"]` is the `[N, h, w]` `torch.uint8` egocentric label map (`dtsim_bev`, include/dtsim.h: cell
(i, j) = the class at the point (h - rows_behind - i - 0.5) cells ahead of the AGENT and (j + 0.5 - w / 2) cells to its right -- the mesh
class of the lowest-indexed visible object whose collision rectangle holds the point, else the nearest texel's class of the tile under it,
else 2, the ground; never 0 or 1, never filtered), and with `bev_instances=True` `info["bev_instances"]` the id map of the same launch
(o + 1 / 0, the ids of `info["instances"]`).  It reads the state, not the camera, so it composes with everything: `camera_rand` and
`motion_blur` are allowed -- under `motion_blur` the observation blends the frames of the window's states, and the map is that of the state
after the last sub-update, the newest of them.

Ground projection (`ipm_shape=(h, w)`, `ipm_cell`, `ipm_rows_behind` as the bird's-eye options; `ipm_valid=True` needs it): `info["ipm"]` is
the camera frame warped onto the floor plane in `info["bev"]`'s cell geometry (`dtsim_ipm`, include/dtsim.h: Duckietown's ground projection,
inverse perspective mapping) -- `[N, 3, h, w]` `torch.uint8`, `[N, h, w, 3]` with `chw=False`; cell (i, j) shows the frame pixel that the
floor point of `info["bev"]`'s cell (i, j) projects to through the env's own camera and fisheye, 0, 0, 0 where there is none -- and with
`ipm_valid=True` `info["ipm_valid"]` the `[N, h, w]` flags (1 / 0) of the same launch.  Input and target of a camera-to-BEV head come
aligned.  Nearest pixel, never filtered; a flat-world projection (no occlusion; what stands on the floor smears away from the camera).  It
projects through each env's camera and calibration itself and reads no table, so `domain_rand` and `camera_rand` are allowed;
`motion_blur` (the blended frame shows several cameras), `undistort=True` and `render=False` raise ValueError.

Optical flow (`flow_shape=(h, w)`; `flow_valid=True` needs it): `info["flow"]` is the `[N, 2, h, w]` `torch.float32` flow map (`dtsim_flow`,
include/dtsim.h: per pixel where the surface point that sets the depth there -- moved with its duckie, if one owns it -- stood in the
PREVIOUS shown state's image, minus where it stands now; camera pixels, x right and y down, so `prev_frame[p + flow]` is what
`cur_frame[p]` shows; through the fisheye's forward model with `distortion=True`), and with `flow_valid=True` `info["flow_valid"]` the
`[N, h, w]` flags of the same launch (0: sky, the fisheye's border, a previous point behind the camera or outside the image; the flow
there is 0, 0).  A camera post-pass like depth, under the same rules, but the one output of TWO states: `reset()` and `step()` end with one
`dtsim_flow_mark` of every env, after all passes, so an env that went on shows the motion since the last step's shown state, across all
`frame_skip` sub-updates; an env restarted in the step has no mark of its new episode: its rows are all 0 (flow and flags); with
`final_obs=True` `info["final_flow"]` is the finished env's last flow.  After `reset()` the map is all 0 too.  `motion_blur`,
`camera_rand` (even with `camera_rand_maps`) and `undistort=True` raise ValueError.

One launch for the camera maps (`fused_maps=True`, opt-in): those of `depth_shape`, `label_shape`, `instance_shape` and `flow_shape` that are
set must be equal, and at least one must be set (else ValueError, before a device is touched).  Every place above where the depth, label,
instance and flow passes stand then holds ONE `BatchedSimulator.camera_maps` call (`dtsim_camera_maps`, include/dtsim.h), which classifies
each pixel once and writes all of them; boxes, bev and ipm follow as before.  The outputs are the same quantities in the same tensors, and
everything composes as without the option, byte for byte (tests/test_gpu_rerender_maps.py drives both past mesh objects).  With
`fused_maps=False` (the default) the env makes the calls above, call for call.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np

from . import _ffi
from .batched import BatchedSimulator


class _Aux(NamedTuple):
    """One auxiliary output of the env.  The constructor lists them in pass order; allocation, the final rows and `info` go by that list."""
    name: str                       # env.<name> and info["<name>"]; the finished envs' rows: info["final_<name>"]
    dtype: str                      # torch's name of the element type
    tail: Optional[Tuple[int, ...]]  # the shape after N; None: the output is off
    camera: bool                    # a camera post-pass: it reads the distortion table(s) and ONE rendered state, so its option went
    #                                 through _camera_map_shape (no motion_blur, camera_rand only with camera_rand_maps, a size that divides the camera's)


class DuckietownVecEnv:
    def __init__(self, map_name="small_loop", num_envs: int = 1024, obs_shape: Optional[Tuple[int, int]] = (120, 160),
                 chw: bool = True, normalize: bool = True, action_mode: str = "vel_steer", device: int = 0,
                 seed: Optional[int] = 0, final_obs: bool = False, frame_stack: int = 1, grayscale: bool = False,
                 motion_blur: Union[bool, Sequence[int]] = False, depth_shape: Optional[Tuple[int, int]] = None,
                 depth_dtype: str = "float32", label_shape: Optional[Tuple[int, int]] = None,
                 instance_shape: Optional[Tuple[int, int]] = None, boxes: bool = False,
                 bev_shape: Optional[Tuple[int, int]] = None, bev_cell: float = 0.02, bev_rows_behind: int = 0,
                 bev_instances: bool = False, ipm_shape: Optional[Tuple[int, int]] = None, ipm_cell: float = 0.02,
                 ipm_rows_behind: int = 0, ipm_valid: bool = False, camera_rand_maps: bool = False,
                 flow_shape: Optional[Tuple[int, int]] = None, flow_valid: bool = False, fused_maps: bool = False, **sim_kwargs):
        # (the argument errors come before a device or the simulator is touched)
        if isinstance(frame_stack, bool) or not isinstance(frame_stack, (int, np.integer)) or not 1 <= frame_stack <= _ffi.OBS_MAX_DEPTH:
            raise ValueError(f"frame_stack must be an integer in 1 .. {_ffi.OBS_MAX_DEPTH}, got {frame_stack!r}")
        self.frame_stack, self.grayscale = int(frame_stack), bool(grayscale)
        self._stacked = self.frame_stack > 1 or self.grayscale
        if self._stacked and obs_shape is None:
            raise ValueError("frame_stack > 1 / grayscale need obs_shape (the raw camera frames are not stacked)")
        if self._stacked and not chw:
            raise ValueError("frame_stack > 1 / grayscale need chw=True (there are no HWC stacks)")
        self._blur = self._blur_window(motion_blur)                 # the window's integer weights, oldest frame first, or None
        if depth_dtype not in BatchedSimulator._DEPTH_DTYPES:
            raise ValueError(f"depth_dtype {depth_dtype!r}: 'float32' or 'float16'")
        self.depth_dtype = depth_dtype
        cam = (int(sim_kwargs.get("camera_height", 480)), int(sim_kwargs.get("camera_width", 640)))
        self._per_env_tables_refused = bool(sim_kwargs.get("camera_rand")) and not camera_rand_maps
        self.depth_shape = self._camera_map_shape("depth_shape", depth_shape, cam)
        self.label_shape = self._camera_map_shape("label_shape", label_shape, cam)
        if boxes and instance_shape is None:
            raise ValueError("boxes=True needs instance_shape (the boxes are those of the instance map, in its pixels)")
        self.instance_shape = self._camera_map_shape("instance_shape", instance_shape, cam)
        if flow_valid and flow_shape is None:
            raise ValueError("flow_valid=True needs flow_shape (the flags are those of the flow map, in its pixels)")
        if flow_shape is not None and sim_kwargs.get("camera_rand"):
            raise ValueError("flow_shape with camera_rand is not supported (a distortion table per env: the flow goes through one calibration)")
        if flow_shape is not None and sim_kwargs.get("undistort"):
            raise ValueError("flow_shape with undistort=True is not supported (the frames show UndistortWrapper's view, not the camera's)")
        self.flow_shape = self._camera_map_shape("flow_shape", flow_shape, cam)
        self.fused_maps = bool(fused_maps)
        if self.fused_maps:
            named = {k: v for k, v in (("depth_shape", self.depth_shape), ("label_shape", self.label_shape),
                                       ("instance_shape", self.instance_shape), ("flow_shape", self.flow_shape)) if v is not None}
            if not named:
                raise ValueError("fused_maps=True needs at least one of depth_shape, label_shape, instance_shape, flow_shape (it fuses their passes)")
            if len(set(named.values())) != 1:
                raise ValueError(f"fused_maps=True needs one size for all camera maps (one launch fills them), got {named}")
            self._fused_shape = next(iter(named.values()))
        self.bev_shape, self.bev_cell, self.bev_rows_behind = None, bev_cell, bev_rows_behind
        if bev_shape is None:
            if bev_instances:
                raise ValueError("bev_instances=True needs bev_shape (the ids are those of the bird's-eye map, in its cells)")
        else:
            try:
                bh, bw = (int(v) for v in bev_shape)
                brb, bc = int(bev_rows_behind), float(bev_cell)
            except (TypeError, ValueError):
                raise ValueError(f"bev_shape must be (h, w), bev_rows_behind an integer and bev_cell a number, got {bev_shape!r}, "
                                 f"{bev_rows_behind!r}, {bev_cell!r}") from None
            if not (1 <= bh <= _ffi.BEV_MAX_SIDE and 1 <= bw <= _ffi.BEV_MAX_SIDE):
                raise ValueError(f"bev_shape {(bh, bw)}: each size must be in 1 .. {_ffi.BEV_MAX_SIDE}")
            if not (np.isfinite(bc) and bc > 0.0):
                raise ValueError(f"bev_cell {bev_cell!r}: metres per cell, finite and > 0")
            if brb != bev_rows_behind or not 0 <= brb <= bh:
                raise ValueError(f"bev_rows_behind {bev_rows_behind!r}: an integer in 0 .. {bh}")
            if sim_kwargs.get("render") is False:
                raise ValueError("bev_shape needs render=True (the pass reads the render tables)")
            self.bev_shape, self.bev_cell, self.bev_rows_behind = (bh, bw), bc, brb
        self.ipm_shape, self.ipm_cell, self.ipm_rows_behind = None, ipm_cell, ipm_rows_behind
        if ipm_shape is None:
            if ipm_valid:
                raise ValueError("ipm_valid=True needs ipm_shape (the flags are those of the ground-projected image, in its cells)")
        else:
            try:
                ih, iw = (int(v) for v in ipm_shape)
                irb, ic = int(ipm_rows_behind), float(ipm_cell)
            except (TypeError, ValueError):
                raise ValueError(f"ipm_shape must be (h, w), ipm_rows_behind an integer and ipm_cell a number, got {ipm_shape!r}, "
                                 f"{ipm_rows_behind!r}, {ipm_cell!r}") from None
            if not (1 <= ih <= _ffi.BEV_MAX_SIDE and 1 <= iw <= _ffi.BEV_MAX_SIDE):
                raise ValueError(f"ipm_shape {(ih, iw)}: each size must be in 1 .. {_ffi.BEV_MAX_SIDE}")
            if not (np.isfinite(ic) and ic > 0.0):
                raise ValueError(f"ipm_cell {ipm_cell!r}: metres per cell, finite and > 0")
            if irb != ipm_rows_behind or not 0 <= irb <= ih:
                raise ValueError(f"ipm_rows_behind {ipm_rows_behind!r}: an integer in 0 .. {ih}")
            if sim_kwargs.get("render") is False:
                raise ValueError("ipm_shape needs render=True (the pass reads the camera frames)")
            if self._blur:
                raise ValueError("ipm_shape with motion_blur is not supported (the blended frame shows the cameras of its window's states: "
                                 "no single camera projects it)")
            if sim_kwargs.get("undistort"):
                raise ValueError("ipm_shape with undistort=True is not supported (the frames show UndistortWrapper's view, not the camera's)")
            self.ipm_shape, self.ipm_cell, self.ipm_rows_behind = (ih, iw), ic, irb
        outputs = (_Aux("depth", depth_dtype, self.depth_shape, True),
                   _Aux("labels", "uint8", self.label_shape, True),
                   _Aux("instances", "uint8", self.instance_shape, True),
                   _Aux("boxes", "int32", (_ffi.MAX_OBJECTS, 5) if boxes else None, True),
                   _Aux("flow", "float32", self.flow_shape and (2, *self.flow_shape), True),
                   _Aux("flow_valid", "uint8", self.flow_shape if flow_valid else None, True),
                   _Aux("bev", "uint8", self.bev_shape, False),
                   _Aux("bev_instances", "uint8", self.bev_shape if bev_instances else None, False),
                   _Aux("ipm", "uint8", self.ipm_shape and ((3, *self.ipm_shape) if chw else (*self.ipm_shape, 3)), False),
                   _Aux("ipm_valid", "uint8", self.ipm_shape if ipm_valid else None, False))
        if self._blur:
            if action_mode != "wheels":
                raise ValueError(f"motion_blur needs action_mode='wheels' (update_physics takes the wheel pair), got {action_mode!r}")
            if sim_kwargs.get("frame_skip", 1) != 1:
                raise ValueError(f"motion_blur needs frame_skip=1 (the window's sub-updates are the step), got {sim_kwargs['frame_skip']!r}")
            # MotionBlurWrapper: env.delta_time / frame_skip, with one sub-update per frame after the window's first
            sim_kwargs["frame_rate"] = sim_kwargs.get("frame_rate", 30) * (len(self._blur) - 1)
        import torch
        self.torch = torch
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        self.stream = torch.cuda.Stream(device=self.device)      # the simulator's launches and our copies share it
        self.sim = BatchedSimulator(map_name, num_envs, action_mode=action_mode, device=device, seed=seed,
                                    device_reset=True, auto_reset=False, stream=self.stream.cuda_stream, do_reset=False,
                                    **sim_kwargs)
        self.num_envs = num_envs
        self.obs_shape, self.chw, self.normalize = obs_shape, chw, normalize
        self.final_obs = bool(final_obs)
        self._final = None                                          # info["final_obs"], allocated at the first step
        # The live tensor of every output and, with final_obs, its final_ twin.  (zeros, once: the rows of envs that have not finished yet, or
        # that a first masked pass leaves out, hold no stale memory -- two envs run alike then return the same bytes in EVERY row, whatever
        # the allocator handed out.)
        self._aux = []                                              # (name, live tensor, final_ twin or None) of the outputs that are on
        for a in outputs:
            live = final = None
            if a.tail is not None:
                live = torch.zeros((num_envs, *a.tail), dtype=getattr(torch, a.dtype), device=self.device)
                final = torch.zeros_like(live) if self.final_obs else None
                self._aux.append((a.name, live, final))
            setattr(self, a.name, live)                             # env.depth, env.labels, ...: the tensor info[name] returns, or None
        sim = self.sim
        self._reward = torch.as_tensor(sim.field_device(_ffi.FIELD_REWARD), device=self.device)
        self._done = torch.as_tensor(sim.field_device(_ffi.FIELD_DONE), device=self.device)
        self._code = torch.as_tensor(sim.field_device(_ffi.FIELD_DONE_CODE), device=self.device)
        self._steps = torch.as_tensor(sim.field_device(_ffi.FIELD_STEP_COUNT), device=self.device)
        self._frames = torch.as_tensor(sim.frames_device(), device=self.device)
        self.action_shape = (num_envs, 2)
        self._all = None                                            # `first` of reset(): every env starts anew (a mask when stacked)
        if self._stacked:
            h, w = int(obs_shape[0]), int(obs_shape[1])
            self._stack = torch.zeros((num_envs, self.frame_stack, 1 if self.grayscale else 3, h, w),
                                      dtype=torch.float32 if normalize else torch.uint8, device=self.device)
            self._all = torch.ones(num_envs, dtype=torch.uint8, device=self.device)
            self._stack_shape = (num_envs, self._stack.shape[1] * self._stack.shape[2], h, w)
        if self._blur:
            self._ring = [torch.empty_like(self._frames) for _ in self._blur]     # slot _cur holds the frame of the current state
            self._cur = 0

    def _camera_map_shape(self, option, shape, cam):
        """The (h, w) of a camera post-pass's option (None: off), or the ValueError that names the option and the cause."""
        if shape is None:
            return None
        cause = None
        if self._blur:
            cause = "with motion_blur is not supported (the blurred observation shows the states of its window: no single state's map belongs to it)"
        elif self._per_env_tables_refused:
            cause = ("with camera_rand needs camera_rand_maps=True (camera_rand installs a distortion table per env; with the option the pass "
                     "reads each env's own table, without it the combination is refused as before)")
        else:
            try:
                h, w = (int(v) for v in shape)
            except (TypeError, ValueError):
                cause = f"must be (h, w), got {shape!r}"
            else:
                if h <= 0 or w <= 0 or cam[0] % h or cam[1] % w:
                    cause = f"{(h, w)}: each size must divide the camera's {cam} (the map is point-sampled, never filtered)"
        if cause:
            raise ValueError(f"{option} {cause}")
        return h, w

    @staticmethod
    def _blur_window(motion_blur):
        if motion_blur is None or motion_blur is False:
            return None
        if motion_blur is True:
            return (80, 15, 4, 1)                                   # wrappers.py:29, in hundredths
        try:
            w = tuple(motion_blur)
            ok = all(not isinstance(v, bool) and isinstance(v, (int, np.integer)) for v in w)
        except TypeError:
            w, ok = (), False
        if not ok or not 2 <= len(w) <= _ffi.BLEND_MAX or any(not 0 <= v <= 255 for v in w) or not 1 <= sum(w) <= 256:
            raise ValueError(f"motion_blur must be a bool or 2 .. {_ffi.BLEND_MAX} integer weights in 0 .. 255 with a sum in 1 .. 256 "
                             f"(oldest frame first), got {motion_blur!r}")
        return tuple(int(v) for v in w)

    # ------------------------------------------------------------------------------------------------
    def _show(self, mask=None, first=None, render=True):
        """render -> `obs` of the frame batch in the form the env was built with: the raw frames, the observe buffer, or the history view
        (observe as uint8 CHW into the simulator's own buffer -> push; `first`: the envs whose history starts anew).  `mask`: only those
        envs, every call of it."""
        sim = self.sim
        if render:
            sim.render(mask=mask)
        if self.obs_shape is None:
            return self._frames                                     # [N, H, W, 3] uint8, the raw camera frames
        h, w = self.obs_shape[0], self.obs_shape[1]
        if not self._stacked:
            return self.torch.as_tensor(sim.observe(h, w, chw=self.chw, normalize=self.normalize, mask=mask), device=self.device)
        o = sim.observe(h, w, chw=True, normalize=False, mask=mask)
        sim.push_observation(self._stack, o, first=first, mask=mask, grayscale=self.grayscale)
        return self._stack.view(self._stack_shape)

    def _map_passes(self, mask=None):
        """The passes of the outputs that are on, in the table's order, each into the env's own tensor (`mask`: only those envs' rows): of the
        state the last render() showed the depth, then the labels, then the instances and their boxes -- labels and instances of one shape
        come from one launch --, then the flow since the envs' marks (and its flags); then, of the current state, the bird's-eye map (and its ids); last, of the frame batch as it stands, the
        ground-projected image (and its flags).  fused_maps: the camera maps -- depth, labels, instances, flow -- by one camera_maps call."""
        if self.fused_maps:
            # ONE launch in place of the depth / labels / instances / flow calls below; the rest as without the option
            self.sim.camera_maps(self._fused_shape[0], self._fused_shape[1], depth=self.depth, depth_dtype=self.depth_dtype, labels=self.labels,
                                 instances=self.instances, flow=self.flow, flow_valid=self.flow_valid, mask=mask)
            if self.boxes is not None:
                self.sim.boxes(self.instances, out=self.boxes, mask=mask)
        else:
            self._single_map_passes(mask)
        if self.bev is not None:
            self.sim.bev(self.bev_shape[0], self.bev_shape[1], cell=self.bev_cell, rows_behind=self.bev_rows_behind, out=self.bev, mask=mask,
                         instances_out=self.bev_instances)
        if self.ipm is not None:
            self.sim.ipm(self.ipm_shape[0], self.ipm_shape[1], cell=self.ipm_cell, rows_behind=self.ipm_rows_behind, chw=self.chw, out=self.ipm,
                         mask=mask, valid_out=self.ipm_valid)

    def _single_map_passes(self, mask):
        """The camera maps by their single passes (fused_maps=False): depth, labels, instances and boxes, flow."""
        if self.depth is not None:
            self.sim.depth(self.depth_shape[0], self.depth_shape[1], dtype=self.depth_dtype, out=self.depth, mask=mask)
        fused = self.labels is not None and self.label_shape == self.instance_shape
        if self.labels is not None and not fused:
            self.sim.labels(self.label_shape[0], self.label_shape[1], out=self.labels, mask=mask)
        if self.instances is not None:
            self.sim.instances(self.instance_shape[0], self.instance_shape[1], out=self.instances, mask=mask,
                               labels_out=self.labels if fused else None)
            if self.boxes is not None:
                self.sim.boxes(self.instances, out=self.boxes, mask=mask)
        if self.flow is not None:
            self.sim.flow(self.flow_shape[0], self.flow_shape[1], out=self.flow, mask=mask, valid_out=self.flow_valid)

    def _keep_final(self, obs, done, info):
        """final_obs: the finished envs' rows of `obs` (stacked: of the whole history) and of every output that is on, before the reset
        rewrites them."""
        src = self._stack if self._stacked else obs
        if self._final is None:
            # (zeros, once, on our stream: for the reason the outputs' tensors are)
            self._final = self.torch.zeros_like(src)
        self.sim.copy_rows(self._final, src, done)
        info["final_obs"], info["final_obs_mask"] = self._final.view(self._stack_shape) if self._stacked else self._final, done
        for name, live, final in self._aux:
            self.sim.copy_rows(final, live, done)
            info["final_" + name] = final

    def _enter(self):
        self.stream.wait_stream(self.torch.cuda.current_stream(self.device))     # e.g. the policy that produced the actions

    def _leave(self):
        self.torch.cuda.current_stream(self.device).wait_stream(self.stream)     # consumers run after our launches (GPU-side)

    def reset(self):
        self._enter()
        with self.torch.cuda.stream(self.stream):
            self.sim.reset()                                        # device sampler (dtsim_reset(states = NULL))
            obs = self._show(first=self._all)
            if self.fused_maps and self.flow is not None:
                # camera_maps refuses a flow before the first flow_mark where flow() answers with zeros: a mark of no env gives the handle its
                # (empty) marks, and the reset's map is flow()'s -- all 0
                self.sim.flow_mark(mask=self.torch.zeros(self.num_envs, dtype=self.torch.uint8, device=self.device))
            self._map_passes()
            self._mark()
            if self._blur:
                self._ring[0].copy_(self._frames)                   # the next window's first frame
                self._cur = 0
        self._leave()
        return obs

    def _mark(self):
        """flow_shape: the state every env is left in -- the one `obs` shows -- becomes the previous state of the next step's flow."""
        if self.flow is not None:
            self.sim.flow_mark()

    def _advance(self, actions):
        """The step of the state: dtsim_step, or with motion_blur the clipped wheel pair in L - 1 sub-updates, each rendered into the next
        ring slot (the handle is left bound to the last one)."""
        t, sim, blur = self.torch, self.sim, self._blur
        if isinstance(actions, np.ndarray):
            a = np.ascontiguousarray(actions, np.float32).reshape(1, self.num_envs, 2)
            if blur:
                a = np.clip(a, -1.0, 1.0)
        elif blur:
            a = actions.to(device=self.device, dtype=t.float32).clamp(-1.0, 1.0).contiguous()   # (a new tensor, made on our stream)
        else:
            a = actions.to(device=self.device, dtype=t.float32).contiguous()
            a.record_stream(self.stream)
        if not blur:
            sim.step(a)
            return
        L = len(blur)
        for j in range(1, L):
            sim.step(a, flags=_ffi.STEP_ONE_UPDATE)
            sim.bind_frames(self._ring[(self._cur + j) % L].data_ptr())
            sim.render()

    def step(self, actions):
        """One sequence for every configuration.  With final_obs or motion_blur the batch is shown BEFORE the reset -- what the reference's
        step() returns, blurred: the blend of the ring's L slots in the handle's own frame buffer -- and the restarted envs alone are shown
        again after it, unblurred; else the reset comes first and one pass shows every env.  The pass of a new output goes into _map_passes."""
        t, sim, blur = self.torch, self.sim, self._blur
        self._enter()
        with t.cuda.stream(self.stream):
            self._advance(actions)
            reward = self._reward.to(t.float32)                     # copies: the reset below clears the fields
            done = self._done.to(t.bool)
            code = self._code.clone()
            # (dtsim_step sets done_code nonzero exactly when done: one comparison each)
            info = {"done_code": code, "episode_steps": self._steps.clone(), "truncated": code == _ffi.DONE_MAX_STEPS,
                    "terminated": code == _ffi.DONE_INVALID_POSE}
            if blur:
                L = len(blur)
                sim.blend_frames(self._frames, [self._ring[(self._cur + j) % L] for j in range(L)], blur)
                sim.bind_frames(None)
            if self.final_obs or blur:
                obs = self._show(render=not blur)                   # every env; stacked: every history now ends with this frame
                self._map_passes()
                if self.final_obs:
                    self._keep_final(obs, done, info)
                sim.reset_done()
                if blur:
                    self._cur = (self._cur + L - 1) % L             # the newest slot opens the next window
                    sim.bind_frames(self._ring[self._cur].data_ptr())
                obs = self._show(mask=done, first=done)             # the restarted envs, only they: their first frame (in every slot)
                self._map_passes(mask=done)
                if blur:
                    if self.obs_shape is None:
                        sim.copy_rows(self._frames, self._ring[self._cur], done)   # (`obs` is the handle's own batch, the render went into the slot)
                    sim.bind_frames(None)
            else:
                sim.reset_done()
                obs = self._show(first=done)
                self._map_passes()
            self._mark()
            for name, live, _ in self._aux:
                info[name] = live
        self._leave()
        return obs, reward, done, info

    def close(self):
        self.sim.close()
