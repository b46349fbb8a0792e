"""Throughput of the learner-facing loop (DuckietownVecEnv): step + device reset + render + 160x120 CHW float obs.
FINAL_OBS=1: with final observations (full pass before the reset, row copy, masked render / observe of the restarted envs after it).
STACK=K, GRAY=1, NORMALIZE=0: the observation history kept by the env (frame_stack / grayscale / normalize of DuckietownVecEnv).
EMULATE=1: the plain env plus the history a user keeps in torch (torch.roll of [N, K * 3, h, w], masked refill of the restarted envs).
MOTION_BLUR=1: DuckietownVecEnv(motion_blur=True, action_mode="wheels") -- three sub-updates and renders per step and the blend of four frame
batches; MOTION_BLUR=rerender: the same with the window's first frame rendered again at every step, as the reference's wrapper does (what
reusing the previous window's last frame saves).
DEPTH=1: info["depth"] beside the observation (DuckietownVecEnv(depth_shape=(120, 160)): dtsim_depth after every observe); DEPTH=full: the
camera's own 480 x 640; DEPTH_DTYPE=float16: half maps.  MAP=loop_pedestrians: another map (mesh objects: the depth kernel's triangle loop).
LABELS=1: info["labels"] beside the observation (DuckietownVecEnv(label_shape=(120, 160)): dtsim_labels after every observe); LABELS=full: 480 x 640.
VARIANTS=a,b,...: several variants in ONE process, each warmed up, then timed in alternating order (ROUNDS rounds of K steps each, the
median round is reported); a variant is plain | stack | stack_u8 | gray | gray_u8 | emulate (STACK gives the depth, default 4) | wheels (the plain env with
action_mode="wheels", the blur's baseline) | blur | blur_rerender | depth | depth_f16 | depth_full | depth_full_f16 | labels | labels_full |
depth_labels (both maps at 120 x 160) | instances (info["instances"] + info["boxes"] at 120 x 160: dtsim_instances and dtsim_boxes after every
observe) | instances_full (480 x 640) | instances_only (no boxes) | labels_instances (labels + instances + boxes at 120 x 160: one fused launch
for the two maps).
INSTANCES=1 (or full): the whole step with instances and boxes against the plain step in the SAME run -- VARIANTS=plain,instances (or
plain,instances_full) with ROUNDS=5 unless given.
BEV=1 (or small): the whole step with info["bev"] + info["bev_instances"] (DuckietownVecEnv(bev_shape=(128, 128), bev_cell=0.02,
bev_instances=True); small: (64, 64) at 0.04) against the plain step in the SAME run -- VARIANTS=plain,bev (or plain,bev_small) with ROUNDS=5
unless given; the variants bev | bev_small | bev_only (no id map) can be listed like any other.
IPM=1 (or small): the whole step with info["ipm"] + info["ipm_valid"] (DuckietownVecEnv(ipm_shape=(128, 128), ipm_cell=0.02, ipm_valid=True);
small: (64, 64) at 0.04) against the plain step in the SAME run -- VARIANTS=plain,ipm (or plain,ipm_small) with ROUNDS=5 unless given; the
variants ipm | ipm_small | ipm_only (no flags) | bev_ipm (the bird's-eye maps and the ground projection, input and target) can be listed.
FLOW=1 (or full): the whole step with info["flow"] + info["flow_valid"] (DuckietownVecEnv(flow_shape=(120, 160), flow_valid=True); full:
480 x 640) against the plain step in the SAME run -- VARIANTS=plain,flow (or plain,flow_full) with ROUNDS=5 unless given; the variants
flow | flow_full | flow_only (no flags) can be listed.
FUSED=1: the whole step with depth, labels, instances + boxes and flow + flags at 120 x 160, by the single passes (`all_maps`) and by ONE
dtsim_camera_maps launch (`all_maps_fused`: DuckietownVecEnv(fused_maps=True)), against the plain step in the SAME run --
VARIANTS=plain,all_maps,all_maps_fused with ROUNDS=5 unless given; the two variants can be listed like any other."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-duckietown_amd"))
import torch
from dtsim import DuckietownVecEnv
N = int(os.environ.get("N", "4096"))
FINAL = os.environ.get("FINAL_OBS", "0") == "1"
STACK = int(os.environ.get("STACK", "1"))
GRAY = os.environ.get("GRAY", "0") == "1"
NORMALIZE = os.environ.get("NORMALIZE", "1") == "1"
EMULATE = os.environ.get("EMULATE", "0") == "1"
MOTION_BLUR = os.environ.get("MOTION_BLUR", "0")
DEPTH = os.environ.get("DEPTH", "0")
DEPTH_DTYPE = os.environ.get("DEPTH_DTYPE", "float32")
LABELS = os.environ.get("LABELS", "0")
INSTANCES = os.environ.get("INSTANCES", "0")
BEV = os.environ.get("BEV", "0")
IPM = os.environ.get("IPM", "0")
FLOW = os.environ.get("FLOW", "0")
FUSED = os.environ.get("FUSED", "0")
MAP = os.environ.get("MAP", "small_loop")
MAP_TAG = "" if MAP == "small_loop" else " " + MAP          # (the default map's lines read as they always did)
VARIANTS = [v for v in os.environ.get("VARIANTS", "").split(",") if v]
K = int(os.environ.get("K", "30"))
ROUNDS = int(os.environ.get("ROUNDS", "1"))
if INSTANCES != "0" and not VARIANTS:
    VARIANTS, ROUNDS = ["plain", "instances_full" if INSTANCES == "full" else "instances"], int(os.environ.get("ROUNDS", "5"))
if BEV != "0" and not VARIANTS:
    VARIANTS, ROUNDS = ["plain", "bev_small" if BEV == "small" else "bev"], int(os.environ.get("ROUNDS", "5"))
if IPM != "0" and not VARIANTS:
    VARIANTS, ROUNDS = ["plain", "ipm_small" if IPM == "small" else "ipm"], int(os.environ.get("ROUNDS", "5"))
if FLOW != "0" and not VARIANTS:
    VARIANTS, ROUNDS = ["plain", "flow_full" if FLOW == "full" else "flow"], int(os.environ.get("ROUNDS", "5"))
if FUSED != "0" and not VARIANTS:
    VARIANTS, ROUNDS = ["plain", "all_maps", "all_maps_fused"], int(os.environ.get("ROUNDS", "5"))
a = torch.rand((N, 2), device="cuda") * 2 - 1


class Variant:
    def __init__(self, name, stack=1, gray=False, normalize=True, emulate=False, blur="0", wheels=False, depth="0", depth_dtype="float32", labels="0", instances="0",
                 boxes=True, bev="0", bev_instances=True, ipm="0", ipm_valid=True, flow="0", flow_valid=True, fused=False):
        self.name, self.emulate, self.depth, self.rerender = name, emulate, stack, blur == "rerender"
        kw = {} if emulate or (stack == 1 and not gray) else dict(frame_stack=stack, grayscale=gray)
        if blur != "0":
            kw.update(motion_blur=True, action_mode="wheels")
        elif wheels:
            kw.update(action_mode="wheels")
        if depth != "0":
            kw.update(depth_shape=(480, 640) if depth == "full" else (120, 160), depth_dtype=depth_dtype)
        if labels != "0":
            kw.update(label_shape=(480, 640) if labels == "full" else (120, 160))
        if instances != "0":
            kw.update(instance_shape=(480, 640) if instances == "full" else (120, 160), boxes=boxes)
        if bev != "0":
            kw.update(bev_shape=(64, 64) if bev == "small" else (128, 128), bev_cell=0.04 if bev == "small" else 0.02, bev_instances=bev_instances)
        if ipm != "0":
            kw.update(ipm_shape=(64, 64) if ipm == "small" else (128, 128), ipm_cell=0.04 if ipm == "small" else 0.02, ipm_valid=ipm_valid)
        if flow != "0":
            kw.update(flow_shape=(480, 640) if flow == "full" else (120, 160), flow_valid=flow_valid)
        if fused:
            kw.update(fused_maps=True)
        self.env = DuckietownVecEnv(MAP, N, obs_shape=(120, 160), seed=0, domain_rand=False, distortion=True, final_obs=FINAL,
                                    normalize=normalize, **kw)
        obs = self.env.reset()
        self.hist = obs.repeat(1, stack, 1, 1) if emulate else None
        self.shape, self.dtype = tuple(self.hist.shape if emulate else obs.shape), obs.dtype
        self.ms = []

    def step(self):
        if self.rerender:                                  # the literal wrapper's first render_obs() of a step: the same state, the same bytes
            env = self.env
            env.sim.bind_frames(env._ring[env._cur].data_ptr())
            env.sim.render()
            env.sim.bind_frames(None)
        obs, r, d, info = self.env.step(a)
        if self.emulate:                                   # what a learner does without frame_stack: roll, append, refill the restarted envs
            h = torch.roll(self.hist, -3, dims=1)
            h[:, -3:] = obs
            self.hist = torch.where(d[:, None, None, None], obs.repeat(1, self.depth, 1, 1), h)

    def run(self, steps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(steps):
            self.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / steps


def make(name):
    d = STACK if STACK > 1 else 4
    return {"plain": lambda: Variant("plain"),
            "stack": lambda: Variant(f"K={d} colour float32", d),
            "stack_u8": lambda: Variant(f"K={d} colour uint8", d, normalize=False),
            "gray": lambda: Variant(f"K={d} grey float32", d, gray=True),
            "gray_u8": lambda: Variant(f"K={d} grey uint8", d, gray=True, normalize=False),
            "emulate": lambda: Variant(f"K={d} colour float32, torch emulation", d, emulate=True),
            "depth": lambda: Variant("depth 120 x 160 float32", depth="1"), "depth_f16": lambda: Variant("depth 120 x 160 float16", depth="1", depth_dtype="float16"),
            "depth_full": lambda: Variant("depth 480 x 640 float32", depth="full"),
            "depth_full_f16": lambda: Variant("depth 480 x 640 float16", depth="full", depth_dtype="float16"),
            "labels": lambda: Variant("labels 120 x 160", labels="1"), "labels_full": lambda: Variant("labels 480 x 640", labels="full"),
            "depth_labels": lambda: Variant("depth float32 + labels 120 x 160", depth="1", labels="1"),
            "instances": lambda: Variant("instances + boxes 120 x 160", instances="1"),
            "instances_full": lambda: Variant("instances + boxes 480 x 640", instances="full"),
            "instances_only": lambda: Variant("instances 120 x 160, no boxes", instances="1", boxes=False),
            "labels_instances": lambda: Variant("labels + instances + boxes 120 x 160", labels="1", instances="1"),
            "bev": lambda: Variant("bev + ids 128 x 128 at 0.02 m", bev="1"), "bev_small": lambda: Variant("bev + ids 64 x 64 at 0.04 m", bev="small"),
            "bev_only": lambda: Variant("bev 128 x 128 at 0.02 m, no ids", bev="1", bev_instances=False),
            "ipm": lambda: Variant("ipm + valid 128 x 128 at 0.02 m", ipm="1"), "ipm_small": lambda: Variant("ipm + valid 64 x 64 at 0.04 m", ipm="small"),
            "ipm_only": lambda: Variant("ipm 128 x 128 at 0.02 m, no flags", ipm="1", ipm_valid=False),
            "bev_ipm": lambda: Variant("bev + ids + ipm + valid 128 x 128 at 0.02 m", bev="1", ipm="1"),
            "flow": lambda: Variant("flow + valid 120 x 160", flow="1"), "flow_full": lambda: Variant("flow + valid 480 x 640", flow="full"),
            "flow_only": lambda: Variant("flow 120 x 160, no flags", flow="1", flow_valid=False),
            "all_maps": lambda: Variant("depth + labels + instances + boxes + flow + valid 120 x 160", depth="1", labels="1", instances="1", flow="1"),
            "all_maps_fused": lambda: Variant("the same, fused_maps=True", depth="1", labels="1", instances="1", flow="1", fused=True),
            "wheels": lambda: Variant("plain, wheels"), "blur": lambda: Variant("motion blur", blur="1"),
            "blur_rerender": lambda: Variant("motion blur, first frame rendered again", blur="rerender")}[name]()


if VARIANTS:
    vs = [make(v) for v in VARIANTS]
    for v in vs:
        v.run(5)
    for r in range(ROUNDS):
        for v in (vs if r % 2 == 0 else vs[::-1]):
            v.ms.append(v.run(K) * 1e3)
    for v in vs:
        s = sorted(v.ms)
        print(f"VecEnv{MAP_TAG} N={N}{' final_obs' if FINAL else ''} {v.name:40s} {list(v.shape)} {str(v.dtype)[6:]}: median {s[len(s) // 2]:.3f} ms per step "
              f"(min {s[0]:.3f}, max {s[-1]:.3f}; {ROUNDS} rounds of {K} steps)")
else:
    v = Variant("", STACK, GRAY, NORMALIZE, EMULATE, MOTION_BLUR, depth=DEPTH, depth_dtype=DEPTH_DTYPE, labels=LABELS)
    v.run(5)
    dt = v.run(K)
    what = (f" emulated K={STACK}" if EMULATE else "") + (f" frame_stack={STACK}" if STACK > 1 and not EMULATE else "") + (" grey" if GRAY else "") + \
        ({"0": "", "1": " motion_blur", "rerender": " motion_blur + first frame rendered again"}[MOTION_BLUR]) + \
        ("" if DEPTH == "0" else f" depth {list(v.env.depth.shape[1:])} {DEPTH_DTYPE}") + \
        ("" if LABELS == "0" else f" labels {list(v.env.labels.shape[1:])}")
    print(f"VecEnv{MAP_TAG} N={N}{' final_obs' if FINAL else ''}{what}: {dt*1e3:.3f} ms per step -> {N/dt/1e6:.3f} M env-steps/s with "
          f"{list(v.shape)} {str(v.dtype)[6:]} observations")
