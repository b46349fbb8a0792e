"""GPU: the calls DuckietownVecEnv makes on its BatchedSimulator, per constructor configuration -- the methods, their order and their
`mask` / `first` / `flags` choices, and whether a pass was handed a second map to fill (`labels_out` of instances(): "fused";
`instances_out` of bev(): "ids").  The env's docstring promises that an option left at its default "runs the plain path, call for call",
and a step must not gain or lose a render, an observe, a map pass or a copy: EXPECTED below is a literal recording (this file's tracer run
against an earlier commit's vecenv.py and batched.py, pasted), not of the code under test -- the configurations without AUX of the commit
before reset() and step() were written as one sequence, those of AUX (labels, instances, boxes, bev) of commit 6308dc1 ("Give the vector
env an egocentric bird's-eye label map of every env"), the last one that spelled every auxiliary output out by hand.  The trace is per
call and does not depend on which envs finished, so every step of a configuration gives the same one."""
import inspect

import pytest

from dtsim import DuckietownVecEnv

pytestmark = pytest.mark.gpu

N, STEPS, MAX_STEPS = 4, 4, 3
CAM = dict(camera_width=64, camera_height=48)
TRACED = ("reset", "step", "render", "observe", "push_observation", "depth", "labels", "instances", "boxes", "bev", "copy_rows", "blend_frames",
          "bind_frames", "reset_done")

OBS = {"observe": dict(obs_shape=(24, 32)), "raw": dict(obs_shape=None), "stack": dict(obs_shape=(24, 32), frame_stack=2)}
CONFIGS = {}
for _f in ("plain", "final"):
    for _o in OBS:
        for _d in ("", "_depth"):
            CONFIGS[f"{_f}_{_o}{_d}"] = dict(OBS[_o], final_obs=_f == "final", **(dict(depth_shape=(24, 32)) if _d else {}))
        CONFIGS[f"blur_{_f}_{_o}"] = dict(OBS[_o], final_obs=_f == "final", motion_blur=(3, 1), action_mode="wheels")
# the outputs added after the first recording, alone and together (with every one on, labels and instances share a shape: fused)
AUX = {"labels": dict(label_shape=(24, 32)),
       "instances_boxes": dict(instance_shape=(24, 32), boxes=True),
       "labels_instances_fused": dict(label_shape=(24, 32), instance_shape=(24, 32)),
       "labels_instances_apart": dict(label_shape=(12, 16), instance_shape=(24, 32)),
       "every_map": dict(depth_shape=(24, 32), label_shape=(24, 32), instance_shape=(24, 32), boxes=True, bev_shape=(8, 8), bev_instances=True),
       "blur_bev": dict(bev_shape=(8, 8), motion_blur=(3, 1), action_mode="wheels")}     # the one post-pass allowed under motion_blur
for _f in ("plain", "final"):
    for _a in AUX:
        CONFIGS[f"{_f}_{_a}"] = dict(OBS["observe"], final_obs=_f == "final", **AUX[_a])


def c(name, mask=None, first=None, flags=None, bound=None, second=None):
    return (name, mask, first, flags, bound, second)


# config -> (the calls of reset(), the calls of one step())
EXPECTED = {
    "plain_observe": (
        (c('reset'), c('render'), c('observe'),),
        (c('step', flags=0), c('reset_done'), c('render'), c('observe'),)),
    "plain_observe_depth": (
        (c('reset'), c('render'), c('observe'), c('depth'),),
        (c('step', flags=0), c('reset_done'), c('render'), c('observe'), c('depth'),)),
    "blur_plain_observe": (
        (c('reset'), c('render'), c('observe'),),
        (c('step', flags=1), c('bind_frames', bound='slot'), c('render'), c('blend_frames'), c('bind_frames'), c('observe'), c('reset_done'), c('bind_frames', bound='slot'), c('render', mask='done'), c('observe', mask='done'), c('bind_frames'),)),
    "plain_raw": (
        (c('reset'), c('render'),),
        (c('step', flags=0), c('reset_done'), c('render'),)),
    "plain_raw_depth": (
        (c('reset'), c('render'), c('depth'),),
        (c('step', flags=0), c('reset_done'), c('render'), c('depth'),)),
    "blur_plain_raw": (
        (c('reset'), c('render'),),
        (c('step', flags=1), c('bind_frames', bound='slot'), c('render'), c('blend_frames'), c('bind_frames'), c('reset_done'), c('bind_frames', bound='slot'), c('render', mask='done'), c('copy_rows', mask='done'), c('bind_frames'),)),
    "plain_stack": (
        (c('reset'), c('render'), c('observe'), c('push_observation', first='all'),),
        (c('step', flags=0), c('reset_done'), c('render'), c('observe'), c('push_observation', first='done'),)),
    "plain_stack_depth": (
        (c('reset'), c('render'), c('observe'), c('push_observation', first='all'), c('depth'),),
        (c('step', flags=0), c('reset_done'), c('render'), c('observe'), c('push_observation', first='done'), c('depth'),)),
    "blur_plain_stack": (
        (c('reset'), c('render'), c('observe'), c('push_observation', first='all'),),
        (c('step', flags=1), c('bind_frames', bound='slot'), c('render'), c('blend_frames'), c('bind_frames'), c('observe'), c('push_observation'), c('reset_done'), c('bind_frames', bound='slot'), c('render', mask='done'), c('observe', mask='done'), c('push_observation', mask='done', first='done'), c('bind_frames'),)),
    "final_observe": (
        (c('reset'), c('render'), c('observe'),),
        (c('step', flags=0), c('render'), c('observe'), c('copy_rows', mask='done'), c('reset_done'), c('render', mask='done'), c('observe', mask='done'),)),
    "final_observe_depth": (
        (c('reset'), c('render'), c('observe'), c('depth'),),
        (c('step', flags=0), c('render'), c('observe'), c('depth'), c('copy_rows', mask='done'), c('copy_rows', mask='done'), c('reset_done'), c('render', mask='done'), c('observe', mask='done'), c('depth', mask='done'),)),
    "blur_final_observe": (
        (c('reset'), c('render'), c('observe'),),
        (c('step', flags=1), c('bind_frames', bound='slot'), c('render'), c('blend_frames'), c('bind_frames'), c('observe'), c('copy_rows', mask='done'), c('reset_done'), c('bind_frames', bound='slot'), c('render', mask='done'), c('observe', mask='done'), c('bind_frames'),)),
    "final_raw": (
        (c('reset'), c('render'),),
        (c('step', flags=0), c('render'), c('copy_rows', mask='done'), c('reset_done'), c('render', mask='done'),)),
    "final_raw_depth": (
        (c('reset'), c('render'), c('depth'),),
        (c('step', flags=0), c('render'), c('depth'), c('copy_rows', mask='done'), c('copy_rows', mask='done'), c('reset_done'), c('render', mask='done'), c('depth', mask='done'),)),
    "blur_final_raw": (
        (c('reset'), c('render'),),
        (c('step', flags=1), c('bind_frames', bound='slot'), c('render'), c('blend_frames'), c('bind_frames'), c('copy_rows', mask='done'), c('reset_done'), c('bind_frames', bound='slot'), c('render', mask='done'), c('copy_rows', mask='done'), c('bind_frames'),)),
    "final_stack": (
        (c('reset'), c('render'), c('observe'), c('push_observation', first='all'),),
        (c('step', flags=0), c('render'), c('observe'), c('push_observation'), c('copy_rows', mask='done'), c('reset_done'), c('render', mask='done'), c('observe', mask='done'), c('push_observation', mask='done', first='done'),)),
    "final_stack_depth": (
        (c('reset'), c('render'), c('observe'), c('push_observation', first='all'), c('depth'),),
        (c('step', flags=0), c('render'), c('observe'), c('push_observation'), c('depth'), c('copy_rows', mask='done'), c('copy_rows', mask='done'), c('reset_done'), c('render', mask='done'), c('observe', mask='done'), c('push_observation', mask='done', first='done'), c('depth', mask='done'),)),
    "blur_final_stack": (
        (c('reset'), c('render'), c('observe'), c('push_observation', first='all'),),
        (c('step', flags=1), c('bind_frames', bound='slot'), c('render'), c('blend_frames'), c('bind_frames'), c('observe'), c('push_observation'), c('copy_rows', mask='done'), c('reset_done'), c('bind_frames', bound='slot'), c('render', mask='done'), c('observe', mask='done'), c('push_observation', mask='done', first='done'), c('bind_frames'),)),
    # ---- recorded from commit 6308dc1, with labels / instances / boxes / bev traced ----
    "plain_labels": (
        (c('reset'), c('render'), c('observe'), c('labels'),),
        (c('step', flags=0), c('reset_done'), c('render'), c('observe'), c('labels'),)),
    "plain_instances_boxes": (
        (c('reset'), c('render'), c('observe'), c('instances'), c('boxes'),),
        (c('step', flags=0), c('reset_done'), c('render'), c('observe'), c('instances'), c('boxes'),)),
    "plain_labels_instances_fused": (
        (c('reset'), c('render'), c('observe'), c('instances', second='fused'),),
        (c('step', flags=0), c('reset_done'), c('render'), c('observe'), c('instances', second='fused'),)),
    "plain_labels_instances_apart": (
        (c('reset'), c('render'), c('observe'), c('labels'), c('instances'),),
        (c('step', flags=0), c('reset_done'), c('render'), c('observe'), c('labels'), c('instances'),)),
    "plain_every_map": (
        (c('reset'), c('render'), c('observe'), c('depth'), c('instances', second='fused'), c('boxes'), c('bev', second='ids'),),
        (c('step', flags=0), c('reset_done'), c('render'), c('observe'), c('depth'), c('instances', second='fused'), c('boxes'), c('bev', second='ids'),)),
    "plain_blur_bev": (
        (c('reset'), c('render'), c('observe'), c('bev'),),
        (c('step', flags=1), c('bind_frames', bound='slot'), c('render'), c('blend_frames'), c('bind_frames'), c('observe'), c('bev'), c('reset_done'), c('bind_frames', bound='slot'), c('render', mask='done'), c('observe', mask='done'), c('bev', mask='done'), c('bind_frames'),)),
    "final_labels": (
        (c('reset'), c('render'), c('observe'), c('labels'),),
        (c('step', flags=0), c('render'), c('observe'), c('labels'), c('copy_rows', mask='done'), c('copy_rows', mask='done'), c('reset_done'), c('render', mask='done'), c('observe', mask='done'), c('labels', mask='done'),)),
    "final_instances_boxes": (
        (c('reset'), c('render'), c('observe'), c('instances'), c('boxes'),),
        (c('step', flags=0), c('render'), c('observe'), c('instances'), c('boxes'), c('copy_rows', mask='done'), c('copy_rows', mask='done'), c('copy_rows', mask='done'), c('reset_done'), c('render', mask='done'), c('observe', mask='done'), c('instances', mask='done'), c('boxes', mask='done'),)),
    "final_labels_instances_fused": (
        (c('reset'), c('render'), c('observe'), c('instances', second='fused'),),
        (c('step', flags=0), c('render'), c('observe'), c('instances', second='fused'), c('copy_rows', mask='done'), c('copy_rows', mask='done'), c('copy_rows', mask='done'), c('reset_done'), c('render', mask='done'), c('observe', mask='done'), c('instances', mask='done', second='fused'),)),
    "final_labels_instances_apart": (
        (c('reset'), c('render'), c('observe'), c('labels'), c('instances'),),
        (c('step', flags=0), c('render'), c('observe'), c('labels'), c('instances'), c('copy_rows', mask='done'), c('copy_rows', mask='done'), c('copy_rows', mask='done'), c('reset_done'), c('render', mask='done'), c('observe', mask='done'), c('labels', mask='done'), c('instances', mask='done'),)),
    "final_every_map": (
        (c('reset'), c('render'), c('observe'), c('depth'), c('instances', second='fused'), c('boxes'), c('bev', second='ids'),),
        (c('step', flags=0), c('render'), c('observe'), c('depth'), c('instances', second='fused'), c('boxes'), c('bev', second='ids'), c('copy_rows', mask='done'), c('copy_rows', mask='done'), c('copy_rows', mask='done'), c('copy_rows', mask='done'), c('copy_rows', mask='done'), c('copy_rows', mask='done'), c('copy_rows', mask='done'), c('reset_done'), c('render', mask='done'), c('observe', mask='done'), c('depth', mask='done'), c('instances', mask='done', second='fused'), c('boxes', mask='done'), c('bev', mask='done', second='ids'),)),
    "final_blur_bev": (
        (c('reset'), c('render'), c('observe'), c('bev'),),
        (c('step', flags=1), c('bind_frames', bound='slot'), c('render'), c('blend_frames'), c('bind_frames'), c('observe'), c('bev'), c('copy_rows', mask='done'), c('copy_rows', mask='done'), c('reset_done'), c('bind_frames', bound='slot'), c('render', mask='done'), c('observe', mask='done'), c('bev', mask='done'), c('bind_frames'),)),
}


class Tracer:
    """Wraps the TRACED methods of env.sim on the instance; every call goes through to the real method and leaves (name, mask, first, flags,
    bound, second) in `calls`, the tensors as data pointers until names() knows the step's `done`."""

    def __init__(self, env):
        self.env, self.calls = env, []
        for name in TRACED:
            setattr(env.sim, name, self._wrap(name, getattr(env.sim, name)))

    def _wrap(self, name, real):
        sig = inspect.signature(real)

        def call(*a, **kw):
            args = sig.bind(*a, **kw).arguments
            ptr = lambda t: None if t is None else t.data_ptr()
            second = "fused" if args.get("labels_out") is not None else "ids" if args.get("instances_out") is not None else None
            self.calls.append((name, ptr(args.get("mask")), ptr(args.get("first")), args.get("flags", 0 if "flags" in sig.parameters else None),
                               ("slot" if args["devptr"] else None) if name == "bind_frames" else None, second))
            return real(*a, **kw)
        return call

    def names(self, done=None):
        """The calls since the last names(), each tensor named: "done" = the tensor the step returned, "all" = the env's every-env mask."""
        known = {None: None}
        if done is not None:
            known[done.data_ptr()] = "done"
        if getattr(self.env, "_all", None) is not None:
            known[self.env._all.data_ptr()] = "all"
        out = tuple((n, known.get(m, "other"), known.get(f, "other"), fl, b, s) for n, m, f, fl, b, s in self.calls)
        self.calls = []
        return out


def record(cfg):
    """(reset trace, [step traces], how often each env finished) of one configuration."""
    import torch
    env = DuckietownVecEnv("small_loop", N, seed=3, max_steps=MAX_STEPS, domain_rand=False, **CONFIGS[cfg], **CAM)
    tr = Tracer(env)
    env.reset()
    reset, steps, n_done = tr.names(), [], torch.zeros(N, device="cuda")
    a = torch.full((N, 2), 0.5, device="cuda")
    for _ in range(STEPS):
        _, _, done, _ = env.step(a)
        steps.append(tr.names(done))
        n_done += done.float()
    torch.cuda.synchronize()
    env.close()
    return reset, steps, n_done


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_the_calls_on_the_simulator_are_those_of_the_recording(cfg):
    reset, steps, n_done = record(cfg)
    want_reset, want_step = EXPECTED[cfg]
    assert reset == want_reset, cfg
    for t, got in enumerate(steps):
        assert got == want_step, (cfg, t)
    assert float(n_done.min()) >= 1, cfg                     # every env finished, so every masked call had rows to work on
