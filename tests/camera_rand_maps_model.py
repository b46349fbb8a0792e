"""The expected depth, label and instance maps of an env under per-env distortion tables (DTSIM_MAP_ENV_TABLES, include/dtsim.h), from the
existing models alone, and the inputs the camera_rand map tests share.

The quantity: the map of env e at camera pixel p is the RECTILINEAR map of that env -- depth_model.expected(rmap=None), label_model.expected
(name, e, None), instance_model.expected(name, e, None) -- at pixel s = src_index[env_cal[e]][p] of dtsim.distortion.build_src_index, the
table k_remap_cal gathers the env's frame through; 0 (no depth, DTSIM_LABEL_NONE, DTSIM_INSTANCE_NONE) where s = -1.  The sure masks are
gathered the same way, True where s = -1.  Smaller maps by dm.strided.  tests/test_camera_rand_maps_host.py ties this gather to
dm.remap_nearest of the float maps and holds the oracle against its nudged self through every table.

The calibrations: P = 5 of pdist.sample_calibrations(5, SEED) plus the nominal one, six tables; env e of a batch reads table
(e + e // 64) % 6, so that envs e and e + 64 -- one state under `period` replication -- read different tables.  N = 72: one full chunk of 64
envs and a tail of 8."""
import functools

import numpy as np

import depth_model as dm
import instance_model as im
import label_model as lm
from dtsim import _ffi
from dtsim import distortion as pdist

W, H = dm.W, dm.H
P, SEED = 5, 31
N_CAL = P + 1
N, PERIOD = 72, 64
LABEL_CASES = ("planes_dr", "pedestrians", "town", "marks_straight")      # of label_model.CASES: depth, labels and instances against the oracle
CROWD_CASE = "crowd_side"                                                  # of instance_model: a batch of it cycles through im.CROWD_VIEWS
TWO_MAP_CASES = tuple("two_" + m for m in im.TWO_MAPS)                      # im.make_two_map_sim: 6 envs on two maps


@functools.lru_cache(maxsize=None)
def calibrations():
    """(K [6, 3, 3], D [6, 5]): the five sampled calibrations, then the nominal one."""
    K, D = pdist.sample_calibrations(P, SEED)
    return np.concatenate([K, pdist.CAMERA_MATRIX[None]]), np.concatenate([D, pdist.DIST_COEFS[None]])


@functools.lru_cache(maxsize=None)
def tables():
    """(src_index [6, H * W] int32, rx, ry [6, H, W] float32) of calibrations() at the cases' camera size; read-only."""
    K, D = calibrations()
    src, rx, ry = pdist.build_src_index(K, D, W, H, return_maps=True)
    src = np.ascontiguousarray(src.reshape(N_CAL, H * W))
    for a in (src, rx, ry):
        a.setflags(write=False)
    return src, rx, ry


def env_cal(n=N):
    e = np.arange(n)
    return ((e + e // 64) % N_CAL).astype(np.int32)


def gather(a, src, fill=0):
    """[..., H, W] `a` through one table src [H * W]: out[p] = a[src[p]], `fill` where src[p] = -1."""
    a = np.asarray(a)
    flat = a.reshape(a.shape[:-2] + (-1,))
    out = np.where(src >= 0, flat[..., np.maximum(src, 0)], np.asarray(fill, dtype=a.dtype))
    return out.reshape(a.shape)


# ---- the rectilinear expected maps of one (case, case env) ----------------------------------------------------------------------------------

def case_of(name):
    """(W, H, number of case envs, cap) of a case of either model."""
    if name in lm.CASES:
        c = lm.CASES[name]
        return c.W, c.H, len(c.states), c.cap
    c = im.CASES[name]
    return c.W, c.H, c.n_envs, c.cap


def _buffers(name, e, nudge=False):
    return lm.host_buffers(name, e, nudge) if name in lm.CASES else im.host_buffers(name, e, nudge)


@functools.lru_cache(maxsize=None)
def rect_depth(name, e, nudge=False):
    """depth_model.expected(..., rmap=None) of the case's env: the smallest of the four per-sample depths."""
    d = dm.min_depth(_buffers(name, e, nudge)[0])
    d.setflags(write=False)
    return d


def rect_labels(name, e, nudge=False):
    """(labels, sure) of label_model.expected(name, e, None); the label cases only."""
    return lm.expected(name, e, None, nudge)


@functools.lru_cache(maxsize=None)
def rect_instances(name, e, nudge=False):
    """(instances, sure): instance_model.expected(name, e, None) where the case is one of its own, else its statement on the label model's
    buffers (the four samples on one surface in both runs)."""
    if name in im.CASES:
        return im.expected(name, e, None, nudge)
    d0, s0 = _buffers(name, e, False)
    d1, s1 = _buffers(name, e, True)
    inst = (im.instances_of(d1, s1) if nudge else im.instances_of(d0, s0)).astype(np.uint8)
    sure = (s0 == s0[0]).all(axis=0) & (s1 == s1[0]).all(axis=0) & (s0[0] == s1[0])
    inst.setflags(write=False); sure.setflags(write=False)
    return inst, sure


def expected(what, name, e, c, nudge=False):
    """The full-size expected map of case env e through table c: depth [H, W] float64, or (map uint8, sure) for "labels" / "instances"."""
    src = tables()[0][c]
    if what == "depth":
        return gather(rect_depth(name, e, nudge), src, 0.0)
    m, sure = (rect_labels if what == "labels" else rect_instances)(name, e, nudge)
    return gather(m, src, 0), gather(sure, src, True)


def nudge_share(what, name, e, c):
    """The oracle's map of case env e against its nudged self, both through table c: dict(off = share of ALL pixels that differ, n_off,
    sure_off = differing pixels on the gathered sure mask)."""
    a, sure = expected(what, name, e, c)
    b, _ = expected(what, name, e, c, True)
    diff = a != b
    return dict(off=float(diff.mean()), n_off=int(diff.sum()), sure_off=int((diff & sure).sum()), unsure=float((~sure).mean()))


# ---- the cases on a device (the GPU tests) ---------------------------------------------------------------------------------------------------

def case_env(name, e, period=PERIOD):
    """Which env of the case device env e shows under `period` replication."""
    if name.startswith("crowd_"):
        return 0
    return (e % period) % case_of(name)[2]


def case_name(name, e, period=PERIOD):
    """The case whose oracle run device env e shows: a crowd batch cycles through the views."""
    if name.startswith("crowd_"):
        return "crowd_" + im.CROWD_VIEWS[(e % period) % len(im.CROWD_VIEWS)]
    return name


def make_sim(name, n=N, period=PERIOD, states=None, **kw):
    """The case's states on a device with the fisheye on (distortion=True: the handle takes per-env tables), env e showing case_env(name, e):
    a label case as tests/test_gpu_labels.py builds it, the crowd case as im.make_sim does ("crowd" must be registered in dtsim.assets.MAPS).
    states: the init states in place of dm.init_states(case, n, period)."""
    from dtsim import BatchedSimulator
    import frame_parity as fp
    if name.startswith("crowd_"):
        assert states is None and not kw
        return im.make_sim(name, n, period, kind="fisheye")
    c = lm.CASES[name]
    args = dict(camera_width=c.W, camera_height=c.H, distortion=True, domain_rand=c.dr, seed=1, max_steps=10 ** 6, do_reset=False)
    args.update(kw)
    if c.asset_tree:
        args["asset_root"] = fp.ASSETS
    sim = BatchedSimulator(c.map_name, n, **args)
    sim.reset(states=dm.init_states(c, n, period) if states is None else states)
    if c.wait is not None:
        par = sim.read(_ffi.FIELD_OBJ_PARAMS)                 # [N, MAX_DYNAMIC, (vel, wait_time, wiggle)]
        par[:, :, 1] = c.wait
        sim.write(_ffi.FIELD_OBJ_PARAMS, par)
    if c.steps:
        sim.step(np.zeros((c.steps, n, 2), np.float32), n_steps=c.steps)
    return sim


def install(sim, cal=None):
    """The six calibrations on `sim`, env e reading table cal[e] (default env_cal(N))."""
    K, D = calibrations()
    cal = env_cal(sim.num_envs) if cal is None else np.asarray(cal, np.int32)
    sim.set_camera_calibrations(K, D, cal)
    assert np.array_equal(sim._cal[4].reshape(N_CAL, -1), tables()[0])       # the simulator built the tables the model gathers through
    return cal

