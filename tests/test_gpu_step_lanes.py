"""k_step at every lane count, against the oracle and against itself.

dtsim_create picks how many lanes of a wavefront share one env (csrc/dtsim_api.hip, the step_lanes rule), and each count is its own
instantiation k_step<SAMPLER, L> (csrc/physics.hip) -- other owner lanes for the objects, other shuffle rounds and tails in the penalty
sums, another butterfly.  The scenarios of tests/step_scenarios.py (tests/test_step_scenarios_host.py shows what they reach) run here
at one batch size per lane count, each = 1 (mod 32): env e replicates probe e % 32 and the last env sits alone in the last workgroup.

  a. oracle         probes 0..31 against the oracle while its episode is alive: the comparison of test_gpu_physics._run_traj, plus the
                    dynamic objects at the tolerances of test_dynamic_duckies_match_oracle / test_dynamic_duckiebots_match_oracle
  b. replicas       every env equals its probe bit for bit, on every field, at every step, done envs included
  c. lane counts    the probe rows at 2 lanes and at 1 lane per env equal those at 4 lanes bit for bit (physics.hip: "the same bits
                    for every L")
  d. fused          step(n_steps=T) == T x step()
  e. pool resets    (b) and (c) across auto resets from a spawn pool, which also move envs between maps
"""
import ctypes as C
import functools
import time
from types import SimpleNamespace

import numpy as np
import pytest

import step_scenarios as S
from dtsim import _ffi
from test_gpu_physics import FLOAT_TOL

pytestmark = pytest.mark.gpu

# step_lanes in dtsim_create (csrc/dtsim_api.hip): 4 lanes per env while 4 N <= 32768, 2 while 2 N <= 32768, 1 beyond
N_LANES_4, N_LANES_2, N_LANES_1 = 33, 8193, 16385
SIZES = (N_LANES_4, N_LANES_2, N_LANES_1)
assert 4 * N_LANES_4 <= 32768 < 4 * N_LANES_2 and 2 * N_LANES_2 <= 32768 < 2 * N_LANES_1 and all(n % S.P == 1 for n in SIZES)

# the object tolerances of tests/test_gpu_physics.py (literals there): a walking duckie's centre and active flag are exact and its
# y rotation within 1e-9 (test_dynamic_duckies_match_oracle); a follower's centre within 1e-9 and its y rotation within 1e-7
# (test_dynamic_duckiebots_match_oracle)
DUCKIE_YROT_TOL, BOT_CENTER_TOL, BOT_YROT_TOL = 1e-9, 1e-9, 1e-7

FIELDS = ("POS", "ANGLE", "REWARD", "DONE", "DONE_CODE", "STEP_COUNT", "TILE", "LANE", "IN_LANE", "PROX", "SPEED", "TIMESTAMP", "WHEELS",
          "OBJ_CENTER", "OBJ_ACTIVE", "OBJ_YROT", "OBJ_Y", "OBJ_PARAMS")
CASES = [(sc, pi) for sc in S.SCENARIOS for pi in range(len(S.PARAMS))]
CASE_IDS = [f"{sc}-{S.PARAMS[pi][0]}-fs{S.PARAMS[pi][1]}" for sc, pi in CASES]
POOL_STEPS, POOL_MAX_STEPS = 80, 25


def _read(sim, fields=FIELDS):
    return {f: sim.read(getattr(_ffi, "FIELD_" + f)) for f in fields}


def _bytes(a):
    """[rows, bytes per row]: equality of these is equality bit for bit (NaN payloads and signed zeros included)."""
    a = np.ascontiguousarray(a)
    return a.reshape(a.shape[0], -1).view(np.uint8)


def _replica_mismatch(a):
    """None if every env e of a [N, ...] equals env e % P bit for bit, else the first env that does not."""
    b = _bytes(a)
    N = b.shape[0]
    k = (N - 1) // S.P
    if np.array_equal(b[:k * S.P].reshape(k, S.P, -1), np.broadcast_to(b[:S.P], (k, S.P, b.shape[1]))) and np.array_equal(b[N - 1], b[0]):
        return None
    return int(np.flatnonzero((b != b[np.arange(N) % S.P]).any(axis=1))[0])


@functools.lru_cache(maxsize=None)
def _run(scenario, pi, N):
    """T single steps at batch size N: the probe rows of every field after every step ([T, P, ...]), the first replica mismatch
    (step, field, env) or None, and every field of every env after the last step.  Shared between the tests: read-only."""
    mode, fs = S.PARAMS[pi]
    t0 = time.perf_counter()
    sim = S.make_sim(scenario, N, mode, fs)
    acts = S.tiled_actions(scenario, mode, N)
    probes = {f: [] for f in FIELDS}
    mismatch, last = None, None
    for t in range(S.T):
        sim.step(acts[t])
        last = _read(sim)
        for f, a in last.items():
            probes[f].append(a[:S.P].copy())
            if mismatch is None:
                e = _replica_mismatch(a)
                if e is not None:
                    mismatch = (t, f, e)
    sim.close()
    return SimpleNamespace(probes={f: np.stack(v) for f, v in probes.items()}, mismatch=mismatch, last=last,
                           seconds=time.perf_counter() - t0)


def _first(bad):
    """(step, probe) of the first True of bad [T, P], for the assertion message."""
    t, p = np.argwhere(bad)[0]
    return int(t), int(p)


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("scenario,pi", CASES, ids=CASE_IDS)
def test_probes_match_oracle(scenario, pi, N):
    mode, fs = S.PARAMS[pi]
    rec = S.oracle_record(scenario, mode, fs)
    g = _run(scenario, pi, N).probes
    st = rec.stepped
    for name, dev, ref in (("done", g["DONE"] != 0, rec.done), ("done code", g["DONE_CODE"], rec.code),
                           ("tile", g["TILE"], rec.tile), ("in_lane", g["IN_LANE"] != 0, rec.in_lane),
                           ("step_count", g["STEP_COUNT"], rec.step_count)):
        bad = (dev != ref).reshape(S.T, S.P, -1).any(axis=2) & st
        assert not bad.any(), (name, N, _first(bad), dev[_first(bad)], ref[_first(bad)])
    err = np.max(np.stack([np.abs(g["POS"] - rec.pos).max(axis=2), np.abs(g["ANGLE"] - rec.angle), np.abs(g["REWARD"] - rec.reward),
                           np.abs(g["PROX"] - rec.prox), np.abs(g["LANE"][..., 0] - rec.lane[..., 0]),
                           np.abs(g["LANE"][..., 1] - rec.lane[..., 1]), np.abs(g["LANE"][..., 3] - rec.lane[..., 3]),
                           np.abs(g["SPEED"] - rec.speed) * 1e-2]), axis=0)
    err = np.where(st, err, 0.0)
    print(f"{scenario}/{mode}/fs{fs} N={N}: probe-steps compared {int(st.sum())}, max abs err {err.max():.3e}, "
          f"{_run(scenario, pi, N).seconds:.1f} s on the device")
    assert not (err > FLOAT_TOL).any(), (N, _first(err > FLOAT_TOL), err.max())
    # dynamic objects: slot k of the device is the oracle's k-th non-static object
    obj_err = 0.0
    for p in range(S.P):
        rows = st[:, p]
        for k, kind in enumerate(rec.dyn_kind[p]):
            cen, yrot = g["OBJ_CENTER"][rows, p, k], g["OBJ_YROT"][rows, p, k]
            rcen, ryrot = rec.obj_center[rows, p, k], rec.obj_yrot[rows, p, k]
            if kind == "duckiebot":
                assert np.abs(cen - rcen).max(initial=0.0) <= BOT_CENTER_TOL, (N, p, k)
                assert np.abs(yrot - ryrot).max(initial=0.0) <= BOT_YROT_TOL, (N, p, k)
                obj_err = max(obj_err, np.abs(cen - rcen).max(initial=0.0))
            else:
                assert np.array_equal(cen, rcen), (N, p, k)
                assert np.array_equal(g["OBJ_ACTIVE"][rows, p, k] != 0, rec.obj_active[rows, p, k]), (N, p, k)
                assert np.abs(yrot - ryrot).max(initial=0.0) <= DUCKIE_YROT_TOL, (N, p, k)
    print(f"  followers' centres: max abs err {obj_err:.3e}")


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("scenario,pi", CASES, ids=CASE_IDS)
def test_every_env_replicates_its_probe(scenario, pi, N):
    assert _run(scenario, pi, N).mismatch is None, "(step, field, first env that differs from env % 32)"


@pytest.mark.parametrize("N", (N_LANES_2, N_LANES_1))
@pytest.mark.parametrize("scenario,pi", CASES, ids=CASE_IDS)
def test_lane_count_does_not_change_a_bit(scenario, pi, N):
    a, b = _run(scenario, pi, N_LANES_4).probes, _run(scenario, pi, N).probes
    for f in FIELDS:
        bad = (_bytes(a[f].reshape((S.T * S.P,) + a[f].shape[2:])) != _bytes(b[f].reshape((S.T * S.P,) + b[f].shape[2:]))).any(axis=1)
        assert not bad.any(), (f, N, "first (step, probe):", divmod(int(np.flatnonzero(bad)[0]), S.P))


@pytest.mark.parametrize("N", (N_LANES_2, N_LANES_1))
@pytest.mark.parametrize("scenario,pi", CASES, ids=CASE_IDS)
def test_fused_steps_equal_single_steps(scenario, pi, N):
    mode, fs = S.PARAMS[pi]
    single = _run(scenario, pi, N).last
    sim = S.make_sim(scenario, N, mode, fs)
    sim.step(S.tiled_actions(scenario, mode, N), n_steps=S.T)
    fused = _read(sim)
    sim.close()
    for f in FIELDS:
        bad = (_bytes(fused[f]) != _bytes(single[f])).any(axis=1)
        assert not bad.any(), (f, N, "first env:", int(np.flatnonzero(bad)[0]))


@functools.lru_cache(maxsize=None)
def _pool_run(pi, N):
    """The mixed scenario with auto reset from a pool of the 32 probe starts, permuted: every field after POOL_STEPS fused steps."""
    mode, fs = S.PARAMS[pi]
    sim = S.make_sim("mixed", N, mode, fs, auto_reset=True, max_steps=POOL_MAX_STEPS)
    pool = S.init_states("mixed", S.P, order=np.random.default_rng(7).permutation(S.P))
    _ffi.check(sim._lib, sim._lib.dtsim_set_spawn_pool(sim._h, pool, S.P))
    sim.step(S.tiled_actions("mixed", mode, N)[:POOL_STEPS], n_steps=POOL_STEPS)
    out = _read(sim, FIELDS + ("EPISODE", "MAP_ID"))
    sim.close()
    return out


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("pi", range(len(S.PARAMS)), ids=[f"{m}-fs{fs}" for m, fs in S.PARAMS])
def test_pool_auto_reset(pi, N):
    """N = 1 (mod 32) makes the pool slot (e + episode * N) % 32 of an env that of its probe, so replicas stay replicas."""
    g, ref = _pool_run(pi, N), _pool_run(pi, N_LANES_4)
    assert (g["EPISODE"] >= 2).all(), int(g["EPISODE"].min())          # max_steps = 25: two resets within 52 steps at the latest
    assert len(set(zip(g["MAP_ID"][:S.P].tolist(), [s[0] for s in S.starts("mixed")]))) > 5      # resets moved envs to other maps
    for f, a in g.items():
        assert _replica_mismatch(a) is None, (f, N, _replica_mismatch(a))
        bad = (_bytes(a[:S.P]) != _bytes(ref[f][:S.P])).any(axis=1)
        assert not bad.any(), (f, N, "first probe:", int(np.flatnonzero(bad)[0]))
