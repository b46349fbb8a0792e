"""`not gpu`: the later-episode goldens without domain randomisation (tests/golden/lightcap_*.npz, tests/golden/make_lightcap.py).

They are complete; the oracle's GL-faithful mode reproduces their frames at the tolerance of tests/test_gl_golden.py (>= 99.8 % of the
pixels within +-1/255, mean <= 0.02/255) -- with each record's eye-space light, which from the second episode on is not the first one's;
and where the reference tree and Mesa are present, the recipe reproduces the committed bytes.
"""
import os

import numpy as np
import pytest

import gl_golden as G
from frame_parity import ORACLE_GL, assert_within, stats
from gl_golden import LIGHTCAP_FLOW as FLOW, LIGHTCAP_RESET_CASES as RESET_CASES, load_lightcap as load

FIRST_LIGHT = np.array([0.0, 3.0, 0.0, 1.0])
STATE_KEYS = ("frame", "pos", "angle", "cam_height", "cam_angle", "cam_fov_y", "camera_noise", "horizon", "ground", "light_eye", "light_raw",
              "light_ambient", "light_diffuse", "obj_pos", "obj_yrot", "obj_visible", "obj_pattern")


def records(d, prefix):
    """The `prefix` records of the flow golden as a golden of their own (the keys gl_golden's helpers read)."""
    out = {k[len(prefix):]: v for k, v in d.items() if k.startswith(prefix)}
    out["meta"] = dict(d["meta"], dr=False)
    return out


def test_lightcap_goldens_are_complete():
    assert not any(n.startswith("ref_gl_") for n in RESET_CASES + [FLOW])          # (outside the glob of the ref_gl_* case table)
    for name in RESET_CASES:
        d = load(name)
        n = len(d["frame"])
        assert n >= 4 and n % 2 == 0 and "llvmpipe" in d["meta"]["renderer"] and d["frame"].shape[1:] == (d["meta"]["H"], d["meta"]["W"], 3)
        for k in STATE_KEYS:
            assert len(d[k]) == n, (name, k)
        assert np.array_equal(d["light_eye"][0], FIRST_LIGHT)                     # the first episode: GL's light as set at the identity
        after = d["light_eye"][1::2]
        assert (np.abs(after - FIRST_LIGHT).max(-1) > 0.1).all(), name            # every later episode has a light of its own
        assert np.array_equal(d["light_eye"][1:-1:2], d["light_eye"][2::2])       # fixed for the whole episode
    d = load(FLOW)
    S, T = d["traj_done"].shape
    assert S == len(d["meta"]["seeds"]) == 3 and T == d["meta"]["n_steps"]
    for k in ("pos", "angle", "speed", "reward", "actions"):
        assert d["traj_" + k].shape[:2] == (S, T), k
    for s in range(S):
        assert int(d["traj_done"][s].sum()) >= 2                                   # >= 3 episodes per seed
        resets = np.nonzero(d["reset_seed_index"] == s)[0]
        assert list(d["reset_at_step"][resets]) == [-1] + list(np.nonzero(d["traj_done"][s])[0])   # one recorded reset per done
    for k in STATE_KEYS:
        assert len(d["reset_" + k]) == len(d["reset_seed_index"]) and len(d["kept_" + k]) == len(d["kept_seed_index"]), k
    assert (d["reset_light_raw"] == FIRST_LIGHT).all()
    assert (np.abs(d["kept_light_eye"] - FIRST_LIGHT).max(-1) > 0.1).sum() >= 20   # kept frames of later episodes


@pytest.mark.parametrize("name", RESET_CASES + [FLOW])
def test_oracle_reproduces_the_lightcap_frames(name):
    d = load(name)
    if name == FLOW:
        d = records(d, "kept_")
    worst = dict(mean=0.0, gt1=0.0)
    for k in range(len(d["frame"])):
        s = stats(G.oracle_frame(d, k, "gouraud"), d["frame"][k])
        assert_within(s, ORACLE_GL, (name, k))
        for key in worst:
            worst[key] = max(worst[key], s[key])
    print(f"\n{name}: worst of {len(d['frame'])} frames: beyond +-1 {worst['gt1']:.5f}, mean abs {worst['mean']:.5f} / 255")


@pytest.mark.parametrize("name", RESET_CASES + [FLOW])
def test_committed_lightcap_goldens_are_what_the_recipe_produces(name):
    from oracle.gl import refgl
    if not refgl.available():
        pytest.skip("reference tree or swrast driver not present")
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_lightcap", os.path.join(G.GOLDEN, "make_lightcap.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    fresh = mk.build(name)
    d = load(name)
    assert set(fresh) == set(d)
    for key in fresh:
        if key != "meta":
            assert np.array_equal(np.asarray(fresh[key]), d[key]), (name, key)
