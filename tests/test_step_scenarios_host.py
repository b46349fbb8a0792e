"""The scenarios of tests/step_scenarios.py on the oracle alone: the inputs reach what tests/test_gpu_step_lanes.py is meant to hold
k_step to -- collisions with every object class, road exits, survivors, several proximity penalties summed in one step, a finished
walk, moving followers -- so that the GPU comparison cannot pass on trajectories where nothing happens.  Runs on a CPU."""
import numpy as np
import pytest

import step_scenarios as S
from oracle import sim as osim
from util import EXT

CASES = [(sc, mode, fs) for sc in S.SCENARIOS for mode, fs in S.PARAMS]


def _ended_by(rec, cause):
    return [p for p in range(S.P) if cause in rec.causes[p]]


def test_maps_have_the_object_counts_the_scenarios_rely_on():
    for (name, md), (ns, nd) in zip(S.map_datas("mixed"), S.MIXED_COUNTS):
        objs = md["objects"]
        assert (sum(1 for o in objs if o.get("static", True)), sum(1 for o in objs if not o.get("static", True))) == (ns, nd), name
    objs = S.cluster_map()["objects"]
    ns, nd = sum(1 for o in objs if o["static"]), sum(1 for o in objs if not o["static"])
    assert (ns, nd) == (5, 3)
    assert ns % 2 and ns % 4 and nd % 2 and nd % 4            # a tail round for 2 and for 4 lanes per env
    assert {S.probe_map("mixed", p) for p in range(5)} == set(range(5))      # every map within any 5 adjacent envs


@pytest.mark.parametrize("scenario", S.SCENARIOS)
def test_starts_are_valid_poses(scenario):
    for p, o in enumerate(S.make_oracles(scenario, 1)):
        assert o._valid_pose(o.cur_pos, o.cur_angle), (scenario, p)


def test_cluster_flanks_the_lane_without_blocking_it():
    o = osim.OracleSim(S.cluster_map(), EXT, do_reset=False)
    for t in (0.4, 0.5, 0.6):
        x, z, ang = S.lane_pose(o.map, 2, 1, 1, t)
        o.set_pose([x, 0.0, z], ang)
        assert S.contributing(o) >= 3 and o._valid_pose(o.cur_pos, o.cur_angle), t


@pytest.mark.parametrize("scenario,mode,frame_skip", CASES)
def test_coverage(scenario, mode, frame_skip):
    rec = S.oracle_record(scenario, mode, frame_skip)
    st = rec.stepped
    assert np.array_equal((rec.prox < 0) & st, (rec.contributing > 0) & st)
    assert _ended_by(rec, "static"), "no episode ends on a static object"
    assert _ended_by(rec, "walker_moved"), "no episode ends on a duckie that has started walking"
    assert _ended_by(rec, "road"), "no episode ends by leaving the road"
    assert int(rec.alive_at_end.sum()) >= 8
    assert rec.reversed.any(), "no walking duckie finished its walk"
    if scenario == "mixed":
        assert _ended_by(rec, "follower"), "no episode ends on a follower Duckiebot"
        for mid, (ns, nd) in enumerate(S.MIXED_COUNTS):
            if ns + nd:
                assert ((rec.prox < 0) & st)[:, rec.map_id == mid].any(), f"no proximity penalty on map {mid}"
        assert int(((rec.contributing >= 2) & st).sum()) >= 1
        assert rec.follower_moved.max() > 0.5 * 0.585
    else:
        assert int(((rec.contributing >= 3) & st).sum()) >= 20
    print(f"{scenario}/{mode}/fs{frame_skip}: ends " + ", ".join(f"{c} {len(_ended_by(rec, c))}" for c in
          ("static", "walker_moved", "follower", "road")) + f"; alive {int(rec.alive_at_end.sum())}; probe-steps with >=2 / >=3 terms "
          f"{int(((rec.contributing >= 2) & st).sum())} / {int(((rec.contributing >= 3) & st).sum())}")
