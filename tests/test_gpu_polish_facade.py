"""GPU: RRT_Planner.polish and planners.RRT.polish_runs on plans made from the golden action tape."""
import random

import numpy as np
import pytest
import torch

from tests import polish_ref as R
from tests.test_gpu_facades import _tape_planner

pytestmark = pytest.mark.gpu

SETTINGS = dict(rollouts=256, iterations=8, sigma=(1.0, 0.1), hold=8, seed=1)


def test_plan_then_polish_returns_a_shorter_replayable_plan():
    g, pl = _tape_planner("easy", 1)
    path0, actions0 = pl.plan()
    assert pl._engine.goal_node is not None and len(actions0) == 45
    time0 = pl.results["path_time"]
    path, actions = pl.polish(**SETTINGS)
    res = pl.results
    assert path is res["path"] and actions is res["actions"]
    assert path.dtype == np.float32 and actions.dtype == np.float32 and path.shape[1] == 6 and actions.shape[1] == 2
    assert len(path) == len(actions) + 1 and len(actions) <= len(actions0)
    assert res["path_time"] == len(path) * pl.env_dt <= time0
    pol = res["polish"]
    assert set(pol) == {"status", "rows_in", "rows_out", "arrival_in", "arrival_out", "trace"}
    assert pol["status"] == "ok" and pol["rows_in"] == 45 and pol["rows_out"] == len(actions) and pol["arrival_out"] <= pol["arrival_in"]
    assert len(pol["trace"]["rows"]) == SETTINGS["iterations"]
    # the oracle replays the returned float32 actions to the goal, without a collision, at exactly their last row
    rp = R.replay(pl.maze, pl.start_node.state, np.asarray(pl.env.goal, dtype=np.float64), actions.astype(np.float64))
    assert rp["status"] == R.OK and rp["rows"] == len(actions)
    assert np.abs(rp["states"] - path).max() < 1e-5
    assert np.array_equal(path[0], pl.start_node.state.astype(np.float32))


def test_polish_of_a_plan_without_a_goal_node_returns_it_unchanged():
    g, pl = _tape_planner("race", 1)
    path0, actions0 = pl.plan()
    assert pl._engine.goal_node is None
    before = dict(pl.results)
    path, actions = pl.polish(**SETTINGS)
    assert path is path0 and actions is actions0
    assert pl.results["polish"]["status"] == "no_goal" and pl.results["polish"]["trace"] is None
    assert all(pl.results[k] is before[k] for k in before)


def test_polish_runs_equals_the_single_polishes():
    from ditreeonlineplanner_amd.planners.RRT import polish_runs
    g, pl = _tape_planner("easy", 1)
    seeds = [42, 7]
    runs = pl.plan_runs(seeds)
    assert runs[0]["goal_reached"]
    out = polish_runs(pl, runs, **SETTINGS)
    assert out is runs
    for s, run in zip(seeds, runs):
        random.seed(s)
        np.random.seed(s)
        torch.manual_seed(s)
        pl.reset()
        pl.plan()
        pl.polish(**SETTINGS)
        one = pl.results
        assert run["polish"]["status"] == one["polish"]["status"]
        assert run["polish"]["rows_out"] == one["polish"]["rows_out"] and run["polish"]["arrival_out"] == one["polish"]["arrival_out"]
        assert run["path_time"] == one["path_time"]
        if run["path"] is None:
            assert one["path"] is None
        else:
            assert np.array_equal(run["path"], one["path"]) and np.array_equal(run["actions"], one["actions"])
    assert runs[0]["polish"]["status"] == "ok" and len(runs[0]["path"]) == len(runs[0]["actions"]) + 1

