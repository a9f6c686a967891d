"""CPU: the planner setting ``solution`` ("first" | "best_of_round" | "anytime") where no GPU is needed -- the finish rule of the
run scheduler (planners/_runs.py run_jobs) per mode and the two new result keys on a stub engine, the refusals of
``RRT_Planner`` by message with a placeholder context (nothing of the device is touched before they are raised), the
shared-settings error of ``plan_scenario_runs``, and the two new entry points in the header, the binding and the library."""
import os
import re
import types

import numpy as np
import pytest

from ditreeonlineplanner_amd.planners import RRT as F
from ditreeonlineplanner_amd.planners._runs import Job, run_jobs
from tests.test_forest_host import StubEngine, StubPlanner
from tests.util import REPO, load_maze


def test_accept_best_symbols_declared_bound_and_exported():
    from ditreeonlineplanner_amd import _lib
    hdr = open(os.path.join(REPO, "include", "ditree.h")).read()
    for name in ("ditree_accept_best", "ditree_forest_accept_best"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name), name
    assert _lib.lib().ditree_version() == 400


# ---------------------------------------------------------------------- the run scheduler on stubs
class ModePlanner(StubPlanner):
    def __init__(self, tag, max_candidates, env_dt, solution):
        super().__init__(tag, max_candidates, env_dt)
        self.solution = solution


class ModeEngine(StubEngine):
    """StubEngine whose goal run ("d") reaches the goal in its second round with node 7 (two goal nodes that round) and
    finds a better node, 5, in its third (one more goal node): ``goal_node`` is the incumbent."""

    def expand_round(self, s, c, **kw):
        import torch
        counts = kw["counts_per_tree"]
        cnt = super().expand_round(s, c, **kw)
        self.last_solutions = torch.zeros(2, dtype=torch.int64)
        for t, n in enumerate(counts):
            if n and self.tag_of[t] == self.goal_tag:
                if self.rounds_of[t] == 2:
                    self.last_solutions[t] = 2
                elif self.rounds_of[t] == 3:
                    self.goal[t] = 5
                    self.last_solutions[t] = 1
                if self.goal[t] is not None:
                    cnt[t, 1] = 1000 + t                               # the incumbent stays in the counter row
        return cnt

    def round_solutions(self, B):
        return self.last_solutions


@pytest.mark.parametrize("solution", ["first", "best_of_round", "anytime"])
def test_run_jobs_finish_rule_and_result_keys_per_mode(monkeypatch, solution):
    """Jobs a (5 candidates), d (12, reaches the goal in its second round of 4) and e (5) on two trees at batch 4.  "first" and
    "best_of_round": d ends with its goal round (8 candidates, node 7).  "anytime": d runs to its 12 candidates and returns
    the incumbent of its third round (node 5).  Runs without a goal end on their budget with the fallback node in every
    mode."""
    from ditreeonlineplanner_amd.common import map_utils
    monkeypatch.setattr(map_utils, "add_cc_calls", lambda n: None)
    pa, pd = ModePlanner(100.0, 5, 0.1, solution), ModePlanner(200.0, 12, 0.25, solution)
    eng = ModeEngine(goal_tag="d")
    out = [None] * 3
    spec = [(pa, 10, "a"), (pd, 13, "d"), (pa, 14, "e")]
    res = run_jobs(eng, [Job(pl, seed, (out, i), (tag,)) for i, (pl, seed, tag) in enumerate(spec)], 4, "cpu")
    assert res == out
    a, d, e = out
    anytime = solution == "anytime"
    assert d["goal_reached"] and d["success"]
    assert d["iterations"] == 2 * (12 if anytime else 8) and d["number_of_nodes"] == (13 if anytime else 9)
    assert len(d["path"]) == (6 if anytime else 8) and d["path_time"] == len(d["path"]) * 0.25
    assert d["first_solution_candidates"] == 8
    assert d["solutions"] == {"first": 1, "best_of_round": 2, "anytime": 3}[solution]
    for r in (a, e):
        assert not r["goal_reached"] and r["success"] and len(r["path"]) == 6         # the fallback: the last of 5 nodes
        assert r["solutions"] == 0 and r["first_solution_candidates"] is None and r["iterations"] == 10
    # e takes d's tree when d ends with its goal round; in "anytime" it takes a's, and d goes on beside it
    assert [r[0] for r in eng.rounds] == ([[4, 4], [1, 4], [4, 4], [1, 0]] if anytime else [[4, 4], [1, 4], [0, 4], [0, 1]])


# ---------------------------------------------------------------------- refusals, before the device is touched
def _car_args(**kw):
    from ditreeonlineplanner_amd.car_env import CarEnv
    env = CarEnv(maze_map=load_maze("boxes"), collision_checking=False)
    start = np.array([*env.cell_rowcol_to_xy(np.array([18, 13])), 0.0, 0.0, 0.0, 0.0])
    goal = np.array([*env.cell_rowcol_to_xy(np.array([18, 17])), 0, 0, 0, 0.0])
    args = dict(env_id="carmaze", environment=env, sampler=object(), ctx=object(), solution="anytime")   # ctx: never used
    args.update(kw)
    return start, goal, args


class _AntEnv:
    """What BasePlanner's constructor reads of a gym ant env."""

    def __init__(self):
        maze = load_maze("boxes")
        self.maze_data = types.SimpleNamespace(maze_map=maze, x_map_center=40.0, y_map_center=40.0, map_width=20, map_length=20,
                                               cell_xy_to_rowcol=lambda xy: np.array([1, 1]))

    def reset(self, options=None):
        return {"desired_goal": np.zeros(2)}, {}


@pytest.mark.parametrize("solution", ["best_of_round", "anytime"])
def test_planner_refuses_by_name(solution):
    start, goal, args = _car_args(solution=solution)
    with pytest.raises(NotImplementedError, match=f"solution='{solution}': one rank"):
        F.RRT_Planner(start, goal, **dict(args, world_size=2))
    with pytest.raises(NotImplementedError, match=f"solution='{solution}': run_type 0 only"):
        F.RRT_Planner(start, goal, **dict(args, run_type=2))
    with pytest.raises(ValueError, match=f"solution='{solution}' and emulate_sticky_done=True"):
        F.RRT_Planner(start, goal, **dict(args, emulate_sticky_done=True))
    with pytest.raises(NotImplementedError, match=f"solution='{solution}': the car only"):
        F.RRT_Planner(np.zeros(29), np.zeros(29), **dict(args, env_id="antmaze", environment=_AntEnv()))
    with pytest.raises(ValueError, match="solution must be one of"):
        F.RRT_Planner(start, goal, **dict(args, solution="shortest"))


def test_engine_scope_check():
    from ditreeonlineplanner_amd.engine import check_solution
    check_solution("first", True, 4, 3)                      # the default mode keeps every scope it had
    check_solution("anytime", False)
    with pytest.raises(ValueError, match="emulate_sticky_done=False"):
        check_solution("best_of_round", True)
    with pytest.raises(NotImplementedError, match="one rank"):
        check_solution("anytime", False, world_size=2)
    with pytest.raises(NotImplementedError, match="run_type 0"):
        check_solution("anytime", False, run_type=1)


def test_shared_settings_error_names_solution():
    eng = types.SimpleNamespace(A=8, P=64, lm_n=20, lm_scale=0.2, s_global=1.0, k_steps=1, norm=np.zeros(4), sticky=0, early_exit=1,
                                schedule=[64])
    sampler, ctx = object(), object()

    def planner(solution):
        return types.SimpleNamespace(ctx=ctx, sampler=sampler, _engine=eng, batch=16, solution=solution)
    F._check_shared_settings([planner("anytime"), planner("anytime")], F._scene_settings, "plan_scenario_runs")
    with pytest.raises(ValueError, match=r"planner 1 differs from planner 0 in solution \('first' != 'anytime'\)"):
        F._check_shared_settings([planner("anytime"), planner("first")], F._scene_settings, "plan_scenario_runs")
