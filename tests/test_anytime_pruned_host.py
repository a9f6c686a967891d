"""CPU: ``solution="anytime_pruned"`` where no GPU is needed -- the new entry points in the header, the binding and the library,
the descriptor's layout, the planner's refusals by message with a placeholder context (nothing of the device is touched before
they are raised), the run scheduler's finish rule for an exhausted run on a stub engine, and the preconditions of the device
tests, asserted on the sequential restatement (tests/anytime_pruned_ref.py) and never on the device.

The scenario is that of tests/test_gpu_solution_modes.py: boxes, (18, 13) -> (18, 17), edge length 32, batch 64, action tape 5,
sample seed 13.  Its figures below were found on the CPU oracle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ditreeonlineplanner_amd.planners import RRT as F
from ditreeonlineplanner_amd.planners._runs import Job, run_jobs
from oracle import rrt as ORRT
from tests.accept_best_ref import SolutionOracle
from tests.anytime_pruned_ref import (BATCH, NO_BOUND, ROUNDS, SEED, h_ref, masked_nn_fast, masked_nn_ref, scenario_planner,
                                      scenario_run)
from tests.test_solution_modes_host import ModeEngine, ModePlanner, _AntEnv, _car_args
from tests.util import REPO

NEW_CALLS = ["ditree_bound_keys", "ditree_nn_argmin_bounded", "ditree_forest_nn_argmin_bounded", "ditree_expand_round_bounded",
             "ditree_forest_expand_round_bounded", "ditree_accept_bounded", "ditree_forest_accept_bounded"]
NEW_KEYS = ("pruned_candidates", "closed_nodes", "bound_exhausted")


def test_bounded_symbols_declared_bound_and_exported():
    from ditreeonlineplanner_amd import _lib
    hdr = open(os.path.join(REPO, "include", "ditree.h")).read()
    for name in NEW_CALLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name), name
    assert _lib.lib().ditree_version() == 400


def test_bound_descriptor_layout_matches_the_header():
    from ditreeonlineplanner_amd import _lib
    hdr = open(os.path.join(REPO, "include", "ditree.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} ditree_bound;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(?:const\s+)?(int32_t|double)\s*(\*?)\s*(\w+);", body)
    assert [f[2] for f in fields] == [n for n, _ in _lib.Bound._fields_]
    for (typ, star, name), (_, ctype) in zip(fields, _lib.Bound._fields_):
        assert ctype is (C.c_void_p if star else C.c_double), name
    assert C.sizeof(_lib.Bound) == 6 * 8


def test_the_mode_is_listed_with_the_scope_of_the_other_two():
    from ditreeonlineplanner_amd.engine import SOLUTIONS, check_solution
    assert SOLUTIONS == ("first", "best_of_round", "anytime", "anytime_pruned")
    check_solution("anytime_pruned", False)
    with pytest.raises(ValueError, match="emulate_sticky_done=False"):
        check_solution("anytime_pruned", True)
    with pytest.raises(NotImplementedError, match="one rank"):
        check_solution("anytime_pruned", False, world_size=2)
    with pytest.raises(NotImplementedError, match="run_type 0"):
        check_solution("anytime_pruned", False, run_type=1)


def test_planner_refuses_by_name():
    sol = "anytime_pruned"
    start, goal, args = _car_args(solution=sol)
    with pytest.raises(NotImplementedError, match=f"solution='{sol}': the car only"):
        F.RRT_Planner(np.zeros(29), np.zeros(29), **dict(args, env_id="antmaze", environment=_AntEnv()))
    with pytest.raises(NotImplementedError, match=f"solution='{sol}': one rank"):
        F.RRT_Planner(start, goal, **dict(args, world_size=2))
    with pytest.raises(NotImplementedError, match=f"solution='{sol}': run_type 0 only"):
        F.RRT_Planner(start, goal, **dict(args, run_type=2))
    with pytest.raises(ValueError, match=f"solution='{sol}' and emulate_sticky_done=True"):
        F.RRT_Planner(start, goal, **dict(args, emulate_sticky_done=True))
    with pytest.raises(NotImplementedError, match=f"solution='{sol}': a single prop_duration entry"):
        F.RRT_Planner(start, goal, **dict(args, prop_duration=[32, 64]))
    for bad in (0, -1.0, float("nan"), float("inf"), "5", None, True):
        with pytest.raises(ValueError, match="bound_speed must be a positive finite number"):
            F.RRT_Planner(start, goal, **dict(args, bound_speed=bad))
    for other in ("first", "best_of_round", "anytime"):
        with pytest.raises(ValueError, match="bound_speed belongs to solution='anytime_pruned'"):
            F.RRT_Planner(start, goal, **dict(args, solution=other, bound_speed=5.0))


def test_engine_refuses_reach_by_name():
    from ditreeonlineplanner_amd.engine import ExpansionEngine, check_reach
    assert check_reach(0.1) == 0.1
    for bad in (0.0, -0.1, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError, match="reach must be a positive finite number"):
            check_reach(bad)
    maze = np.zeros((4, 4), dtype=np.float32)
    with pytest.raises(ValueError, match="reach belongs to solution='anytime_pruned'"):
        ExpansionEngine(object(), maze, np.zeros(6), np.zeros(6), emulate_sticky_done=False, solution="anytime", reach=0.1)
    with pytest.raises(NotImplementedError, match="a single prop_duration entry"):
        ExpansionEngine(object(), maze, np.zeros(6), np.zeros(6), emulate_sticky_done=False, solution="anytime_pruned",
                        prop_duration=[32, 64])


# ---------------------------------------------------------------------- the run scheduler on stubs
class PrunedEngine(ModeEngine):
    """ModeEngine (the goal run "d": node 7 in its second round, node 5 in its third) whose tree of the goal run is exhausted
    after that run's round ``exhaust_round``; it has pruned 3 candidates per round since its first goal."""

    def __init__(self, goal_tag, exhaust_round):
        super().__init__(goal_tag)
        self.exhaust_round = exhaust_round

    def _goal_rounds(self, t):
        return max(0, self.rounds_of[t] - 2) if self.tag_of[t] == self.goal_tag else 0

    def exhausted(self, t):
        return (self.exhaust_round is not None and self.tag_of[t] == self.goal_tag and self.goal[t] is not None
                and self.rounds_of[t] >= self.exhaust_round)

    def pruned_candidates(self, t):
        return 3 * self._goal_rounds(t)

    def closed_nodes(self, t):
        return 2 if self.goal[t] is not None else 0


@pytest.mark.parametrize("exhaust_round", [2, 3, None])
def test_run_jobs_ends_an_exhausted_run_and_reuses_its_slot(monkeypatch, exhaust_round):
    """Jobs a (5 candidates), d (16, reaches the goal in its second round of 4) and e (5) on two trees at batch 4.  Exhausted
    after its second round, d ends there with node 7 and e takes its tree; after its third, with node 5; never: d spends its
    16 candidates as an "anytime" run does."""
    from ditreeonlineplanner_amd.common import map_utils
    monkeypatch.setattr(map_utils, "add_cc_calls", lambda n: None)
    pa, pd = ModePlanner(100.0, 5, 0.1, "anytime_pruned"), ModePlanner(200.0, 16, 0.25, "anytime_pruned")
    eng = PrunedEngine("d", exhaust_round)
    out = [None] * 3
    spec = [(pa, 10, "a"), (pd, 13, "d"), (pa, 14, "e")]
    res = run_jobs(eng, [Job(pl, seed, (out, i), (tag,)) for i, (pl, seed, tag) in enumerate(spec)], 4, "cpu")
    assert res == out
    a, d, e = out
    rounds_d = {2: 2, 3: 3, None: 4}[exhaust_round]
    assert d["goal_reached"] and d["success"] and d["iterations"] == 2 * 4 * rounds_d and d["number_of_nodes"] == 4 * rounds_d + 1
    assert len(d["path"]) == (8 if rounds_d == 2 else 6) and d["first_solution_candidates"] == 8
    assert d["solutions"] == (2 if rounds_d == 2 else 3)
    assert d["bound_exhausted"] == (exhaust_round is not None)
    assert d["pruned_candidates"] == 3 * (rounds_d - 2) and d["closed_nodes"] == 2
    for r in (a, e):
        assert not r["goal_reached"] and r["success"] and r["solutions"] == 0 and r["iterations"] == 10
        assert r["pruned_candidates"] == 0 and r["closed_nodes"] == 0 and r["bound_exhausted"] is False
    for r in out:
        assert all(k in r for k in NEW_KEYS)
    want = {2: [[4, 4], [1, 4], [0, 4], [0, 1]], 3: [[4, 4], [1, 4], [4, 4], [1, 0]],
            None: [[4, 4], [1, 4], [4, 4], [1, 4]]}[exhaust_round]
    assert [r[0] for r in eng.rounds] == want


@pytest.mark.parametrize("solution", ["first", "best_of_round", "anytime"])
def test_run_jobs_keeps_the_other_modes_dicts(monkeypatch, solution):
    from ditreeonlineplanner_amd.common import map_utils
    monkeypatch.setattr(map_utils, "add_cc_calls", lambda n: None)
    out = [None]
    run_jobs(ModeEngine(goal_tag="d"), [Job(ModePlanner(200.0, 12, 0.25, solution), 13, (out, 0), ("d",))], 4, "cpu")
    assert not any(k in out[0] for k in NEW_KEYS)


# ---------------------------------------------------------------------- the restatement and its preconditions
def test_heuristic_restatement():
    g = np.array([1.0, -2.0])
    assert h_ref(1.0, -2.0, g, 0.5, 0.1) == 0 and h_ref(1.3, -2.4, g, 0.5, 0.1) == 0         # at the goal, on the disc's edge
    assert h_ref(1.0 + 0.5 + 1e-9, -2.0, g, 0.5, 0.1) == 1 and h_ref(4.0, 2.0, g, 0.5, 0.1) == 45
    assert h_ref(float("nan"), 0.0, g, 0.5, 0.1) == 0 and h_ref(float("inf"), 0.0, g, 0.5, 0.1) == 2 ** 30
    assert h_ref(1e150, 0.0, g, 0.5, 1e-3) == 2 ** 30


def test_masked_search_restatements_agree():
    rng = np.random.RandomState(0)
    xy = rng.uniform(-5, 5, (300, 2))
    xy[7] = xy[3]                                             # a duplicate: the lower index wins while it is open
    xy[11] = np.nan
    q = np.concatenate([rng.uniform(-5, 5, (40, 2)), xy[[3]], [[np.nan, 0.0]]])
    key = rng.randint(0, 100, 300)
    for U in (0, 30, 50, 101, NO_BOUND):
        assert np.array_equal(masked_nn_ref(q, xy, key, U), masked_nn_fast(q, xy, key, U))
    assert masked_nn_ref(xy[[3]], xy, key, NO_BOUND)[0] == 3
    key[3] = 99
    assert masked_nn_ref(xy[[3]], xy, key, 99)[0] == (7 if key[7] < 99 else masked_nn_fast(xy[[3]], xy, key, 99)[0])


def _anytime():
    so = SolutionOracle(scenario_planner(), "anytime")
    so.plan(ORRT.RandomTape(SEED), ROUNDS * BATCH, BATCH)
    return so


def test_preconditions_at_the_default_bound():
    po, so = scenario_run(), _anytime()
    r = po.rounds
    assert len(r) == ROUNDS and not po.exhausted and po.key[0] == 36
    # through the first goal-reaching round (the second) the run is "anytime": the same ids, parents and incumbent
    assert not r[0]["goals"] and r[1]["goals"] and r[0]["U"] == r[1]["U"] == NO_BOUND
    for k in (0, 1):
        assert np.array_equal(r[k]["node_id"], so.rounds[k]["node_id"]) and np.array_equal(r[k]["parent"], so.rounds[k]["parent"])
        assert not r[k]["pruned"] and r[k]["incumbent"] == so.rounds[k]["incumbent"]
    assert po.cost[r[1]["incumbent"]] == 68 and r[1]["nodes_after"] == 117
    assert po.cost[:117] == so.cost[:117]
    # the third round: U = 68, 88 of 117 nodes closed, most parents differ from the unmasked search's, some candidates are
    # pruned, and the incumbent is replaced by a 66-row path
    assert r[2]["U"] == 68 and r[2]["closed_before"] == 88 and r[2]["nodes_before"] == 117
    assert (r[2]["parent"] != r[2]["unmasked_parent"]).sum() > BATCH // 2
    assert 0 < len(r[2]["pruned"]) < BATCH and r[2]["replaced"] and po.cost[r[2]["incumbent"]] == 66
    assert all(po.key[p] < 68 for p in r[2]["parent"])
    # every goal node appended after the first incumbent replaced it
    assert all(rr["replaced"] for rr in r[2:] if rr["goals"])
    # after four rounds the tree is smaller than plain anytime's, and the path no longer
    assert len(po.key) == 138 and len(so.cost) == 177
    assert po.cost[po.incumbent] == 66 <= so.cost[so.incumbent]
    assert len(po.path) == 66 and po.pruned == sum(len(rr["pruned"]) for rr in r) > 0


def test_preconditions_at_bound_speed_2_5():
    po = scenario_run(bound_speed=2.5)
    assert po.key[0] == 71
    assert len(po.rounds) == 2 and po.pl.candidates == 2 * BATCH and po.exhausted
    assert po.cost[po.incumbent] == 68 and po.rounds[1]["U"] == NO_BOUND and po.pruned == 0
    assert po.closed_nodes() == len(po.key) == 117
    # the random streams sit where a plan of two rounds leaves them
    tape = ORRT.RandomTape(SEED)
    H, W = po.pl.maze.shape
    for _ in range(2):
        tape.draw_round(BATCH, W, H, po.pl.goal_state, goal_sample_rate=po.pl.gsr, goal_conditioning_bias=po.pl.gcb)
    assert tape.py.getstate() == po.tape.py.getstate()
    a, b = tape.np.get_state(), po.tape.np.get_state()
    assert np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.mark.parametrize("seed", [3, 5])
def test_preconditions_of_the_forest_seeds(seed):
    """Seeds 3 and 5 replace their incumbent in a bounded round."""
    po = scenario_run(seed=seed)
    assert any(rr["replaced"] and rr["U"] != NO_BOUND for rr in po.rounds)
