"""GPU: the planner setting ``solution`` through ``RRT_Planner`` on action tapes (no network): "best_of_round" returns the
cheapest goal node of the first goal-reaching round, "anytime" the cheapest found within the budget, both equal to the
restatement of tests/accept_best_ref.py on the CPU oracle; forests of seeded runs equal their sequential ``plan()``; and the
default mode is untouched.

The car scenario (boxes, (18, 13) -> (18, 17), edge length 32, batch 64) with sample seed 13 and action tape 5 was found on
the CPU oracle: its first goal-reaching round (the second) holds goal candidates 16 and 45 with path costs 69 and 68, and the
third round a cheaper goal node still.  The tests assert these conditions on the restatement, never on the device output."""
import random

import numpy as np
import pytest
import torch

from oracle import geometry as G
from oracle import rrt as ORRT
from oracle.tapes import ActionTape
from tests.accept_best_ref import SolutionOracle
from tests.test_gpu_forest import _planner
from tests.util import load_maze

pytestmark = pytest.mark.gpu

SEED, TAPE, BATCH, ROUNDS = 13, 5, 64, 4
# the f64 states agree with the oracle to 1e-9 (the geometry tests' bound); a path is their float32 rounding, whose last
# place at |x| < 16 is 1.9e-6 -- the facade tests' bound for a path against a stored trace
PATH_TOL = 1e-5


class Tape:
    def __init__(self, seed=TAPE):
        self.tape = ActionTape(seed)

    def sample_round(self, first, B, n_chunks, P):
        return np.stack([self.tape.actions(np.arange(first, first + B), j) for j in range(n_chunks)], axis=1)


def planner(solution=None, **kw):
    args = dict(batch=BATCH, max_candidates=ROUNDS * BATCH, capacity=1024)
    if solution is not None:
        args["solution"] = solution
    args.update(kw)
    return _planner(Tape(), **args)


def seeded_plan(pl, seed=SEED):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    pl.reset()
    return pl.plan()


_ORACLE = {}


def oracle(solution):
    """The restatement's run of the scenario in one mode (computed once, shared, left unchanged)."""
    if solution not in _ORACLE:
        maze = load_maze("boxes")                             # the scenario of tests.test_gpu_forest._planner
        start = np.array([*G.cell_rowcol_to_xy([18, 13], maze), 0.0, 0, 0, 0])
        goal = np.array([*G.cell_rowcol_to_xy([18, 17], maze), 0, 0, 0, 0])
        op = ORRT.OraclePlanner(maze, start, goal, ActionTape(TAPE).sampler(), edge_length=32, emulate_sticky_done=False)
        so = SolutionOracle(op, solution)
        so.path, so.actions = so.plan(ORRT.RandomTape(SEED), ROUNDS * BATCH, BATCH)
        _ORACLE[solution] = so
    return _ORACLE[solution]


def same_path(got, want):
    return got.shape == want.shape and np.abs(got - want).max() < PATH_TOL


def test_best_of_round_returns_the_cheapest_goal_of_the_round():
    first, best = oracle("first"), oracle("best_of_round")
    # the precondition, on the restatement: the plan ends in the same round in both modes, which holds at least two goal
    # candidates of different cost, and the lowest-index one is not the cheapest
    assert len(first.rounds) == len(best.rounds) and best.first_solution_candidates == first.first_solution_candidates
    last = best.rounds[-1]
    costs = [best.cost[last["node_id"][b]] for b in last["goals"]]
    assert len(last["goals"]) >= 2 and len(set(costs)) >= 2 and costs[0] != min(costs)
    g_first, g_best = last["goals"][0], min(last["goals"], key=lambda b: (best.cost[last["node_id"][b]], b))
    assert first.rounds[-1]["goals"] == [g_first] and first.incumbent == first.rounds[-1]["node_id"][g_first]
    assert best.incumbent == last["node_id"][g_best] != last["node_id"][g_first]
    pf, pb = planner("first", emulate_sticky_done=False), planner("best_of_round")
    assert np.array_equal(pf.start_node.state, first.pl.start_state) and np.array_equal(pf.goal_state, first.pl.goal_state)
    path_f, act_f = seeded_plan(pf)
    ids_f = pf._engine.rb.node_id[:BATCH].cpu().numpy()
    path_b, act_b = seeded_plan(pb)
    ids_b = pb._engine.rb.node_id[:BATCH].cpu().numpy()
    assert pb._engine.goal_node == best.incumbent and pf._engine.goal_node == first.incumbent
    assert np.array_equal(ids_b, last["node_id"]) and np.array_equal(ids_f, first.rounds[-1]["node_id"])
    assert np.array_equal(ids_f[:g_first + 1], ids_b[:g_first + 1]) and (ids_f[g_first + 1:] == -1).all()
    assert same_path(path_b, best.path) and np.array_equal(act_b, best.actions)
    assert same_path(path_f, first.path) and np.array_equal(act_f, first.actions)
    assert len(path_b) == best.cost[best.incumbent] < len(path_f) == first.cost[first.incumbent]
    assert pb.results["path_time"] == len(path_b) * pb.env_dt
    for pl, so in ((pf, first), (pb, best)):
        assert pl.results["solutions"] == so.solutions and pl.results["first_solution_candidates"] == so.first_solution_candidates
        assert pl.results["number_of_nodes"] == len(so.pl.tree) and pl.results["iterations"] == so.pl.iterations
    assert pf.results["solutions"] == 1 and pb.results["solutions"] == len(last["goals"])


def test_anytime_returns_the_best_goal_of_the_budget():
    so = oracle("anytime")
    # on the restatement: the budget's four rounds ran, and a later round replaced the incumbent of an earlier one
    assert len(so.rounds) == ROUNDS and so.pl.candidates == ROUNDS * BATCH
    first_round = next(k for k, r in enumerate(so.rounds) if r["goals"])
    assert any(r["replaced"] for r in so.rounds[first_round + 1:])
    pl = planner("anytime")
    path, actions = seeded_plan(pl)
    eng = pl._engine
    assert eng.goal_node == so.incumbent
    assert same_path(path, so.path) and np.array_equal(actions, so.actions)
    assert len(path) == so.cost[so.incumbent] and pl.results["path_time"] == len(path) * pl.env_dt
    assert pl.results["solutions"] == so.solutions and pl.results["first_solution_candidates"] == so.first_solution_candidates
    assert pl.results["number_of_nodes"] == len(so.pl.tree) and pl.results["iterations"] == so.pl.iterations
    n = eng.tree.n_nodes_host
    assert np.array_equal(eng.tree.cost[:n].cpu().numpy(), so.cost)
    assert np.array_equal(eng.tree.parent[:n].cpu().numpy(), so.pl.tree.parents)
    # shorter than what the first goal-reaching round alone gives
    assert len(path) < oracle("best_of_round").cost[oracle("best_of_round").incumbent]


NEW_KEYS = ("solutions", "first_solution_candidates")


def check_runs_equal_sequential(planners, seeds, runs):
    """runs[i][k] against ``random.seed(s); np.random.seed(s); torch.manual_seed(s); planners[i].reset(); planners[i].plan()``."""
    for pl, ss, rr in zip(planners, seeds, runs):
        for s, r in zip(ss, rr):
            path, actions = seeded_plan(pl, s)
            assert r["seed"] == s
            for k in ("iterations", "number_of_nodes") + NEW_KEYS:
                assert r[k] == pl.results[k], (s, k, r[k], pl.results[k])
            assert r["goal_reached"] == (pl._engine.goal_node is not None)
            for got, want in ((r["path"], path), (r["actions"], actions)):
                assert (got is None) == (want is None) and (got is None or np.array_equal(got, want)), s
            if path is not None:
                assert r["path_time"] == pl.results["path_time"]


def test_anytime_forests_equal_sequential_seeded_plans():
    pl = planner("anytime")
    seeds = [0, 1, 2]
    runs = pl.plan_runs(seeds, concurrent=2)
    check_runs_equal_sequential([pl], [seeds], [runs])
    assert any(r["solutions"] > 1 for r in runs) and all(r["iterations"] > 0 for r in runs)
    # anytime runs spend their whole budget: the candidates of four rounds, whenever the first goal came
    assert all(r["first_solution_candidates"] is None or r["first_solution_candidates"] <= ROUNDS * BATCH for r in runs)


def test_anytime_scene_forest_equals_sequential_seeded_plans():
    from ditreeonlineplanner_amd.car_env import CarEnv
    from ditreeonlineplanner_amd.planners.RRT import RRT_Planner, plan_scenario_runs
    sampler = Tape()
    p0 = _planner(sampler, batch=BATCH, max_candidates=ROUNDS * BATCH, capacity=1024, solution="anytime")
    maze = load_maze("shapes")
    env = CarEnv(maze_map=maze, collision_checking=False)
    free = np.argwhere(maze == 0)
    rc_s = free[len(free) // 2]
    rc_g = next(rc for rc in free if 2 <= abs(rc[0] - rc_s[0]) + abs(rc[1] - rc_s[1]) <= 3)
    start = np.array([*env.cell_rowcol_to_xy(np.array(rc_s)), 0.0, 0.0, 0.0, 0.0])
    goal = np.array([*env.cell_rowcol_to_xy(np.array(rc_g)), 0, 0, 0, 0.0])
    p1 = RRT_Planner(start, goal, env_id="carmaze", environment=env, sampler=sampler, ctx=p0.ctx, action_horizon=8,
                     local_map_size=20, local_map_scale=0.2, global_map_scale=1.0, goal_conditioning_bias=0.85, prop_duration=[32],
                     time_budget=600, batch=BATCH, max_candidates=2 * BATCH, capacity=1024, solution="anytime")
    seeds = [[3, 4], [5]]
    runs = plan_scenario_runs([p0, p1], seeds, concurrent=2)
    check_runs_equal_sequential([p0, p1], seeds, runs)
    assert all(r["number_of_nodes"] > 50 for rr in runs for r in rr) and all(r["solutions"] > 0 for rr in runs for r in rr)
    p2 = _planner(sampler, batch=BATCH, max_candidates=ROUNDS * BATCH, capacity=1024, emulate_sticky_done=False, ctx=p0.ctx)
    with pytest.raises(ValueError, match="solution"):
        plan_scenario_runs([p0, p2], seeds)


def test_default_mode_is_untouched():
    """solution="first" and no kwarg at all: the same tree, counters and results on the same tape, no cost array."""
    snaps = []
    for pl in (planner(None), planner("first")):
        path, actions = seeded_plan(pl)
        eng = pl._engine
        assert eng.solution == "first" and eng.tree.cost is None
        n = eng.tree.n_nodes_host
        snaps.append((path, actions, eng.tree.counters.cpu().numpy(), eng.tree.parent[:n].cpu().numpy(),
                      eng.tree.state[:n].cpu().numpy(), eng.tree.num_visit[:n].cpu().numpy(),
                      (random.getstate(), np.random.get_state()[1].copy()), dict(pl.results, time=0, path=None, actions=None)))
        assert pl.results["solutions"] == int(eng.goal_node is not None)
        assert (pl.results["first_solution_candidates"] is None) == (eng.goal_node is None)
    a, b = snaps[0], snaps[1]
    for x, y in zip(a[:6], b[:6]):
        assert np.array_equal(x, y)
    assert a[6][0] == b[6][0] and np.array_equal(a[6][1], b[6][1]) and a[7] == b[7]
    # an engine asked for the default mode keeps the sticky-done emulation's default; the new modes turn it off
    assert snaps[0][2][1] >= 0                                 # the tape reaches the goal
    assert planner(None)._engine.sticky == 1 and planner("anytime")._engine.sticky == 0
