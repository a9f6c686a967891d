"""GPU: ``RRT_Planner(sparse_cell=...)`` on the action tape of tests/test_gpu_solution_modes.py, per mode, with and without
``near_radius``.  Every round of a plan is held against the restated planner of tests/sparse_tree_ref.py -- parents, node ids,
costs --, the active flags after the plan against ``active_ref`` from scratch, ``results`` against the restated counts, the path
and the actions against the restatement's.  The setting is the one whose preconditions tests/test_sparse_tree_host.py asserts on
the CPU (seed 5, eight rounds of 64, cells of 0.5 m, one heading: candidates dominated, nodes retired, parents moved).  Then: the
samples and the generators of a run do not depend on the kwarg, and forests of seeded runs equal their sequential ``plan()``."""
import numpy as np
import pytest

from tests.anytime_pruned_ref import BATCH
from tests.sparse_tree_ref import active_ref, sparse_run
from tests.test_gpu_forest import _planner, _rng_states, _same_states
from tests.test_gpu_solution_modes import PATH_TOL, Tape, check_runs_equal_sequential, seeded_plan
from tests.util import load_maze

pytestmark = pytest.mark.gpu

SEED, ROUNDS, CELL, HEADINGS, RADIUS = 5, 8, 0.5, 1, 1.0
MODES = ["best_of_round", "anytime", "anytime_pruned"]
KEYS = ("dominated_candidates", "retired_nodes", "active_nodes")


def planner(solution, sparse_cell=CELL, near_radius=None, **kw):
    args = dict(batch=BATCH, max_candidates=ROUNDS * BATCH, capacity=1024, solution=solution)
    if sparse_cell is not None:
        args.update(sparse_cell=sparse_cell, sparse_headings=HEADINGS)
    if near_radius is not None:
        args["near_radius"] = near_radius
    args.update(kw)
    return _planner(Tape(), **args)


class RoundLog:
    """Per round of a planner's engine: the samples, and behind its accept the parents, the node ids and the node count."""

    def __init__(self, pl):
        self.rounds = []
        eng = self.eng = pl._engine
        expand, accept = eng.expand_round, eng.accept

        def logged_expand(samples, cond_goal, **kw):
            self.samples = samples.cpu().numpy()
            return expand(samples, cond_goal, **kw)

        def logged_accept(B=None):
            B = eng._B if B is None else B
            cnt = accept(B)
            self.rounds.append(dict(samples=self.samples[:B].copy(), parent=eng.rb.parent[:B].cpu().numpy(),
                                    node_id=eng.rb.node_id[:B].cpu().numpy(), nodes=eng.tree.n_nodes_host))
            return cnt
        eng.expand_round, eng.accept = logged_expand, logged_accept


@pytest.mark.parametrize("near", [None, RADIUS])
@pytest.mark.parametrize("solution", MODES)
def test_every_round_is_the_restated_planners(solution, near):
    o = sparse_run(solution, CELL, headings=HEADINGS, near_radius=near, seed=SEED, rounds=ROUNDS)
    pl = planner(solution, near_radius=near)
    assert pl._engine.sparse == (CELL, HEADINGS)
    log = RoundLog(pl)
    path, actions = seeded_plan(pl, SEED)
    eng = pl._engine
    assert len(log.rounds) == len(o.rounds)
    for k, (got, r) in enumerate(zip(log.rounds, o.rounds)):
        assert np.array_equal(got["parent"], r["parent"]), (k, np.nonzero(got["parent"] != np.asarray(r["parent"]))[0][:5])
        assert np.array_equal(got["node_id"], r["node_id"]), (k, np.nonzero(got["node_id"] != r["node_id"])[0][:5])
        assert got["nodes"] == r["nodes_after"]
    n = eng.tree.n_nodes_host
    assert n == len(o.cost) and eng.goal_node == o.incumbent
    assert np.array_equal(eng.tree.parent[:n].cpu().numpy(), o.pl.tree.parents)
    assert np.array_equal(eng.tree.cost[:n].cpu().numpy(), o.cost)
    # the active flags: the restated planner's, and a pure function of the tree
    flags = eng.tree.active[:n].cpu().numpy()
    act, _ = active_ref(eng.tree.state[:n].cpu().numpy(), eng.tree.cost[:n].cpu().numpy(), o.grid)
    assert np.array_equal(flags, np.array(o.active, dtype=np.uint8)) and np.array_equal(flags, act)
    res = pl.results
    assert (res["dominated_candidates"], res["retired_nodes"], res["active_nodes"]) == (o.dominated, o.retired, o.active_nodes())
    assert res["number_of_nodes"] == n and res["solutions"] == o.solutions
    assert res["first_solution_candidates"] == o.first_solution_candidates
    if solution == "anytime_pruned":
        assert np.array_equal(eng.tree.key[:n].cpu().numpy(), o.key) and res["pruned_candidates"] == o.pruned
    assert path.shape == o.path.shape and np.abs(path - o.path).max() < PATH_TOL and np.array_equal(actions, o.actions)
    assert o.incumbent is not None and len(path) == o.cost[o.incumbent]
    # conditions: the rule was at work (its figures are asserted on the CPU for "anytime" without near_radius)
    assert o.dominated > 0 and int(eng.tree.counters[6].item()) == 0
    if solution == "anytime" and near is None:
        assert (o.dominated, o.retired, n) == (216, 3, 141)


def test_without_the_kwarg_every_dominated_candidate_gets_a_node():
    """The same plan without ``sparse_cell``: more nodes, no sparse keys -- and the same samples, round for round, and the same
    generator states at the end (an "anytime" plan always runs its budget's rounds)."""
    runs = []
    for cell in (CELL, None):
        pl = planner("anytime", sparse_cell=cell)
        log = RoundLog(pl)
        seeded_plan(pl, SEED)
        runs.append(([r["samples"] for r in log.rounds], _rng_states(), dict(pl.results), pl._engine))
    (sa, ga, ra, ea), (sb, gb, rb, eb) = runs
    assert ea.sparse is not None and eb.sparse is None and eb.tree.active is None
    assert len(sa) == len(sb) == ROUNDS and all(np.array_equal(a, b) for a, b in zip(sa, sb))
    assert _same_states(ga, gb)
    assert all(k in ra for k in KEYS) and not any(k in rb for k in KEYS)
    assert rb["number_of_nodes"] > ra["number_of_nodes"] + 100


@pytest.mark.parametrize("solution,near", [("anytime", None), ("anytime_pruned", RADIUS)])
def test_sparse_forests_equal_sequential_seeded_plans(solution, near):
    pl = planner(solution, near_radius=near)
    seeds = [3, 5, 13]
    runs = pl.plan_runs(seeds, concurrent=2)
    check_runs_equal_sequential([pl], [seeds], [runs])
    for s, r in zip(seeds, runs):                              # the new keys too, run by run
        seeded_plan(pl, s)
        assert all(r[k] == pl.results[k] for k in KEYS), (s, [(r[k], pl.results[k]) for k in KEYS])
    o = sparse_run(solution, CELL, headings=HEADINGS, near_radius=near, seed=SEED, rounds=ROUNDS)
    r = runs[1]                                                # seed 5: the restated planner's run
    assert r["number_of_nodes"] == len(o.cost) and (r["dominated_candidates"], r["retired_nodes"]) == (o.dominated, o.retired)
    assert np.abs(r["path"] - o.path).max() < PATH_TOL and np.array_equal(r["actions"], o.actions)


def test_sparse_scene_forest_equals_sequential_seeded_plans():
    from ditreeonlineplanner_amd.car_env import CarEnv
    from ditreeonlineplanner_amd.planners.RRT import RRT_Planner, plan_scenario_runs
    sampler = Tape()
    kw = dict(batch=BATCH, capacity=1024, solution="anytime", sparse_cell=CELL, sparse_headings=HEADINGS)
    p0 = _planner(sampler, max_candidates=ROUNDS * BATCH, **kw)
    maze = load_maze("shapes")
    env = CarEnv(maze_map=maze, collision_checking=False)
    free = np.argwhere(maze == 0)
    rc_s = free[len(free) // 2]
    rc_g = next(rc for rc in free if 2 <= abs(rc[0] - rc_s[0]) + abs(rc[1] - rc_s[1]) <= 3)
    start = np.array([*env.cell_rowcol_to_xy(np.array(rc_s)), 0.0, 0.0, 0.0, 0.0])
    goal = np.array([*env.cell_rowcol_to_xy(np.array(rc_g)), 0, 0, 0, 0.0])
    p1 = RRT_Planner(start, goal, env_id="carmaze", environment=env, sampler=sampler, ctx=p0.ctx, action_horizon=8,
                     local_map_size=20, local_map_scale=0.2, global_map_scale=1.0, goal_conditioning_bias=0.85, prop_duration=[32],
                     time_budget=600, max_candidates=3 * BATCH, **kw)
    seeds = [[3, 5], [5]]
    runs = plan_scenario_runs([p0, p1], seeds, concurrent=2)
    check_runs_equal_sequential([p0, p1], seeds, runs)
    for pl, ss, rr in zip([p0, p1], seeds, runs):
        for s, r in zip(ss, rr):
            seeded_plan(pl, s)
            assert all(r[k] == pl.results[k] for k in KEYS), (s, [(r[k], pl.results[k]) for k in KEYS])
    o = sparse_run("anytime", CELL, headings=HEADINGS, seed=SEED, rounds=ROUNDS)
    assert runs[0][1]["number_of_nodes"] == len(o.cost) and runs[0][1]["dominated_candidates"] == o.dominated
    assert sum(r["dominated_candidates"] for r in runs[1]) > 0
    # a round-settings mismatch between the planners is refused like the others
    for other in (dict(sparse_cell=1.0), dict(sparse_headings=4), dict(sparse_cell=None, sparse_headings=None)):
        p2 = _planner(sampler, max_candidates=ROUNDS * BATCH, ctx=p0.ctx, **dict(kw, **other))
        with pytest.raises(ValueError, match="sparse_headings" if "sparse_cell" not in other else "sparse_cell"):
            plan_scenario_runs([p0, p2], seeds)
