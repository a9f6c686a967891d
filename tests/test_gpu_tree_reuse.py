"""GPU: ``RRT_Planner(reuse_tree=True)`` on action tapes (no network) -- plan once, drive the planner's own env along the plan,
put a wall across a later part of it, and ``reset(start_state=curr_state)``: the device tree must equal the restatement of
tests/tree_rebase_ref.py applied to the tree read back before the reset, every kept node's path must be the tail of its old
one, and the next round must be the round of an engine loaded with the restatement's arrays.

The scenario (a 10 x 10 room, (7, 2) -> (7, 5), edge length 16, batch 16, sample seed 11, action tape 1) was found on the CPU
oracle: its plan runs root -> two whole edges -> the goal edge through the cells (7, 2) (7, 3) (7, 4) (7, 5), and a wall in
(7, 4) cuts its last edge.  What must survive and go is asserted on the restatement, never on the device."""
import random

import numpy as np
import pytest
import torch

from oracle import geometry as G
from oracle.tapes import ActionTape
from tests import tree_rebase_ref as R
from tests.test_gpu_forest import _rng_states, _same_states, dev

pytestmark = pytest.mark.gpu

SEED, TAPE, BATCH, ROUNDS, A, EDGE = 11, 1, 16, 4, 8, 16
FIELDS = ("state", "xy", "parent", "last_action", "has_prev", "num_visit", "edge_states", "edge_actions", "edge_nstates",
          "edge_nactions")


def room():
    m = np.zeros((10, 10))
    m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = 1
    return m


def walled():
    m = room()
    m[7, 4] = 1
    return m


class Tape:
    def __init__(self, seed=TAPE):
        self.tape = ActionTape(seed)

    def sample_round(self, first, B, n_chunks, P):
        return np.stack([self.tape.actions(np.arange(first, first + B), j) for j in range(n_chunks)], axis=1)


def planner(**kw):
    from ditreeonlineplanner_amd.car_env import CarEnv
    from ditreeonlineplanner_amd.planners.RRT import RRT_Planner
    maze = room()
    env = CarEnv(maze_map=maze, collision_checking=False)
    start = np.array([*env.cell_rowcol_to_xy(np.array([7, 2])), 0.0, 0.0, 0.0, 0.0])
    goal = np.array([*env.cell_rowcol_to_xy(np.array([7, 5])), 0, 0, 0, 0.0])
    args = dict(env_id="carmaze", environment=env, sampler=Tape(), action_horizon=A, local_map_size=20, local_map_scale=0.2,
                global_map_scale=1.0, goal_conditioning_bias=0.85, prop_duration=[EDGE], time_budget=600, batch=BATCH,
                max_candidates=ROUNDS * BATCH, capacity=256, emulate_sticky_done=False, reuse_tree=True)
    args.update(kw)
    pl = RRT_Planner(start, goal, **args)
    pl.test_start, pl.test_goal = start, goal
    return pl


def seeded_plan(pl, seed=SEED):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    return pl.plan()


def read_tree(eng):
    """The engine's tree as host arrays over its n nodes, and its 8 counters."""
    t, n = eng.tree, eng.tree.n_nodes_host
    host = {name: getattr(t, name)[:n].cpu().numpy() for name in FIELDS}
    if t.cost is not None:
        host["cost"] = t.cost[:n].cpu().numpy()
    return host, t.counters.cpu().numpy().copy()


def drive(pl, actions, k):
    """k actions of the plan on the planner's own env, from the plan's start."""
    pl.env.reset(options=pl.options)
    pl.env.set_state(pl.test_start.copy())
    for a in actions[:k]:
        pl.env.step(np.asarray(a, dtype=np.float64))
    return np.asarray(pl.env.state, dtype=np.float64).copy()


def where_on_first_edge(chain, ns, na, k):
    """The car after k actions of the plan's first edge (whole chunks of A + 1 rows): the rebase arguments, worked out from k
    alone."""
    assert ns[1] == (EDGE // A) * (A + 1) and na[1] == EDGE and 0 < k <= EDGE
    if k == EDGE:
        return chain[1], 0, 0
    return chain[1], (k // A) * (A + 1) + k % A + 1, k


def as_paths(host):
    """A read-back tree in the shape tests.tree_rebase_ref.path_rows walks."""
    n = len(host["parent"])
    return dict(parent=host["parent"], state=host["state"], last_action=host["last_action"],
                edge_states=[host["edge_states"][m, :host["edge_nstates"][m]] for m in range(n)],
                edge_actions=[host["edge_actions"][m, :host["edge_nactions"][m]] for m in range(n)])


def restate(before, counters, maze, anchor, ds, da, car):
    want = R.rebase_ref(before, counters, maze, anchor, car if ds > 0 else None, ds, da)
    if ds == 0:                                          # the car's real state becomes the root, not the planned row
        want["state"][0], want["xy"][0] = car, car[:2]
    return want


def assert_tree_is(eng, want):
    got, cnt = read_tree(eng)
    assert np.array_equal(cnt, want["counters"]), (cnt, want["counters"])
    for name in ("state", "xy", "parent", "last_action", "has_prev", "num_visit", "edge_nstates", "edge_nactions", "cost"):
        if name in got:
            assert np.array_equal(got[name], want[name]), name
    for i in range(want["n"]):
        assert np.array_equal(got["edge_states"][i, :want["edge_nstates"][i]], want["edge_states"][i]), i
        assert np.array_equal(got["edge_actions"][i, :want["edge_nactions"][i]], want["edge_actions"][i]), i


def planned(pl):
    path, actions = seeded_plan(pl)
    mem = pl._remembered
    assert path is not None and pl._engine.goal_node == mem.chain[-1] and len(mem.chain) >= 4
    return path, actions, mem


@pytest.mark.parametrize("k", [3, A, EDGE], ids=["inside_a_chunk", "chunk_boundary", "at_a_node"])
@pytest.mark.parametrize("solution", ["first", "anytime"])
def test_reset_rebases_the_tree_at_the_car(solution, k):
    pl = planner(solution=solution)
    path, actions, mem = planned(pl)
    eng = pl._engine
    car = drive(pl, actions, k)
    before, counters = read_tree(eng)
    old = as_paths(before)
    anchor, ds, da = where_on_first_edge(mem.chain, mem.ns, mem.na, k)
    pl.update_maze(walled())
    want = restate(before, counters, walled(), anchor, ds, da, car)
    kept = [m for m in range(len(want["new_id"])) if want["new_id"][m] >= 0]
    # on the restatement: the anchor and more survive, the wall takes the end of the plan, and what is not below the car goes
    assert want["status"] == 0 and len(kept) >= 2 and anchor in kept
    assert want["new_id"][mem.chain[-1]] < 0 and len(kept) < len(R.descendants(before["parent"], counters[0], anchor)) < counters[0]
    pl.reset(start_state=car, goal_state=pl.test_goal)
    assert eng.tree.n_nodes_host == want["n"]
    assert_tree_is(eng, want)
    assert pl.results["reused_nodes"] == len(kept) and pl.results["dropped_nodes"] == counters[0] - len(kept)
    assert eng.goal_node is None                          # the goal node stood behind the wall
    # the suffix contract, for every kept node: the path is the old path's tail from the car's row on
    now, _ = read_tree(eng)
    new = as_paths(now)
    for m in kept:
        i = int(want["new_id"][m])
        rows, acts = R.path_rows(new, i)
        rows_old, acts_old = R.path_rows(old, m)
        assert np.array_equal(rows[0], car) and np.array_equal(rows[1:], rows_old[len(rows_old) - len(rows) + 1:])
        assert np.array_equal(acts, acts_old[len(acts_old) - len(acts):])
        if m == anchor:                                  # the car's row is the one the helper matched, k actions into the plan
            assert len(acts_old) - len(acts) == k and np.abs(rows_old[len(rows_old) - len(rows)][:4] - car[:4]).max() <= pl.reuse_tol
        p32, a32 = eng.path_to(i)
        assert np.array_equal(p32, rows.astype(np.float32)) and (a32 is None and not len(acts) or np.array_equal(a32, acts.astype(np.float32)))
        if "cost" in now:
            assert now["cost"][i] == len(p32)


def test_next_round_sees_the_rebased_tree_alone():
    """Two resets, so that the second one compacts into a tree that still holds the first plan's nodes in its later slots; then
    one round on it against the same round on an engine whose tree is the restatement's arrays and nothing else."""
    from ditreeonlineplanner_amd.engine import ExpansionEngine
    pl = planner()
    path, actions, mem = planned(pl)
    eng = pl._engine
    pl.reset(start_state=pl.test_start, goal_state=pl.test_goal)         # as online.plan_path leaves it; swaps the two trees
    car = drive(pl, actions, 3)
    before, counters = read_tree(eng)
    anchor, ds, da = where_on_first_edge(mem.chain, mem.ns, mem.na, 3)
    pl.update_maze(walled())
    want = restate(before, counters, walled(), anchor, ds, da, car)
    assert 2 <= want["n"] < counters[0]
    pl.reset(start_state=car, goal_state=pl.test_goal)
    n = want["n"]
    assert eng.tree.n_nodes_host == n and float(eng.tree.xy[n:counters[0]].abs().sum()) > 0     # stale slots behind the tree
    other = ExpansionEngine(pl.ctx, walled(), car, pl.test_goal, edge_length=EDGE, action_horizon=A, pred_horizon=eng.P,
                            local_map_size=eng.lm_n, local_map_scale=eng.lm_scale, s_global=eng.s_global, batch=BATCH,
                            capacity=256, emulate_sticky_done=False, early_exit=bool(eng.early_exit), goal_scale=eng.goal_scale,
                            prop_duration=[EDGE])
    other.env_goal = eng.env_goal.copy()
    t = other.tree
    for name in ("state", "xy", "parent", "last_action", "has_prev", "num_visit", "edge_nstates", "edge_nactions"):
        getattr(t, name)[:n].copy_(dev(want[name]).to(getattr(t, name).dtype))
    for i in range(n):
        t.edge_states[i, :want["edge_nstates"][i]].copy_(dev(want["edge_states"][i].reshape(-1, 6)))
        t.edge_actions[i, :want["edge_nactions"][i]].copy_(dev(want["edge_actions"][i].reshape(-1, 2)))
    t.counters.copy_(dev(want["counters"]).to(torch.int32))
    t.n_nodes_host = n
    rng = np.random.default_rng(5)
    s = np.zeros((BATCH, 6))
    s[:, 0], s[:, 1] = rng.uniform(-4, 4, BATCH), rng.uniform(-4, 4, BATCH)
    c = s[:, :2].copy()
    acts = dev(Tape().sample_round(1000, BATCH, EDGE // A, eng.P))
    rounds = []
    for e in (eng, other):
        cnt = e.expand_round(dev(s), dev(c), inject_actions=acts)
        rb, m = e.rb, int(cnt[0])
        rounds.append(dict(cnt=np.asarray(cnt).copy(), status=rb.status[:BATCH].cpu().numpy(), parent=rb.parent[:BATCH].cpu().numpy(),
                           node_id=rb.node_id[:BATCH].cpu().numpy(), tree=read_tree(e)[0]))
    a, b = rounds
    assert np.array_equal(a["cnt"], b["cnt"]) and a["cnt"][0] > n                # nodes were appended
    for name in ("status", "parent", "node_id"):
        assert np.array_equal(a[name], b[name]), name
    assert (a["parent"] < n).all()
    for name in FIELDS:
        x, y = a["tree"][name], b["tree"][name]
        if name in ("edge_states", "edge_actions"):
            counts = a["tree"]["edge_nstates" if name == "edge_states" else "edge_nactions"]
            assert all(np.array_equal(x[i, :counts[i]], y[i, :counts[i]]) for i in range(len(x))), name
        else:
            assert np.array_equal(x, y), name


def test_kept_goal_node_is_returned_at_once():
    pl = planner()
    path, actions, mem = planned(pl)
    k = 3
    car = drive(pl, actions, k)
    n_before = pl._engine.tree.n_nodes_host
    pl.reset(start_state=car, goal_state=pl.test_goal)                   # the maze is as it was
    assert 0 < pl.results["reused_nodes"] < n_before and pl._engine.goal_node is not None
    rng = _rng_states()
    p2, a2 = pl.plan()
    assert _same_states(rng, _rng_states())
    assert pl.results["iterations"] == 0 and pl.results["number_of_nodes"] == pl.results["reused_nodes"] + 1
    r = (k // A) * (A + 1) + k % A                                       # the car's row of the first edge; the root is row 0
    assert np.array_equal(p2[0], car.astype(np.float32)) and np.array_equal(p2[1:], path[1 + r + 1:])
    assert np.array_equal(a2, actions[k:]) and pl.results["path_time"] == len(p2) * pl.env_dt


def test_second_rebase_inside_the_same_edge():
    """Two re-plans while the car is still on the plan's first edge: the second reset finds the car on an edge whose front
    rows the first one took off, and still counts its actions right."""
    pl = planner()
    path, actions, mem = planned(pl)
    eng = pl._engine
    car = drive(pl, actions, 3)
    pl.reset(start_state=car, goal_state=pl.test_goal)
    p2, a2 = pl.plan()
    assert np.array_equal(a2, actions[3:])
    pl.test_start = car
    car2 = drive(pl, a2, 2)
    before, counters = read_tree(eng)
    want = restate(before, counters, room(), 1, 2, 2, car2)              # row 1 of what is left of the edge, 2 more actions
    assert want["status"] == 0 and want["n"] == counters[0] > 2           # nothing is blocked: only the old root goes
    pl.reset(start_state=car2, goal_state=pl.test_goal)
    assert pl.results["reused_nodes"] == counters[0] - 1 and pl.results["dropped_nodes"] == 1
    assert_tree_is(eng, want)
    p3, a3 = pl.plan()
    assert pl.results["iterations"] == 0 and np.array_equal(a3, actions[5:])
    assert np.array_equal(p3[0], car2.astype(np.float32)) and np.array_equal(p3[1:], path[1 + 5 + 1:])


def test_plan_path_leaves_the_tree_as_planned():
    from ditreeonlineplanner_amd.online import plan_path
    pl = planner()
    random.seed(SEED)
    np.random.seed(SEED)
    torch.manual_seed(SEED)
    pl.reset(start_state=pl.test_start, goal_state=pl.test_goal)
    path, actions = pl.plan()
    before, counters = read_tree(pl._engine)
    pl.reset(start_state=pl.test_start, goal_state=pl.test_goal)
    after, counters2 = read_tree(pl._engine)
    assert counters[0] > 20 and pl.results["reused_nodes"] == counters[0] and pl.results["dropped_nodes"] == 0
    assert list(counters2) == [counters[0], counters[1], 0, 0, 0, 0, 0, -1] and counters[1] >= 0
    for name in FIELDS:
        assert np.array_equal(before[name], after[name]), name
    # and through the driver's own function, from a fresh planner
    pl2 = planner()
    random.seed(SEED)
    np.random.seed(SEED)
    torch.manual_seed(SEED)
    stats = {"iterations": 0}
    p2, a2 = plan_path(pl2, pl2.test_start, pl2.test_goal, stats)
    again, counters3 = read_tree(pl2._engine)
    assert np.array_equal(p2, path) and np.array_equal(a2, actions) and list(counters3) == list(counters2)
    for name in FIELDS:
        assert np.array_equal(before[name], again[name]), name


def test_off_the_plan_or_another_goal_is_a_fresh_tree():
    pl = planner()
    path, actions, mem = planned(pl)
    car = drive(pl, actions, 3)
    off = car.copy()
    off[0] += 10 * pl.reuse_tol
    pl.reset(start_state=off, goal_state=pl.test_goal)
    assert pl._engine.tree.n_nodes_host == 1 and pl.results["reused_nodes"] == 0 and pl.results["dropped_nodes"] == 0
    assert np.array_equal(pl._engine.tree.state[0].cpu().numpy(), off) and pl._remembered is None
    pl = planner()
    path, actions, mem = planned(pl)
    goal2 = pl.test_goal.copy()
    goal2[1] += 1.0
    pl.reset(start_state=drive(pl, actions, 3), goal_state=goal2)
    assert pl._engine.tree.n_nodes_host == 1 and pl.results["reused_nodes"] == 0
    assert int(pl._engine.tree.counters[1].item()) == -1


def test_anytime_keeps_the_incumbent_and_replaces_it_by_a_cheaper_one():
    pl = planner(solution="anytime", max_candidates=8 * BATCH)
    path, actions, mem = planned(pl)
    eng = pl._engine
    k = 3
    car = drive(pl, actions, k)
    before, counters = read_tree(eng)
    anchor, ds, da = where_on_first_edge(mem.chain, mem.ns, mem.na, k)
    want = restate(before, counters, room(), anchor, ds, da, car)
    g = int(want["counters"][1])
    assert g >= 0 and want["cost"][g] == before["cost"][counters[1]] - (ds - 1) - 1 == len(path) - (ds - 1) - 1
    pl.reset(start_state=car, goal_state=pl.test_goal)
    assert_tree_is(eng, want)
    assert eng.goal_node == g and int(eng.tree.cost[g].item()) == want["cost"][g]
    # make the kept incumbent dearer than any path this room admits: the first goal node of the next rounds must replace it
    eng.tree.cost[g] = 10 ** 6
    p2, a2 = seeded_plan(pl, SEED + 1)
    g2 = eng.goal_node
    assert pl.results["iterations"] > 0 and pl.results["solutions"] >= 1 and pl.results["first_solution_candidates"] == 0
    assert g2 != g and g2 >= want["n"] and len(p2) == int(eng.tree.cost[g2].item()) < 10 ** 6


def test_default_resets_to_one_node():
    pl = planner(reuse_tree=False)
    random.seed(SEED)
    np.random.seed(SEED)
    torch.manual_seed(SEED)
    path, actions = pl.plan()
    assert path is not None and pl._engine.tree.n_nodes_host > 20 and pl._remembered is None
    car = drive(pl, actions, 3)
    pl.reset(start_state=car, goal_state=pl.test_goal)
    assert pl._engine.tree.n_nodes_host == 1 and "reused_nodes" not in pl.results
    assert getattr(pl._engine, "_spare_tree", None) is None
