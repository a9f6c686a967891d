"""GPU: ditree_accept_best / ditree_forest_accept_best (accept_scan_kernel<best>, accept_commit_kernel's cost column and
accept_pick_kernel) against the sequential restatement of tests/accept_best_ref.py, on rounds written straight into the device
arrays: round sizes around the wave (63 / 64 / 65), around the scan's 1024-wide pass (1024 / 1025) and past two passes
(2500); forests of 1, 3 and 64 trees with empty candidate ranges.  Every comparison is exact: node ids, whole counter rows,
the cost column, num_visit and every tree array.  Then the invariant the planner relies on -- a node's cost is the number of
rows of its path -- on an engine grown by four tape rounds."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import geometry as G
from oracle import rrt as ORRT
from oracle.tapes import ActionTape
from tests.accept_best_ref import COLLIDED, GAC, GOAL, OK, SolutionOracle, accept_best_ref
from tests.test_gpu_forest import ctx, dev, scenario  # noqa: F401
from tests.util import load_maze

pytestmark = pytest.mark.gpu

I32 = torch.int32
TREE_FIELDS = ("state", "xy", "parent", "last_action", "has_prev", "num_visit", "edge_states", "edge_actions", "edge_nstates",
               "edge_nactions", "cost")
CAP = 2700                                   # single tree: room for the 2500-candidate round
SIZES = [1, 63, 64, 65, 1024, 1025, 2500]
CASES = ["no_goal", "one_goal", "distinct_costs", "equal_costs", "incumbent_better", "incumbent_equal", "incumbent_worse",
         "goal_past_capacity", "goal_at_collision", "all_collided"]


@pytest.fixture(scope="module")
def single(ctx):
    from ditreeonlineplanner_amd.engine import ExpansionEngine
    maze, start, goal = scenario()
    return ExpansionEngine(ctx, maze, start, goal, edge_length=16, action_horizon=8, batch=2500, capacity=CAP,
                           emulate_sticky_done=False, solution="anytime")


@pytest.fixture(scope="module")
def plain(ctx):
    """The same tree shape under the default mode: ditree_accept's side of the comparison (and no cost column)."""
    from ditreeonlineplanner_amd.engine import ExpansionEngine
    maze, start, goal = scenario()
    return ExpansionEngine(ctx, maze, start, goal, edge_length=16, action_horizon=8, batch=2500, capacity=CAP,
                           emulate_sticky_done=False)


def random_tree_state(rng, N, rows):
    """Every array of an N-slot tree filled with random values (an untouched slot is recognisable); ``rows`` counter rows
    with random iteration / candidate counts and values in [2] and [5] that the call must leave alone."""
    host = dict(state=rng.uniform(1, 2, (N, 6)), parent=rng.integers(-1, N, N).astype(np.int32),
                last_action=rng.uniform(1, 2, (N, 2)), has_prev=rng.integers(0, 2, N).astype(np.uint8),
                num_visit=rng.integers(0, 6, N).astype(np.int32), edge_states=rng.uniform(1, 2, (N, 18, 6)),
                edge_actions=rng.uniform(1, 2, (N, 16, 2)), edge_nstates=rng.integers(0, 19, N).astype(np.int32),
                edge_nactions=rng.integers(0, 17, N).astype(np.int32), cost=rng.integers(1, 400, N).astype(np.int32))
    host["xy"] = host["state"][:, :2].copy()
    cnt = np.zeros((rows, 8), dtype=np.int32)
    cnt[:, 1], cnt[:, 7] = -1, 5
    cnt[:, 2], cnt[:, 5] = rng.integers(0, 9, rows), rng.integers(0, 9, rows)
    cnt[:, 3], cnt[:, 4] = rng.integers(0, 50, rows), rng.integers(0, 50, rows)
    host["counters"] = cnt
    return host


def random_rows(rng, B, status, parent_lo, parent_n):
    """B candidate rows: the given statuses, parents among nodes [parent_lo, parent_lo + parent_n) (few nodes, many candidates:
    repeats), 1 or 2 chunks run, random state / action rows with a tenth of them all zero."""
    rnd = dict(status=np.asarray(status, dtype=np.int32), parent=(parent_lo + rng.integers(0, parent_n, B)).astype(np.int32),
               chunks_run=rng.integers(1, 3, B).astype(np.int32), end_state=rng.uniform(1, 2, (B, 6)),
               states=rng.uniform(1, 2, (B, 2, 9, 6)), actions=rng.uniform(1, 2, (B, 2, 8, 2)), node_id=np.full(B, -7, np.int32))
    rnd["states"][rng.random((B, 2, 9)) < 0.1] = 0.0
    rnd["actions"][rng.random((B, 2, 8)) < 0.1] = 0.0
    return rnd


def edge_rows_kept(rnd, b):
    run = int(rnd["chunks_run"][b])
    return int((~(rnd["states"][b, :run].reshape(-1, 6) == 0).all(axis=1)).sum())


def upload_round(rb, rnd, B):
    for name in ("status", "parent", "chunks_run", "end_state", "states", "actions", "node_id"):
        getattr(rb, name)[:B].copy_(dev(rnd[name]))


def upload_tree(tree, host, counters):
    for name in TREE_FIELDS:
        if getattr(tree, name, None) is not None:
            getattr(tree, name).copy_(dev(host[name]))
    counters.copy_(dev(host["counters"]).reshape(counters.shape))


def compare_tree(tree, counters, rb, host, rnd, B, fields=TREE_FIELDS):
    got = counters.cpu().numpy().reshape(host["counters"].shape)
    assert np.array_equal(got, host["counters"]), (got, host["counters"])
    nid = rb.node_id[:B].cpu().numpy()
    assert np.array_equal(nid, rnd["node_id"]), np.nonzero(nid != rnd["node_id"])[0][:10]
    for name in fields:
        a = getattr(tree, name).cpu().numpy()
        assert np.array_equal(a, host[name]), (name, np.nonzero((a != host[name]).reshape(len(a), -1).any(axis=1))[0][:10])


def accept_best(ctx, eng, B, cost="own"):
    from ditreeonlineplanner_amd import _lib
    eng.ensure_maze()
    rd = eng.rb.desc(0, B)
    cp = eng.tree.cost.data_ptr() if cost == "own" else cost
    return _lib.lib().ditree_accept_best(ctx._h, C.byref(eng.tree.desc), C.byref(rd), cp, ctx.stream)


def build_case(case, B, rng):
    """-> (host, rnd, n0).  The goal rows, their parents' costs, the incumbent and the fill of the tree are set so that the
    restatement goes through the case; the test asserts that on the restatement's output."""
    host = random_tree_state(rng, CAP, 1)
    n0 = 40
    status = np.where(rng.random(B) < 0.3, COLLIDED, OK)
    status[rng.random(B) < 0.05] = COLLIDED | GAC
    goals = []
    if case == "one_goal":
        goals = [B // 2]
    elif case in ("distinct_costs", "equal_costs", "incumbent_better", "incumbent_equal", "incumbent_worse"):
        goals = sorted(set([B // 3, B // 2, B - 1, min(B - 1, 1023), min(B - 1, 1024)]))
    elif case == "goal_past_capacity":
        goals = [B - 1]
    elif case == "goal_at_collision":
        status[[0, B // 2, B - 1]] = COLLIDED | GAC
    elif case == "all_collided":
        status[:] = COLLIDED
        status[B // 2] = COLLIDED | GAC
    status[goals] = GOAL
    rnd = random_rows(rng, B, status, 0, n0)
    if case == "equal_costs":                                        # the same parent cost, chunks and kept rows for every goal
        for b in goals:
            rnd["chunks_run"][b] = 2
            rnd["states"][b] = rng.uniform(1, 2, (2, 9, 6))
            host["cost"][rnd["parent"][b]] = 77
    if case == "distinct_costs":                                     # the cheapest is neither the first nor the last goal
        for k, b in enumerate(goals):                                 # one parent each, 40 apart: an edge keeps 18 rows at most
            rnd["parent"][b] = k
            host["cost"][k] = 300 - 40 * k if k < len(goals) - 1 else 290
    if case.startswith("incumbent_"):
        for k, b in enumerate(goals):
            rnd["parent"][b] = k
        best = min(int(host["cost"][rnd["parent"][b]]) + edge_rows_kept(rnd, b) + 1 for b in goals)
        inc = n0 - 1                                                  # an existing node that is nobody's parent among the goals
        host["cost"][inc] = best + {"incumbent_better": -1, "incumbent_equal": 0, "incumbent_worse": 1}[case]
        host["counters"][0, 1] = inc
    if case == "goal_past_capacity":                                 # the tree fills up one node before the goal row's turn
        n0 = CAP - int((status[:B - 1] & 0xff != COLLIDED).sum())
        rnd["parent"] = rng.integers(0, n0, B).astype(np.int32)
    host["counters"][0, 0] = n0
    return host, rnd, goals


@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("case", CASES)
def test_accept_best_against_the_sequential_restatement(ctx, single, case, B):
    rng = np.random.default_rng(1000 * CASES.index(case) + B)
    host, rnd, goals = build_case(case, B, rng)
    before = host["counters"][0].copy()
    cost_before = host["cost"].copy()
    upload_tree(single.tree, host, single.tree.counters)
    upload_round(single.rb, rnd, B)
    assert accept_best(ctx, single, B) == 0
    accept_best_ref(host, rnd, host["counters"][0], 0, B, 0, CAP)
    compare_tree(single.tree, single.tree.counters, single.rb, host, rnd, B)
    check_case(case, B, host, rnd, goals, before, cost_before)


def check_case(case, B, host, rnd, goals, before, cost_before):
    """The restatement itself went through the case (a condition on the test's inputs, not on the device)."""
    cnt, nid = host["counters"][0], rnd["node_id"]
    accepted = int((rnd["status"] & 0xff != COLLIDED).sum())
    assert cnt[2] == before[2] and cnt[5] == before[5] and cnt[7] == -1
    assert cnt[4] - before[4] == B and cnt[3] - before[3] == rnd["chunks_run"].sum()
    goal_cost = {b: int(host["cost"][nid[b]]) for b in goals if nid[b] >= 0}
    if case in ("no_goal", "goal_at_collision", "all_collided"):
        assert cnt[1] == -1 and cnt[0] == before[0] + accepted and (accepted == 0 or case != "all_collided")
    elif case == "one_goal":
        assert cnt[1] == nid[goals[0]] >= 0
    elif case == "distinct_costs":
        assert len(set(goal_cost.values())) == len(goals)
        best = min(goal_cost, key=goal_cost.get)
        assert cnt[1] == nid[best] and (len(goals) < 3 or goals[0] < best < goals[-1])
    elif case == "equal_costs":
        assert len(set(goal_cost.values())) == 1 and cnt[1] == nid[goals[0]]
    elif case in ("incumbent_better", "incumbent_equal"):
        assert cnt[1] == before[1] and min(goal_cost.values()) - cost_before[before[1]] == (case == "incumbent_better")
    elif case == "incumbent_worse":
        best = min(goal_cost, key=lambda b: (goal_cost[b], b))
        assert cnt[1] == nid[best] != before[1] and goal_cost[best] == cost_before[before[1]] - 1
    elif case == "goal_past_capacity":
        assert cnt[0] == CAP and cnt[6] == 1 and nid[B - 1] == -1 and cnt[1] == -1 and not goal_cost


@pytest.mark.parametrize("B", SIZES)
def test_without_goals_the_tree_is_ditree_accepts(ctx, single, plain, B):
    """A round whose goal statuses are taken out: scan and commit leave what ditree_accept with emulate_sticky = 0 leaves --
    node ids, every tree array, and the counters the two scans share."""
    from ditreeonlineplanner_amd import _lib
    rng = np.random.default_rng(50 + B)
    host = random_tree_state(rng, CAP, 1)
    host["counters"][0, 0] = 30
    status = rng.choice([OK, GOAL, COLLIDED, COLLIDED | GAC], B, p=[0.5, 0.1, 0.3, 0.1])
    status[status == GOAL] = OK
    rnd = random_rows(rng, B, status, 0, 30)
    assert plain.tree.cost is None and plain.solution == "first"
    for eng in (single, plain):
        upload_tree(eng.tree, host, eng.tree.counters)
        upload_round(eng.rb, rnd, B)
    assert accept_best(ctx, single, B) == 0
    rd = plain.rb.desc(0, B)
    _lib.check(ctx._h, _lib.lib().ditree_accept(ctx._h, C.byref(plain.tree.desc), C.byref(rd), 0, ctx.stream), "accept")
    assert torch.equal(single.rb.node_id[:B], plain.rb.node_id[:B])
    for name in TREE_FIELDS[:-1]:
        assert torch.equal(getattr(single.tree, name), getattr(plain.tree, name)), name
    a, b = single.tree.counters.cpu().numpy(), plain.tree.counters.cpu().numpy()
    assert np.array_equal(a[[0, 1, 3, 4, 6]], b[[0, 1, 3, 4, 6]]) and a[7] == -1


# ---------------------------------------------------------------------- forests
FORESTS = {1: (1, 200, [70]), 3: (3, 1200, [0, 1100, 0]),
           64: (64, 40, [0, 0, 5, 30, 1, 0, 0, 17] + [(7 * t) % 23 for t in range(8, 63)] + [0])}


@pytest.mark.parametrize("T", list(FORESTS))
def test_forest_accept_best_against_the_sequential_restatement(ctx, T):
    """Two rounds on one forest: every tree's range through the restatement, all trees in one call.  Empty ranges first, last
    and adjacent (their trees untouched), trees with an incumbent that is cheaper or dearer than the round's best goal, and a
    tree that runs out of slots; the second round meets the incumbents the first one left."""
    from ditreeonlineplanner_amd import _lib
    from ditreeonlineplanner_amd.forest import ForestEngine
    T, Cap, counts = FORESTS[T]
    maze, start, goal = scenario()
    forest = ForestEngine(ctx, maze, start, goal, T, Cap, edge_length=16, action_horizon=8, batch=sum(counts),
                          emulate_sticky_done=False, solution="anytime")
    rng = np.random.default_rng(7 + T)
    host = random_tree_state(rng, T * Cap, T)
    n0 = rng.integers(1, 6, T)
    full = T - 2 if T > 1 else 0                                      # this tree has three free slots
    n0[full] = Cap - 3
    host["counters"][:, 0] = n0
    for t in range(0, T, 2):                # an incumbent: cost 1 (no goal beats it) or 399 (any goal does: 299 + 18 + 1 at most)
        inc = t * Cap + int(rng.integers(0, n0[t]))
        host["counters"][t, 1] = inc
        host["cost"][t * Cap: t * Cap + n0[t]] = rng.integers(2, 300, n0[t])
        host["cost"][inc] = 1 if t % 4 == 0 else 399
    upload_tree(forest.tree, host, forest.fcounters)
    replaced = kept = 0
    for rounds in range(2):
        off = np.concatenate([[0], np.cumsum(counts)])
        B = int(off[-1])
        status = rng.choice([OK, GOAL, COLLIDED, COLLIDED | GAC], B, p=[0.5, 0.12, 0.3, 0.08])
        rnd = random_rows(rng, B, status, 0, 1)
        for t in range(T):
            rnd["parent"][off[t]:off[t + 1]] = t * Cap + rng.integers(0, host["counters"][t, 0], counts[t])
        upload_round(forest.rb, rnd, B)
        forest._set_offsets(counts)
        forest.ensure_maze()
        rd = forest.rb.desc(0, B)
        before = host["counters"].copy()
        _lib.check(ctx._h, _lib.lib().ditree_forest_accept_best(ctx._h, C.byref(forest.tree.desc), C.byref(forest.fdesc), C.byref(rd),
                                                                forest.tree.cost.data_ptr(), ctx.stream), "forest_accept_best")
        for t in range(T):
            accept_best_ref(host, rnd, host["counters"][t], int(off[t]), int(off[t + 1]), t * Cap, Cap)
        compare_tree(forest.tree, forest.fcounters, forest.rb, host, rnd, B)
        cnt = host["counters"]
        empty = [t for t in range(T) if counts[t] == 0]
        assert np.array_equal(cnt[empty], before[empty])
        for t in range(T):
            has_goal = ((rnd["status"][off[t]:off[t + 1]] & 0xff == GOAL) & (rnd["node_id"][off[t]:off[t + 1]] >= 0)).any()
            if before[t, 1] >= 0 and has_goal:
                replaced += int(cnt[t, 1] != before[t, 1])
                kept += int(cnt[t, 1] == before[t, 1])
            assert cnt[t, 1] < 0 or t * Cap <= cnt[t, 1] < t * Cap + cnt[t, 0]
        if counts[full] > 3:
            assert cnt[full, 0] == Cap and cnt[full, 6] == 1
        counts = {1: [65], 3: [40, 0, 30], 64: counts[::-1]}[T]       # the second round: other ranges are empty
    if T == 64:
        assert replaced >= 1 and kept >= 1, (replaced, kept)


def test_accept_best_refuses_by_name_without_launching(ctx, single):
    """No cost array, or a sharded round: DITREE_E_ARG with the message, node ids and counters untouched -- both entry points."""
    from ditreeonlineplanner_amd import _lib
    from ditreeonlineplanner_amd.forest import ForestEngine
    maze, start, goal = scenario()
    forest = ForestEngine(ctx, maze, start, goal, 2, 16, edge_length=16, action_horizon=8, batch=8, emulate_sticky_done=False,
                          solution="best_of_round")
    forest._set_offsets([3, 1])
    h, L = ctx._h, _lib.lib()
    for eng, counters in ((single, single.tree.counters), (forest, forest.fcounters)):
        eng.tree.reset(eng.start_state)
        eng.rb.node_id.fill_(-7)
        eng.rb.parent.zero_()
        eng.rb.status.fill_(GOAL)
        cnt = counters.clone()
        for cost, shard, msg in ((None, 0, b"accept_best: cost array missing"),
                                 (eng.tree.cost.data_ptr(), 2, b"accept_best: one rank (round->shard must be 0)")):
            rd = eng.rb.desc(0, 4)
            rd.shard = shard
            if eng is single:
                rc = L.ditree_accept_best(h, C.byref(eng.tree.desc), C.byref(rd), cost, ctx.stream)
            else:
                rc = L.ditree_forest_accept_best(h, C.byref(eng.tree.desc), C.byref(eng.fdesc), C.byref(rd), cost, ctx.stream)
            assert rc == -1 and L.ditree_last_error(h) == msg, L.ditree_last_error(h)
        torch.cuda.synchronize()
        assert (eng.rb.node_id == -7).all() and torch.equal(counters, cnt)


# ---------------------------------------------------------------------- cost == rows of the path
class ZeroRowTape(ActionTape):
    """The action tape with step 3 of every chunk of every fifth candidate zeroed: an action row the accept filters while the
    state row behind it stays."""

    def actions(self, cand_idx, chunk):
        a = super().actions(cand_idx, chunk)
        a[np.asarray(cand_idx) % 5 == 2, 3] = 0.0
        return a


def test_cost_is_the_number_of_rows_of_the_path(ctx):
    """Four tape rounds of 64 candidates at edge length 16: for every node len(path_to(n)[0]) == cost[n], and the tree is the
    restatement's.  The rounds hold both kinds of edge whose stored rows are fewer than the rows that ran."""
    from ditreeonlineplanner_amd.engine import ExpansionEngine
    maze = load_maze("boxes")
    start = np.array([*G.cell_rowcol_to_xy([18, 13], maze), 0.0, 0, 0, 0])
    goal = np.array([*G.cell_rowcol_to_xy([18, 15], maze), 0, 0, 0, 0])
    tape = ZeroRowTape(7)
    eng = ExpansionEngine(ctx, maze, start, goal, edge_length=16, action_horizon=8, batch=64, capacity=512,
                          emulate_sticky_done=False, solution="anytime")
    so = SolutionOracle(ORRT.OraclePlanner(maze, start, goal, tape.sampler(), edge_length=16, emulate_sticky_done=False), "anytime")
    rt = ORRT.RandomTape(0)
    for k in range(4):
        s, c = rt.draw_round(64, maze.shape[1], maze.shape[0], goal)
        acts = np.stack([tape.actions(np.arange(64 * k, 64 * k + 64), j) for j in range(2)], axis=1)
        ref = so.round(s, c)
        cnt = eng.expand_round(dev(s), dev(c), inject_actions=dev(acts))
        assert np.array_equal(eng.rb.node_id[:64].cpu().numpy(), ref["node_id"])
        assert eng.goal_node == so.incumbent and int(cnt[1]) == (-1 if so.incumbent is None else so.incumbent)
    # on the restatement: a goal in mid-chunk (the rows behind it are zero and filtered) and a filtered all-zero action row
    mid = zero_action = 0
    for r in so.rounds:
        for b in np.nonzero(r["node_id"] >= 0)[0]:
            run = int(r["chunks_run"][b])
            if r["status"][b] == G.STATUS_GOAL and r["chunk_steps"][b, run - 1] < 8:
                mid += 1
                assert (r["states"][b, run - 1, r["chunk_steps"][b, run - 1] + 1:] == 0).all()
            zero_action += int(((r["actions"][b, :run] == 0).all(axis=2) & ~(r["states"][b, :run, 1:] == 0).all(axis=2)).any())
    assert mid >= 1 and zero_action >= 1, (mid, zero_action)
    n = eng.tree.n_nodes_host
    cost = eng.tree.cost[:n].cpu().numpy()
    assert n == len(so.pl.tree) and np.array_equal(cost, so.cost)
    assert np.array_equal(eng.tree.parent[:n].cpu().numpy(), so.pl.tree.parents)
    for node in range(n):
        assert len(eng.path_to(node)[0]) == cost[node] == len(so.pl.path_to(node)[0]), node
