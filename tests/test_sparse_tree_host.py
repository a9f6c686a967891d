"""CPU: the planner's ``sparse_cell`` (include/ditree.h "sparse tree").  The restatement of tests/sparse_tree_ref.py is held against
its own invariant -- after every round the incrementally kept active flags and table equal ``active_ref`` from scratch -- on
random synthetic rounds and on the restated planner, against the one-at-a-time SST rule at batch 1, and on designed cases (goal
candidates, ties, cell edges).  Then what reaches the library from the engines, the refusals by name, and the preconditions of
the GPU plan test."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from ditreeonlineplanner_amd import _lib
from ditreeonlineplanner_amd import engine as E
from ditreeonlineplanner_amd.planners import RRT as F
from tests import sparse_tree_ref as SR
from tests.sparse_tree_ref import COLLIDED, EMPTY, GOAL, OK, TWO_PI, active_ref, cell_ref, grid_ref, sparse_accept_ref
from tests.test_engine_dispatch_host import B, CAP, COUNTS, KINDS, StubContext, make_engine, rec, round_inputs  # noqa: F401
from tests.test_solution_modes_host import _AntEnv, _car_args
from tests.util import REPO

NEW_CALLS = ["ditree_sparse_rebuild", "ditree_accept_sparse", "ditree_forest_accept_sparse", "ditree_nn_argmin_sparse",
             "ditree_forest_nn_argmin_sparse", "ditree_chunk_budget_sparse", "ditree_expand_round_sparse",
             "ditree_forest_expand_round_sparse"]


def test_sparse_symbols_declared_bound_and_exported():
    hdr = open(os.path.join(REPO, "include", "ditree.h")).read()
    for name in NEW_CALLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name), name
    assert _lib.lib().ditree_version() == 400


def test_sparse_descriptor_layout_matches_the_header():
    hdr = open(os.path.join(REPO, "include", "ditree.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} ditree_sparse;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(?:const\s+)?(int32_t|double|uint64_t|uint8_t)\s*(\*?)\s*(\w+);", body)
    assert [f[2] for f in fields] == [n for n, _ in _lib.Sparse._fields_]
    for (typ, star, name), (_, ctype) in zip(fields, _lib.Sparse._fields_):
        want = (C.POINTER(C.c_int32) if name == "dims_host" else C.c_void_p) if star else {"double": C.c_double, "int32_t": C.c_int32}[typ]
        assert ctype is want, name
    assert C.sizeof(_lib.Sparse) == 2 * 8 + 2 * 4 + 8 * 8


# ---------------------------------------------------------------------- the cell function
GRID = grid_ref(4, 3, 1.0, 0.5, 4)                        # 3 m x 4 m, 6 x 8 x 4 cells, w = pi / 2


def cell_of(x, y, psi, grid=GRID):
    return int(cell_ref(grid, np.array([[x, y, psi, 0, 0, 0.0]]))[0])


def parts(c, grid=GRID):
    return (c // grid["nh"]) % grid["nx"], c // (grid["nh"] * grid["nx"]), c % grid["nh"]       # ix, iy, ih


def test_cell_edges():
    g = GRID
    assert (g["nx"], g["ny"], g["cells"]) == (6, 8, 192) and g["w"] == TWO_PI / 4
    # x = -W/2 is the first cell, x = +W/2 would be cell nx and is clamped into the last; past the map either way
    assert parts(cell_of(-1.5, 0.0, 0.0))[0] == 0 and parts(cell_of(1.5, 0.0, 0.0))[0] == 5
    assert parts(cell_of(-99.0, 0.0, 0.0))[0] == 0 and parts(cell_of(1e300, 0.0, 0.0))[0] == 5
    assert parts(cell_of(0.0, -2.0, 0.0))[1] == 0 and parts(cell_of(0.0, 2.0, 0.0))[1] == 7
    assert parts(cell_of(np.nextafter(-1.0, -2.0), 0.0, 0.0))[0] == 0 and parts(cell_of(-1.0, 0.0, 0.0))[0] == 1
    # headings: negative and above 2 pi wrap; exact bin borders belong to the bin that starts there
    w = g["w"]
    for psi, ih in ((0.0, 0), (w, 1), (-w, 3), (TWO_PI, 0), (2 * TWO_PI, 0), (-TWO_PI, 0), (np.nextafter(w, 0.0), 0), (-1e-300, 3),
                    (7.0, 0), (-7.0, 3), (3 * w, 3), (TWO_PI + w, 1)):
        assert parts(cell_of(0.0, 0.0, psi))[2] == ih, psi
    # -1e-300 wraps to exactly 2 pi, whose bin would be nh: clamped into the last
    assert (-1e-300) - TWO_PI * math.floor(-1e-300 / TWO_PI) == TWO_PI
    for bad in (np.nan, np.inf, -np.inf):
        assert cell_of(bad, 0.0, 0.0) == cell_of(0.0, bad, 0.0) == cell_of(0.0, 0.0, bad) == -1
    # one heading bin: every finite heading is bin 0
    g1 = grid_ref(4, 3, 1.0, 0.5, 1)
    assert all(parts(cell_of(0.3, 0.3, p, g1), g1)[2] == 0 for p in (-7.0, 0.0, 3.0, TWO_PI, 100.0))
    # a cell that does not divide the map: the last column is narrower, never out of range
    g2 = grid_ref(4, 3, 1.0, 0.7, 2)
    assert (g2["nx"], g2["ny"]) == (5, 6) and parts(cell_of(1.49, 1.99, 0.0, g2), g2)[:2] == (4, 5)


def test_active_ref_is_the_lexicographic_minimum_per_cell():
    st = np.zeros((6, 6))
    st[:, :3] = [[0.1, 0.1, 0.1], [0.2, 0.2, 0.2], [0.3, 0.3, 0.3], [1.2, 0.1, 0.1], [np.nan, 0, 0], [0.15, 0.15, 0.15]]
    act, table = active_ref(st, [5, 3, 3, 9, 1, 2], GRID, base=100)
    assert act.tolist() == [0, 0, 0, 1, 0, 1]                          # the NaN node has no cell and is never active
    c = cell_of(0.1, 0.1, 0.1)
    assert table[c] == SR.table_key(2, 105) and (table != EMPTY).sum() == 2
    act, _ = active_ref(st[:3], [3, 3, 3], GRID)
    assert act.tolist() == [1, 0, 0]                                   # equal costs: the lower id


# ---------------------------------------------------------------------- the accept on host arrays
def host_arrays(rng, N):
    host = dict(state=rng.uniform(1, 2, (N, 6)), parent=rng.integers(-1, N, N).astype(np.int32),
                last_action=rng.uniform(1, 2, (N, 2)), has_prev=rng.integers(0, 2, N).astype(np.uint8),
                num_visit=rng.integers(0, 6, N).astype(np.int32), edge_states=rng.uniform(1, 2, (N, 18, 6)),
                edge_actions=rng.uniform(1, 2, (N, 16, 2)), edge_nstates=rng.integers(0, 19, N).astype(np.int32),
                edge_nactions=rng.integers(0, 17, N).astype(np.int32), cost=rng.integers(1, 400, N).astype(np.int32),
                active=rng.integers(0, 2, N).astype(np.uint8), key=rng.integers(1, 400, N).astype(np.int32))
    host["xy"] = host["state"][:, :2].copy()
    return host


def rows(rng, Bn, status, n_nodes, grid):
    rnd = dict(status=np.asarray(status, dtype=np.int32), parent=rng.integers(0, n_nodes, Bn).astype(np.int32),
               chunks_run=rng.integers(1, 3, Bn).astype(np.int32), end_state=SR.synthetic_states(rng, Bn, grid),
               states=rng.uniform(1, 2, (Bn, 2, 9, 6)), actions=rng.uniform(1, 2, (Bn, 2, 8, 2)), node_id=np.full(Bn, -7, np.int32))
    rnd["states"][rng.random((Bn, 2, 9)) < 0.1] = 0.0
    return rnd


def counters(n0):
    return np.array([n0, -1, 0, 0, 0, 0, 0, -1], dtype=np.int32)


def check_invariant(host, table, n, grid, base=0):
    act, tab = active_ref(host["state"][base:base + n], host["cost"][base:base + n], grid, base=base, stride=len(table))
    assert np.array_equal(host["active"][base:base + n], act), np.nonzero(host["active"][base:base + n] != act)[0][:8]
    assert np.array_equal(table, tab)
    return int(act.sum())


@pytest.mark.parametrize("bounded", [False, True])
def test_incremental_accept_keeps_the_invariant_on_random_rounds(bounded):
    rng = np.random.default_rng(3 + bounded)
    cap, n0 = 900, 30
    host = host_arrays(rng, cap)
    table = SR.synthetic_tree(rng, host, 0, n0, GRID, GRID["cells"], cost_hi=60)
    cnt, sst = counters(n0), np.array([0, 0, int(host["active"][:n0].sum()), 0], dtype=np.int32)
    bound = None
    if bounded:
        # an incumbent of 45 rows on a tree whose nodes cost 2 .. 60, one metre per row: about half of the candidates are pruned
        bound = dict(goal=np.array([0.5, 0.5]), radius=0.5, reach=1.0, stats=np.array([45, 0, 0, 0], dtype=np.int32))
        host["cost"][n0 - 1], cnt[1] = 45, n0 - 1
        host["key"][0] = 1
        host["active"][:n0], table = active_ref(host["state"][:n0], host["cost"][:n0], GRID)
        sst[2] = host["active"][:n0].sum()
    seen = dict(dominated=0, retired=0, goal_inactive=0, no_cell=0, pruned=0)
    for r in range(6):
        Bn = [1, 40, 200, 7, 300, 64][r]
        status = rng.choice([OK, GOAL, COLLIDED], Bn, p=[0.7, 0.0, 0.3] if bounded else [0.6, 0.1, 0.3])     # bounded: the incumbent stays
        rnd = rows(rng, Bn, status, int(cnt[0]), GRID)
        before = cnt.copy()
        sparse_accept_ref(host, rnd, cnt, sst, table, 0, Bn, 0, cap, GRID, bound)
        n = int(cnt[0])
        assert check_invariant(host, table, n, GRID) == sst[2]
        nid = rnd["node_id"]
        alive = status != COLLIDED
        assert cnt[4] - before[4] == Bn and (nid[~alive] == -1).all()
        pruned = 0 if bound is None else int(bound["stats"][3])
        assert (nid >= 0).sum() + sst[3] + pruned == alive.sum() and n - before[0] == (nid >= 0).sum()
        goal_rows = np.nonzero(status == GOAL)[0]
        if bound is None:
            assert (nid[goal_rows] >= 0).all()                         # a goal candidate always gets its node
        seen["goal_inactive"] += int(sum(nid[b] >= 0 and not host["active"][nid[b]] for b in goal_rows))
        seen["no_cell"] += int(sum(nid[b] >= 0 and cell_ref(GRID, rnd["end_state"][b][None])[0] < 0 for b in range(Bn)))
        seen["dominated"], seen["retired"], seen["pruned"] = int(sst[0]), int(sst[1]), seen["pruned"] + pruned
    # conditions on the inputs: every rule was at work
    assert seen["dominated"] > 100 and seen["retired"] > 10 and seen["no_cell"] > 0, seen
    assert seen["pruned"] > 100 if bounded else seen["goal_inactive"] > 0, seen


def sst_step(nodes, reps, parent, c_edge, end_state, status, grid):
    """SST's sequential rule for one candidate on (nodes = [(state, cost, active)], reps = {cell: node}) -> the node id or -1."""
    if status == COLLIDED:
        return -1
    c = nodes[parent][1] + c_edge + 1
    cell = int(cell_ref(grid, np.asarray(end_state)[None])[0])
    rep = reps.get(cell)
    better = cell >= 0 and (rep is None or c < nodes[rep][1])
    if not better and cell >= 0 and status != GOAL:
        return -1
    nodes.append([end_state, c, 1 if better else 0])
    if better:
        if rep is not None:
            nodes[rep][2] = 0
        reps[cell] = len(nodes) - 1
    return len(nodes) - 1


def test_batch_one_is_the_sequential_sst_rule():
    rng = np.random.default_rng(11)
    cap = 400
    host = host_arrays(rng, cap)
    host["state"][0, :3], host["cost"][0], host["active"][0] = [0.1, 0.2, 0.3], 1, 1
    table = active_ref(host["state"][:1], host["cost"][:1], GRID)[1]
    cnt, sst = counters(1), np.array([0, 0, 1, 0], dtype=np.int32)
    nodes, reps = [[host["state"][0].copy(), 1, 1]], {cell_of(0.1, 0.2, 0.3): 0}
    for step in range(600):
        status = rng.choice([OK, GOAL, COLLIDED], 1, p=[0.7, 0.1, 0.2])
        rnd = rows(rng, 1, status, int(cnt[0]), GRID)
        rnd["end_state"][0, :2] = rng.uniform(-0.6, 0.6, 2)            # a few cells: many contests
        kept = int((~(rnd["states"][0, :rnd["chunks_run"][0]].reshape(-1, 6) == 0).all(axis=1)).sum())
        want = sst_step(nodes, reps, int(rnd["parent"][0]), kept, rnd["end_state"][0].copy(), int(status[0]), GRID)
        sparse_accept_ref(host, rnd, cnt, sst, table, 0, 1, 0, cap, GRID)
        assert int(rnd["node_id"][0]) == want
    n = int(cnt[0])
    assert n == len(nodes) and 40 < n < 400 and sst[0] > 100 and sst[1] > 10
    assert host["cost"][:n].tolist() == [m[1] for m in nodes] and host["active"][:n].tolist() == [m[2] for m in nodes]
    check_invariant(host, table, n, GRID)


def designed(end_states, statuses, parent_costs, rep_cost=None):
    """One round of len(end_states) candidates, each with its own parent (cost given) and one kept edge row, on a tree whose
    node 1 (cost ``rep_cost``; None: absent) sits at the first candidate's end state."""
    Bn = len(end_states)
    rng = np.random.default_rng(5)
    cap = 2 + 2 * Bn
    host = host_arrays(rng, cap)
    n0 = 2 + Bn
    host["state"][:n0, :3] = [[-1.4, -1.9, 0.1 + 0.01 * k] for k in range(n0)]        # out of the way, one cell
    host["cost"][:n0] = 1
    if rep_cost is not None:
        host["state"][1] = end_states[0]
        host["cost"][1] = rep_cost
    for k, c in enumerate(parent_costs):
        host["cost"][2 + k] = c
    host["xy"][:n0] = host["state"][:n0, :2]
    act, table = active_ref(host["state"][:n0], host["cost"][:n0], GRID)
    host["active"][:n0] = act
    rnd = rows(rng, Bn, statuses, n0, GRID)
    rnd["end_state"][:] = end_states
    rnd["parent"][:] = 2 + np.arange(Bn)
    rnd["chunks_run"][:] = 1
    rnd["states"][:, 0, 0] = 1.5
    rnd["states"][:, 0, 1:] = 0.0                                      # one kept row: c = parent's cost + 2
    cnt, sst = counters(n0), np.array([0, 0, int(act.sum()), 0], dtype=np.int32)
    sparse_accept_ref(host, rnd, cnt, sst, table, 0, Bn, 0, cap, GRID)
    check_invariant(host, table, int(cnt[0]), GRID)
    return host, rnd, cnt, sst, table


def test_ties_and_goals_on_designed_rounds():
    here = np.array([0.3, 0.3, 0.3, 0, 0, 0.0])
    near = np.array([0.31, 0.32, 0.33, 0, 0, 0.0])                     # the same cell
    # equal costs among candidates: the lower index is the contender; the others are dominated
    host, rnd, cnt, sst, _ = designed([here, near, near], [OK, OK, OK], [10, 10, 10])
    assert rnd["node_id"].tolist() == [5, -1, -1] and host["active"][5] == 1 and sst.tolist() == [2, 0, 2, 2]
    # the cheaper candidate wins whatever its index
    host, rnd, cnt, sst, _ = designed([here, near, near], [OK, OK, OK], [10, 9, 10])
    assert rnd["node_id"].tolist() == [-1, 5, -1] and host["cost"][5] == 11
    # an equal cost does not displace the representative (strict '<'), one row cheaper does
    host, rnd, cnt, sst, table = designed([here, near], [OK, OK], [10, 11], rep_cost=12)
    assert rnd["node_id"].tolist() == [-1, -1] and host["active"][1] == 1 and sst.tolist() == [2, 0, 2, 2]
    host, rnd, cnt, sst, table = designed([here, near], [OK, OK], [9, 11], rep_cost=12)
    assert rnd["node_id"].tolist() == [4, -1] and host["active"][1] == 0 and host["active"][4] == 1 and sst.tolist() == [1, 1, 2, 1]
    assert table[cell_of(*here[:3])] == SR.table_key(11, 4)
    # goal candidates always get a node: inactive when they did not win the cell, and the pick sees them all
    host, rnd, cnt, sst, _ = designed([here, near, near], [GOAL, OK, GOAL], [10, 8, 20], rep_cost=9)
    assert rnd["node_id"].tolist() == [5, -1, 6] and host["active"][5] == 0 and host["active"][6] == 0 and host["active"][1] == 1
    assert cnt[1] == 5 and sst.tolist() == [1, 0, 2, 1]
    # a goal candidate that is the contender and beats the representative is active like any winner
    host, rnd, cnt, sst, _ = designed([here, near], [OK, GOAL], [10, 5], rep_cost=9)
    assert rnd["node_id"].tolist() == [-1, 4] and host["active"][4] == 1 and host["active"][1] == 0 and cnt[1] == 4
    # a collided candidate takes no part in the contest; a candidate without a cell gets its node and is never active
    nowhere = np.array([np.nan, 0.3, 0.3, 0, 0, 0.0])
    host, rnd, cnt, sst, _ = designed([here, near, nowhere], [COLLIDED, OK, OK], [1, 10, 10])
    assert rnd["node_id"].tolist() == [-1, 5, 6] and host["active"][5] == 1 and host["active"][6] == 0 and sst.tolist() == [0, 0, 2, 0]


def test_a_winner_past_the_capacity_does_not_become_the_representative():
    rng = np.random.default_rng(8)
    cap, n0 = 12, 10
    host = host_arrays(rng, cap)
    table = SR.synthetic_tree(rng, host, 0, n0, GRID, GRID["cells"])
    free = [c for c in range(GRID["cells"]) if table[c] == EMPTY][:4]
    rnd = rows(rng, 4, [OK] * 4, n0, GRID)
    for b, c in enumerate(free):                                       # four candidates, four free cells, two slots
        ix, iy, ih = parts(c)
        rnd["end_state"][b, :3] = [-1.5 + (ix + 0.5) * 0.5, -2.0 + (iy + 0.5) * 0.5, (ih + 0.5) * GRID["w"]]
    cnt, sst = counters(n0), np.array([0, 0, int(host["active"][:n0].sum()), 0], dtype=np.int32)
    a0 = int(sst[2])
    sparse_accept_ref(host, rnd, cnt, sst, table, 0, 4, 0, cap, GRID)
    assert rnd["node_id"].tolist() == [10, 11, -1, -1] and cnt[0] == cap and cnt[6] == 1
    assert table[free[2]] == EMPTY and table[free[3]] == EMPTY and sst.tolist() == [0, 0, a0 + 2, 0]
    check_invariant(host, table, cap, GRID)


# ---------------------------------------------------------------------- the restated planner
CASES = [("best_of_round", None), ("anytime", None), ("anytime", 1.0), ("anytime_pruned", None), ("anytime_pruned", 1.0)]


@pytest.mark.parametrize("solution,near", CASES)
def test_restated_planner_keeps_the_invariant_every_round(solution, near):
    o = SR.sparse_run(solution, 0.5, near_radius=near)
    states = np.array(o.pl.tree.states)
    assert len(o.rounds) >= 1 and len(states) == len(o.cost)
    for r in o.rounds:
        n = r["nodes_after"]
        act, _ = active_ref(states[:n], r["cost_after"], o.grid)
        assert np.array_equal(act, np.array(r["active_after"], dtype=np.uint8))
        for b in r["goals"]:
            assert r["node_id"][b] >= 0
    assert o.active_nodes() == len(o.rep) and o.incumbent is not None
    assert len(o.cost) - 1 + o.dominated + o.pruned <= o.pl.candidates and o.dominated > 0


def test_preconditions_of_the_gpu_plan_test():
    """The scratch run of the issue -- boxes, (18, 13) -> (18, 17), edge length 32, tape 5, batch 64, 8 rounds, seed 5,
    ``sparse_cell`` 0.5, 1 heading -- re-established on this restatement with the seed unchanged: 216 dominated, 3 retired, 68
    parents moved, 141 nodes, an incumbent of 68 rows.  And the scenario the plan test runs per mode (seed 13, four rounds, 8
    headings): the rule is at work there too."""
    o = SR.sparse_run("anytime", 0.5, headings=1, seed=5, rounds=8)
    moved = sum(int((np.asarray(r["parent"]) != r["dense_parent"]).sum()) for r in o.rounds)
    assert (o.dominated, o.retired, moved, len(o.cost)) == (216, 3, 68, 141)
    assert o.dominated >= 100 and o.retired >= 1 and moved >= 10 and o.incumbent is not None and o.cost[o.incumbent] == 68
    o = SR.sparse_run("anytime", 0.5)
    moved = sum(int((np.asarray(r["parent"]) != r["dense_parent"]).sum()) for r in o.rounds)
    assert (len(o.cost), o.dominated, moved, o.cost[o.incumbent]) == (104, 73, 10, 66)


# ---------------------------------------------------------------------- refusals
def test_planner_refuses_by_name():
    start, goal, args = _car_args(solution="anytime", sparse_cell=0.5)
    with pytest.raises(ValueError, match="sparse_cell needs a solution other than 'first'"):
        F.RRT_Planner(start, goal, **dict(args, solution="first"))
    for sol in ("best_of_round", "anytime", "anytime_pruned"):
        with pytest.raises(ValueError, match="sparse_headings belongs to sparse_cell"):
            F.RRT_Planner(start, goal, **dict(args, solution=sol, sparse_cell=None, sparse_headings=8))
    for bad in (0, -1.0, float("nan"), float("inf"), "1", True):
        with pytest.raises(ValueError, match="sparse_cell must be a positive finite number of metres"):
            F.RRT_Planner(start, goal, **dict(args, sparse_cell=bad))
    for bad in (0, 65, -1, 2.0, "8", True):
        with pytest.raises(ValueError, match="sparse_headings must be an integer from 1 to 64"):
            F.RRT_Planner(start, goal, **dict(args, sparse_headings=bad))
    with pytest.raises(ValueError, match="more than 4194304 per tree"):
        F.RRT_Planner(start, goal, **dict(args, sparse_cell=0.001))
    with pytest.raises(NotImplementedError, match="sparse_cell: the car only"):
        F.RRT_Planner(np.zeros(29), np.zeros(29), **dict(args, env_id="antmaze", environment=_AntEnv()))
    with pytest.raises(NotImplementedError, match="sparse_cell: one rank"):
        F.RRT_Planner(start, goal, **dict(args, world_size=2))
    with pytest.raises(NotImplementedError, match="sparse_cell: run_type 0 only"):
        F.RRT_Planner(start, goal, **dict(args, run_type=2))
    with pytest.raises(NotImplementedError, match="sparse_cell: a single prop_duration entry"):
        F.RRT_Planner(start, goal, **dict(args, prop_duration=[32, 64]))


def test_engine_refuses_by_name():
    assert E.check_sparse(None, None, "first") is None
    assert E.check_sparse(0.5, None, "anytime") == (0.5, 8) and E.check_sparse(1, 3, "anytime_pruned") == (1.0, 3)
    with pytest.raises(ValueError, match="sparse_headings belongs to sparse_cell"):
        E.check_sparse(None, 4, "anytime")
    with pytest.raises(ValueError, match="sparse_cell needs a solution other than 'first'"):
        E.check_sparse(0.5, 8, "first")
    with pytest.raises(NotImplementedError, match="sparse_cell: the car only"):
        E.check_sparse(0.5, 8, "anytime", ant=True)
    assert E.sparse_grid((31, 20), 1.0, 0.5, 8) == (20.0, 31.0, 40, 62)
    assert E.sparse_grid((4, 3), 2.0, 0.7, 1) == (6.0, 8.0, 9, 12)
    with pytest.raises(ValueError, match="more than 4194304 per tree"):
        E.sparse_grid((31, 31), 1.0, 0.01, 8)
    maze = np.zeros((4, 4), dtype=np.float32)
    with pytest.raises(NotImplementedError, match="sparse_cell: a single prop_duration entry"):
        E.ExpansionEngine(object(), maze, np.zeros(6), np.zeros(6), emulate_sticky_done=False, solution="anytime",
                          prop_duration=[32, 64], sparse_cell=0.5)
    with pytest.raises(NotImplementedError, match="one rank"):
        E.ExpansionEngine(object(), maze, np.zeros(6), np.zeros(6), emulate_sticky_done=False, solution="anytime", world_size=2,
                          sparse_cell=0.5)


# ---------------------------------------------------------------------- what reaches the library
def one_round(rec, eng, forest):
    rec.calls.clear()
    samples, cond, acts, extra = round_inputs(eng, False)
    if forest:
        extra["counts_per_tree"] = COUNTS
    eng.expand_round(samples, cond, inject_actions=acts, **extra)
    assert rec.problems == []


@pytest.mark.parametrize("kind", ["single", "forest", "scene"])
@pytest.mark.parametrize("mode", ["first", "best_of_round", "anytime", "anytime_pruned"])
def test_without_sparse_cell_no_sparse_entry_is_reached(rec, kind, mode):
    eng, _ = make_engine(rec, kind, mode)
    assert eng.sparse is None and eng.tree.active is None and "sparse" not in eng.entries.expand + eng.entries.accept
    one_round(rec, eng, KINDS[kind][1])
    assert not any("sparse" in n for n in rec.names())
    kw = eng.round_settings()
    assert kw["sparse_cell"] is None and kw["sparse_headings"] is None


@pytest.mark.parametrize("kind", ["single", "forest", "scene"])
@pytest.mark.parametrize("mode", ["best_of_round", "anytime", "anytime_pruned"])
@pytest.mark.parametrize("near", [None, 1.5])
def test_with_sparse_cell_round_and_accept_take_the_sparse_entries(rec, kind, mode, near):
    """The rebuild of every reset tree first, then one expand entry -- [scenes or NULL], round, parameters, the bound or NULL, the
    near descriptor or NULL, the sparse descriptor -- and one accept entry: the cost column, the bound or NULL, the descriptor."""
    _, forest, scenes, _ = KINDS[kind]
    more = {} if near is None else dict(near_radius=near, near_reach=0.05)
    eng, _ = make_engine(rec, kind, mode, sparse_cell=0.5, sparse_headings=4, **more)
    assert eng.sparse == (0.5, 4) and eng.tree.active is not None and eng.tree.cost is not None
    one_round(rec, eng, forest)
    f = "forest_" if forest else ""
    pruned = mode == "anytime_pruned"
    T = eng.T if forest else 1
    names = [n for n in rec.names() if n != "ditree_bound_keys"]
    assert names == ["ditree_sparse_rebuild", f"ditree_{f}expand_round_sparse", f"ditree_{f}accept_sparse"]
    rb, ex, ac = (next(c for c in rec.calls if c.name == n) for n in names)
    assert rb.raw[-3:-1] == (0, T) and rb.raw[-4] == eng.tree.cost.data_ptr()
    sp = ex.args[-2]
    assert isinstance(sp, _lib.Sparse) and (sp.cell, sp.w, sp.nh) == (0.5, 2.0 * np.pi / 4, 4)
    assert sp.stride == 12 * 12 * 4 and sp.active == eng.tree.active.data_ptr() and sp.cand == eng._sparse_cand.data_ptr()
    assert sp.stats == (eng.fsparse if forest else eng.tree.sparse_stats).data_ptr()
    assert [sp.dims_host[k] for k in range(2 * T)] == [12, 12] * T
    assert np.array_equal(eng._sparse_extent.numpy(), np.tile([6.0, 6.0], (T, 1)))
    assert (ex.raw[-4] is None) == (not pruned) and (ex.raw[-3] is None) == (near is None)
    if pruned:
        assert ex.raw[-4]._obj is eng.bound and ac.raw[-3]._obj is eng.bound
    else:
        assert ac.raw[-3] is None
    assert ac.raw[-4] == eng.tree.cost.data_ptr() and isinstance(ac.args[-2], _lib.Sparse)
    # a second round rebuilds nothing; a reset tree is rebuilt alone
    one_round(rec, eng, forest)
    assert "ditree_sparse_rebuild" not in rec.names()
    if forest:
        eng.reset_tree(1, *((1,) if scenes else ()))
        one_round(rec, eng, forest)
        rb = [c for c in rec.calls if c.name == "ditree_sparse_rebuild"]
        assert len(rb) == 1 and rb[0].raw[-3:-1] == (1, 1)
    kw = eng.round_settings()
    assert (kw["sparse_cell"], kw["sparse_headings"]) == (0.5, 4)


def test_the_planner_hands_cell_and_headings_to_its_engine(rec):
    start, goal, args = _car_args(solution="anytime", ctx=StubContext(rec), batch=8, capacity=64, prop_duration=[16])
    pl = F.RRT_Planner(start, goal, **dict(args, sparse_cell=1))
    assert (pl.sparse_cell, pl.sparse_headings) == (1.0, 8) and pl._engine.sparse == (1.0, 8)
    pl.reset()
    assert (pl.results["dominated_candidates"], pl.results["retired_nodes"], pl.results["active_nodes"]) == (0, 0, 1)
    settings = dict(F._scene_settings(pl))
    assert settings["sparse_cell"] == 1.0 and settings["sparse_headings"] == 8
    pl = F.RRT_Planner(start, goal, **args)
    pl.reset()
    assert pl.sparse_cell is None and pl._engine.sparse is None and "active_nodes" not in pl.results
