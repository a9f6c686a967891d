"""GPU: ditree_accept_bounded / ditree_forest_accept_bounded (accept_cost_kernel, accept_scan_kernel<bounded>, the commit
kernel's key column, the pick's stats row) against the sequential restatement of tests/anytime_pruned_ref.py, on rounds written
straight into the device arrays in the manner of tests/test_gpu_accept_best.py and at its sizes.  Every comparison is exact:
node ids, whole counter and stats rows, the cost and key columns, num_visit and every tree array."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.accept_best_ref import COLLIDED, GAC, GOAL, OK
from tests.anytime_pruned_ref import NO_BOUND, accept_bounded_ref, h_ref
from tests.test_gpu_accept_best import (CAP, SIZES, TREE_FIELDS, accept_best, compare_tree, edge_rows_kept, random_rows,
                                        random_tree_state, single, upload_round, upload_tree)  # noqa: F401
from tests.test_gpu_forest import ctx, dev, scenario  # noqa: F401

pytestmark = pytest.mark.gpu

FIELDS = TREE_FIELDS + ("key",)
GOAL_XY = np.array([1.5, 6.0])           # end states lie in [1, 2]^2: 3.5 to 5 m away, h = 35 .. 46 rows at 0.1 m per row
RADIUS, REACH = 0.5, 0.1
CASES = ["no_incumbent", "boundary", "goal_rows", "zero_rows", "all_pruned", "mixed", "capacity_exact", "capacity_over"]
N0 = 40


@pytest.fixture(scope="module")
def pruned(ctx):
    from ditreeonlineplanner_amd.engine import ExpansionEngine
    maze, start, goal = scenario()
    return ExpansionEngine(ctx, maze, start, goal, edge_length=16, action_horizon=8, batch=2500, capacity=CAP,
                           emulate_sticky_done=False, solution="anytime_pruned", reach=REACH)


def bound_desc(eng, goals, stats, reach=REACH):
    from ditreeonlineplanner_amd._lib import Bound
    return Bound(eng.tree.cost.data_ptr(), eng.tree.key.data_ptr(), goals.data_ptr(), RADIUS, reach, stats.data_ptr())


def f_of(host, rnd, b, goal=GOAL_XY):
    return (int(host["cost"][rnd["parent"][b]]) + edge_rows_kept(rnd, b) + 1
            + h_ref(rnd["end_state"][b, 0], rnd["end_state"][b, 1], goal, RADIUS, REACH))


def set_f(host, rnd, b, parent, f):
    """Row b gets its own parent, whose cost makes the row's f exactly ``f``."""
    rnd["parent"][b] = parent
    host["cost"][parent] = 0
    host["cost"][parent] = f - f_of(host, rnd, b)
    assert host["cost"][parent] >= 1


def special_rows(B):
    return sorted(set([0, B // 3, B // 2, B - 1, min(B - 1, 1023), min(B - 1, 1024)]))


def build_case(case, B, rng):
    host = random_tree_state(rng, CAP, 1)
    host["key"] = rng.integers(1, 400, CAP).astype(np.int32)
    n0, inc, Ub = N0, N0 - 1, 300
    status = np.where(rng.random(B) < 0.3, COLLIDED, OK)
    status[rng.random(B) < 0.05] = COLLIDED | GAC
    rows = special_rows(B)
    status[rows] = GOAL if case == "goal_rows" else OK
    rnd = random_rows(rng, B, status, 6, n0 - 7)                      # parents 6 .. n0 - 2: the special rows own 0 .. 5
    host["cost"][:n0] = rng.integers(150, 300, n0)                    # f of the other rows: on both sides of 300
    want = {}
    if case in ("boundary", "goal_rows"):
        for k, b in enumerate(rows):
            if case == "goal_rows":
                rnd["end_state"][b, :2] = GOAL_XY + rng.uniform(-0.3, 0.3, 2)       # inside the goal disc: h = 0
            want[b] = Ub + (k % 3) - 1
            set_f(host, rnd, b, k, want[b])
    elif case == "zero_rows":
        for k, b in enumerate(rows):
            rnd["chunks_run"][b] = 2
            rnd["states"][b] = rng.uniform(1, 2, (2, 9, 6))
            set_f(host, rnd, b, k, Ub)                                # with every row kept the candidate is pruned
            if k % 2 == 0:
                rnd["states"][b, 1, 4 + k // 2:] = 0.0                # a goal in mid-chunk leaves zero rows: now f < U
            want[b] = f_of(host, rnd, b)
    elif case == "all_pruned":
        Ub = 1
    elif case.startswith("capacity"):
        fs = np.array([f_of(host, rnd, b) for b in range(B)])
        fit = int(((status & 0xff != COLLIDED) & (fs < Ub)).sum())
        n0 = CAP - fit + (2 if case == "capacity_over" and fit >= 2 else 0)
        inc = n0 - 1
        host["cost"][n0 - N0:n0] = host["cost"][:N0]                   # the parents' costs travel with them
        rnd["parent"] = (rnd["parent"] + n0 - N0).astype(np.int32)
    if case != "no_incumbent":
        host["counters"][0, 1] = inc
        host["cost"][inc] = Ub
    host["counters"][0, 0] = n0
    stats = np.array([NO_BOUND if case == "no_incumbent" else Ub, int(rng.integers(0, 9)), 0, 7], dtype=np.int32)
    return host, rnd, stats, rows, want, Ub


def run_bounded(ctx, eng, B, goals, stats, reach=REACH):
    from ditreeonlineplanner_amd import _lib
    eng.ensure_maze()
    rd = eng.rb.desc(0, B)
    bd = bound_desc(eng, goals, stats, reach)
    return _lib.lib().ditree_accept_bounded(ctx._h, C.byref(eng.tree.desc), C.byref(rd), C.byref(bd), ctx.stream)


def upload(eng, host):
    upload_tree(eng.tree, host, eng.tree.counters)
    if eng.tree.key is not None:
        eng.tree.key.copy_(dev(host["key"]))


@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("case", CASES)
def test_accept_bounded_against_the_sequential_restatement(ctx, pruned, single, case, B):
    rng = np.random.default_rng(2000 * CASES.index(case) + B)
    host, rnd, stats_h, rows, want, Ub = build_case(case, B, rng)
    before, stats_before = host["counters"][0].copy(), stats_h.copy()
    upload(pruned, host)
    upload_round(pruned.rb, rnd, B)
    goals, stats = dev(GOAL_XY[None]), dev(stats_h)
    if case == "no_incumbent":                                        # the other side: ditree_accept_best on the same arrays
        upload(single, host)
        upload_round(single.rb, rnd, B)
        assert accept_best(ctx, single, B) == 0
    assert run_bounded(ctx, pruned, B, goals, stats) == 0
    accept_bounded_ref(host, rnd, host["counters"][0], stats_h, 0, B, 0, CAP, GOAL_XY, RADIUS, REACH)
    compare_tree(pruned.tree, pruned.tree.counters, pruned.rb, host, rnd, B, fields=FIELDS)
    assert np.array_equal(stats.cpu().numpy(), stats_h), (stats.cpu().numpy(), stats_h)
    # the restatement itself went through the case (conditions on the test's inputs, not on the device)
    cnt, nid = host["counters"][0], rnd["node_id"]
    alive = rnd["status"] & 0xff != COLLIDED
    assert cnt[4] - before[4] == B and cnt[3] - before[3] == rnd["chunks_run"].sum() and cnt[7] == -1
    assert stats_h[1] - stats_before[1] == stats_h[3] and stats_h[3] + (nid >= 0).sum() + (cnt[6] and 1) <= alive.sum()
    if case == "no_incumbent":
        assert stats_h[3] == 0 and (nid[alive] >= 0).all()
        assert torch.equal(pruned.rb.node_id[:B], single.rb.node_id[:B])
        for name in TREE_FIELDS:
            assert torch.equal(getattr(pruned.tree, name), getattr(single.tree, name)), name
        assert torch.equal(pruned.tree.counters, single.tree.counters)
        new = nid[nid >= 0]
        assert all(host["key"][k] == host["cost"][k] + h_ref(*host["xy"][k], GOAL_XY, RADIUS, REACH) for k in new)
    elif case in ("boundary", "goal_rows"):
        for b in rows:
            assert (nid[b] >= 0) == (want[b] == Ub - 1), (b, want[b])
        if case == "goal_rows" and any(want[b] == Ub - 1 for b in rows):
            assert before[1] != cnt[1] == nid[min(b for b in rows if want[b] == Ub - 1)] and stats_h[0] == Ub - 1
    elif case == "zero_rows":
        for k, b in enumerate(rows):
            assert (nid[b] >= 0) == (k % 2 == 0) and (want[b] < Ub) == (k % 2 == 0)
    elif case == "all_pruned":
        assert (nid == -1).all() and stats_h[3] == alive.sum() and cnt[0] == before[0] and cnt[6] == 0 and stats_h[2] == 1
    elif case == "mixed":
        assert B < 63 or (0 < stats_h[3] < alive.sum() and (~alive).any())
    elif case == "capacity_exact":
        assert cnt[0] == CAP and cnt[6] == 0 and (B < 63 or before[0] + alive.sum() > CAP)
    elif case == "capacity_over":
        assert cnt[0] == CAP and (B < 63 or (cnt[6] == 1 and (nid[alive] == -1).sum() == stats_h[3] + 2))


# ---------------------------------------------------------------------- forests
FORESTS = {1: (1, 200, [70]), 3: (3, 1200, [0, 1100, 0]),
           64: (64, 40, [0, 0, 5, 30, 1, 0, 0, 17] + [(7 * t) % 23 for t in range(8, 63)] + [0])}


@pytest.mark.parametrize("T", list(FORESTS))
def test_forest_accept_bounded_against_the_sequential_restatement(ctx, T):
    """Two rounds on one forest, every tree with its own goal and its own bound: trees without an incumbent, with one that
    prunes about half and with one that prunes everything, empty ranges (tree and stats row untouched), a tree that runs out of
    slots; the second round meets the incumbents and bounds the first one left."""
    from ditreeonlineplanner_amd import _lib
    from ditreeonlineplanner_amd._lib import Bound
    from ditreeonlineplanner_amd.forest import ForestEngine
    T, Cap, counts = FORESTS[T]
    maze, start, goal = scenario()
    forest = ForestEngine(ctx, maze, start, goal, T, Cap, edge_length=16, action_horizon=8, batch=sum(counts),
                          emulate_sticky_done=False, solution="anytime_pruned", reach=REACH)
    rng = np.random.default_rng(11 + T)
    host = random_tree_state(rng, T * Cap, T)
    host["key"] = rng.integers(1, 400, T * Cap).astype(np.int32)
    gl = np.stack([GOAL_XY + [0.0, 0.5 * (t % 5)] for t in range(T)])
    n0 = rng.integers(2, 6, T)
    full = T - 2 if T > 1 else 0
    n0[full] = Cap - 3
    host["counters"][:, 0] = n0
    stats_h = np.tile(np.array([NO_BOUND, 0, 0, 0], dtype=np.int32), (T, 1))
    host["cost"][:] = rng.integers(150, 300, T * Cap)
    for t in range(T):
        if t % 3 and t != full:                          # an incumbent: bound 300 (about half pruned) or 1 (everything pruned)
            inc = t * Cap + int(n0[t]) - 1
            host["counters"][t, 1] = inc
            host["cost"][inc] = stats_h[t, 0] = 300 if t % 3 == 1 else 1
    upload_tree(forest.tree, host, forest.fcounters)
    forest.tree.key.copy_(dev(host["key"]))
    goals, stats = dev(gl), dev(stats_h)
    bd = Bound(forest.tree.cost.data_ptr(), forest.tree.key.data_ptr(), goals.data_ptr(), RADIUS, REACH, stats.data_ptr())
    pruned_total = 0
    for rounds in range(2):
        off = np.concatenate([[0], np.cumsum(counts)])
        B = int(off[-1])
        status = rng.choice([OK, GOAL, COLLIDED, COLLIDED | GAC], B, p=[0.5, 0.12, 0.3, 0.08])
        rnd = random_rows(rng, B, status, 0, 1)
        for t in range(T):
            lo, hi = int(off[t]), int(off[t + 1])
            rnd["parent"][lo:hi] = t * Cap + rng.integers(0, max(1, host["counters"][t, 0] - 1), counts[t])
            g = lo + np.nonzero(rnd["status"][lo:hi] == GOAL)[0]
            rnd["end_state"][g, :2] = gl[t] + rng.uniform(-0.3, 0.3, (len(g), 2))
        upload_round(forest.rb, rnd, B)
        forest._set_offsets(counts)
        forest.ensure_maze()
        rd = forest.rb.desc(0, B)
        before, sbefore = host["counters"].copy(), stats_h.copy()
        _lib.check(ctx._h, _lib.lib().ditree_forest_accept_bounded(ctx._h, C.byref(forest.tree.desc), C.byref(forest.fdesc),
                                                                   C.byref(rd), C.byref(bd), ctx.stream), "forest_accept_bounded")
        for t in range(T):
            accept_bounded_ref(host, rnd, host["counters"][t], stats_h[t], int(off[t]), int(off[t + 1]), t * Cap, Cap, gl[t],
                               RADIUS, REACH)
        compare_tree(forest.tree, forest.fcounters, forest.rb, host, rnd, B, fields=FIELDS)
        assert np.array_equal(stats.cpu().numpy(), stats_h)
        empty = [t for t in range(T) if counts[t] == 0]
        assert np.array_equal(host["counters"][empty], before[empty]) and np.array_equal(stats_h[empty], sbefore[empty])
        pruned_total += int(stats_h[:, 3][[t for t in range(T) if counts[t]]].sum())
        for t in range(T):
            if counts[t] and sbefore[t, 0] == 1:
                assert host["counters"][t, 0] == before[t, 0] and stats_h[t, 2] == 1
            if counts[t] and sbefore[t, 0] == NO_BOUND:
                assert stats_h[t, 3] == 0
        if counts[full] > 3:
            assert host["counters"][full, 0] == Cap and host["counters"][full, 6] == 1
        counts = {1: [65], 3: [40, 0, 30], 64: counts[::-1]}[T]
    assert T == 1 or pruned_total > 0


def test_accept_bounded_refuses_by_name_without_launching(ctx, pruned):
    """A missing key column, reach <= 0, a sharded round ...: DITREE_E_ARG with the message, node ids, counters and stats
    untouched -- both entry points."""
    from ditreeonlineplanner_amd import _lib
    from ditreeonlineplanner_amd._lib import Bound
    from ditreeonlineplanner_amd.forest import ForestEngine
    maze, start, goal = scenario()
    forest = ForestEngine(ctx, maze, start, goal, 2, 16, edge_length=16, action_horizon=8, batch=8, emulate_sticky_done=False,
                          solution="anytime_pruned")
    forest._set_offsets([3, 1])
    h, L = ctx._h, _lib.lib()
    for eng, counters, T in ((pruned, pruned.tree.counters, 1), (forest, forest.fcounters, 2)):
        eng.tree.reset(eng.start_state)
        eng.rb.node_id.fill_(-7)
        eng.rb.parent.zero_()
        eng.rb.status.fill_(GOAL)
        cnt = counters.clone()
        goals = torch.zeros(T, 2, dtype=torch.float64, device="cuda")
        stats = torch.full((T, 4), 3, dtype=torch.int32, device="cuda")
        c, k, g, s = eng.tree.cost.data_ptr(), eng.tree.key.data_ptr(), goals.data_ptr(), stats.data_ptr()
        for bd, shard, msg in ((Bound(c, None, g, 0.5, 0.1, s), 0, b"bound: key column missing"),
                               (Bound(None, k, g, 0.5, 0.1, s), 0, b"bound: cost array missing"),
                               (Bound(c, k, g, 0.5, 0.0, s), 0, b"bound: reach must be > 0"),
                               (Bound(c, k, g, 0.5, -0.1, s), 0, b"bound: reach must be > 0"),
                               (Bound(c, k, None, 0.5, 0.1, s), 0, b"bound: goal_xy missing"),
                               (Bound(c, k, g, 0.5, 0.1, None), 0, b"bound: stats rows missing"),
                               (Bound(c, k, g, 0.5, 0.1, s), 2, b"bound: one rank (round->shard must be 0)")):
            rd = eng.rb.desc(0, 4)
            rd.shard = shard
            if eng is pruned:
                rc = L.ditree_accept_bounded(h, C.byref(eng.tree.desc), C.byref(rd), C.byref(bd), ctx.stream)
            else:
                rc = L.ditree_forest_accept_bounded(h, C.byref(eng.tree.desc), C.byref(eng.fdesc), C.byref(rd), C.byref(bd), ctx.stream)
            assert rc == -1 and L.ditree_last_error(h) == msg, L.ditree_last_error(h)
        torch.cuda.synchronize()
        assert (eng.rb.node_id == -7).all() and torch.equal(counters, cnt) and (stats == 3).all()
