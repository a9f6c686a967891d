"""GPU: ditree_tree_rebase at the sizes it runs at -- trees past one and two trips of rebase_scan_kernel's 1024-node walk,
edges of 36 and 144 rows (second and third steps of rebase_valid_kernel's row loop and rebase_move_kernel's copy loops),
chains that need the last pointer-doubling pass, maps that are not square, and ExpansionEngine.rebase on a tree grown by
rounds -- against the plain-loop restatement of tests/tree_rebase_ref.py.  Every comparison is exact (``run`` of
tests/test_gpu_tree_rebase.py: the kept slots of every array, the 8 counters, the old-id -> new-id table, src untouched, the
sentinel behind the kept slots of dst).  Every case asserts on the restatement's own output that its inputs reach the path it is
there for, before the device is called.

The restatement asks the oracle's collision test row by row; at 2600 nodes of 37 rows that is 20 s.  Here it looks the answers
up in a table filled by one vectorised oracle call (``R.collision_table``), and ``checked_table`` asserts the table against the
row-by-row test on 500 sampled rows and on every row that collides.  Trees and restatements are built once per module.

What the restatement keeps and drops (asserted below as bounds, listed here as they come out):
  A  n 2600 in 4096, 36-row edges: 1405 kept (746 / 400 / 259 per trip), 1195 dropped, 1358 survivors change id
  B  n 1023 .. 2048 in 2048, 3-row edges: 449, 450, 451, 1020, 1020 kept, 574 .. 1028 dropped
  C  n 2600 in 4096, anchor 1100 with 998 nodes below it: 568 kept behind the fresh root, 430 dropped below the anchor
  D  n 1500 in 2048: the chain keeps 1500, 1400 and 3; the star keeps 1001
  E  n 150 in 256, edges of 9, 63, 72 and 144 rows: one blocked row drops 3 .. 11 nodes; the fresh root keeps 150 or 1
  F  n 300 in 2048: 206 kept on 7 x 13 and on 21 x 24, 266 on 24 x 21
  G  1198 nodes in 4096 grown by ten rounds: 659 kept and 539 dropped, then 345 kept of those"""
import functools

import numpy as np
import pytest
import torch

from tests import tree_rebase_ref as R
from tests.test_gpu_forest import ctx, dev  # noqa: F401
from tests.test_gpu_tree_rebase import Pair, free_cells, make_tree, run
from tests.util import load_maze

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ helpers (host only)
def wall_cells(maze):
    return [(int(r), int(c)) for r, c in np.argwhere(maze == 1)]


def block(t, m, row, maze, cell):
    """Move one row of node ``m`` (``row`` None: its own state) onto the centre of the wall cell ``cell``."""
    assert maze[cell] == 1
    s = R.cell_state(maze, *cell)
    if row is None:
        t["state"][m], t["xy"][m] = s, s[:2]
    else:
        assert 0 <= row < t["edge_nstates"][m]
        t["edge_states"][m, row] = s


def checked_table(t, n, maze, blocked, seed=0):
    """The collision table of the first n nodes, asserted equal to the restatement's row loop on 500 sampled rows, on every
    row of ``blocked`` ((node, row) with row None for the node's state; None: a grown tree, whatever collides) and on every other
    used row the table calls colliding, of which a hand-made tree has none."""
    tab = R.collision_table(t, n, maze)
    ens = t["edge_nstates"][:n]
    used = [(m, r) for m in range(n) for r in range(-1, int(ens[m]))]            # row -1: the node's own state
    rng = np.random.default_rng(seed)
    sample = {used[i] for i in rng.choice(len(used), min(500, len(used)), replace=False)}
    hits = {(m, r) for m, r in used if (tab["state"][m] if r < 0 else tab["edge_states"][m, r])}
    marked = hits if blocked is None else {(m, -1 if r is None else r) for m, r in blocked}
    assert marked <= hits and len(sample) >= min(500, len(used))
    for m, r in sorted(sample | hits):
        row, have = (t["state"][m], tab["state"][m]) if r < 0 else (t["edge_states"][m, r], tab["edge_states"][m, r])
        assert R.row_collides(row, maze) == bool(have), (m, r)
    assert hits == marked, "a row placed in a free cell collides"
    return tab


def copy_tree(t):
    return {k: v.copy() for k, v in t.items()}


def subtree(parents, n, node):
    return set(R.descendants(np.asarray(parents), n, node))


def window_parents(rng, n, width):
    """parent < child, drawn from the ``width`` ids below each node."""
    return [-1] + [int(rng.integers(max(0, m - width), m)) for m in range(1, n)]


def kept_of(want):
    return np.flatnonzero(want["new_id"] >= 0)


# ------------------------------------------------------------------------------------------------ A, C: the default edge
BIG = dict(cap=4096, nch=4, a=8)                           # 36 state rows, 32 action rows per edge
N_BIG = 2600                                               # three trips of the scan, the last one partial (2600 = 2 * 1024 + 552)


@functools.lru_cache(maxsize=None)
def tree_a():
    """Case A: n = 2600 on ``shapes``, parents from the 60 ids below, 40 blocked nodes (any row of the edge, or the state)."""
    maze = load_maze("shapes")
    rng = np.random.default_rng(2616)
    parents = window_parents(rng, N_BIG, 60)
    t, cnt = make_tree(parents, 2600, maze=maze, free_list=free_cells(maze), **BIG)
    walls, blocked = wall_cells(maze), []
    for m in rng.choice(np.arange(1, N_BIG), 40, replace=False):
        row = int(rng.integers(0, 37))
        blocked.append((int(m), None if row == 36 else row))
        block(t, int(m), blocked[-1][1], maze, walls[rng.integers(len(walls))])
    tab = checked_table(t, N_BIG, maze, blocked)
    want = R.rebase_ref(t, cnt, maze, 0, collides=tab)
    return maze, t, cnt, tab, want


@functools.lru_cache(maxsize=None)
def tree_c():
    """Case C: the anchor at old id 1100; about two thirds of the later nodes hang below it (parents from
    the 30 latest of them), 25 of those are blocked."""
    maze = load_maze("shapes")
    rng = np.random.default_rng(1100)
    anchor = 1100
    parents = window_parents(rng, anchor + 1, 60)
    below, rest = [anchor], list(range(anchor - 60, anchor))
    for m in range(anchor + 1, N_BIG):
        if rng.random() < 0.66:
            parents.append(int(below[-30:][rng.integers(len(below[-30:]))]))
            below.append(m)
        else:
            parents.append(int(rest[-40:][rng.integers(len(rest[-40:]))]))
            rest.append(m)
    t, cnt = make_tree(parents, 1100, maze=maze, free_list=free_cells(maze), **BIG)
    walls, blocked = wall_cells(maze), []
    for m in rng.choice(np.array(below[40:]), 25, replace=False):
        row = int(rng.integers(0, 37))
        blocked.append((int(m), None if row == 36 else row))
        block(t, int(m), blocked[-1][1], maze, walls[rng.integers(len(walls))])
    tab = checked_table(t, N_BIG, maze, blocked)
    return maze, t, cnt, tab, anchor, parents, [m for m, _ in blocked]


@pytest.fixture(scope="module")
def big_pair(ctx):
    return Pair(ctx, **BIG)


@pytest.mark.parametrize("goal", ["kept", "dropped"])
def test_a_scan_over_three_trips(big_pair, goal):
    maze, t, cnt, tab, base = tree_a()
    new_id, kept = base["new_id"], kept_of(base)
    n_kept = len(kept)
    # on the restatement: both answers in every trip and a survivor in every wave, so that every wave offset and both carries
    # between trips are non-zero and differ from the old ids
    assert base["status"] == 0 and base["n"] == n_kept and 4 * n_kept >= N_BIG and 4 * (N_BIG - n_kept) >= N_BIG
    for lo in range(0, N_BIG, 1024):
        part = new_id[lo:lo + 1024]
        assert (part >= 0).sum() >= 50 and (part < 0).sum() >= 50, lo
    assert all((new_id[lo:lo + 64] >= 0).any() for lo in range(0, N_BIG, 64))
    assert (new_id[kept] != kept).sum() >= 1000
    third = np.arange(2048, N_BIG)
    g = int(third[new_id[third] >= 0][-1] if goal == "kept" else third[new_id[third] < 0][-1])
    cnt = cnt.copy()
    cnt[1] = g
    want = R.rebase_ref(t, cnt, maze, 0, collides=tab)
    assert np.array_equal(want["new_id"], new_id)
    assert want["counters"][1] == (new_id[g] if goal == "kept" else -1) and (goal == "dropped" or 0 <= new_id[g] != g)
    run(big_pair, t, cnt, 0, maze=maze, collides=tab)


@pytest.mark.parametrize("cost", [True, False], ids=["cost", "no_cost"])
def test_c_anchor_in_the_second_trip_behind_a_fresh_root(ctx, big_pair, cost):
    maze, t, cnt, tab, anchor, parents, blocked = tree_c()
    fc = free_cells(maze)
    root = R.cell_state(maze, *fc[len(fc) // 2], 0.7, 0.1, -0.1)
    ds, da = 5, 4
    tt = copy_tree(t)
    if not cost:
        tt.pop("cost")
    cnt = cnt.copy()
    want = R.rebase_ref(tt, cnt, maze, anchor, root, ds, da, collides=tab)
    below = subtree(parents, N_BIG, anchor)
    kept = kept_of(want)
    assert anchor >= 1100 and len(below) >= 600 and (want["new_id"][:anchor] == -1).all()
    lost = below - set(kept.tolist())
    assert len(lost - set(blocked)) >= 100 and len(kept) >= 100                  # dropped through a blocked ancestor
    assert want["n"] == len(kept) + 1 and want["new_id"][anchor] == 1 and want["new_id"][kept].min() == 1
    assert want["edge_nstates"][1] == 36 - ds and want["edge_nactions"][1] == 32 - da
    cnt[1] = int(kept[-1])                                                       # a goal node of the third trip, remapped
    want = R.rebase_ref(tt, cnt, maze, anchor, root, ds, da, collides=tab)
    assert kept[-1] >= 2048 and want["counters"][1] == want["new_id"][kept[-1]] > 0
    pair = big_pair if cost else Pair(ctx, cost=False, **BIG)
    want, got = run(pair, t, cnt, anchor, root, ds, da, maze=maze, collides=tab)
    if cost:                                                                     # cost = rows on the path
        rows = np.zeros(want["n"], dtype=np.int64)
        for i in range(want["n"]):
            rows[i] = (rows[want["parent"][i]] if i else 0) + want["edge_nstates"][i] + 1
        assert np.array_equal(want["cost"], rows) and np.array_equal(got["cost"][:want["n"]], rows)
        for i in (0, 1, want["n"] // 2, want["n"] - 1):
            assert got["cost"][i] == len(R.path_rows(want, i)[0])
        assert len(set(rows.tolist())) >= 10
    else:
        assert "cost" not in got and "cost" not in want


# ------------------------------------------------------------------------------------------------ B, D, F: short edges
SMALL = dict(cap=2048, nch=1, a=2)                         # 3 state rows, 2 action rows per edge


@functools.lru_cache(maxsize=None)
def tree_b():
    """Case B: 2048 nodes on ``shapes``; 1023 and 1024 are children of the root that the draw leaves clear."""
    maze = load_maze("shapes")
    rng = np.random.default_rng(1032)
    parents = window_parents(rng, 2048, 60)
    parents[1023] = parents[1024] = 0
    t, cnt = make_tree(parents, 1024, maze=maze, free_list=free_cells(maze), **SMALL)
    walls, blocked = wall_cells(maze), []
    pool = np.array([m for m in range(1, 2048) if m not in (1023, 1024)])
    for m in rng.choice(pool, 60, replace=False):
        row = int(rng.integers(0, 4))
        blocked.append((int(m), None if row == 3 else row))
        block(t, int(m), blocked[-1][1], maze, walls[rng.integers(len(walls))])
    return maze, t, cnt, blocked


@pytest.fixture(scope="module")
def small_pair(ctx):
    return Pair(ctx, **SMALL)


@pytest.mark.parametrize("n", [1023, 1024, 1025, 2047, 2048])
def test_b_trip_boundaries(small_pair, n):
    """The tree is the first n nodes of one 2048-node tree: src holds well-formed nodes behind counters[0], which are not part
    of it."""
    maze, t, cnt, blocked = tree_b()
    cnt = cnt.copy()
    cnt[0] = n
    tab = checked_table(t, n, maze, [b for b in blocked if b[0] < n])
    want = R.rebase_ref(t, cnt, maze, 0, collides=tab)
    kept = want["new_id"] >= 0
    assert want["status"] == 0 and 0.35 * n <= kept.sum() <= 0.65 * n            # about half
    for b in (1024, 2048):                                                       # both answers on both sides of a boundary
        for lo in (b - 64, b):
            part = kept[lo:min(lo + 64, n)]
            if len(part) >= 32:
                assert part.any() and not part.all(), (b, lo)
    run(small_pair, t, cnt, 0, maze=maze, collides=tab)


@pytest.mark.parametrize("n", [1025, 2048])
@pytest.mark.parametrize("gone", [1023, 1024])
def test_b_last_and_first_node_of_a_trip(small_pair, n, gone):
    maze, t, cnt, blocked = tree_b()
    t, cnt = copy_tree(t), cnt.copy()
    cnt[0] = n
    walls = wall_cells(maze)
    block(t, gone, None, maze, walls[len(walls) // 2])
    tab = checked_table(t, n, maze, [b for b in blocked if b[0] < n] + [(gone, None)])
    want = R.rebase_ref(t, cnt, maze, 0, collides=tab)
    stays = 1023 + 1024 - gone
    assert want["new_id"][gone] == -1 and want["new_id"][stays] >= 0
    if gone == 1023:                                                             # the carry into the second trip
        assert want["new_id"][1024] == (want["new_id"][:1023] >= 0).sum()
    run(small_pair, t, cnt, 0, maze=maze, collides=tab)


@functools.lru_cache(maxsize=None)
def tree_d(shape):
    maze = load_maze("shapes")
    parents = [-1] + (list(range(1499)) if shape == "chain" else [0] * 1499)
    t, cnt = make_tree(parents, 1500, maze=maze, free_list=free_cells(maze), **SMALL)
    return maze, t, cnt


@pytest.mark.parametrize("at,n_kept", [(None, 1500), (1400, 1400), (3, 3)])
def test_d_chain_of_1500(small_pair, at, n_kept):
    """Deeper than capacity / 2 = 1024 hops: node 1499 reaches the anchor only in the 11th and last pass, over six blocks."""
    maze, t, cnt = tree_d("chain")
    t = copy_tree(t)
    blocked = []
    if at is not None:
        blocked = [(at, 1)]
        block(t, at, 1, maze, wall_cells(maze)[40])
    tab = checked_table(t, 1500, maze, blocked)
    want = R.rebase_ref(t, cnt, maze, 0, collides=tab)
    assert want["n"] == n_kept and (want["new_id"][:n_kept] == np.arange(n_kept)).all() and (want["new_id"][n_kept:] == -1).all()
    run(small_pair, t, cnt, 0, maze=maze, collides=tab)


def test_d_star_of_1500(small_pair):
    maze, t, cnt = tree_d("star")
    t = copy_tree(t)
    blocked = [(m, None) for m in range(3, 1500, 3)]
    walls = wall_cells(maze)
    for k, (m, _) in enumerate(blocked):
        block(t, m, None, maze, walls[k % len(walls)])
    tab = checked_table(t, 1500, maze, blocked)
    want = R.rebase_ref(t, cnt, maze, 0, collides=tab)
    gone = np.array([m for m, _ in blocked])
    assert want["n"] == 1500 - len(gone) == 1001 and (want["new_id"][gone] == -1).all()
    run(small_pair, t, cnt, 0, maze=maze, collides=tab)


def far_cell(maze, r, c):
    """A cell that a map with swapped extents does not have: column >= rows on a wide map, row >= columns on a tall one."""
    H, W = maze.shape
    return c >= H if W > H else r >= W


MAPS = {"race_track_7x13": lambda: load_maze("Race_Track"), "shapes_21x24": lambda: load_maze("shapes"),
        "shapes_transposed_24x21": lambda: np.ascontiguousarray(load_maze("shapes").T)}


@pytest.mark.parametrize("name", list(MAPS))
def test_f_maps_that_are_not_square(ctx, name):
    maze = MAPS[name]()
    H, W = maze.shape
    assert H != W
    n = 300
    rng = np.random.default_rng(H * 100 + W)
    parents = window_parents(rng, n, 40)
    t, cnt = make_tree(parents, H * 100 + W, maze=maze, free_list=free_cells(maze), **SMALL)
    far_walls = [c for c in wall_cells(maze) if far_cell(maze, *c)]
    near_walls = [c for c in wall_cells(maze) if not far_cell(maze, *c)]
    blocked, on_far = [], []
    for k, m in enumerate(rng.choice(np.arange(60, n), 14, replace=False)):
        cells = far_walls if k < 8 else near_walls
        row = int(rng.integers(0, 4))
        blocked.append((int(m), None if row == 3 else row))
        block(t, int(m), blocked[-1][1], maze, cells[rng.integers(len(cells))])
        if k < 8:
            on_far.append(int(m))
    tab = checked_table(t, n, maze, blocked)
    tt = dict(t, obstacle_ahead=np.zeros(SMALL["cap"]))
    want = R.rebase_ref(tt, cnt, maze, 0, collides=tab)
    rows = np.concatenate([t["edge_states"][:n], t["state"][:n, None]], axis=1)            # (n, 4, 6); node 0's edge is unused
    rc = R.G.cell_xy_to_rowcol(rows[..., :2], maze).astype(int)
    far = np.vectorize(lambda r, c: far_cell(maze, r, c))(rc[..., 0], rc[..., 1])
    far[0, :3] = False
    kept = want["new_id"] >= 0
    assert far.sum() >= 30 and len(on_far) >= 5 and (far[kept].any(axis=1)).sum() >= 20
    assert all(want["new_id"][m] == -1 for m in on_far)
    flags = want["obstacle_ahead"]
    assert (flags == 0).sum() >= 10 and (flags == 1).sum() >= 10 and want["n"] >= 60 and (~kept).sum() >= 14
    pair = Pair(ctx, flags=True, **SMALL)
    want, got = run(pair, t, cnt, 0, maze=maze, collides=tab)
    again = ctx.obstacle_ahead(pair.dst.state[:want["n"]].contiguous()).cpu().numpy()       # the round's own flag kernel
    assert np.array_equal(got["obstacle_ahead"][1:want["n"]], again[1:])


# ------------------------------------------------------------------------------------------------ E: long edges
LONG = dict(cap=256, nch=16, a=8)                          # 144 state rows, 128 action rows per edge
N_LONG = 150
# node -> (chunks of its edge, its one blocked row; None: its own state).  ns = 9 chunks: rows 0..62, the state is row 63 of
# the row loop (the last lane of its first step); ns = 72: the state is row 72; ns = 144: row 144, the third step.
BLOCKS = {"row_0": (16, 0), "row_63": (8, 63), "row_64": (8, 64), "row_64_of_144": (16, 64), "row_128": (16, 128),
          "row_143": (16, 143), "row_62_of_63": (7, 62), "state_after_9": (1, None), "state_after_63": (7, None),
          "state_after_72": (8, None), "state_after_144": (16, None)}


@functools.lru_cache(maxsize=None)
def tree_e():
    """Case E on ``boxes``: node 1 (16 chunks) is the root's only child, everything else hangs below it; edges of 1, 7, 8 and 16
    chunks in turn.  One node per entry of BLOCKS, each with descendants and none below another."""
    maze = load_maze("boxes")
    rng = np.random.default_rng(144)
    parents = [-1, 0] + [int(rng.integers(max(1, m - 12), m)) for m in range(2, N_LONG)]
    chunks = {m: (1, 7, 8, 16)[m % 4] for m in range(1, N_LONG)}
    chunks[1] = 16
    nodes, taken = {}, set()
    for name, (c, _) in BLOCKS.items():
        for m in range(20, N_LONG):
            sub = subtree(parents, N_LONG, m)
            up = set()
            k = m
            while k >= 0:
                up.add(k)
                k = parents[k]
            if chunks[m] == c and 3 <= len(sub) <= 12 and not (sub | up) & taken:
                nodes[name] = m
                taken |= sub
                break
    assert len(nodes) == len(BLOCKS)
    t, cnt = make_tree(parents, 144, maze=maze, free_list=free_cells(maze), chunks=chunks, **LONG)
    return maze, t, cnt, parents, nodes


@pytest.fixture(scope="module")
def long_pair(ctx):
    return Pair(ctx, **LONG)


def test_e_long_edges_copy(long_pair):
    maze, t, cnt, parents, nodes = tree_e()
    tab = checked_table(t, N_LONG, maze, [])
    want = R.rebase_ref(t, cnt, maze, 0, collides=tab)
    assert want["n"] == N_LONG and sorted(set(want["edge_nstates"][1:].tolist())) == [9, 63, 72, 144]
    assert sorted(set(want["edge_nactions"][1:].tolist())) == [8, 56, 64, 128]
    run(long_pair, t, cnt, 0, maze=maze, collides=tab)


@pytest.mark.parametrize("name", list(BLOCKS))
def test_e_one_blocked_row_takes_the_subtree_and_nothing_else(long_pair, name):
    maze, t, cnt, parents, nodes = tree_e()
    t = copy_tree(t)
    m, (c, row) = nodes[name], BLOCKS[name]
    assert t["edge_nstates"][m] == c * 9 and (row is None or row < c * 9)
    block(t, m, row, maze, wall_cells(maze)[len(wall_cells(maze)) // 3])
    tab = checked_table(t, N_LONG, maze, [(m, row)])
    want = R.rebase_ref(t, cnt, maze, 0, collides=tab)
    gone = subtree(parents, N_LONG, m)
    assert len(gone) >= 3 and set(np.flatnonzero(want["new_id"] < 0).tolist()) == gone and want["n"] == N_LONG - len(gone)
    run(long_pair, t, cnt, 0, maze=maze, collides=tab)


@pytest.mark.parametrize("wall_row,n_new", [(69, N_LONG), (70, 1)], ids=["wall_in_the_dropped_rows", "wall_in_the_kept_rows"])
def test_e_fresh_root_70_rows_into_a_144_row_edge(long_pair, wall_row, n_new):
    maze, t, cnt, parents, nodes = tree_e()
    t = copy_tree(t)
    ds, da = 70, 62                                       # 62 actions: 7 whole chunks of 9 rows, 6 into the next, the car's row
    assert t["edge_nstates"][1] == 144 and t["edge_nactions"][1] == 128
    block(t, 1, wall_row, maze, wall_cells(maze)[len(wall_cells(maze)) // 3])
    tab = checked_table(t, N_LONG, maze, [(1, wall_row)])
    fc = free_cells(maze)
    root = R.cell_state(maze, *fc[7], -2.0, 0.05, 0.15)
    want = R.rebase_ref(t, cnt, maze, 1, root, ds, da, collides=tab)
    assert want["status"] == 0 and want["n"] == n_new
    if n_new > 1:                                         # all of the old tree but its root; the anchor keeps 74 and 66 rows
        assert want["edge_nstates"][1] == 74 and want["edge_nactions"][1] == 66
        assert (want["new_id"][1:] == np.arange(1, N_LONG)).all()
    else:
        assert (want["new_id"] == -1).all()
    run(long_pair, t, cnt, 1, root, ds, da, maze=maze, collides=tab)


# ------------------------------------------------------------------------------------------------ G: the engine's tree swap
G_CAP, G_BATCH, G_EDGE, G_A = 4096, 512, 32, 8
G_ROUNDS = (1, 2, 8, 32, 128, 512, 512)                    # the first candidate alone: most of the tree hangs below one node


def grown_planner():
    """``RRT_Planner(reuse_tree=True)`` on ``boxes`` with the default 4 x 8 edge at capacity 4096, its tree grown by action-tape
    rounds (no network) of growing size towards samples in free cells, until it holds more than 1100 nodes."""
    from ditreeonlineplanner_amd.car_env import CarEnv
    from ditreeonlineplanner_amd.planners.RRT import RRT_Planner
    from tests.test_gpu_tree_reuse import Tape
    maze = load_maze("boxes")
    env = CarEnv(maze_map=maze, collision_checking=False)
    start = np.array([*env.cell_rowcol_to_xy(np.array([18, 8])), 0.0, 0.0, 0.0, 0.0])
    goal = np.array([*env.cell_rowcol_to_xy(np.array([1, 1])), 0, 0, 0, 0.0])
    pl = RRT_Planner(start, goal, env_id="carmaze", environment=env, sampler=Tape(), action_horizon=G_A, local_map_size=20,
                     local_map_scale=0.2, global_map_scale=1.0, goal_conditioning_bias=0.85, prop_duration=[G_EDGE],
                     time_budget=600, batch=G_BATCH, max_candidates=8 * G_BATCH, capacity=G_CAP, emulate_sticky_done=False,
                     reuse_tree=True, solution="anytime")
    eng = pl._engine
    rng = np.random.default_rng(4096)
    fc = np.array(free_cells(maze))
    first = 0
    for k in range(16):                                    # candidates that collide add no node: rounds of 512 until it is enough
        if eng.tree.n_nodes_host > 1100:
            break
        B = G_ROUNDS[min(k, len(G_ROUNDS) - 1)]
        s = np.zeros((B, 6))
        s[:, :2] = R.G.cell_rowcol_to_xy(fc[rng.integers(len(fc), size=B)], maze) + rng.uniform(-0.4, 0.4, (B, 2))
        eng.expand_round(dev(s), dev(s[:, :2].copy()), inject_actions=dev(Tape().sample_round(first, B, G_EDGE // G_A, eng.P)))
        first += B
    return pl, maze, start, goal


def restated(before, counters, maze, anchor, ds, da, car):
    """tests.test_gpu_tree_reuse.restate with the collision table in place of the row loop."""
    n = int(counters[0])
    tab = checked_table(before, n, maze, None)
    want = R.rebase_ref(before, counters, maze, anchor, car if ds > 0 else None, ds, da, collides=tab)
    if ds == 0:                                            # the car's real state becomes the root, not the planned row
        want["state"][0], want["xy"][0] = car, car[:2]
    return want


def wall_across(before, counters, maze, anchor, ds, da, car, below):
    """``maze`` with free cells walled one at a time -- the cells under the states of the anchor's descendants, from the oldest
    on -- keeping a cell when the restatement still keeps 100 nodes and 40 % of the subtree with it, until it drops 100 nodes
    and a quarter of the subtree.  The choice looks at the restatement alone."""
    n = int(counters[0])
    walled, tried = maze.copy(), set()
    for m in sorted(below - {anchor}):
        cell = tuple(int(v) for v in R.G.cell_xy_to_rowcol(before["state"][m, :2], maze))
        if cell in tried:
            continue
        tried.add(cell)
        trial = walled.copy()
        trial[cell] = 1
        want = R.rebase_ref(before, counters, trial, anchor, car if ds > 0 else None, ds, da,
                            collides=R.collision_table(before, n, trial))
        kept = int((want["new_id"] >= 0).sum())
        if kept >= max(100, 0.4 * len(below)):
            walled = trial
            if len(below) - kept >= max(100, 0.25 * len(below)):
                return walled
    raise AssertionError("no wall found that splits the subtree")


@pytest.mark.parametrize("where", ["as_the_root", "inside_an_edge"])
def test_g_engine_rebases_a_grown_tree_twice(where):
    from ditreeonlineplanner_amd.engine import ExpansionEngine
    from tests.test_gpu_tree_reuse import FIELDS, Tape, assert_tree_is, read_tree
    pl, maze, start, goal = grown_planner()
    eng = pl._engine
    before, counters = read_tree(eng)
    n0 = int(counters[0])
    assert n0 > 1100 and n0 == eng.tree.n_nodes_host and before["edge_states"].shape[1:] == (36, 6)
    # the "plan": the chain from the root through its child with the most descendants to the deepest node below that; the car
    # has left the root for this child
    depth, size = np.zeros(n0, dtype=int), np.ones(n0, dtype=int)
    for m in range(1, n0):
        depth[m] = depth[before["parent"][m]] + 1
    for m in range(n0 - 1, 0, -1):
        size[before["parent"][m]] += size[m]
    anchor = int(max(np.flatnonzero(depth == 1), key=lambda m: size[m]))
    below = subtree(before["parent"], n0, anchor)
    chain = [int(max(below, key=lambda m: depth[m]))]
    while chain[-1] > 0:
        chain.append(int(before["parent"][chain[-1]]))
    assert chain[-2] == anchor and len(chain) >= 4 and len(below) == size[anchor] >= 300
    assert before["edge_nstates"][anchor] == 36 and before["edge_nactions"][anchor] == 32
    if where == "as_the_root":
        ds, da = 0, 0
        car = before["state"][anchor] + np.array([1e-4, -1e-4, 1e-4, 0, 0, 0])
    else:
        ds, da = 13, 11                                    # 11 actions: one whole chunk of 9 rows, 3 into the next, the car's row
        car = before["edge_states"][anchor, ds - 1] + np.array([1e-4, -1e-4, 1e-4, 0, 0, 0])
    walled = wall_across(before, counters, maze, anchor, ds, da, car, below)
    want = restated(before, counters, walled, anchor, ds, da, car)
    kept = kept_of(want)
    assert want["status"] == 0 and len(kept) >= 100 and len(below) - len(kept) >= 100 and n0 - len(kept) >= 100
    assert (walled != maze).sum() >= 1 and want["n"] == len(kept) + (ds > 0)
    print(f"{where}: {n0} nodes, anchor {anchor} with {len(below)} below it, {len(kept)} kept, {n0 - len(kept)} dropped")
    pl.update_maze(walled)                                 # the planner's own maze update
    got = eng.rebase(anchor, root_state=car, drop_states=ds, drop_actions=da)
    assert got == (len(kept), n0 - len(kept)) and eng.tree.n_nodes_host == want["n"]
    assert_tree_is(eng, want)
    assert np.array_equal(eng.rebase_ids[:n0].cpu().numpy(), want["new_id"])
    # the second re-base: the spare tree is the first one, whole and stale
    now, counters1 = read_tree(eng)
    n1 = int(counters1[0])
    sizes = np.ones(n1, dtype=int)
    for m in range(n1 - 1, 0, -1):
        sizes[now["parent"][m]] += sizes[m]
    second = int(min(range(1, n1), key=lambda m: abs(2 * sizes[m] - n1)))                  # the subtree nearest to half the tree
    car2 = now["state"][second] + np.array([-1e-4, 1e-4, 0, 0, 0, 0])
    want2 = restated(now, counters1, walled, second, 0, 0, car2)
    assert want2["n"] >= 50 and n1 - want2["n"] >= 50 and float(eng._spare_tree.xy[:n0].abs().sum()) > 0
    print(f"second re-base: {n1} nodes, anchor {second}, {want2['n']} kept")
    got2 = eng.rebase(second, root_state=car2)
    n2 = want2["n"]
    assert got2 == (n2, n1 - n2) and eng.tree.n_nodes_host == n2
    assert_tree_is(eng, want2)
    assert float(eng.tree.xy[n2:n0].abs().sum()) > 0                             # stale slots behind the tree
    # one round on it against the same round of a fresh engine that holds the restatement's arrays and nothing else
    other = ExpansionEngine(pl.ctx, walled, car2, goal, edge_length=G_EDGE, action_horizon=G_A, pred_horizon=eng.P,
                            local_map_size=eng.lm_n, local_map_scale=eng.lm_scale, s_global=eng.s_global, batch=G_BATCH,
                            capacity=G_CAP, emulate_sticky_done=False, early_exit=bool(eng.early_exit), goal_scale=eng.goal_scale,
                            prop_duration=[G_EDGE], solution="anytime")
    other.env_goal = eng.env_goal.copy()
    t = other.tree
    for name in ("state", "xy", "parent", "last_action", "has_prev", "num_visit", "edge_nstates", "edge_nactions", "cost"):
        getattr(t, name)[:n2].copy_(dev(want2[name]).to(getattr(t, name).dtype))
    es = np.zeros((n2, 36, 6))
    ea = np.zeros((n2, 32, 2))
    for i in range(n2):
        es[i, :want2["edge_nstates"][i]], ea[i, :want2["edge_nactions"][i]] = want2["edge_states"][i], want2["edge_actions"][i]
    t.edge_states[:n2].copy_(dev(es))
    t.edge_actions[:n2].copy_(dev(ea))
    t.counters.copy_(dev(want2["counters"]).to(torch.int32))
    t.n_nodes_host = n2
    rng = np.random.default_rng(5)
    s = np.zeros((G_BATCH, 6))
    s[:, :2] = now["state"][rng.integers(n1, size=G_BATCH), :2] + rng.uniform(-1, 1, (G_BATCH, 2))
    acts = dev(Tape().sample_round(10 ** 6, G_BATCH, G_EDGE // G_A, eng.P))
    rounds = []
    for e in (eng, other):
        cnt = e.expand_round(dev(s), dev(s[:, :2].copy()), inject_actions=acts)
        rb = e.rb
        rounds.append(dict(cnt=np.asarray(cnt).copy(), status=rb.status[:G_BATCH].cpu().numpy(),
                           parent=rb.parent[:G_BATCH].cpu().numpy(), node_id=rb.node_id[:G_BATCH].cpu().numpy(),
                           tree=read_tree(e)[0]))
    a, b = rounds
    assert np.array_equal(a["cnt"], b["cnt"]) and a["cnt"][0] > n2          # nodes were appended
    for name in ("status", "parent", "node_id"):
        assert np.array_equal(a[name], b[name]), name
    assert (a["parent"] < n2).all() and len(set(a["parent"].tolist())) >= 3
    for name in FIELDS + ("cost",):
        x, y = a["tree"][name], b["tree"][name]
        if name in ("edge_states", "edge_actions"):
            counts = a["tree"]["edge_nstates" if name == "edge_states" else "edge_nactions"]
            assert all(np.array_equal(x[i, :counts[i]], y[i, :counts[i]]) for i in range(len(x))), name
        else:
            assert np.array_equal(x, y), name
