"""GPU: ditree_tree_rebase (rebase_valid_kernel, rebase_keep_pass_kernel, rebase_scan_kernel, rebase_move_kernel) against the
numpy restatement of tests/tree_rebase_ref.py, on trees written straight into the device arrays: capacity 64, 2 chunks at
A = 2, an 8 x 8 maze with a border and two inner walls, states placed by hand in free and occupied cells.  Every comparison is
exact, over the kept slots of every array and all 8 counters; every case first asserts on the restatement's own output how
many nodes survive and how many go."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import tree_rebase_ref as R
from tests.test_gpu_forest import ctx, dev  # noqa: F401

pytestmark = pytest.mark.gpu

CAP, NCH, A, S, D = 64, 2, 2, 6, 2
ES, EA = NCH * (A + 1), NCH * A
MAZE = R.maze8()
FREE = [(r, c) for r in range(1, 7) for c in range(1, 7) if MAZE[r, c] == 0]
WALL = R.cell_state(MAZE, 2, 3)
ARRAYS = ("state", "xy", "parent", "last_action", "has_prev", "num_visit", "edge_states", "edge_actions", "edge_nstates",
          "edge_nactions", "obstacle_ahead", "edge_owner", "cost")
SENTINEL = 77


def free_cells(maze):
    """The free cells off the map's border, in row-major order."""
    return [(r, c) for r in range(1, maze.shape[0] - 1) for c in range(1, maze.shape[1] - 1) if maze[r, c] == 0]


def make_tree(parents, seed=0, short=(), cap=CAP, nch=NCH, a=A, maze=MAZE, free_list=FREE, chunks=None):
    """Host arrays of a tree with the given parents (parent < child): every state and edge row in a free cell, whole edges of
    ``nch`` chunks (``short``: nodes with one chunk; ``chunks``: node -> its number of chunks), random actions, visits and a
    cost column that counts path rows.  The defaults are the module's shape: capacity 64, 2 chunks at A = 2, the 8 x 8 maze."""
    rng = np.random.default_rng(seed)
    n = len(parents)
    es, ea = nch * (a + 1), nch * a

    def free():
        r, c = free_list[rng.integers(len(free_list))]
        return R.cell_state(maze, r, c, rng.uniform(-np.pi, np.pi), *rng.uniform(-0.2, 0.2, 2))

    t = dict(state=np.zeros((cap, S)), parent=np.full(cap, -1, dtype=np.int32), last_action=np.zeros((cap, D)),
             has_prev=np.zeros(cap, dtype=np.uint8), num_visit=np.zeros(cap, dtype=np.int32), edge_states=np.zeros((cap, es, S)),
             edge_actions=np.zeros((cap, ea, D)), edge_nstates=np.zeros(cap, dtype=np.int32),
             edge_nactions=np.zeros(cap, dtype=np.int32), cost=np.zeros(cap, dtype=np.int32),
             edge_owner=np.full(cap, -1, dtype=np.int32))
    for m in range(n):
        t["parent"][m] = parents[m]
        t["state"][m] = free()
        t["num_visit"][m] = rng.integers(0, 5)
        t["cost"][m] = 1
        if m:
            c = chunks[m] if chunks is not None and m in chunks else 1 if m in short else nch
            t["edge_nstates"][m], t["edge_nactions"][m] = c * (a + 1), c * a
            t["edge_states"][m, :c * (a + 1)] = [free() for _ in range(c * (a + 1))]
            t["edge_actions"][m, :c * a] = rng.uniform(-1, 1, (c * a, D))
            t["last_action"][m], t["has_prev"][m] = t["edge_actions"][m, c * a - 1], 1
            t["cost"][m] = t["cost"][parents[m]] + c * (a + 1) + 1
    t["xy"] = t["state"][:, :2].copy()
    return t, np.array([n, -1, 1, 40, 50, 1, 1, 3], dtype=np.int32)


class Pair:
    """Two device trees of the shape under test and the call's scratch."""

    def __init__(self, ctx, cost=True, flags=False, cap_dst=None, cap=CAP, nch=NCH, a=A):
        from ditreeonlineplanner_amd.engine import DeviceTree
        self.ctx, self.cap = ctx, cap
        self.src = DeviceTree(ctx, cap, nch, a, track_obstacle_ahead=flags, cost=cost)
        self.dst = DeviceTree(ctx, cap if cap_dst is None else cap_dst, nch, a, track_obstacle_ahead=flags, cost=cost)
        self.scratch = torch.zeros(3 * cap, dtype=torch.int32, device=ctx.device)

    def upload(self, t, counters):
        for name in ARRAYS:
            a, b = getattr(self.src, name, None), getattr(self.dst, name, None)
            if a is not None:
                a.copy_(dev(t[name] if name in t else np.zeros(self.cap)).to(a.dtype).reshape(a.shape))
                b.fill_(SENTINEL)
        self.src._cnt_buf[:8].copy_(dev(counters))
        self.dst._cnt_buf[:8].fill_(SENTINEL)

    def call(self, anchor, root=None, ds=0, da=0, cost="both", scratch="own", src=None, dst=None, ctx=None):
        from ditreeonlineplanner_amd import _lib
        ctx = ctx or self.ctx
        r = None if root is None else np.ascontiguousarray(root, dtype=np.float64)
        rp = None if r is None else r.ctypes.data_as(C.POINTER(C.c_double))
        has = self.src.cost is not None
        cs, cd = (self.src.cost.data_ptr(), self.dst.cost.data_ptr()) if has and cost in ("both", "src") else (None, None)
        if cost == "src":
            cd = None
        rc = _lib.lib().ditree_tree_rebase(ctx._h, C.byref((src or self.src).desc), C.byref((dst or self.dst).desc), anchor, rp, ds,
                                           da, cs, cd, self.scratch.data_ptr() if scratch == "own" else None, ctx.stream)
        _lib.check(ctx._h, rc, "tree_rebase")

    def read(self, tree):
        return {name: getattr(tree, name).cpu().numpy() for name in ARRAYS if getattr(tree, name, None) is not None}


def run(pair, t, counters, anchor, root=None, ds=0, da=0, maze=MAZE, collides=None):
    """Upload, call, and compare dst with the restatement over its n slots; src must come back as it went in.  ``collides``:
    the restatement's collision table (tests.tree_rebase_ref.collision_table) in place of its row loop."""
    pair.ctx.upload_maze(maze)
    pair.upload(t, counters)
    tt = dict(t)
    if pair.src.cost is None:
        tt.pop("cost")
    if pair.src.obstacle_ahead is not None:
        tt["obstacle_ahead"] = np.zeros(pair.cap)
    want = R.rebase_ref(tt, counters, maze, anchor, root, ds, da, collides)
    before = pair.read(pair.src)
    pair.call(anchor, root, ds, da)
    got, cnt = pair.read(pair.dst), pair.dst._cnt_buf[:8].cpu().numpy()
    after = pair.read(pair.src)
    for name in before:
        assert np.array_equal(before[name], after[name], equal_nan=True), name
    assert np.array_equal(pair.src._cnt_buf[:8].cpu().numpy(), counters)
    if want["status"] != 0:
        assert cnt[0] == want["status"] and (cnt[1:] == SENTINEL).all()
        for name in got:
            assert (got[name] == SENTINEL).all(), name
        return want, got
    assert np.array_equal(cnt, want["counters"]), (cnt, want["counters"])
    n = want["n"]
    for name in ("state", "xy", "parent", "last_action", "has_prev", "num_visit", "edge_nstates", "edge_nactions", "cost",
                 "obstacle_ahead"):
        if name in got:
            assert np.array_equal(got[name][:n], want[name], equal_nan=True), (name, got[name][:n], want[name])
    for i in range(n):
        assert np.array_equal(got["edge_states"][i, :want["edge_nstates"][i]], want["edge_states"][i], equal_nan=True), i
        assert np.array_equal(got["edge_actions"][i, :want["edge_nactions"][i]], want["edge_actions"][i]), i
    assert (got["edge_owner"][:n] == -1).all()
    for name in got:                                     # nothing is written behind the kept slots
        assert (got[name][n:] == SENTINEL).all(), name
    ids = pair.scratch[2 * pair.cap: 2 * pair.cap + counters[0]].cpu().numpy()
    assert np.array_equal(ids, want["new_id"])
    return want, got


@pytest.fixture(scope="module")
def pair(ctx):
    return Pair(ctx)


#            0   1  2  3  4  5  6  7  8  9 10 11
BUSHY = [-1, 0, 0, 1, 1, 2, 3, 3, 4, 5, 6, 8]


def test_a_anchor_root_nothing_blocked_is_a_copy(pair):
    t, cnt = make_tree(BUSHY, 1, short=(4, 9))
    want, got = run(pair, t, cnt, 0)
    assert want["n"] == 12 and list(want["new_id"]) == list(range(12))
    src = pair.read(pair.src)
    for name in ("state", "xy", "parent", "last_action", "has_prev", "num_visit", "edge_nstates", "edge_nactions", "cost"):
        assert np.array_equal(got[name][:12], src[name][:12]), name
    for m in range(12):
        assert np.array_equal(got["edge_states"][m, :src["edge_nstates"][m]], src["edge_states"][m, :src["edge_nstates"][m]])
        assert np.array_equal(got["edge_actions"][m, :src["edge_nactions"][m]], src["edge_actions"][m, :src["edge_nactions"][m]])


def test_b_anchor_in_mid_tree_drops_siblings_and_ancestors(pair):
    t, cnt = make_tree(BUSHY, 2)
    want, _ = run(pair, t, cnt, 3)
    assert want["n"] == 4 and [m for m in range(12) if want["new_id"][m] >= 0] == [3, 6, 7, 10]
    assert list(want["parent"]) == [-1, 0, 0, 1] and want["edge_nstates"][0] == 0 and want["has_prev"][0] == 0
    assert want["num_visit"][0] == t["num_visit"][3]


def test_c_fresh_root_inside_the_anchors_edge(pair):
    t, cnt = make_tree(BUSHY, 3)
    root = R.cell_state(MAZE, 6, 1, 0.7, 0.1, -0.1)
    want, _ = run(pair, t, cnt, 1, root, 2, 1)
    assert want["n"] == 9 and (want["new_id"][[0, 2, 5, 9]] == -1).all() and want["new_id"][1] == 1
    assert want["edge_nstates"][1] == ES - 2 and want["edge_nactions"][1] == EA - 1 and want["num_visit"][0] == 0
    assert np.array_equal(want["state"][0], root) and list(want["parent"][:2]) == [-1, 0]


def test_d_blocked_edge_takes_its_whole_subtree(pair):
    #          0  1  2  3  4  5  6  7  8  9
    parents = [-1, 0, 1, 2, 3, 3, 4, 5, 6, 1]            # 3 is blocked in mid-chain; 4 5 6 7 8 hang behind it
    t, cnt = make_tree(parents, 4)
    t["edge_states"][3, 4] = WALL
    want, _ = run(pair, t, cnt, 0)
    assert want["n"] == 4 and [m for m in range(10) if want["new_id"][m] < 0] == [3, 4, 5, 6, 7, 8]


def test_e_collision_among_the_dropped_rows_does_not_block(pair):
    t, cnt = make_tree(BUSHY, 5)
    t["edge_states"][1, 1] = WALL                        # the car has driven past it
    root = R.cell_state(MAZE, 6, 1)
    want, _ = run(pair, t, cnt, 1, root, 2, 0)
    assert want["n"] == 9
    want, _ = run(pair, t, cnt, 1, root, 1, 0)           # one row less dropped: now it counts
    assert want["n"] == 1


def test_f_blocked_remainder_of_the_anchors_edge_leaves_the_root(pair):
    t, cnt = make_tree(BUSHY, 6)
    t["edge_states"][1, 4] = WALL
    root = R.cell_state(MAZE, 6, 1)
    want, got = run(pair, t, cnt, 1, root, 2, 1)
    assert want["n"] == 1 and (want["new_id"] == -1).all() and list(want["counters"]) == [1, -1, 0, 0, 0, 0, 0, -1]
    # the anchor as the root: a colliding pose keeps the root alone
    t, cnt = make_tree(BUSHY, 6)
    t["state"][3] = WALL
    t["xy"][3] = WALL[:2]
    want, _ = run(pair, t, cnt, 3)
    assert want["n"] == 1 and want["new_id"][3] == 0


def test_g_nan_row_counts_as_blocked(pair):
    t, cnt = make_tree(BUSHY, 7)
    t["edge_states"][4, 2, 0] = np.nan
    t["state"][7, 2] = np.nan
    want, _ = run(pair, t, cnt, 0)
    assert [m for m in range(12) if want["new_id"][m] < 0] == [4, 7, 8, 11] and want["n"] == 8


def test_h_goal_node_remapped_then_lost(pair):
    t, cnt = make_tree(BUSHY, 8)
    cnt[1] = 10
    want, _ = run(pair, t, cnt, 3)
    assert want["counters"][1] == 3 and want["n"] == 4
    t["state"][6] = WALL
    t["xy"][6] = WALL[:2]
    want, _ = run(pair, t, cnt, 3)
    assert want["counters"][1] == -1 and want["n"] == 2
    cnt[1] = 2                                           # a goal node outside the subtree
    want, _ = run(pair, t, cnt, 3)
    assert want["counters"][1] == -1


def test_i_chain_of_48_and_star_of_48(pair):
    t, cnt = make_tree([-1] + list(range(47)), 9)
    want, _ = run(pair, t, cnt, 0)
    assert want["n"] == 48
    t["edge_states"][40, 0] = WALL                       # near the deep end: 8 nodes go
    want, _ = run(pair, t, cnt, 1, R.cell_state(MAZE, 6, 1), 3, 2)
    assert want["n"] == 40 and (want["new_id"][40:] == -1).all()
    t, cnt = make_tree([-1] + [0] * 47, 10)
    t["state"][20] = WALL
    t["xy"][20] = WALL[:2]
    want, _ = run(pair, t, cnt, 0)
    assert want["n"] == 47 and want["new_id"][20] == -1 and want["new_id"][47] == 46


def test_j_full_tree(pair):
    rng = np.random.default_rng(11)
    parents = [-1] + [int(rng.integers(0, m)) for m in range(1, CAP)]
    t, cnt = make_tree(parents, 11)
    for m in (9, 30, 55):
        t["edge_states"][m, 3] = WALL
    assert cnt[0] == CAP
    want, _ = run(pair, t, cnt, 0)
    assert 1 < want["n"] < CAP
    anchor = next(m for m in range(1, CAP) if parents.count(m) >= 2 and m not in (9, 30, 55))
    want, _ = run(pair, t, cnt, anchor, R.cell_state(MAZE, 6, 1), 1, 0)
    assert 2 <= want["n"] <= CAP and want["new_id"][anchor] == 1


def test_k_cost_column_is_the_rows_of_the_path(pair):
    from ditreeonlineplanner_amd.engine import tree_path
    t, cnt = make_tree(BUSHY, 12, short=(3, 8))
    for anchor, root, ds, da in ((1, None, 0, 0), (1, R.cell_state(MAZE, 6, 1), 4, 2), (3, R.cell_state(MAZE, 6, 1), 1, 0)):
        want, got = run(pair, t, cnt, anchor, root, ds, da)
        assert want["n"] >= 4 and len(set(want["cost"])) >= 3
        for i in range(want["n"]):
            path, _ = tree_path(pair.dst, i, want["n"])
            assert got["cost"][i] == len(path) == len(R.path_rows(want, i)[0])


def test_k_without_a_cost_column(ctx):
    p = Pair(ctx, cost=False)
    t, cnt = make_tree(BUSHY, 13)
    want, got = run(p, t, cnt, 2)
    assert want["n"] == 3 and "cost" not in got


def test_l_obstacle_flags_follow_the_current_maze(ctx):
    p = Pair(ctx, cost=False, flags=True)
    t, cnt = make_tree(BUSHY + [0] * 20, 14)
    want, got = run(p, t, cnt, 0)
    n = want["n"]
    assert n == 32 and {0, 1} <= set(want["obstacle_ahead"][1:]) and want["obstacle_ahead"][0] == 0
    flags = ctx.obstacle_ahead(p.dst.state[:n].contiguous()).cpu().numpy()
    assert np.array_equal(got["obstacle_ahead"][1:n], flags[1:]) and got["obstacle_ahead"][0] == 0
    # another map, other flags: they are evaluated, not copied
    maze2 = MAZE.copy()
    maze2[2, 2] = maze2[2, 3] = maze2[4, 5] = maze2[5, 5] = 0
    want2, got2 = run(p, t, cnt, 0, maze=maze2)
    assert want2["n"] == 32 and not np.array_equal(want2["obstacle_ahead"], want["obstacle_ahead"])
    flags2 = ctx.obstacle_ahead(p.dst.state[:32].contiguous()).cpu().numpy()
    assert np.array_equal(got2["obstacle_ahead"][1:32], flags2[1:])


@pytest.mark.parametrize("anchor,ds,da,status", [(1, ES, 0, R.E_DROP), (1, 0, 0, R.E_DROP), (1, 1, EA, R.E_DROP), (1, 1, -1, R.E_DROP),
                                                 (0, 1, 0, R.E_DROP), (4, 4, 0, R.E_DROP), (12, 1, 0, R.E_ANCHOR)])
def test_m_drop_counts_are_checked_on_the_device(pair, anchor, ds, da, status):
    t, cnt = make_tree(BUSHY, 15, short=(4,))
    want, _ = run(pair, t, cnt, anchor, R.cell_state(MAZE, 6, 1), ds, da)
    assert want["status"] == status


def test_m_anchor_past_the_nodes_without_a_root_state(pair):
    t, cnt = make_tree(BUSHY, 15)
    want, _ = run(pair, t, cnt, 12)
    assert want["status"] == R.E_ANCHOR


def test_n_host_side_refusals(ctx, pair):
    from ditreeonlineplanner_amd._lib import DitreeError
    from ditreeonlineplanner_amd.engine import DeviceTree
    from ditreeonlineplanner_amd.ops import Context
    t, cnt = make_tree(BUSHY, 16)
    ctx.upload_maze(MAZE)
    pair.upload(t, cnt)
    root = R.cell_state(MAZE, 6, 1)
    ant = DeviceTree(ctx, CAP, NCH, A, state_dim=29, action_dim=8, hist=True)
    with pytest.raises(DitreeError, match="tree_rebase: the car"):
        pair.call(0, src=ant, dst=DeviceTree(ctx, CAP, NCH, A, state_dim=29, action_dim=8, hist=True))
    with pytest.raises(DitreeError, match="tree_rebase: src and dst share a buffer"):
        pair.call(0, dst=pair.src)
    with pytest.raises(DitreeError, match="tree_rebase: src and dst differ in shape"):
        pair.call(0, dst=DeviceTree(ctx, CAP, NCH, 4, cost=True))
    with pytest.raises(DitreeError, match="tree_rebase: dst->capacity below src->capacity"):
        pair.call(0, dst=DeviceTree(ctx, CAP // 2, NCH, A, cost=True))
    with pytest.raises(DitreeError, match="tree_rebase: obstacle_ahead in one tree only"):
        pair.call(0, dst=DeviceTree(ctx, CAP, NCH, A, track_obstacle_ahead=True, cost=True))
    for anchor in (-1, CAP):
        with pytest.raises(DitreeError, match="tree_rebase: anchor out of range"):
            pair.call(anchor)
    with pytest.raises(DitreeError, match="tree_rebase: drop counts belong to a root_state"):
        pair.call(1, None, 1, 0)
    with pytest.raises(DitreeError, match="tree_rebase: cost_src and cost_dst come together"):
        pair.call(0, cost="src")
    with pytest.raises(DitreeError, match="tree_rebase: scratch missing"):
        pair.call(0, scratch=None)
    bare = Context(0)
    try:
        with pytest.raises(DitreeError, match="tree_rebase: no maze uploaded"):
            pair.call(1, root, 2, 1, ctx=bare)
    finally:
        bare.close()
    # nothing was launched: dst is as it was uploaded
    assert all((a == SENTINEL).all() for a in pair.read(pair.dst).values()) and (pair.dst._cnt_buf[:8] == SENTINEL).all()
