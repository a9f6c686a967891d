"""GPU: ditree_accept_sparse / ditree_forest_accept_sparse / ditree_sparse_rebuild (sparse_cost_kernel, the SPARSE scan, the
rebuild kernels) against the sequential restatement of tests/sparse_tree_ref.py, on rounds written straight into the device
arrays in the manner of tests/test_gpu_accept_best.py.  Round sizes around the wave and around the scan's 1 024-wide pass, trees
of 1 and about 3 000 nodes, all candidates in one cell, every candidate in a cell of its own, a winner ranked past the capacity,
both accept rules (best, and bounded with an incumbent, where bound-pruned rows come before the grid), a forest with an empty
range, and the rebuild after a re-base.  Every comparison is exact: node ids, whole counter and stats rows, cost, key, every tree
array, the active column, the table and the contender words."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import sparse_tree_ref as SR
from tests.accept_best_ref import COLLIDED, GAC, GOAL, OK
from tests.sparse_tree_ref import EMPTY, NO_BOUND, active_ref, cell_ref, grid_ref, sparse_accept_ref
from tests.test_gpu_accept_best import TREE_FIELDS, random_rows, random_tree_state, upload_round, upload_tree
from tests.test_gpu_forest import ctx, dev, scenario  # noqa: F401

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 2049]
TREES = [1, 3000]
CAP = 5200                                                   # room for the 3 000-node tree and the 2 049-candidate round
GRID = grid_ref(8, 8, 1.0, 0.25, 4)                          # 32 x 32 x 4 = 4 096 cells: one for every candidate of a round
CASES = ["best", "bounded", "one_cell", "own_cells", "capacity"]
GOAL_XY, RADIUS, REACH = np.array([0.5, 0.5]), 0.5, 1.0


def engine(ctx, solution, **kw):
    from ditreeonlineplanner_amd.engine import ExpansionEngine
    maze, start, goal = scenario()
    return ExpansionEngine(ctx, maze, start, goal, edge_length=16, action_horizon=8, batch=2049, capacity=CAP,
                           emulate_sticky_done=False, solution=solution, sparse_cell=0.5, **kw)


@pytest.fixture(scope="module")
def best(ctx):
    return engine(ctx, "anytime")


@pytest.fixture(scope="module")
def pruned(ctx):
    return engine(ctx, "anytime_pruned", reach=REACH)


def compare_tree(tree, counters, rb, host, rnd, B, fields):
    """tests/test_gpu_accept_best.compare_tree on bit patterns: the synthetic states hold NaN and inf rows."""
    got = counters.cpu().numpy().reshape(host["counters"].shape)
    assert np.array_equal(got, host["counters"]), (got, host["counters"])
    nid = rb.node_id[:B].cpu().numpy()
    assert np.array_equal(nid, rnd["node_id"]), np.nonzero(nid != rnd["node_id"])[0][:10]
    for name in fields:
        a, w = getattr(tree, name).cpu().numpy(), np.ascontiguousarray(host[name])
        if a.dtype == np.float64:
            a, w = a.view(np.int64), w.view(np.int64)
        assert np.array_equal(a, w), (name, np.nonzero((a != w).reshape(len(a), -1).any(axis=1))[0][:10])


class SparseBuffers:
    """A ditree_sparse descriptor of the tests' own: T trees, each with its own grid."""

    def __init__(self, tree, grids, batch):
        from ditreeonlineplanner_amd._lib import Sparse
        T = len(grids)
        self.grids, self.stride = grids, max(g["cells"] for g in grids)
        self.extent = dev(np.array([[g["W"], g["L"]] for g in grids], dtype=np.float64))
        self.dims = dev(np.array([[g["nx"], g["ny"]] for g in grids], dtype=np.int32))
        self.dims_host = (C.c_int32 * (2 * T))(*[v for g in grids for v in (g["nx"], g["ny"])])
        self.table = torch.full((T, self.stride), -1, dtype=torch.int64, device="cuda")
        self.scratch = torch.full((T, self.stride), -1, dtype=torch.int64, device="cuda")
        self.stats = torch.zeros(T, 4, dtype=torch.int32, device="cuda")
        self.cand = torch.full((2 * batch,), -9, dtype=torch.int32, device="cuda")
        g = grids[0]
        assert all(h["cell"] == g["cell"] and h["nh"] == g["nh"] for h in grids)
        self.desc = Sparse(g["cell"], g["w"], g["nh"], self.stride, self.extent.data_ptr(), self.dims.data_ptr(), self.dims_host,
                           self.table.data_ptr(), self.scratch.data_ptr(), tree.active.data_ptr(), self.stats.data_ptr(),
                           self.cand.data_ptr())

    def upload(self, tables, stats):
        self.table.copy_(dev(np.stack(tables).view(np.int64)))
        self.stats.copy_(dev(np.asarray(stats, dtype=np.int32).reshape(-1, 4)))

    def compare(self, tables, stats):
        got = self.table.cpu().numpy().view(np.uint64)
        for t, tab in enumerate(tables):
            assert np.array_equal(got[t], tab), (t, np.nonzero(got[t] != tab)[0][:8])
        assert np.array_equal(self.stats.cpu().numpy(), np.asarray(stats).reshape(-1, 4)), (self.stats.cpu().numpy(), stats)
        assert bool((self.scratch == -1).all()), "the contender words go back to all ones"


def cell_centre(grid, c):
    nh, nx = grid["nh"], grid["nx"]
    ih, ix, iy = c % nh, (c // nh) % nx, c // (nh * nx)
    return [-grid["W"] / 2 + (ix + 0.5) * grid["cell"], -grid["L"] / 2 + (iy + 0.5) * grid["cell"], (ih + 0.5) * grid["w"]]


def build_case(case, B, n0, rng):
    host = random_tree_state(rng, CAP, 1)
    host["active"] = rng.integers(0, 2, CAP).astype(np.uint8)
    host["key"] = rng.integers(1, 400, CAP).astype(np.int32)
    table = SR.synthetic_tree(rng, host, 0, n0, GRID, GRID["cells"])
    status = rng.choice([OK, GOAL, COLLIDED, COLLIDED | GAC], B, p=[0.6, 0.08, 0.27, 0.05])
    rnd = random_rows(rng, B, status, 0, n0)
    rnd["end_state"] = SR.synthetic_states(rng, B, GRID)
    bound_stats = None
    if case == "one_cell":                                           # one contest: a few rows share the smallest cost
        c = int(rng.integers(0, GRID["cells"]))
        rnd["end_state"][:, :3] = np.array(cell_centre(GRID, c)) + rng.uniform(-0.1, 0.1, (B, 3))
        host["cost"][:n0] = np.maximum(1, rng.integers(50, 54, n0))
        host["cost"][0] = 1
        act, table = active_ref(host["state"][:n0], host["cost"][:n0], GRID)
        host["active"][:n0] = act
    elif case == "own_cells":
        cells = rng.permutation(GRID["cells"])[:B]
        rnd["end_state"][:, :3] = [cell_centre(GRID, int(c)) for c in cells]
    elif case == "capacity":                                         # the tree fills up two winners before the round ends
        pass
    elif case == "bounded":                                          # an incumbent in the middle of the candidates' costs
        inc = n0 - 1 if n0 > 1 else 0
        host["counters"][0, 1] = inc
        if n0 > 1:
            host["cost"][inc] = 215
            act, table = active_ref(host["state"][:n0], host["cost"][:n0], GRID)
            host["active"][:n0] = act
        bound_stats = np.array([int(host["cost"][inc]), int(rng.integers(0, 9)), 0, 7], dtype=np.int32)
    host["counters"][0, 0] = n0
    sstats = np.array([int(rng.integers(0, 9)), int(rng.integers(0, 9)), int(host["active"][:n0].sum()), 5], dtype=np.int32)
    return host, rnd, table, sstats, bound_stats


def run_accept(ctx, eng, sp, B, bound=None):
    from ditreeonlineplanner_amd import _lib
    eng.ensure_maze()
    rd = eng.rb.desc(0, B)
    return _lib.lib().ditree_accept_sparse(ctx._h, C.byref(eng.tree.desc), C.byref(rd), eng.tree.cost.data_ptr(),
                                           None if bound is None else C.byref(bound), C.byref(sp.desc), ctx.stream)


def upload(eng, host):
    upload_tree(eng.tree, host, eng.tree.counters)
    eng.tree.active.copy_(dev(host["active"]))
    if eng.tree.key is not None:
        eng.tree.key.copy_(dev(host["key"]))


def prepare(case, B, n0):
    """-> (host, rnd, table, sparse stats, bound stats or None) of a case, as uploaded."""
    rng = np.random.default_rng(1000 * CASES.index(case) + 10 * B + (n0 > 1))
    host, rnd, table, sstats, bstats = build_case(case, B, n0, rng)
    if case == "capacity":                                           # what the restatement appends with room to spare, less two
        trial = {k: v.copy() for k, v in host.items()}
        trnd = {k: v.copy() for k, v in rnd.items()}
        sparse_accept_ref(trial, trnd, trial["counters"][0], sstats.copy(), table.copy(), 0, B, 0, CAP, GRID)
        fit = int((trnd["node_id"] >= 0).sum())
        n_new = n0 + fit - min(2, fit)
        # the tree is moved to the end of its slots: the same nodes, costs and flags, their ids shifted
        shift = CAP - n_new
        for name in TREE_FIELDS + ("active", "key"):
            host[name][shift:shift + n0] = host[name][:n0].copy()
        rnd["parent"] = (rnd["parent"] + shift).astype(np.int32)
        host["counters"][0, 0] = shift + n0
        _, table = active_ref(host["state"][shift:shift + n0], host["cost"][shift:shift + n0], GRID, base=shift)
        # nodes below ``shift`` are the tree's too: give them no cell, so that they take no part
        host["state"][:shift, 0] = np.nan
        host["xy"][:shift, 0] = np.nan
        host["active"][:shift] = 0
    return host, rnd, table, sstats, bstats


def restate(case, host, rnd, table, sstats, bstats, B, n0):
    """The restatement on the prepared arrays, and the conditions on the test's inputs (not on the device): it went through
    the case."""
    bdict = dict(goal=GOAL_XY, radius=RADIUS, reach=REACH, stats=bstats) if case == "bounded" else None
    before, sbefore = host["counters"][0].copy(), sstats.copy()
    sparse_accept_ref(host, rnd, host["counters"][0], sstats, table, 0, B, 0, CAP, GRID, bdict)
    cnt, nid = host["counters"][0], rnd["node_id"]
    alive = rnd["status"] & 0xff != COLLIDED
    goal = rnd["status"] & 0xff == GOAL
    assert cnt[4] - before[4] == B and sstats[0] - sbefore[0] == sstats[3]
    n = int(cnt[0])
    act, tab = active_ref(host["state"][:n], host["cost"][:n], GRID)
    assert np.array_equal(act, host["active"][:n]) and np.array_equal(tab, table) and act.sum() == sstats[2]
    if case == "one_cell":
        assert (nid[alive & ~goal] >= 0).sum() <= 1 and (nid[goal] >= 0).all() and (B < 63 or sstats[3] > B // 3)
    elif case == "own_cells":
        assert B < 63 or (nid[alive] >= 0).sum() > alive.sum() // 2
        if n0 == 1:
            assert sstats[3] <= 1 and sstats[1] - sbefore[1] == 0    # at most the root's own cell is taken
    elif case == "capacity":
        assert cnt[0] == CAP and (B < 63 or (cnt[6] == 1 and (nid[alive] == -1).sum() == sstats[3] + 2))
    elif case == "bounded":
        assert bstats[3] + sstats[3] + (nid >= 0).sum() == alive.sum()
        assert n0 == 1 or B < 1023 or (bstats[3] > 0 and sstats[3] > 0 and (nid >= 0).sum() > 0)
    elif B >= 1023:
        assert sstats[3] > 0 and (n0 == 1 or sstats[1] > sbefore[1]) and (goal & (nid >= 0)).any()


@pytest.mark.parametrize("n0", TREES)
@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("case", CASES)
def test_accept_sparse_against_the_sequential_restatement(ctx, best, pruned, case, B, n0):
    from ditreeonlineplanner_amd._lib import Bound
    host, rnd, table, sstats, bstats = prepare(case, B, n0)
    eng = pruned if case == "bounded" else best
    sp = SparseBuffers(eng.tree, [GRID], 2049)
    upload(eng, host)
    upload_round(eng.rb, rnd, B)
    sp.upload([table], sstats)
    bound = None
    if case == "bounded":
        goals, bst = dev(GOAL_XY[None]), dev(bstats)
        bound = Bound(eng.tree.cost.data_ptr(), eng.tree.key.data_ptr(), goals.data_ptr(), RADIUS, REACH, bst.data_ptr())
    assert run_accept(ctx, eng, sp, B, bound) == 0
    restate(case, host, rnd, table, sstats, bstats, B, n0)
    fields = TREE_FIELDS + ("active",) + (("key",) if case == "bounded" else ())
    compare_tree(eng.tree, eng.tree.counters, eng.rb, host, rnd, B, fields=fields)
    sp.compare([table], sstats)
    if case == "bounded":
        assert np.array_equal(bst.cpu().numpy(), bstats), (bst.cpu().numpy(), bstats)


def test_forest_accept_sparse_with_an_empty_range(ctx):
    """Two rounds on a forest of three trees, each with its own map extents; tree 1 has no candidate in the first round: its
    nodes, its table row and its stats row stay untouched."""
    from ditreeonlineplanner_amd import _lib
    from ditreeonlineplanner_amd.forest import ForestEngine
    T, Cap, counts = 3, 1500, [1100, 0, 300]
    maze, start, goal = scenario()
    forest = ForestEngine(ctx, maze, start, goal, T, Cap, edge_length=16, action_horizon=8, batch=1400,
                          emulate_sticky_done=False, solution="anytime", sparse_cell=0.5)
    grids = [grid_ref(8, 8, 1.0, 0.25, 4), grid_ref(5, 7, 1.0, 0.25, 4), grid_ref(6, 3, 1.0, 0.25, 4)]
    rng = np.random.default_rng(17)
    host = random_tree_state(rng, T * Cap, T)
    host["active"] = rng.integers(0, 2, T * Cap).astype(np.uint8)
    sp = SparseBuffers(forest.tree, grids, 1400)
    n0 = [40, 25, 1]
    tables = []
    for t in range(T):
        tab = SR.synthetic_tree(rng, host, t * Cap, n0[t], grids[t], sp.stride)
        tables.append(tab)
    host["counters"][:, 0] = n0
    sstats = np.array([[3, 4, int(host["active"][t * Cap:t * Cap + n0[t]].sum()), 9] for t in range(T)], dtype=np.int32)
    upload_tree(forest.tree, host, forest.fcounters)
    forest.tree.active.copy_(dev(host["active"]))
    sp.upload(tables, sstats)
    for rounds in range(2):
        off = np.concatenate([[0], np.cumsum(counts)])
        B = int(off[-1])
        status = rng.choice([OK, GOAL, COLLIDED, COLLIDED | GAC], B, p=[0.6, 0.08, 0.27, 0.05])
        rnd = random_rows(rng, B, status, 0, 1)
        for t in range(T):
            lo, hi = int(off[t]), int(off[t + 1])
            rnd["parent"][lo:hi] = t * Cap + rng.integers(0, host["counters"][t, 0], counts[t])
            rnd["end_state"][lo:hi] = SR.synthetic_states(rng, counts[t], grids[t])
        upload_round(forest.rb, rnd, B)
        forest._set_offsets(counts)
        forest.ensure_maze()
        rd = forest.rb.desc(0, B)
        before, sbefore, tbefore = host["counters"].copy(), sstats.copy(), [t.copy() for t in tables]
        _lib.check(ctx._h, _lib.lib().ditree_forest_accept_sparse(
            ctx._h, C.byref(forest.tree.desc), C.byref(forest.fdesc), C.byref(rd), forest.tree.cost.data_ptr(), None,
            C.byref(sp.desc), ctx.stream), "forest_accept_sparse")
        for t in range(T):
            sparse_accept_ref(host, rnd, host["counters"][t], sstats[t], tables[t], int(off[t]), int(off[t + 1]), t * Cap, Cap,
                              grids[t])
        compare_tree(forest.tree, forest.fcounters, forest.rb, host, rnd, B, fields=TREE_FIELDS + ("active",))
        sp.compare(tables, sstats)
        for t in range(T):
            if counts[t] == 0:
                assert np.array_equal(host["counters"][t], before[t]) and np.array_equal(sstats[t], sbefore[t])
                assert np.array_equal(tables[t], tbefore[t])
            else:
                assert sstats[t, 3] > 0
            n = int(host["counters"][t, 0])
            act, tab = active_ref(host["state"][t * Cap:t * Cap + n], host["cost"][t * Cap:t * Cap + n], grids[t], base=t * Cap,
                                  stride=sp.stride)
            assert np.array_equal(act, host["active"][t * Cap:t * Cap + n]) and np.array_equal(tab, tables[t])
        counts = [200, 600, 0]


@pytest.mark.parametrize("n0", [1, 2999])
def test_rebuild_equals_active_ref(ctx, best, n0):
    """ditree_sparse_rebuild on a synthetic tree, from garbage in the table, the flags and the stats row."""
    from ditreeonlineplanner_amd import _lib
    rng = np.random.default_rng(n0)
    host = random_tree_state(rng, CAP, 1)
    host["active"] = rng.integers(0, 2, CAP).astype(np.uint8)
    table = SR.synthetic_tree(rng, host, 0, n0, GRID, GRID["cells"], cost_hi=6)          # few costs: many ties on (cost, id)
    host["counters"][0, 0] = n0
    sp = SparseBuffers(best.tree, [GRID], 2049)
    garbage = host["active"].copy()
    garbage[:n0] = rng.integers(0, 2, n0)
    upload_tree(best.tree, host, best.tree.counters)
    best.tree.active.copy_(dev(garbage))
    sp.table.copy_(dev(rng.integers(0, 2 ** 40, (1, GRID["cells"]))))
    sp.scratch.copy_(dev(rng.integers(0, 2 ** 40, (1, GRID["cells"]))))
    sp.stats.fill_(7)
    _lib.check(ctx._h, _lib.lib().ditree_sparse_rebuild(ctx._h, C.byref(best.tree.desc), None, C.byref(sp.desc),
                                                        best.tree.cost.data_ptr(), 0, 1, ctx.stream), "sparse_rebuild")
    assert np.array_equal(best.tree.active.cpu().numpy(), host["active"])               # slots past n0 untouched
    sp.compare([table], [0, 0, int(host["active"][:n0].sum()), 0])


def test_the_rebuild_after_a_rebase_equals_active_ref_on_the_rebased_tree():
    """``reuse_tree=True`` with ``sparse_cell``: after the re-base the flags are those of the re-based tree from scratch, and
    a node that was retired is active again where its representative was dropped."""
    from tests import test_gpu_tree_reuse as TR
    pl = TR.planner(solution="anytime", sparse_cell=0.5, sparse_headings=2, max_candidates=6 * TR.BATCH)
    eng = pl._engine
    path, actions = TR.seeded_plan(pl)
    assert path is not None and pl.results["dominated_candidates"] > 0

    def flags():
        n = eng.tree.n_nodes_host
        grid = grid_ref(*TR.room().shape, 1.0, 0.5, 2)
        st, cost = eng.tree.state[:n].cpu().numpy(), eng.tree.cost[:n].cpu().numpy()
        act, _ = active_ref(st, cost, grid)
        assert np.array_equal(eng.tree.active[:n].cpu().numpy(), act)
        return act
    before = flags()
    assert pl.results["active_nodes"] == before.sum()
    car = TR.drive(pl, actions, 3)
    old_active = eng.tree.active
    pl.reset(start_state=car, goal_state=pl.test_goal)
    assert pl.results["reused_nodes"] > 0 and eng.tree.active is not old_active
    after = flags()
    assert eng.active_nodes == after.sum() and eng.dominated_candidates == 0 and eng.retired_nodes == 0
    pl.max_candidates = TR.BATCH                               # one re-plan round on the re-based flags keeps the invariant
    TR.seeded_plan(pl, TR.SEED + 1)
    flags()


def test_accept_sparse_refuses_by_name_without_launching(ctx, best):
    from ditreeonlineplanner_amd import _lib
    from ditreeonlineplanner_amd._lib import Sparse
    L, h = _lib.lib(), ctx._h
    sp = SparseBuffers(best.tree, [GRID], 2049)
    best.tree.reset(best.start_state)
    best.rb.node_id.fill_(-7)
    best.rb.parent.zero_()
    cnt = best.tree.counters.clone()

    def variant(**kw):
        d = Sparse.from_buffer_copy(sp.desc)
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    small = (C.c_int32 * 2)(64, 64)
    cases = [(variant(cell=0.0), 0, b"sparse: cell must be > 0 and finite"), (variant(nh=65), 0, b"sparse: nh must be 1..64 and w > 0"),
             (variant(w=0.0), 0, b"sparse: nh must be 1..64 and w > 0"), (variant(extent=None), 0, b"sparse: extent / dims missing"),
             (variant(active=None), 0, b"sparse: table, scratch, active or stats missing"),
             (variant(stride=2 ** 22 + 1), 0, b"sparse: stride must be 1..2^22"),
             (variant(dims_host=small), 0, b"sparse: nx * ny * nh of tree 0 exceeds the stride"),
             (variant(cand=None), 0, b"sparse: cand scratch missing"), (sp.desc, 2, b"sparse: one rank (round->shard must be 0)")]
    for d, shard, msg in cases:
        rd = best.rb.desc(0, 4)
        rd.shard = shard
        rc = L.ditree_accept_sparse(h, C.byref(best.tree.desc), C.byref(rd), best.tree.cost.data_ptr(), None, C.byref(d), ctx.stream)
        assert rc == -1 and L.ditree_last_error(h) == msg, L.ditree_last_error(h)
    rd = best.rb.desc(0, 4)
    assert L.ditree_accept_sparse(h, C.byref(best.tree.desc), C.byref(rd), None, None, C.byref(sp.desc), ctx.stream) == -1
    assert L.ditree_last_error(h) == b"sparse: cost array missing"
    assert L.ditree_accept_sparse(h, C.byref(best.tree.desc), C.byref(rd), best.tree.cost.data_ptr(), None, None, ctx.stream) == -1
    assert L.ditree_last_error(h) == b"sparse: descriptor missing"
    torch.cuda.synchronize()
    assert (best.rb.node_id == -7).all() and torch.equal(best.tree.counters, cnt) and bool((sp.table == -1).all())
