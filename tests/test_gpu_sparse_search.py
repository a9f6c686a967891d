"""GPU: the searches over the ACTIVE nodes of a sparse tree (ditree_nn_argmin_sparse, ditree_forest_nn_argmin_sparse,
ditree_chunk_budget_sparse: the MASK_ACTIVE instantiations of the four nearest-node kernels) against the restatements of
tests/near_parent_ref.py restricted to the active set, index for index.  Trees of 1, 511, 512, 513 and 4 099 nodes (a wave trip is
512 nodes); the active patterns are random, only the root, and all nodes; plain, near, bounded (active and open) and chunk-budget
searches, single tree and forest."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.near_parent_ref import near_parent_fast
from tests.test_gpu_forest import ctx, dev  # noqa: F401

pytestmark = pytest.mark.gpu

NS = [1, 511, 512, 513, 4099]
PATTERNS = ["random", "root", "all"]
KINDS = ["plain", "near", "bounded", "bounded_near"]
CAP = 4100
B = 261                                                      # a last wave of one query
U_MID, RADIUS, REACH = 500, 1.5, 0.1


@pytest.fixture(scope="module")
def tree(ctx):
    from ditreeonlineplanner_amd.engine import DeviceTree
    return DeviceTree(ctx, 3 * CAP, 1, 1, cost=True, key=True, active=True)


def sparse_of(tree):
    """A descriptor whose active column the searches read; the grid fields only have to pass the check."""
    from ditreeonlineplanner_amd._lib import Sparse
    keep = dict(extent=torch.ones(3, 2, dtype=torch.float64, device="cuda"), dims=torch.ones(3, 2, dtype=torch.int32, device="cuda"),
                dims_host=(C.c_int32 * 6)(1, 1, 1, 1, 1, 1), words=torch.full((2, 3, 4), -1, dtype=torch.int64, device="cuda"),
                stats=torch.zeros(3, 4, dtype=torch.int32, device="cuda"))
    d = Sparse(0.5, 2.0 * np.pi / 4, 4, 4, keep["extent"].data_ptr(), keep["dims"].data_ptr(), keep["dims_host"],
               keep["words"][0].data_ptr(), keep["words"][1].data_ptr(), tree.active.data_ptr(), keep["stats"].data_ptr(), None)
    return d, keep


def fill(tree, rng, base, N, pattern):
    xy = rng.uniform(-10, 10, (N, 2))
    if N > 8:
        xy[5] = np.nan                                        # a node whose distance never wins
        xy[7] = xy[3]                                         # a tie on the distance: the lower index
    cost = rng.integers(1, 400, N).astype(np.int32)
    key = rng.integers(0, 2 * U_MID, N).astype(np.int32)
    key[0] = 0
    active = {"random": (rng.random(N) < 0.4), "root": np.zeros(N, dtype=bool), "all": np.ones(N, dtype=bool)}[pattern]
    active[0] = True
    sl = slice(base, base + N)
    tree.state[sl].copy_(dev(rng.uniform(-1, 1, (N, 6))))
    tree.state[sl, :2] = dev(xy)
    tree.xy[sl].copy_(dev(xy))
    tree.last_action[sl].copy_(dev(rng.uniform(-1, 1, (N, 2))))
    tree.has_prev[sl].copy_(dev(rng.integers(0, 2, N).astype(np.uint8)))
    tree.cost[sl].copy_(dev(cost))
    tree.key[sl].copy_(dev(key))
    tree.active[sl].copy_(dev(active.astype(np.uint8)))
    return xy, cost, key, active


def want_parents(q, xy, cost, key, active, kind, U):
    mask = active & (key < U) if kind.startswith("bounded") else active
    radius = RADIUS if kind.endswith("near") else 1e-300      # a radius of nothing: the nearest node (ties on g go to it)
    pseudo = np.where(mask, 0, 1)
    parents, nearest, _ = near_parent_fast(q, xy, cost, radius, REACH, key=pseudo, U=1, detail=True)
    return parents if kind.endswith("near") else nearest


def descriptors(tree, kind, stats=None):
    from ditreeonlineplanner_amd._lib import Bound, Near
    near = Near(tree.cost.data_ptr(), RADIUS, REACH) if kind.endswith("near") else None
    bound = Bound(tree.cost.data_ptr(), tree.key.data_ptr(), None, 0.5, 0.1, None) if kind.startswith("bounded") else None
    return near, bound


def ref(x):
    return None if x is None else C.byref(x)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("N", NS)
def test_single_tree_search_over_the_active_nodes(ctx, tree, N, pattern, kind):
    from ditreeonlineplanner_amd import _lib
    rng = np.random.default_rng(100 * N + PATTERNS.index(pattern))
    xy, cost, key, active = fill(tree, rng, 0, N, pattern)
    inc = N - 1 if kind.startswith("bounded") else -1
    U = U_MID
    if inc >= 0:
        tree.cost[inc] = U_MID
        cost[inc] = U_MID
    tree.counters.copy_(dev(np.array([N, inc, 0, 0, 0, 0, 0, -1], dtype=np.int32)))
    q = rng.uniform(-11, 11, (B, 2))
    qd = dev(q)
    sp, keep = sparse_of(tree)
    near, bound = descriptors(tree, kind)
    out = torch.full((B,), -5, dtype=torch.int32, device="cuda")
    s = torch.zeros(B, 6, dtype=torch.float64, device="cuda")
    a = torch.zeros(B, 2, dtype=torch.float64, device="cuda")
    hp = torch.zeros(B, dtype=torch.uint8, device="cuda")
    _lib.check(ctx._h, _lib.lib().ditree_nn_argmin_sparse(ctx._h, C.byref(tree.desc), C.byref(sp), ref(near), ref(bound),
                                                          qd.data_ptr(), 2, B, N, out.data_ptr(), s.data_ptr(), a.data_ptr(),
                                                          hp.data_ptr(), ctx.stream), "nn_argmin_sparse")
    want = want_parents(q, xy, cost, key, active, kind, U)
    got = out.cpu().numpy()
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    idx = out.long()
    assert torch.equal(s.view(torch.int64), tree.state[idx].view(torch.int64)) and torch.equal(a, tree.last_action[idx])
    assert torch.equal(hp, tree.has_prev[idx])
    # conditions on the inputs: only active nodes are chosen, and the mask matters where it should
    assert active[want].all() and (pattern != "root" or (want == 0).all())
    if pattern == "random" and N > 8:
        dense = want_parents(q, xy, cost, key, np.ones(N, dtype=bool), kind, U)
        assert (dense != want).any()


@pytest.mark.parametrize("kind", KINDS)
def test_forest_search_over_each_trees_active_nodes(ctx, tree, kind):
    from ditreeonlineplanner_amd import _lib
    from ditreeonlineplanner_amd._lib import Forest
    rng = np.random.default_rng(77)
    sizes, counts = [513, 1, 4099], [120, 3, 138]
    filled = [fill(tree, rng, t * CAP, sizes[t], ["random", "root", "random"][t]) for t in range(3)]
    cnt = np.zeros((3, 8), dtype=np.int32)
    cnt[:, 0], cnt[:, 1], cnt[:, 7] = sizes, -1, -1
    if kind.startswith("bounded"):                            # trees 0 and 2 hold an incumbent, tree 1 none
        for t in (0, 2):
            inc = sizes[t] - 1
            cnt[t, 1] = t * CAP + inc
            tree.cost[t * CAP + inc] = U_MID
            filled[t][1][inc] = U_MID
    counters = dev(cnt)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    off_host = (C.c_int32 * 4)(*off.tolist())
    off_dev = dev(off)
    fd = Forest(3, CAP, counters.data_ptr(), off_dev.data_ptr(), off_host)
    Bq = int(off[-1])
    q = rng.uniform(-11, 11, (Bq, 2))
    qd = dev(q)
    sp, keep = sparse_of(tree)
    near, bound = descriptors(tree, kind)
    out = torch.full((Bq,), -5, dtype=torch.int32, device="cuda")
    _lib.check(ctx._h, _lib.lib().ditree_forest_nn_argmin_sparse(ctx._h, C.byref(tree.desc), C.byref(fd), C.byref(sp), ref(near),
                                                                 ref(bound), qd.data_ptr(), 2, Bq, out.data_ptr(), None, None,
                                                                 None, ctx.stream), "forest_nn_argmin_sparse")
    got = out.cpu().numpy()
    for t in range(3):
        xy, cost, key, active = filled[t]
        U = U_MID if cnt[t, 1] >= 0 else 2 ** 31 - 1
        want = t * CAP + want_parents(q[off[t]:off[t + 1]], xy, cost, key, active, kind, U)
        assert np.array_equal(got[off[t]:off[t + 1]], want), (t, np.nonzero(got[off[t]:off[t + 1]] != want)[0][:8])


@pytest.mark.parametrize("bounded", [False, True])
@pytest.mark.parametrize("N", [1, 513, 4099])
def test_chunk_budget_counts_the_visits_of_the_nearest_active_node(ctx, tree, N, bounded):
    from ditreeonlineplanner_amd import _lib
    rng = np.random.default_rng(5 * N + bounded)
    xy, cost, key, active = fill(tree, rng, 0, N, "random")
    if N > 8:
        active[:] = False
        active[rng.choice(N, 6, replace=False)] = True        # few parents: many candidates share one
        active[0] = True
        tree.active[:N].copy_(dev(active.astype(np.uint8)))
    visits = rng.integers(0, 3, N).astype(np.int32)
    tree.num_visit[:N].copy_(dev(visits))
    inc = N - 1 if bounded else -1
    if bounded:
        tree.cost[inc] = U_MID
        cost[inc] = U_MID
    tree.counters.copy_(dev(np.array([N, inc, 0, 0, 0, 0, 0, -1], dtype=np.int32)))
    samples = rng.uniform(-11, 11, (B, 6))
    sd = dev(samples)
    sched = [3, 1, 2, 4]
    sched_c = (C.c_int32 * 4)(*sched)
    big = DeviceTreeChunks(tree, 4)
    sp, keep = sparse_of(tree)
    _, bound = descriptors(tree, "bounded" if bounded else "plain")
    par = torch.full((B,), -5, dtype=torch.int32, device="cuda")
    bud = torch.full((B,), -5, dtype=torch.int32, device="cuda")
    _lib.check(ctx._h, _lib.lib().ditree_chunk_budget_sparse(ctx._h, C.byref(big), None, C.byref(sp), ref(bound), sd.data_ptr(), B, N,
                                                             sched_c, 4, par.data_ptr(), bud.data_ptr(), ctx.stream),
               "chunk_budget_sparse")
    want_par = want_parents(samples[:, :2], xy, cost, key, active, "bounded" if bounded else "plain", U_MID)
    assert np.array_equal(par.cpu().numpy(), want_par)
    seen = visits.copy()
    want = np.empty(B, dtype=np.int32)
    for b in range(B):
        want[b] = sched[min(max(int(seen[want_par[b]]), 0), 3)]
        seen[want_par[b]] += 1
    assert np.array_equal(bud.cpu().numpy(), want) and (N == 1 or len(set(want.tolist())) > 1)


def DeviceTreeChunks(tree, n_chunks):
    """The tree's descriptor with room for ``n_chunks`` chunks per edge (the schedule's entries are checked against it)."""
    from ditreeonlineplanner_amd._lib import Tree
    d = Tree.from_buffer_copy(tree.desc)
    d.n_chunks = n_chunks
    return d
