"""GPU: the near-parent search (ditree_nn_argmin_near, ditree_forest_nn_argmin_near: nn_near_kernel, nn_forest_near_kernel,
both near_parent -- nearest, then the second pass with the cost column --) against the sequential restatement of tests/near_parent_ref.py, parent index for index.  Every comparison is exact.

Sizes: a trip of either pass covers 512 nodes (64 lanes x 8 loads) and a wave serves four queries, so N runs over one and two
nodes, around one lane row (63 / 64 / 65), around a trip (511 / 512 / 513), over several trips (4097) and over a tree of real
size (100 003, an odd count whose last trip is clamped); B around a wave's four queries and over many blocks (1024).  The
queries of one N are one set and every B is a prefix of it, so each (N, mask) computes its reference once.

Designed cases sit on integer coordinates with reach 1 or 1/2, so every d2 and every g is exact in f64."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.near_parent_ref import NO_BOUND, near_parent_fast, near_parent_ref
from tests.test_gpu_forest import ctx, dev  # noqa: F401

pytestmark = pytest.mark.gpu

NS = [1, 2, 63, 64, 65, 511, 512, 513, 4097, 100003]
BS = [1, 3, 4, 5, 1024]
MASKS = ["unmasked", "no_bound", "mid", "all_closed"]
CAP = 100010
U_MID = 500
REACH = 0.1


@pytest.fixture(scope="module")
def tree(ctx):
    from ditreeonlineplanner_amd.engine import DeviceTree
    return DeviceTree(ctx, CAP, 1, 1, cost=True, key=True)


def bound_of(tree):
    from ditreeonlineplanner_amd._lib import Bound
    return Bound(tree.cost.data_ptr(), tree.key.data_ptr(), None, 0.5, 0.1, None)


def set_nodes(tree, xy, cost, key=None, n=None, incumbent=-1, rng=None):
    """The first len(xy) slots of the tree: positions (state columns 0, 1 and the xy copy), costs, keys; the other state
    columns, the last actions and the flags are random where ``rng`` is given.  ``incumbent``: the node the counter row names."""
    k = len(xy)
    if rng is not None:
        tree.state[:k].copy_(dev(rng.uniform(-1, 1, (k, 6))))
        tree.last_action[:k].copy_(dev(rng.uniform(-1, 1, (k, 2))))
        tree.has_prev[:k].copy_(dev(rng.integers(0, 2, k).astype(np.uint8)))
    tree.state[:k, :2] = dev(xy)
    tree.xy[:k].copy_(dev(xy))
    tree.cost[:k].copy_(dev(np.asarray(cost, dtype=np.int32)))
    if key is not None:
        tree.key[:k].copy_(dev(np.asarray(key, dtype=np.int32)))
    tree.counters.copy_(dev(np.array([k if n is None else n, incumbent, 0, 0, 0, 0, 0, -1], dtype=np.int32)))


def search(ctx, tree, q, N, radius, reach=REACH, masked=False, gather=True):
    out = ctx.nn_argmin_near(q, tree, tree.cost, radius, reach, n_nodes=N, bound=bound_of(tree) if masked else None, gather=gather)
    return out if gather else (out,)


def check_gather(tree, idx, s, a, hp):
    bits = torch.int64
    assert torch.equal(s.view(bits), tree.state[idx.long()].view(bits)) and torch.equal(a, tree.last_action[idx.long()])
    assert torch.equal(hp, tree.has_prev[idx.long()])


def radius_for(N):
    """About ten nodes in a disc of this radius at N uniform nodes on the 20 x 20 square, at most 4 m."""
    return float(min(4.0, np.sqrt(10 * 400.0 / (np.pi * N))))


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("N", NS)
def test_search_against_the_restatement(ctx, tree, N, mask):
    rng = np.random.default_rng(N)
    xy = rng.uniform(-10, 10, (N + 1, 2))
    cost = rng.integers(1, 400, N + 1)
    key = rng.integers(0, 2 * U_MID, N + 1)
    key[0] = U_MID - 1 if N > 1 else key[0]
    inc, U = -1, NO_BOUND
    if mask == "mid":
        U = U_MID
    elif mask == "all_closed":
        U = 0
    if U != NO_BOUND:                                          # the incumbent is slot N, outside the scanned nodes
        inc, cost[N] = N, U
    set_nodes(tree, xy, cost, key, n=N, incumbent=inc, rng=rng)
    masked = mask != "unmasked"
    radius = radius_for(N)
    qh = rng.uniform(-10, 10, (max(BS), 6))
    qh[0, :2] = xy[rng.integers(0, N)]                         # a query on a node
    kw = dict(key=key, U=U) if masked else {}
    want, star, size = near_parent_fast(qh[:, :2], xy, cost, radius, REACH, hi=N, detail=True, **kw)
    if N <= 65:
        assert np.array_equal(want, near_parent_ref(qh[:, :2], xy, cost, radius, REACH, hi=N, **kw))
    if mask == "all_closed":
        assert (want == 0).all()
    elif N >= 63:
        assert (want != star).any() and size.max() > 1        # the rule is not the nearest node here
    if mask == "mid":
        assert (key[want[size > 0]] < U).all() and (want[size == 0] == 0).all()      # no open node: node 0, as the plain scans
    for B in BS:
        idx, s, a, hp = search(ctx, tree, dev(qh[:B]), N, radius, masked=masked)
        got = idx.cpu().numpy()
        assert np.array_equal(got, want[:B]), (B, np.nonzero(got != want[:B])[0][:5])
        check_gather(tree, idx, s, a, hp)


# ---------------------------------------------------------------------- designed cases
FAR = 1.0e6


def designed(N, at):
    """N nodes far away (distinct integer points beyond every radius here, cost 1) with the designed nodes ``at``:
    {index: (x, y, cost)}."""
    xy = np.stack([FAR + np.arange(N, dtype=np.float64), np.full(N, FAR)], axis=1)
    cost = np.ones(N, dtype=np.int64)
    for i, (x, y, c) in at.items():
        xy[i] = (x, y)
        cost[i] = c
    return xy, cost


def run_designed(ctx, tree, xy, cost, radius, reach, key=None, U=NO_BOUND, queries=((0.0, 0.0),)):
    N = len(xy)
    inc = -1
    if key is not None and U != NO_BOUND:
        xy, cost, key = np.concatenate([xy, [[FAR, -FAR]]]), np.concatenate([cost, [U]]), np.concatenate([key, [0]])
        inc = N
    set_nodes(tree, xy, cost, key, n=N, incumbent=inc)
    q = np.zeros((len(queries), 6))
    q[:, :2] = queries
    got = search(ctx, tree, dev(q), N, radius, reach, masked=key is not None, gather=False)[0].cpu().numpy()
    kw = {} if key is None else dict(key=key, U=U)
    assert np.array_equal(got, near_parent_ref(q[:, :2], xy, cost, radius, reach, hi=N, **kw))
    return got


# where the designed nodes sit: next to each other, in one lane (64 apart), in different trips of one lane (512 apart), and in
# the clamped last trip
PLACES = [(6, (0, 1, 2, 3, 4)), (70, (0, 1, 65, 3, 67)), (600, (5, 517, 69, 581, 599)), (1100, (1029, 5, 517, 1093, 1099))]


@pytest.mark.parametrize("N,at", PLACES)
@pytest.mark.parametrize("reach", [1.0, 0.5])
def test_designed_ties_and_the_edge_of_the_near_set(ctx, tree, N, at, reach):
    i0, i1, i2, i3, i4 = at
    s = int(1 / reach)                                        # rows per metre: g = cost + s * distance, an integer

    def nodes(c0, c1, c2, c3, c4):                            # distances 0, 5, 10, 5, 5 from the origin
        return designed(N, {i0: (0, 0, c0), i1: (3, 4, c1), i2: (6, 8, c2), i3: (0, 5, c3), i4: (-5, 0, c4)})
    # a cheaper node inside the radius: g = 20, 10 + 5 s, ...
    assert run_designed(ctx, tree, *nodes(20 * s, 10 * s, 4 * s, 15 * s, 15 * s), 5.0, reach)[0] == i1
    # a still cheaper node exactly on tau2 = 100 is a member, one ulp of radius less and it is not
    assert run_designed(ctx, tree, *nodes(20 * s, 10 * s, 4 * s, 15 * s, 15 * s), 10.0, reach)[0] == i2
    assert run_designed(ctx, tree, *nodes(20 * s, 10 * s, 4 * s, 15 * s, 15 * s), np.nextafter(10.0, 0.0), reach)[0] == i1
    # equal g, different d2: the smaller d2 (the nearest node itself)
    assert run_designed(ctx, tree, *nodes(20 * s, 30 * s, 40 * s, 15 * s, 15 * s), 5.0, reach)[0] == i0
    # equal g and equal d2: the lower index, wherever the two sit
    assert run_designed(ctx, tree, *nodes(30 * s, 30 * s, 40 * s, 15 * s, 15 * s), 5.0, reach)[0] == min(i3, i4)
    assert run_designed(ctx, tree, *nodes(30 * s, 15 * s, 40 * s, 15 * s, 15 * s), 5.0, reach)[0] == min(i1, i3, i4)
    # the nearest node is a member whatever the radius: tiny radius, n* alone
    assert run_designed(ctx, tree, *nodes(90 * s, 1, 1, 1, 1), 1e-300, reach)[0] == i0
    # two nearest nodes at equal distance (5) from a query that sees no node at 0: n* is the lower index, both are members
    xy, cost = designed(N, {i1: (3, 4, 30 * s), i3: (0, 5, 20 * s), i4: (-5, 0, 20 * s)})
    assert run_designed(ctx, tree, xy, cost, 0.5, reach)[0] == min(i3, i4)


@pytest.mark.parametrize("N,at", PLACES)
def test_designed_nan_rows_and_a_closed_nearest_node(ctx, tree, N, at):
    i0, i1, i2, i3, i4 = at
    xy, cost = designed(N, {i0: (0, 0, 20), i1: (3, 4, 10), i2: (6, 8, 4), i3: (0, 5, 15), i4: (-5, 0, 15)})
    # NaN rows never win and are no members, however cheap
    xn, cn = xy.copy(), cost.copy()
    xn[i1] = (np.nan, 4)
    cn[i1] = 0
    assert run_designed(ctx, tree, xn, cn, 5.0, 1.0)[0] == i0                  # g = 20 at d 0 against 20 at d 5
    xn[i0] = (0, np.nan)
    assert run_designed(ctx, tree, xn, cn, 5.0, 1.0)[0] == i2                  # n* at distance 5 now; tau = 10 takes i2 in: g = 14
    cn[i2] = 40
    assert run_designed(ctx, tree, xn, cn, 5.0, 1.0)[0] == min(i3, i4)
    # a query with a NaN coordinate sees only NaN distances -> node 0, and the other queries of its wave are not disturbed
    got = run_designed(ctx, tree, xy, cost, 5.0, 1.0, queries=((0, 0), (np.nan, 0), (0, 0), (3, np.nan), (0, 0)))
    assert got.tolist() == [i1, 0, i1, 0, i1]
    # n* closed under the mask: the nearest OPEN node leads and sets tau2
    key = np.zeros(N, dtype=np.int64)
    key[i0] = 7
    got = run_designed(ctx, tree, xy, cost, 1.0, 1.0, key=key, U=7)
    assert got[0] == i1                                                       # n* = the first node at 5; tau = 6: g = 15, 20, 20
    key[i1] = 9
    assert run_designed(ctx, tree, xy, cost, 5.0, 1.0, key=key, U=7)[0] == i2   # n* at 5, tau 10: i2 with g = 14
    key[i2] = 7                                                               # at the bound: closed
    assert run_designed(ctx, tree, xy, cost, 5.0, 1.0, key=key, U=7)[0] == min(i3, i4)
    assert run_designed(ctx, tree, xy, cost, 5.0, 1.0, key=np.full(N, 7), U=7)[0] == 0       # nothing open
    assert run_designed(ctx, tree, xy, cost, 5.0, 1.0, key=key, U=NO_BOUND)[0] == i1          # no incumbent: everything open


@pytest.mark.parametrize("N", NS)
def test_equal_costs_give_the_existing_searches_bit_for_bit(ctx, tree, N):
    """All of C at one cost: the parent is the nearest node -- ditree_nn_argmin's and ditree_nn_argmin_bounded's result,
    gathered rows included."""
    from ditreeonlineplanner_amd import _lib
    rng = np.random.default_rng(N + 7)
    xy = rng.uniform(-10, 10, (N + 1, 2))
    xy[N // 2] = np.nan
    xy[N - 1] = xy[0]                                          # a duplicate: the lower index
    key = rng.integers(0, 2 * U_MID, N + 1)
    cost = np.full(N + 1, 37)
    cost[N] = U_MID
    set_nodes(tree, xy, cost, key, n=N, incumbent=N, rng=rng)
    for B in BS:
        q = dev(np.concatenate([np.pad(xy[[0]], ((0, 0), (0, 4))), rng.uniform(-10, 10, (B, 6))])[:B])
        want = ctx.nn_argmin(q, tree.xy, n_nodes=N, gather=(tree.state, tree.last_action, tree.has_prev))
        outs = [torch.empty_like(w) for w in want]
        _lib.check(ctx._h, _lib.lib().ditree_nn_argmin_bounded(ctx._h, C.byref(tree.desc), C.byref(bound_of(tree)), q.data_ptr(), 6, B,
                                                               N, *[o.data_ptr() for o in outs], ctx.stream), "nn_argmin_bounded")
        for radius in (0.3, 30.0):
            for got, ref in ((search(ctx, tree, q, N, radius), want), (search(ctx, tree, q, N, radius, masked=True), outs)):
                for g, w in zip(got, ref):
                    bits = torch.int64 if g.dtype == torch.float64 else g.dtype
                    assert torch.equal(g.view(bits), w.view(bits))


# ---------------------------------------------------------------------- forests
FORESTS = {1: (1, 600, [9]), 3: (3, 700, [0, 300, 0]), 64: (64, 70, [0, 0, 5, 3, 1, 0, 0, 17] + [(7 * t) % 5 for t in range(8, 63)] + [0]),
           5: (5, 1, [1, 1, 1, 1, 1])}


@pytest.mark.parametrize("solution", ["anytime", "anytime_pruned"])
@pytest.mark.parametrize("T", list(FORESTS))
def test_forest_search_against_the_restatement(ctx, T, solution):
    """Uneven candidate ranges, empty ranges, one query per tree; trees of one node, full trees; with the mask every tree under
    its own bound (none, 50, 0 = nothing open).  Then all costs equal: the existing segmented searches bit for bit."""
    from ditreeonlineplanner_amd import _lib
    from ditreeonlineplanner_amd.forest import ForestEngine
    from tests.test_gpu_forest import scenario
    T, Cap, counts = FORESTS[T]
    maze, start, goal = scenario()
    f = ForestEngine(ctx, maze, start, goal, T, Cap, edge_length=16, action_horizon=8, batch=max(sum(counts), 1),
                     emulate_sticky_done=False, solution=solution)
    masked = solution == "anytime_pruned"
    rng = np.random.default_rng(T)
    st = rng.uniform(-10, 10, (T * Cap, 6))
    f.tree.state.copy_(dev(st))
    f.tree.xy.copy_(dev(st[:, :2]))
    f.tree.last_action.copy_(dev(rng.uniform(-1, 1, (T * Cap, 2))))
    f.tree.has_prev.copy_(dev(rng.integers(0, 2, T * Cap).astype(np.uint8)))
    n = rng.integers(1, Cap + 1, T)
    n[T // 2] = Cap
    if T > 1:
        n[-1] = 1
    cnt = np.zeros((T, 8), dtype=np.int32)
    cnt[:, 0], cnt[:, 1], cnt[:, 7] = n, -1, -1
    key = rng.integers(0, 100, T * Cap).astype(np.int32)
    cost = rng.integers(1, 400, T * Cap).astype(np.int32)
    bounds = np.full(T, NO_BOUND, dtype=np.int64)
    if masked:
        for t in range(T):
            kind = t % 3                                       # 0: no incumbent; 1: bound 50; 2: bound 0, nothing open
            if kind and n[t] > 1:
                inc = t * Cap + int(rng.integers(1, n[t]))
                bounds[t] = 50 if kind == 1 else 0
                cnt[t, 1], cost[inc] = inc, bounds[t]
        f.tree.key.copy_(dev(key))
    f.fcounters.copy_(dev(cnt))
    f.tree.cost.copy_(dev(cost))
    off = f._set_offsets(counts)
    B = int(off[-1])
    qh = rng.uniform(-10, 10, (B, 6))
    q = dev(qh)
    radius = 2.0
    bd = bound_of(f.tree) if masked else None
    idx, s, a, hp = ctx.nn_argmin_near(q, f.tree, f.tree.cost, radius, REACH, bound=bd, forest=f.fdesc, gather=True)
    got = idx.cpu().numpy()
    differs = 0
    for t in range(T):
        lo, hi = int(off[t]), int(off[t + 1])
        kw = dict(key=key, U=bounds[t]) if masked else {}
        want, star, _ = near_parent_fast(qh[lo:hi, :2], st[:, :2], cost, radius, REACH, lo=t * Cap, hi=t * Cap + int(n[t]), detail=True, **kw)
        assert np.array_equal(got[lo:hi], want), t
        differs += int((want != star).sum())
        if bounds[t] == 0:
            assert (got[lo:hi] == t * Cap).all()
    assert differs > 0 or Cap == 1
    check_gather(f.tree, idx, s, a, hp)
    # one cost in every tree (a tree with an incumbent: the incumbent's, so the bound stays)
    flat = np.repeat(np.where(bounds == NO_BOUND, 37, bounds), Cap).astype(np.int32)
    f.tree.cost.copy_(dev(flat))
    ref = torch.full((B,), -9, dtype=torch.int32, device="cuda")
    L = _lib.lib()
    if masked:
        _lib.check(ctx._h, L.ditree_forest_nn_argmin_bounded(ctx._h, C.byref(f.tree.desc), C.byref(f.fdesc), C.byref(bd), q.data_ptr(),
                                                             6, B, ref.data_ptr(), None, None, None, ctx.stream), "forest_nn_argmin_bounded")
    else:
        _lib.check(ctx._h, L.ditree_forest_nn_argmin(ctx._h, C.byref(f.tree.desc), C.byref(f.fdesc), q.data_ptr(), 6, B, ref.data_ptr(),
                                                     ctx.stream), "forest_nn_argmin")
    idx, s, a, hp = ctx.nn_argmin_near(q, f.tree, f.tree.cost, radius, REACH, bound=bd, forest=f.fdesc, gather=True)
    assert torch.equal(idx, ref)
    check_gather(f.tree, idx, s, a, hp)


# ---------------------------------------------------------------------- refusals
def test_every_refusal_by_name(ctx, tree):
    from ditreeonlineplanner_amd import _lib
    from ditreeonlineplanner_amd._lib import Bound, Near, RoundParams
    from ditreeonlineplanner_amd.forest import ForestEngine
    from tests.test_gpu_forest import scenario
    L, h = _lib.lib(), ctx._h
    maze, start, goal = scenario()
    f = ForestEngine(ctx, maze, start, goal, 2, 16, edge_length=16, action_horizon=8, batch=4, emulate_sticky_done=False,
                     solution="anytime_pruned")
    f._set_offsets([2, 2])
    q = torch.zeros(4, 6, dtype=torch.float64, device="cuda")
    idx = torch.full((4,), -9, dtype=torch.int32, device="cuda")
    f.rb.parent.fill_(-9)
    c = f.tree.cost.data_ptr()
    bad = [(None, b"near: descriptor missing"), (Near(None, 1.0, 0.1), b"near: cost array missing")]
    for r in (0.0, -1.0, float("nan"), float("inf")):
        bad.append((Near(c, r, 0.1), b"near: radius must be > 0 and finite"))
        bad.append((Near(c, 1.0, r), b"near: reach must be > 0 and finite"))
    rd, sharded = f.rb.desc(0, 4), f.rb.desc(0, 4, shard=2)
    rp = RoundParams()
    tr, fd = C.byref(f.tree.desc), C.byref(f.fdesc)

    def refused(nr, bd, msg, which=slice(None), **kw):
        n = None if nr is None else C.byref(nr)
        b = None if bd is None else C.byref(bd)
        fns = [lambda: L.ditree_nn_argmin_near(h, tr, n, b, q.data_ptr(), 6, 4, 1, idx.data_ptr(), None, None, None, ctx.stream),
               lambda: L.ditree_forest_nn_argmin_near(h, tr, fd, n, b, q.data_ptr(), 6, 4, idx.data_ptr(), None, None, None,
                                                      ctx.stream),
               lambda: L.ditree_expand_round_near(h, tr, C.byref(kw.get("rdesc", rd)), C.byref(kw.get("p", rp)), b, n, ctx.stream),
               lambda: L.ditree_forest_expand_round_near(h, tr, fd, None, C.byref(kw.get("rdesc", rd)), C.byref(kw.get("p", rp)), b, n,
                                                         ctx.stream)]
        for fn in fns[which]:
            assert fn() == -1 and L.ditree_last_error(h) == msg, L.ditree_last_error(h)
    for nr, msg in bad:
        refused(nr, None, msg)
    ok = Near(c, 1.0, 0.1)
    refused(ok, None, b"near: one rank (round->shard must be 0)", slice(2, 4), rdesc=sharded)
    budget = RoundParams()
    budget.chunk_budget = idx.data_ptr()
    refused(ok, None, b"expand_round_near: chunk budgets are not built (p->chunk_budget must be NULL)", slice(2, 4), p=budget)
    # with a bound, the bound's own refusals
    refused(ok, Bound(c, None, None, 0.5, 0.1, None), b"bound: key column missing")
    refused(ok, Bound(None, f.tree.key.data_ptr(), None, 0.5, 0.1, None), b"bound: cost array missing")
    torch.cuda.synchronize()
    assert (idx == -9).all() and (f.rb.parent == -9).all()     # nothing was launched
