"""GPU: the masked nearest-node search of ``solution="anytime_pruned"`` (ditree_nn_argmin_bounded,
ditree_forest_nn_argmin_bounded: nn_argmin_kernel<MASK_KEY>, nn_forest_kernel<false, MASK_KEY>, i.e. scan_nodes under the key's
mask behind tree_search / forest_search) and the key kernel (ditree_bound_keys)
against the numpy restatement of tests/anytime_pruned_ref.py.  Every comparison is exact.

Sizes: a trip of the scan covers 512 nodes (64 lanes x 8 loads) and a wave serves four queries, so N runs around one lane
row (63 / 64 / 65), around a trip (511 / 512 / 513) and over several trips (4097), B around a wave's four queries and over
many blocks (257)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.anytime_pruned_ref import NO_BOUND, h_ref, masked_nn_fast
from tests.test_gpu_forest import ctx, dev  # noqa: F401

pytestmark = pytest.mark.gpu

NS = [1, 63, 64, 65, 511, 512, 513, 4097]
BS = [1, 3, 4, 5, 257]
MASKS = ["all", "root", "last", "none", "alternating", "tail"]
CAP = 4100
U = 500


def mask_of(name, N):
    m = np.zeros(N, dtype=bool)
    if name == "all":
        m[:] = True
    elif name == "root":
        m[0] = True
    elif name == "last":
        m[N - 1] = True
    elif name == "alternating":
        m[::2] = True
    elif name == "tail":                                   # open nodes only in the last trip, whose tail loads are clamped
        m[512 * ((N - 1) // 512) + ((N - 1) % 512) // 2:] = True
    return m


@pytest.fixture(scope="module")
def tree(ctx):
    from ditreeonlineplanner_amd.engine import DeviceTree
    return DeviceTree(ctx, CAP, 2, 8, cost=True, key=True)


def bound_of(tree, goals=None, reach=0.1, stats=None):
    from ditreeonlineplanner_amd._lib import Bound
    return Bound(tree.cost.data_ptr(), tree.key.data_ptr(), None if goals is None else goals.data_ptr(), 0.5, reach,
                 None if stats is None else stats.data_ptr())


def fill_tree(tree, rng, N, mask, bound=U):
    """Random nodes; open nodes get keys below the bound, closed ones keys at or above it (the first closed one exactly at
    it); the incumbent is the last slot of the tree, outside the scanned nodes."""
    st = rng.uniform(-10, 10, (CAP, 6))
    tree.state.copy_(dev(st))
    tree.xy.copy_(dev(st[:, :2]))
    tree.last_action.copy_(dev(rng.uniform(-1, 1, (CAP, 2))))
    tree.has_prev.copy_(dev(rng.integers(0, 2, CAP).astype(np.uint8)))
    key = np.where(mask_pad(mask), rng.integers(0, bound, CAP), rng.integers(bound, bound + 50, CAP)).astype(np.int32)
    closed = np.nonzero(~mask)[0]
    if len(closed):
        key[closed[0]] = bound
    opened = np.nonzero(mask)[0]
    if len(opened):
        key[opened[0]] = bound - 1
    tree.key.copy_(dev(key))
    cost = rng.integers(1, 400, CAP).astype(np.int32)
    cost[CAP - 1] = bound
    tree.cost.copy_(dev(cost))
    cnt = np.array([N, CAP - 1, 0, 0, 0, 0, 0, -1], dtype=np.int32)
    tree.counters.copy_(dev(cnt))
    return st, key


def mask_pad(mask):
    m = np.zeros(CAP, dtype=bool)
    m[:len(mask)] = mask
    return m


def search(ctx, tree, q, N, gather=True):
    from ditreeonlineplanner_amd import _lib
    B = q.shape[0]
    idx = torch.full((B,), -9, dtype=torch.int32, device="cuda")
    outs = (torch.zeros(B, 6, dtype=torch.float64, device="cuda"), torch.zeros(B, 2, dtype=torch.float64, device="cuda"),
            torch.zeros(B, dtype=torch.uint8, device="cuda"))
    bd = bound_of(tree)
    ptrs = [o.data_ptr() for o in outs] if gather else [None] * 3
    _lib.check(ctx._h, _lib.lib().ditree_nn_argmin_bounded(ctx._h, C.byref(tree.desc), C.byref(bd), q.data_ptr(), q.shape[1], B, N,
                                                           idx.data_ptr(), *ptrs, ctx.stream), "nn_argmin_bounded")
    return (idx, *outs)


@pytest.mark.parametrize("N", NS)
def test_masked_search_against_numpy(ctx, tree, N):
    rng = np.random.default_rng(N)
    for name in MASKS:
        mask = mask_of(name, N)
        st, key = fill_tree(tree, rng, N, mask)
        for B in BS:
            qh = rng.uniform(-10, 10, (B, 6))
            qh[0, :2] = st[rng.integers(0, N), :2]                # a query on a node
            idx, s, a, hp = search(ctx, tree, dev(qh), N)
            want = masked_nn_fast(qh[:, :2], st[:N, :2], key[:N], U)
            got = idx.cpu().numpy()
            assert np.array_equal(got, want), (name, B, np.nonzero(got != want)[0][:5])
            if name == "none":
                assert (got == 0).all()                            # what an all-NaN scan returns
            else:
                assert mask[got].all()
            assert torch.equal(s, tree.state[idx.long()]) and torch.equal(a, tree.last_action[idx.long()])
            assert torch.equal(hp, tree.has_prev[idx.long()])


@pytest.mark.parametrize("N", [65, 513, 4097])
def test_a_closed_duplicate_loses_to_the_open_one_behind_it(ctx, tree, N):
    """Two nodes on one point, the lower index closed: the higher one wins and its rows are gathered; with both open the
    lower index wins, as in the unmasked search."""
    rng = np.random.default_rng(N + 1)
    mask = np.ones(N, dtype=bool)
    lo, hi = N // 3, N - 2
    mask[lo] = False
    st, key = fill_tree(tree, rng, N, mask)
    st[hi, :2] = st[lo, :2]
    tree.state.copy_(dev(st))
    tree.xy.copy_(dev(st[:, :2]))
    q = dev(np.concatenate([st[[lo]], rng.uniform(-10, 10, (4, 6))]))
    idx, s, a, hp = search(ctx, tree, q, N)
    assert int(idx[0]) == hi and torch.equal(s[0], tree.state[hi]) and torch.equal(a[0], tree.last_action[hi])
    assert int(hp[0]) == int(tree.has_prev[hi])
    assert np.array_equal(idx.cpu().numpy(), masked_nn_fast(q.cpu().numpy()[:, :2], st[:N, :2], key[:N], U))
    tree.key[lo] = U - 1
    assert int(search(ctx, tree, q, N)[0][0]) == lo


@pytest.mark.parametrize("N", [64, 513])
def test_nan_coordinates_never_win(ctx, tree, N):
    rng = np.random.default_rng(N + 2)
    mask = mask_of("alternating", N)
    st, key = fill_tree(tree, rng, N, mask)
    st[0:N:4, 0] = np.nan                                          # every second open node
    tree.state.copy_(dev(st))
    tree.xy.copy_(dev(st[:, :2]))
    qh = rng.uniform(-10, 10, (9, 6))
    qh[3, 1] = np.nan                                              # and a query that sees only NaN distances -> node 0
    idx = search(ctx, tree, dev(qh), N, gather=False)[0].cpu().numpy()
    assert np.array_equal(idx, masked_nn_fast(qh[:, :2], st[:N, :2], key[:N], U)) and idx[3] == 0
    ok = np.delete(idx, 3)
    assert mask[ok].all() and not np.isnan(st[ok, 0]).any()


@pytest.mark.parametrize("N", NS)
def test_without_an_incumbent_the_search_is_the_existing_one_bit_for_bit(ctx, tree, N):
    rng = np.random.default_rng(N + 3)
    st, key = fill_tree(tree, rng, N, mask_of("alternating", N))
    st[N // 2, :2] = np.nan
    st[N - 1, :2] = st[0, :2]
    tree.state.copy_(dev(st))
    tree.xy.copy_(dev(st[:, :2]))
    tree.counters[1] = -1                                          # U = INT32_MAX: every key is below it
    tree.key[0] = NO_BOUND - 1
    for B in BS:
        q = dev(np.concatenate([st[[0]], rng.uniform(-10, 10, (B, 6))])[:B])
        got = search(ctx, tree, q, N)
        want = ctx.nn_argmin(q, tree.xy, n_nodes=N, gather=(tree.state, tree.last_action, tree.has_prev))
        for g, w in zip(got, want):                                 # bit for bit: the gathered NaN coordinates too
            bits = torch.int64 if g.dtype == torch.float64 else g.dtype
            assert torch.equal(g.view(bits), w.view(bits))


# ---------------------------------------------------------------------- forests
FORESTS = {1: (1, 600, [9]), 3: (3, 700, [0, 300, 0]), 64: (64, 70, [0, 0, 5, 3, 1, 0, 0, 17] + [(7 * t) % 5 for t in range(8, 63)] + [0])}


@pytest.mark.parametrize("T", list(FORESTS))
def test_forest_masked_search_per_tree_bounds(ctx, T):
    """Every tree under its own bound: trees without an incumbent (everything open), with one (about half closed), with no open
    node (the root comes back), with one node, and with empty candidate ranges."""
    from ditreeonlineplanner_amd import _lib
    from ditreeonlineplanner_amd.forest import ForestEngine
    from tests.test_gpu_forest import scenario
    T, Cap, counts = FORESTS[T]
    maze, start, goal = scenario()
    f = ForestEngine(ctx, maze, start, goal, T, Cap, edge_length=16, action_horizon=8, batch=max(sum(counts), 1),
                     emulate_sticky_done=False, solution="anytime_pruned")
    rng = np.random.default_rng(T)
    st = rng.uniform(-10, 10, (T * Cap, 6))
    f.tree.state.copy_(dev(st))
    f.tree.xy.copy_(dev(st[:, :2]))
    f.tree.last_action.copy_(dev(rng.uniform(-1, 1, (T * Cap, 2))))
    f.tree.has_prev.copy_(dev(rng.integers(0, 2, T * Cap).astype(np.uint8)))
    n = rng.integers(1, Cap + 1, T)
    n[T // 2] = Cap
    n[-1] = 1
    cnt = np.zeros((T, 8), dtype=np.int32)
    cnt[:, 0], cnt[:, 1], cnt[:, 7] = n, -1, -1
    key = rng.integers(0, 100, T * Cap).astype(np.int32)
    cost = rng.integers(1, 400, T * Cap).astype(np.int32)
    bounds = np.full(T, NO_BOUND, dtype=np.int64)
    for t in range(T):
        kind = t % 3                                               # 0: no incumbent; 1: bound 50; 2: bound 0, nothing open
        if kind:
            inc = t * Cap + int(rng.integers(0, n[t]))
            bounds[t] = 50 if kind == 1 else 0
            cnt[t, 1], cost[inc] = inc, bounds[t]
    f.fcounters.copy_(dev(cnt))
    f.tree.key.copy_(dev(key))
    f.tree.cost.copy_(dev(cost))
    off = f._set_offsets(counts)
    B = int(off[-1])
    qh = rng.uniform(-10, 10, (B, 6))
    q = dev(qh)
    idx = torch.full((B,), -9, dtype=torch.int32, device="cuda")
    outs = (torch.zeros(B, 6, dtype=torch.float64, device="cuda"), torch.zeros(B, 2, dtype=torch.float64, device="cuda"),
            torch.zeros(B, dtype=torch.uint8, device="cuda"))
    bd = bound_of(f.tree)
    L = _lib.lib()
    _lib.check(ctx._h, L.ditree_forest_nn_argmin_bounded(ctx._h, C.byref(f.tree.desc), C.byref(f.fdesc), C.byref(bd), q.data_ptr(), 6,
                                                         B, idx.data_ptr(), *[o.data_ptr() for o in outs], ctx.stream),
               "forest_nn_argmin_bounded")
    got = idx.cpu().numpy()
    for t in range(T):
        lo, hi = int(off[t]), int(off[t + 1])
        want = masked_nn_fast(qh[lo:hi, :2], st[:, :2], key, bounds[t], lo=t * Cap, hi=t * Cap + int(n[t]))
        assert np.array_equal(got[lo:hi], want), t
        if t % 3 == 2:
            assert (got[lo:hi] == t * Cap).all()
    assert torch.equal(outs[0], f.tree.state[idx.long()]) and torch.equal(outs[1], f.tree.last_action[idx.long()])
    assert torch.equal(outs[2], f.tree.has_prev[idx.long()])
    # no tree with an incumbent: the existing segmented search, bit for bit
    f.fcounters[:, 1] = -1
    ref = torch.full((B,), -9, dtype=torch.int32, device="cuda")
    _lib.check(ctx._h, L.ditree_forest_nn_argmin(ctx._h, C.byref(f.tree.desc), C.byref(f.fdesc), q.data_ptr(), 6, B, ref.data_ptr(),
                                                 ctx.stream), "forest_nn_argmin")
    _lib.check(ctx._h, L.ditree_forest_nn_argmin_bounded(ctx._h, C.byref(f.tree.desc), C.byref(f.fdesc), C.byref(bd), q.data_ptr(), 6,
                                                         B, idx.data_ptr(), None, None, None, ctx.stream), "forest_nn_argmin_bounded")
    assert torch.equal(idx, ref)


def test_search_refuses_by_name(ctx, tree):
    from ditreeonlineplanner_amd import _lib
    from ditreeonlineplanner_amd._lib import Bound
    L, h = _lib.lib(), ctx._h
    q = torch.zeros(4, 6, dtype=torch.float64, device="cuda")
    idx = torch.full((4,), -9, dtype=torch.int32, device="cuda")
    for bd, msg in ((Bound(tree.cost.data_ptr(), None, None, 0.5, 0.1, None), b"bound: key column missing"),
                    (Bound(None, tree.key.data_ptr(), None, 0.5, 0.1, None), b"bound: cost array missing")):
        rc = L.ditree_nn_argmin_bounded(h, C.byref(tree.desc), C.byref(bd), q.data_ptr(), 6, 4, 1, idx.data_ptr(), None, None, None,
                                        ctx.stream)
        assert rc == -1 and L.ditree_last_error(h) == msg
    assert L.ditree_nn_argmin_bounded(h, C.byref(tree.desc), None, q.data_ptr(), 6, 4, 1, idx.data_ptr(), None, None, None,
                                      ctx.stream) == -1 and L.ditree_last_error(h) == b"bound: descriptor missing"
    torch.cuda.synchronize()
    assert (idx == -9).all()


# ---------------------------------------------------------------------- keys
def ulp_steps(x):
    return [np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)]


@pytest.mark.parametrize("reach", [0.1, 0.05])
def test_keys_against_the_restatement(ctx, tree, reach):
    """Points at distances goal_radius + k * reach from the goal and one ulp either side, along an axis and along a diagonal,
    inside the radius, at the goal, at NaN and far away; a node range that starts past slot 0; slots outside it untouched."""
    from ditreeonlineplanner_amd import _lib
    rng = np.random.default_rng(int(reach * 1000))
    goal = np.array([1.25, -3.5])
    pts = [goal.copy(), goal + [0.2, 0.1], goal + [0.5, 0.0], [np.nan, 0.0], [0.0, np.nan], [1e200, 0.0], [1e6, 1e6]]
    for k in list(range(0, 12)) + [100, 1000, 12345]:
        for d in ulp_steps(0.5 + k * reach):
            pts.append(goal + [d, 0.0])
            pts.append(goal + [0.0, -d])
            pts.append(goal + np.array([0.6, 0.8]) * d)
    pts = np.array(pts, dtype=np.float64)
    n, first = len(pts), 37
    xy = rng.uniform(-10, 10, (CAP, 2))
    xy[first:first + n] = pts
    cost = rng.integers(1, 5000, CAP).astype(np.int32)
    tree.xy.copy_(dev(xy))
    tree.cost.copy_(dev(cost))
    tree.key.fill_(-5)
    goals = dev(goal[None])
    stats = torch.zeros(4, dtype=torch.int32, device="cuda")
    bd = bound_of(tree, goals, reach, stats)
    _lib.check(ctx._h, _lib.lib().ditree_bound_keys(ctx._h, C.byref(tree.desc), C.byref(bd), first, n, 0, ctx.stream), "bound_keys")
    got = tree.key.cpu().numpy()
    hs = np.array([h_ref(p[0], p[1], goal, 0.5, reach) for p in pts])
    assert np.array_equal(got[first:first + n], cost[first:first + n] + hs)
    assert (got[:first] == -5).all() and (got[first + n:] == -5).all()
    # the restatement went through the cases: zeros inside the disc and at NaN, the cap, and both sides of a boundary
    assert hs[0] == hs[1] == hs[3] == hs[4] == 0 and hs[5] == 2 ** 30 and 0 < hs[6] < 2 ** 30
    assert len(set(hs[7:7 + 9 * 3])) > 3


def test_keys_per_tree_goals_and_refusals(ctx, tree):
    """A forest's numbering: node n uses the goal row of tree n / C.  And the by-name refusals, which leave the column alone."""
    from ditreeonlineplanner_amd import _lib
    from ditreeonlineplanner_amd._lib import Bound
    rng = np.random.default_rng(5)
    Cn, T = 100, 7
    xy = rng.uniform(-10, 10, (CAP, 2))
    cost = rng.integers(1, 500, CAP).astype(np.int32)
    gl = rng.uniform(-10, 10, (T, 2))
    tree.xy.copy_(dev(xy))
    tree.cost.copy_(dev(cost))
    tree.key.fill_(-5)
    goals, stats = dev(gl), torch.zeros(T, 4, dtype=torch.int32, device="cuda")
    L, h = _lib.lib(), ctx._h
    _lib.check(h, L.ditree_bound_keys(h, C.byref(tree.desc), C.byref(bound_of(tree, goals, 0.1, stats)), 50, 600, Cn, ctx.stream),
               "bound_keys")
    got = tree.key.cpu().numpy()
    want = np.array([cost[k] + h_ref(xy[k, 0], xy[k, 1], gl[k // Cn], 0.5, 0.1) for k in range(50, 650)])
    assert np.array_equal(got[50:650], want) and (got[:50] == -5).all() and (got[650:] == -5).all()
    tree.key.fill_(-5)
    c, k, g, s = tree.cost.data_ptr(), tree.key.data_ptr(), goals.data_ptr(), stats.data_ptr()
    for bd, msg in ((Bound(c, None, g, 0.5, 0.1, s), b"bound: key column missing"),
                    (Bound(c, k, g, 0.5, 0.0, s), b"bound: reach must be > 0"),
                    (Bound(c, k, g, 0.5, -1.0, s), b"bound: reach must be > 0"),
                    (Bound(c, k, g, 0.5, float("nan"), s), b"bound: reach must be > 0"),
                    (Bound(c, k, None, 0.5, 0.1, s), b"bound: goal_xy missing"),
                    (Bound(c, k, g, 0.5, 0.1, None), b"bound: stats rows missing")):
        assert L.ditree_bound_keys(h, C.byref(tree.desc), C.byref(bd), 0, 10, 0, ctx.stream) == -1
        assert L.ditree_last_error(h) == msg, L.ditree_last_error(h)
    assert L.ditree_bound_keys(h, C.byref(tree.desc), C.byref(bound_of(tree, goals, 0.1, stats)), CAP - 5, 10, 0, ctx.stream) == -1
    torch.cuda.synchronize()
    assert (tree.key == -5).all()
