"""GPU: the forest kernels (nn_forest_kernel, i.e. forest_search over tree_of_query, nearest and write_parent; accept_scan_kernel<first> /
accept_commit_kernel on a forest's trees, row_scene_kernel, tree_of_query's third user, and the SCENES rollout) against plain numpy / Python written here and the oracle's own functions, at the tree sizes real runs reach:
trees past the 512-node trip of the search, 256 trees of one candidate, 2 500 candidates of one tree, a full scene table.
The entry points are called directly on tree contents and rounds written straight into the device arrays.  Every comparison is
exact (indices, flags, counters, copied doubles) except the scene rollout's states (1e-9, test_rollout_chunk_vs_oracle's bound).

The big forest has edge_length 16 (two chunks of 8), not 8: the accept's iteration counter sums chunks_run, which one chunk
would pin to 1.  That is 1.1 KB of edge storage per node, 15 MB for its 12 x 1100 slots."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import geometry as G
from tests.test_gpu_forest import ctx, dev, scenario  # noqa: F401
from tests.util import load_maze

pytestmark = pytest.mark.gpu

T_BIG, C_BIG = 12, 1100
T_WIDE, C_WIDE = 256, 66
I32 = torch.int32


@pytest.fixture(scope="module")
def big(ctx):
    from ditreeonlineplanner_amd.forest import ForestEngine
    maze, start, goal = scenario()
    return ForestEngine(ctx, maze, start, goal, T_BIG, C_BIG, edge_length=16, action_horizon=8, batch=2600)


@pytest.fixture(scope="module")
def wide(ctx):
    from ditreeonlineplanner_amd.forest import ForestEngine
    maze, start, goal = scenario()
    return ForestEngine(ctx, maze, start, goal, T_WIDE, C_WIDE, prop_duration=[8, 16], action_horizon=8, batch=T_WIDE)


def set_sizes(forest, sizes):
    forest.fcounters[:, 0] = dev(np.asarray(sizes), I32)


# ====================================================================== 1. segmented nearest node
def nn_case(T, Cap, sizes, seed):
    """Random node coordinates with poison: P[t] is a query of tree t; every slot at or beyond n_t holds P[t] (distance 0),
    and so do the last live slot of tree t - 1 and the root of tree t + 1; the last dead slot of a tree with two or more holds
    P[t + 1], so the slot just below a segment is poisoned as well."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-9.0, 9.0, (T * Cap, 2))
    P = rng.uniform(-9.0, 9.0, (T, 2))
    for t in range(T):
        xy[t * Cap + sizes[t]:(t + 1) * Cap] = P[t]
        if Cap - sizes[t] >= 2 and t + 1 < T:
            xy[(t + 1) * Cap - 1] = P[t + 1]
    for t in range(T):
        if t > 0:
            xy[(t - 1) * Cap + sizes[t - 1] - 1] = P[t]
        if t + 1 < T:
            xy[(t + 1) * Cap] = P[t]
    return xy, P, rng


def nn_queries(rng, xy, P, Cap, sizes, counts):
    """Per tree: P[t] first, then (from three queries on) the tree's own root and last live node, then random points."""
    rows = []
    for t, c in enumerate(counts):
        q = rng.uniform(-9.0, 9.0, (c, 2))
        if c:
            q[0] = P[t]
        if c >= 3:
            q[1], q[2] = xy[t * Cap], xy[t * Cap + sizes[t] - 1]
        rows.append(q)
    return np.concatenate(rows), np.concatenate([[0], np.cumsum(counts)])


def nn_ref(xy, q, off, Cap, sizes, lo_ext=0, hi_ext=0):
    """G.nn_argmin per query on the slots [t*C - lo_ext, t*C + n_t + hi_ext) of its tree (the extensions: what a scan that
    leaves its segment would read)."""
    out = np.full(len(q), -1, dtype=np.int64)
    for t in range(len(sizes)):
        if off[t + 1] > off[t]:
            a = max(t * Cap - lo_ext, 0)
            b = min(t * Cap + sizes[t] + hi_ext, len(xy))
            out[off[t]:off[t + 1]] = a + G.nn_argmin(q[off[t]:off[t + 1]], xy[a:b])
    return out


def check_poison(xy, q, off, Cap, sizes, ref):
    """A condition on the inputs: a scan one slot too long at either end returns another index for the tree's first query."""
    lo, hi = nn_ref(xy, q, off, Cap, sizes, lo_ext=1), nn_ref(xy, q, off, Cap, sizes, hi_ext=1)
    searched = [t for t in range(len(sizes)) if off[t + 1] > off[t]]
    n_lo = sum(lo[off[t]] != ref[off[t]] for t in searched if t > 0)
    n_hi = sum(hi[off[t]] != ref[off[t]] for t in searched if t + 1 < len(sizes))
    assert n_lo >= (len(searched) - 1) // 2 and n_hi >= (len(searched) - 1) // 2, (n_lo, n_hi, len(searched))


def forest_nn(ctx, forest, q, stride):
    from ditreeonlineplanner_amd import _lib
    B = len(q)
    qs = np.full((B, stride), 7.5)
    qs[:, :2] = q
    qd = dev(qs)
    out = torch.full((B,), -9, dtype=I32, device="cuda")
    _lib.check(ctx._h, _lib.lib().ditree_forest_nn_argmin(ctx._h, C.byref(forest.tree.desc), C.byref(forest.fdesc), qd.data_ptr(),
                                                          stride, B, out.data_ptr(), ctx.stream), "forest_nn_argmin")
    return out.cpu().numpy().astype(np.int64)


BIG_SIZES = [513, 1, 2, 63, 64, 65, 511, 512, 1025, 1100, 700, 1099]
# the first layout: an empty range first, two adjacent empty ranges in the middle, an empty range last; the second searches
# the trees the first left out
BIG_COUNTS = [[0, 1, 3, 64, 65, 0, 0, 3, 65, 64, 1, 0], [65, 3, 0, 1, 0, 64, 65, 1, 3, 0, 64, 3]]
TIE_TREE = 9                                   # n = 1100: local 37, 37 + 64, 37 + 512, 37 + 1024 hold one point,
TIE_A, TIE_B = (37, 101, 549, 1061), (200, 139, 713)   # and 200 / 139 / 713 (three lanes, two trips) another


@pytest.mark.parametrize("layout", [0, 1])
def test_segmented_nearest_node_past_the_first_trip(ctx, big, layout):
    """Trees of 1 .. 1100 nodes (one, two and three trips of 512, sizes around the wave and the trip), 0 .. 65 queries per tree
    with empty ranges first, adjacent and last, poison just outside every segment, exact ties across lanes and trips (lowest
    index wins) and NaN queries (the segment's first slot, never -1)."""
    counts = BIG_COUNTS[layout]
    xy, P, rng = nn_case(T_BIG, C_BIG, BIG_SIZES, 100 + layout)
    base = TIE_TREE * C_BIG
    za, zb = np.array([50.0, 50.0]), np.array([-40.0, 45.0])
    xy[[base + i for i in TIE_A]] = za
    xy[[base + i for i in TIE_B]] = zb
    q, off = nn_queries(rng, xy, P, C_BIG, BIG_SIZES, counts)
    special = None
    if counts[TIE_TREE] >= 10:
        special = off[TIE_TREE] + 3
        q[special:special + 6] = [za, za + [0.25, 0.0], zb, zb + [0.0, -0.5], [np.nan, 1.0], [np.nan, np.nan]]
    ref = nn_ref(xy, q, off, C_BIG, BIG_SIZES)
    check_poison(xy, q, off, C_BIG, BIG_SIZES, ref)
    big.tree.xy.copy_(dev(xy))
    set_sizes(big, BIG_SIZES)
    big._set_offsets(counts)
    got = forest_nn(ctx, big, q, 3)
    assert np.array_equal(got, ref), np.nonzero(got != ref)[0][:10]
    assert (got >= 0).all()
    if special is not None:
        assert list(got[special:special + 6]) == [base + 37, base + 37, base + 139, base + 139, base, base]
    else:
        assert layout == 1


def wide_sizes():
    return [1 + t % C_WIDE for t in range(T_WIDE)]


WIDE_COUNTS = [[1] * T_WIDE, [0 if t % 3 == 2 else 1 for t in range(T_WIDE)]]


@pytest.mark.parametrize("layout", [0, 1])
def test_one_candidate_per_tree_of_256_trees(ctx, wide, layout):
    """The headline shape: 256 trees of 1 .. 66 nodes, one query each (every wave another tree, a 256-entry search of `off`),
    then with every third range empty -- through ditree_forest_nn_argmin, through ditree_forest_chunk_budget (its parents and
    the budgets schedule[clip(num_visit[parent])]) and through a tape round's gather (parent ids and the parent's state as
    the rollout's first row)."""
    from ditreeonlineplanner_amd import _lib
    sizes, counts = wide_sizes(), WIDE_COUNTS[layout]
    xy, P, rng = nn_case(T_WIDE, C_WIDE, sizes, 200 + layout)
    q, off = nn_queries(rng, xy, P, C_WIDE, sizes, counts)
    B = len(q)
    ref = nn_ref(xy, q, off, C_WIDE, sizes)
    check_poison(xy, q, off, C_WIDE, sizes, ref)
    state = np.concatenate([xy, rng.uniform(-3.0, 3.0, (len(xy), 1)), rng.uniform(0.5, 4.0, (len(xy), 3))], axis=1)
    visits = rng.integers(0, 4, len(xy))
    tr = wide.tree
    tr.xy.copy_(dev(xy))
    tr.state.copy_(dev(state))
    tr.num_visit.copy_(dev(visits, I32))
    set_sizes(wide, sizes)
    wide._set_offsets(counts)
    assert np.array_equal(forest_nn(ctx, wide, q, 2), ref)
    # the chunk budget: a two-entry schedule of 1 and 2 chunks (one candidate per tree: no earlier visit of a parent in the round)
    samples = np.concatenate([q, rng.uniform(-1.0, 1.0, (B, 4))], axis=1)
    sd = dev(samples)
    par = torch.full((B,), -9, dtype=I32, device="cuda")
    bud = torch.full((B,), -9, dtype=I32, device="cuda")
    sched = (C.c_int32 * 2)(1, 2)
    _lib.check(ctx._h, _lib.lib().ditree_forest_chunk_budget(ctx._h, C.byref(tr.desc), C.byref(wide.fdesc), sd.data_ptr(), B, sched, 2,
                                                             par.data_ptr(), bud.data_ptr(), ctx.stream), "forest_chunk_budget")
    assert np.array_equal(par.cpu().numpy(), ref)
    want = np.array([1, 2])[np.clip(visits[ref], 0, 1)]
    assert np.array_equal(bud.cpu().numpy(), want) and len(set(want)) == 2
    # a tape round without accept: the gathered parent and its state
    acts = torch.zeros((B, wide.n_chunks, wide.P, 2), dtype=torch.float64, device="cuda")
    wide.expand_round(sd, dev(samples[:, :2]), inject_actions=acts, counts_per_tree=counts, accept=False)
    assert np.array_equal(wide.rb.parent[:B].cpu().numpy(), ref)
    assert np.array_equal(wide.rb.states[:B, 0, 0].cpu().numpy(), state[ref])
    assert np.array_equal(wide._budget[:B].cpu().numpy(), want)


# ---------------------------------------------------------------------- the `off` search of row_scene_kernel
def marker_scenes():
    """64 scenes on one open 10 x 10 map: scene k starts on the centre of interior cell k, which is also its goal.  A car at
    rest with zero actions stays, so a row's first step reports GOAL exactly when the rollout read the row's own scene."""
    maze = np.zeros((10, 10))
    cells = [(1 + k // 8, 1 + k % 8) for k in range(64)]
    out = []
    for rc in cells:
        s = np.array([*G.cell_rowcol_to_xy(list(rc), maze), 0.0, 0, 0, 0])
        out.append((maze, s, s.copy()))
    return out


@pytest.mark.parametrize("T,layouts", [(T_BIG, BIG_COUNTS), (T_WIDE, WIDE_COUNTS)])
def test_row_scene_search_against_searchsorted(ctx, T, layouts):
    """row_scene_kernel's binary search of `off` against np.searchsorted(off, q, 'right') - 1 on the layouts above, read through
    the rollout: every tree holds only its root, on the goal of the tree's own scene and of no other."""
    from ditreeonlineplanner_amd import _lib
    from ditreeonlineplanner_amd.forest import SceneForestEngine
    scenes = marker_scenes()
    forest = SceneForestEngine(ctx, scenes, T, 2, edge_length=8, action_horizon=8, batch=max(sum(c) for c in layouts))
    scene_of = [(5 * t + 3) % 64 for t in range(T)]
    for t in range(T):
        forest.reset_tree(t, scene_of[t])
    # the oracle's outcome of a root of scene k judged by scene j's goal: GOAL on the diagonal only
    k, j = np.divmod(np.arange(64 * 64), 64)
    starts = np.stack([s[1] for s in scenes])
    exp = G.rollout_chunk(starts[k], np.zeros((64 * 64, 8, 2)), scenes[0][0], starts[j][:, :2], 8)
    assert np.array_equal(exp["status"] == G.STATUS_GOAL, k == j)
    for counts in layouts:
        off = np.concatenate([[0], np.cumsum(counts)])
        B = int(off[-1])
        tree_of_row = np.searchsorted(off, np.arange(B), "right") - 1
        assert all(counts[t] > 0 for t in tree_of_row)
        row_scene = np.array(scene_of)[tree_of_row]
        root_scene = row_scene                                    # the parent is the tree's root: that scene's start
        want = exp["status"].reshape(64, 64)[root_scene, row_scene]
        samples = np.zeros((B, 6))
        forest.rb.status.fill_(-5)
        forest.expand_round(dev(samples), dev(samples[:, :2]),
                            inject_actions=torch.zeros((B, 1, forest.P, 2), dtype=torch.float64, device="cuda"),
                            counts_per_tree=counts, accept=False)
        got = forest.rb.status[:B].cpu().numpy()
        assert np.array_equal(got, want) and (got == _lib.ST_GOAL).all()
        assert np.array_equal(forest.rb.parent[:B].cpu().numpy(), tree_of_row * 2)
        assert np.array_equal(forest.rb.chunk_steps[:B, 0].cpu().numpy(), exp["n_steps"].reshape(64, 64)[root_scene, row_scene])


def test_tree_lookup_with_empty_ranges_in_front_and_between(ctx):
    """The one tree lookup of the kernels (tree_of_query) on off = [0, 0, 3, 3, 4, 9], five trees with an empty range in front
    and one in the middle, against np.searchsorted(off, q, 'right') - 1: through the forest nearest-node search (every tree holds
    only its root, so the parent names the tree) and through a scene-forest round (its parents, and row_scene_kernel read through
    the rollout as above: GOAL exactly when the row was judged by its own tree's scene)."""
    from ditreeonlineplanner_amd import _lib
    from ditreeonlineplanner_amd.forest import SceneForestEngine
    counts, T, Cap = [0, 3, 0, 1, 5], 5, 2
    off = np.concatenate([[0], np.cumsum(counts)])
    assert list(off) == [0, 0, 3, 3, 4, 9]
    B = int(off[-1])
    tree_of_row = np.searchsorted(off, np.arange(B), "right") - 1
    assert list(tree_of_row) == [1, 1, 1, 3, 4, 4, 4, 4, 4]
    forest = SceneForestEngine(ctx, marker_scenes(), T, Cap, edge_length=8, action_horizon=8, batch=B)
    for t in range(T):
        forest.reset_tree(t, 13 * t + 5)                          # five different scenes
    forest._set_offsets(counts)
    got = forest_nn(ctx, forest, np.random.default_rng(7).uniform(-9.0, 9.0, (B, 2)), 2)
    assert np.array_equal(got, tree_of_row * Cap)
    samples = np.zeros((B, 6))
    forest.rb.status.fill_(-5)
    forest.expand_round(dev(samples), dev(samples[:, :2]),
                        inject_actions=torch.zeros((B, 1, forest.P, 2), dtype=torch.float64, device="cuda"),
                        counts_per_tree=counts, accept=False)
    assert np.array_equal(forest.rb.parent[:B].cpu().numpy(), tree_of_row * Cap)
    assert (forest.rb.status[:B].cpu().numpy() == _lib.ST_GOAL).all()


# ====================================================================== 2. fallback
FB_SIZES = [3, 1, 65, 2, 513, 3, 514, 700, 1026, 130, 1100, 1099]
FB_TIES = [0, 2, 4, 6, 8, 10]                  # the trees that get a near-tie pair


def sq_rule(p, g):
    """The expansion search's key as nn_forest_kernel computes it: unfused dx*dx + dy*dy."""
    dx, dy = g[0] - p[..., 0], g[1] - p[..., 1]
    return dx * dx + dy * dy


def norm_rule(p, g):
    """The reference's key: np.linalg.norm(state[:2] - goal)."""
    return G.norm2(p[..., 0] - g[0], p[..., 1] - g[1])


def near_tie_pair(g, rng):
    """A node 1 .. 2 from the goal and a copy of it moved 1 - 3 ulp in x, ordered (lower index first) so that the first has the
    larger squared distance and both have the same norm; None if 10 000 draws hold none."""
    for _ in range(20):
        ang, r = rng.uniform(0, 2 * np.pi, 500), rng.uniform(1.0, 2.0, 500)
        p = g + np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1)
        steps, toward = rng.integers(1, 4, 500), np.where(rng.random(500) < 0.5, -np.inf, np.inf)
        x = p[:, 0].copy()
        for s in range(3):
            x = np.where(s < steps, np.nextafter(x, toward), x)
        m = np.stack([x, p[:, 1]], axis=1)
        for a, b in ((p, m), (m, p)):
            ok = (norm_rule(a, g) == norm_rule(b, g)) & (sq_rule(a, g) > sq_rule(b, g))
            if ok.any():
                i = int(np.argmax(ok))
                return a[i].copy(), b[i].copy()
    return None


def fallback_case(goals, seed):
    """Node coordinates of the 12 trees: every other node 5 .. 9 from its tree's goal; the root, the slots at or beyond n_t and
    (for a near-tie tree) the previous tree's last live slot exactly on the goal.  -> xy, the trees that hold a pair."""
    rng = np.random.default_rng(seed)
    T, Cap = T_BIG, C_BIG
    xy = np.zeros((T * Cap, 2))
    for t in range(T):
        ang, r = rng.uniform(0, 2 * np.pi, Cap), rng.uniform(5.0, 9.0, Cap)
        xy[t * Cap:(t + 1) * Cap] = goals[t] + np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1)
        xy[t * Cap] = goals[t]
        xy[t * Cap + FB_SIZES[t]:(t + 1) * Cap] = goals[t]
    ties = []
    for t in FB_TIES:
        pair = near_tie_pair(goals[t], rng)
        if pair is None:
            continue
        n = FB_SIZES[t]
        lo = 1 if n == 3 else int(rng.integers(1, n - 1))
        hi = 2 if n == 3 else int(rng.integers(lo + 1, n))
        xy[t * Cap + lo], xy[t * Cap + hi] = pair
        if t > 0 and FB_SIZES[t - 1] >= 2:
            xy[(t - 1) * Cap + FB_SIZES[t - 1] - 1] = goals[t]
        ties.append(t)
    return xy, ties


def fallback_ref(xy, goals, rule=norm_rule):
    """Per tree 1 + argmin(key) over local nodes 1 .. n_t - 1 (first occurrence), -1 for a tree of its root alone."""
    out = []
    for t, n in enumerate(FB_SIZES):
        out.append(-1 if n < 2 else 1 + int(np.argmin(rule(xy[t * C_BIG + 1:t * C_BIG + n], goals[t]))))
    return out


_G0 = np.array([2.5, -1.5])
FB_CASES = {False: np.tile(_G0, (T_BIG, 1)),
            True: _G0 + np.stack([np.linspace(-6, 6, T_BIG), np.linspace(4, -5, T_BIG) ** 2 / 5], axis=1)}
FB_CASES = {k: (g, *fallback_case(g, 5 + int(k))) for k, g in FB_CASES.items()}       # found at collection time


@pytest.fixture(scope="module")
def single(ctx):
    from ditreeonlineplanner_amd.engine import ExpansionEngine
    maze, start, goal = scenario()
    return ExpansionEngine(ctx, maze, start, goal, edge_length=8, action_horizon=8, batch=8, capacity=C_BIG)


@pytest.mark.parametrize("per_tree_goals", [False, True])
def test_forest_fallback_is_the_first_smallest_norm(ctx, big, single, per_tree_goals):
    """ditree_forest_fallback / _goals against 1 + argmin(norm2) over nodes 1 .. n_t - 1 for scans of 0 .. 1099 nodes, the root
    and every slot outside the segment exactly on the goal, and in six trees a nearest pair whose norms are equal while the
    LOWER index holds the LARGER squared distance: np.argmin of the norms returns the lower index, the squared-distance rule
    the higher.  ditree_fallback_select and ExpansionEngine.fallback_node on each tree's nodes alone return the same node."""
    from ditreeonlineplanner_amd import _lib
    from ditreeonlineplanner_amd.ops import _dbl
    goals, xy, ties = FB_CASES[per_tree_goals]
    assert len(ties) >= 4, f"near-tie pairs found for {len(ties)} trees only"
    ref, by_square = fallback_ref(xy, goals), fallback_ref(xy, goals, sq_rule)
    for t in ties:                                                # a condition on the inputs: the two rules disagree
        assert ref[t] != by_square[t] and ref[t] < by_square[t], (t, ref[t], by_square[t])
    assert all(ref[t] == by_square[t] for t in range(T_BIG) if t not in ties)
    h, L = ctx._h, _lib.lib()
    big.tree.xy.copy_(dev(xy))
    set_sizes(big, FB_SIZES)
    out = torch.full((T_BIG,), -9, dtype=I32, device="cuda")
    if per_tree_goals:
        ga, gp = _dbl(goals)
        _lib.check(h, L.ditree_forest_fallback_goals(h, C.byref(big.tree.desc), C.byref(big.fdesc), gp, out.data_ptr(), ctx.stream),
                   "forest_fallback_goals")
    else:
        ga, gp = _dbl(goals[0])
        _lib.check(h, L.ditree_forest_fallback(h, C.byref(big.tree.desc), C.byref(big.fdesc), gp, out.data_ptr(), ctx.stream),
                   "forest_fallback")
    got = out.cpu().numpy().astype(np.int64)
    got = [int(v) if v < 0 else int(v) - t * C_BIG for t, v in enumerate(got)]
    print("forest fallback", got, "norm rule", ref, "squared rule", by_square)
    assert got == ref, f"forest fallback {got} != first smallest norm {ref} (squared-distance rule: {by_square})"
    # the single-tree kernel on each tree's nodes
    one = torch.full((1,), -9, dtype=I32, device="cuda")
    for t, n in enumerate(FB_SIZES):
        single.tree.xy[:C_BIG].copy_(dev(xy[t * C_BIG:(t + 1) * C_BIG]))
        ga, gp = _dbl(goals[t])
        _lib.check(h, L.ditree_fallback_select(h, C.byref(single.tree.desc), n, gp, None, 0, one.data_ptr(), ctx.stream),
                   "fallback_select")
        assert int(one.item()) == ref[t], t
        single.tree.n_nodes_host = n
        single.goal_state[:2] = goals[t]
        assert single.fallback_node() == (None if ref[t] < 0 else ref[t]), t


# ====================================================================== 3. per-tree accept
OK, GOAL, COLLIDED, GAC = 0, 1, 2, 0x100
TREE_FIELDS = ("state", "xy", "parent", "last_action", "has_prev", "num_visit", "edge_states", "edge_actions", "edge_nstates",
               "edge_nactions")
ACC_N0 = [3, 2, 1, 40, 5, 1, 2, 4, 1, 6, C_BIG - 5, C_BIG - 5]
BIG_TREE = 3


def accept_ref(host, rnd, t, lo, hi):
    """planners/RRT.py:179-217 for the rows [lo, hi) of tree t, one candidate after the other, on the host copy of the forest:
    every candidate counts and visits its parent; a latched env (a collision inside the goal radius left env.done set) makes
    the next candidate a one-step phantom that ends the run as the goal; a collided candidate adds its chunks and nothing else;
    any other becomes a node (end state, parent, edge without all-zero rows, last kept action) and a GOAL ends the range.
    Nodes past the tree's C slots are dropped (node id -1, overflow flag, n = C); ids and the phantom row are global."""
    if hi == lo:
        return
    cnt, base = host["counters"][t], t * C_BIG
    rnd["node_id"][lo:hi] = -1
    cnt[7] = -1
    n = int(cnt[0])

    def append(b, state, es, ea):
        nonlocal n
        if n >= C_BIG:
            cnt[6] = 1
            return -1
        k = base + n
        n += 1
        es, ea = es[~(es == 0).all(axis=1)], ea[~(ea == 0).all(axis=1)]
        host["state"][k], host["xy"][k], host["parent"][k] = state, state[:2], rnd["parent"][b]
        host["has_prev"][k], host["num_visit"][k] = 1, 0
        host["edge_states"][k, :len(es)], host["edge_nstates"][k] = es, len(es)
        host["edge_actions"][k, :len(ea)], host["edge_nactions"][k] = ea, len(ea)
        host["last_action"][k] = ea[-1] if len(ea) else 0.0
        rnd["node_id"][b] = k
        return k
    for b in range(lo, hi):
        cnt[4] += 1
        host["num_visit"][rnd["parent"][b]] += 1
        if cnt[2]:
            cnt[5], cnt[7] = 1, b
            cnt[3] += 1
            s0 = host["state"][rnd["parent"][b]].copy()
            cnt[1] = append(b, s0, np.stack([s0, s0]), rnd["actions"][b, 0, :1])
            break
        run, st = int(rnd["chunks_run"][b]), int(rnd["status"][b])
        cnt[3] += run
        if st & 0xff == COLLIDED:
            if st & GAC:
                cnt[2] = 1
            continue
        k = append(b, rnd["end_state"][b], rnd["states"][b, :run].reshape(-1, 6), rnd["actions"][b, :run].reshape(-1, 2))
        if st & 0xff == GOAL:
            cnt[1] = k
            break
    cnt[0] = n


def random_forest_state(rng):
    """Every array of the 12 x 1100 forest filled with random values (so an untouched slot is recognisable), n_t = ACC_N0."""
    N = T_BIG * C_BIG
    host = dict(state=rng.uniform(1, 2, (N, 6)), parent=rng.integers(-1, N, N).astype(np.int32),
                last_action=rng.uniform(1, 2, (N, 2)), has_prev=rng.integers(0, 2, N).astype(np.uint8),
                num_visit=rng.integers(0, 6, N).astype(np.int32), edge_states=rng.uniform(1, 2, (N, 18, 6)),
                edge_actions=rng.uniform(1, 2, (N, 16, 2)), edge_nstates=rng.integers(0, 19, N).astype(np.int32),
                edge_nactions=rng.integers(0, 17, N).astype(np.int32))
    host["xy"] = host["state"][:, :2].copy()
    cnt = np.zeros((T_BIG, 8), dtype=np.int32)
    cnt[:, 0], cnt[:, 1], cnt[:, 7] = ACC_N0, -1, -1
    cnt[:, 3], cnt[:, 4] = rng.integers(0, 50, T_BIG), rng.integers(0, 50, T_BIG)
    host["counters"] = cnt
    return host


def random_round(rng, host, specs):
    """specs: per tree (count, p_collide, {row: status}).  Parents are global ids among the tree's current nodes (few nodes,
    many candidates: repeats), 1 or 2 chunks run, every state / action row a distinct non-zero code with a tenth of the rows
    all zero."""
    counts = [s[0] for s in specs]
    B = sum(counts)
    off = np.concatenate([[0], np.cumsum(counts)])
    rnd = dict(status=np.zeros(B, np.int32), parent=np.zeros(B, np.int32), chunks_run=rng.integers(1, 3, B).astype(np.int32),
               end_state=rng.uniform(1, 2, (B, 6)), states=rng.uniform(1, 2, (B, 2, 9, 6)), actions=rng.uniform(1, 2, (B, 2, 8, 2)),
               node_id=np.full(B, -7, np.int32))
    rnd["states"][rng.random((B, 2, 9)) < 0.1] = 0.0
    rnd["actions"][rng.random((B, 2, 8)) < 0.1] = 0.0
    for t, (c, p, fixed) in enumerate(specs):
        st = np.where(rng.random(c) < p, COLLIDED, OK)
        for row, v in fixed.items():
            if row < c:
                st[row] = v
        rnd["status"][off[t]:off[t + 1]] = st
        rnd["parent"][off[t]:off[t + 1]] = t * C_BIG + rng.integers(0, host["counters"][t, 0], c)
    return rnd, counts, off


def run_accept(ctx, forest, host, rnd, counts, off):
    """The round through ditree_forest_accept and through accept_ref; every counter row, node id and tree array compared."""
    from ditreeonlineplanner_amd import _lib
    B = int(off[-1])
    rb = forest.rb
    for name in ("status", "parent", "chunks_run", "end_state", "states", "actions", "node_id"):
        getattr(rb, name)[:B].copy_(dev(rnd[name]))
    forest._set_offsets(counts)
    forest.ensure_maze()
    rd = rb.desc(0, B)
    _lib.check(ctx._h, _lib.lib().ditree_forest_accept(ctx._h, C.byref(forest.tree.desc), C.byref(forest.fdesc), C.byref(rd), 1,
                                                       ctx.stream), "forest_accept")
    for t in range(T_BIG):
        accept_ref(host, rnd, t, int(off[t]), int(off[t + 1]))
    got = forest.fcounters.cpu().numpy()
    assert np.array_equal(got, host["counters"]), np.nonzero((got != host["counters"]).any(axis=1))[0]
    nid = rb.node_id[:B].cpu().numpy()
    assert np.array_equal(nid, rnd["node_id"]), np.nonzero(nid != rnd["node_id"])[0][:10]
    for name in TREE_FIELDS:
        a = getattr(forest.tree, name).cpu().numpy()
        assert np.array_equal(a, host[name]), (name, np.nonzero((a != host[name]).reshape(len(a), -1).any(axis=1))[0][:10])


def upload_forest(forest, host):
    for name in TREE_FIELDS:
        getattr(forest.tree, name).copy_(dev(host[name]))
    forest.fcounters.copy_(dev(host["counters"]))


ACCEPT_CASES = {"goal_1023": {1023: GOAL}, "goal_1024": {1024: GOAL, 2300: GOAL}, "goal_2047": {2047: GOAL}, "no_goal": {},
                "goal_at_collision_1023": {1023: COLLIDED | GAC, 2000: GOAL}}


@pytest.mark.parametrize("case", list(ACCEPT_CASES))
def test_forest_accept_against_sequential_reference(ctx, big, case):
    """Twelve adjacent ranges in one call, then a second round on the same forest.  Tree 3 has 2 500 candidates (three passes of
    the 1024-wide scan) with its first GOAL at 1 023 / 1 024 / 2 047 / nowhere, or a goal-at-collision row at 1 023 whose phantom
    (1 024) lies across the pass boundary and wins over a later GOAL.  Tree 0 ends in GOAL and tree 1 starts with a
    goal-at-collision row (phantom = its row 1); tree 7 ends in one (it only latches: its row 0 of the second round is the
    phantom) and tree 8 starts with GOAL; tree 6 has a GOAL before its goal-at-collision row (the goal wins); tree 4 has one
    candidate, trees 2 and 5 none (rows and slots untouched); tree 9 only collides (n unchanged, iterations and candidates
    counted); tree 10 lands on C + 1 (overflow flag, n = C, the last node dropped) and tree 11 exactly on C (no flag, the root of
    nobody overwritten)."""
    rng = np.random.default_rng(31)
    host = random_forest_state(rng)
    upload_forest(big, host)
    full = {i: OK for i in range(8)}
    specs = [(5, 0.3, {4: GOAL}), (4, 0.3, {0: COLLIDED | GAC}), (0, 0, {}), (2500, 0.7, ACCEPT_CASES[case]), (1, 0.0, {}),
             (0, 0, {}), (8, 0.3, {2: GOAL, 5: COLLIDED | GAC}), (3, 0.3, {2: COLLIDED | GAC}), (3, 0.3, {0: GOAL}),
             (7, 1.0, {}), (8, 0.0, {**full, 1: COLLIDED, 6: COLLIDED}), (7, 0.0, {**full, 0: COLLIDED, 3: COLLIDED})]
    rnd, counts, off = random_round(rng, host, specs)
    before = host["counters"].copy()
    run_accept(ctx, big, host, rnd, counts, off)
    cnt = host["counters"]
    # the reference itself went through the cases named above
    big_goal = {"goal_1023": 1023, "goal_1024": 1024, "goal_2047": 2047, "no_goal": None, "goal_at_collision_1023": 1024}[case]
    if big_goal is None:
        assert cnt[BIG_TREE, 1] == -1 and cnt[BIG_TREE, 4] - before[BIG_TREE, 4] == 2500
    else:
        assert cnt[BIG_TREE, 1] == rnd["node_id"][off[BIG_TREE] + big_goal] >= 0
        assert cnt[BIG_TREE, 4] - before[BIG_TREE, 4] == big_goal + 1
    assert (cnt[BIG_TREE, 7] == off[BIG_TREE] + 1024) == (case == "goal_at_collision_1023")
    assert cnt[0, 1] >= 0 and cnt[1, 7] == off[1] + 1 and cnt[1, 5] == 1
    assert np.array_equal(cnt[[2, 5]], before[[2, 5]])
    assert cnt[6, 1] == rnd["node_id"][off[6] + 2] and cnt[6, 2] == 0 and cnt[6, 4] - before[6, 4] == 3
    assert cnt[7, 2] == 1 and cnt[7, 5] == 0 and cnt[7, 7] == -1
    assert cnt[8, 1] >= 0 and cnt[8, 4] - before[8, 4] == 1 and (rnd["node_id"][off[8] + 1:off[9]] == -1).all()
    assert cnt[9, 0] == before[9, 0] and cnt[9, 4] - before[9, 4] == 7 and cnt[9, 3] > before[9, 3]
    assert cnt[10, 0] == C_BIG and cnt[10, 6] == 1 and rnd["node_id"][off[11] - 1] == -1
    assert cnt[11, 0] == C_BIG and cnt[11, 6] == 0
    # the second round: tree 7's row 0 is the phantom, tree 1 (latched by its phantom) again, tree 10 stays full
    specs2 = [(2, 0.3, {}), (2, 0.3, {}), (1, 0.0, {}), (3, 0.3, {}), (0, 0, {}), (1, 0.0, {}), (0, 0, {}), (3, 0.3, {}),
              (0, 0, {}), (2, 0.0, {}), (2, 0.0, {}), (1, 0.0, {})]
    rnd2, counts2, off2 = random_round(rng, host, specs2)
    run_accept(ctx, big, host, rnd2, counts2, off2)
    assert cnt[7, 7] == off2[7] and cnt[7, 5] == 1 and cnt[7, 1] == rnd2["node_id"][off2[7]] >= 0
    assert cnt[1, 7] == off2[1] and (rnd2["node_id"][off2[10]:off2[11]] == -1).all() and cnt[11, 6] == 1


# ====================================================================== 4. the scene table at its limits
def limit_scenes():
    """64 different maps from the shipped mazes, their transposes and sub-rectangles (a 1 x N and an N x 1 among them), 15 000 to
    16 384 cells in all, the last one past cell 14 000 of the atlas at an offset that is no multiple of 16.  Start: a free cell
    (interior where there is one) with the car moving at 4 m/s; goal: a cell next to it."""
    names = ["boxes", "narrow_short", "random_huge", "random_large", "random_xlarge", "shapes", "val_maze_10", "val_maze_15",
             "val_maze_7", "Race_Track"]
    base = [load_maze(n) for n in names]
    huge, boxes, shapes = base[2], base[0], base[5]                              # base[7]: val_maze_15
    maps = base + [m.T.copy() for m in base]
    maps += [huge[:1, :], huge[:, 5:6]]                                           # 1 x 31 and 31 x 1
    maps += [huge[a:a + 15, b:b + 15] for a in (0, 5, 10, 16) for b in (0, 8, 16)]
    maps += [boxes[a:a + 14, b:b + 17] for a in (0, 3, 6) for b in (0, 3)]
    maps += [shapes[a:a + 15, b:b + 16] for a in (0, 2, 4) for b in (0, 2, 5)]
    maps += [huge[a:a + 12, b:b + 13] for a in (1, 9) for b in (2, 7)]
    maps += [base[7][a:a + 10, b:b + 11] for a, b in ((0, 0), (0, 4), (5, 0), (5, 4), (2, 2))]
    maps += [boxes[2:19, 1:20].T.copy(), shapes[1:20, 3:22].T.copy(), huge[3:27, 4:29], huge[2:20, 0:31], huge[0:20, 1:30]]
    maps += [huge[1:31, 0:31]]
    return [np.ascontiguousarray(m, dtype=np.float64) for m in maps]


def limit_scene(maze, rng):
    H, W = maze.shape
    free = np.argwhere(maze == 0)
    if not len(free):                                              # a border row: every cell a wall
        free = np.argwhere(maze >= 0)
    inner = [rc for rc in free if 0 < rc[0] < H - 1 and 0 < rc[1] < W - 1]
    rc = np.array(inner[rng.integers(len(inner))] if inner else free[rng.integers(len(free))])
    nb = [rc + d for d in ((0, 1), (1, 0), (0, -1), (-1, 0)) if 0 <= (rc + d)[0] < H and 0 <= (rc + d)[1] < W]
    goal_rc = nb[rng.integers(len(nb))] if nb else rc
    start = np.array([*(G.cell_rowcol_to_xy(rc, maze) + rng.uniform(-0.3, 0.3, 2)), rng.uniform(-np.pi, np.pi), 4.0, 1.0, 0.0])
    goal = np.array([*G.cell_rowcol_to_xy(goal_rc, maze), 0, 0, 0, 0])
    return maze, start, goal


def test_scene_forest_on_a_full_scene_table(ctx):
    """64 trees, one per scene of a 64-scene atlas of more than 15 000 cells, two tape rounds of 1 - 3 candidates per tree: every
    candidate's rollout against oracle.geometry.rollout_chunk on its own scene's maze and goal, from the parent the device
    chose among its tree's nodes."""
    from ditreeonlineplanner_amd import _lib
    from ditreeonlineplanner_amd.forest import SceneForestEngine, atlas_layout
    rng = np.random.default_rng(77)
    mazes = limit_scenes()
    offsets, dims, cells = atlas_layout(mazes)
    assert len(mazes) == 64 and cells == sum(m.size for m in mazes), "two scenes share a map"
    assert 15000 <= cells <= 16384 and offsets[-1] > 14000 and offsets[-1] % 16 != 0, (cells, offsets[-1])
    assert any(m.shape[0] == 1 for m in mazes) and any(m.shape[1] == 1 for m in mazes)
    scenes = [limit_scene(m, rng) for m in mazes]
    T, Cap = 64, 8
    forest = SceneForestEngine(ctx, scenes, T, Cap, edge_length=8, action_horizon=8, batch=3 * T)
    for t in range(T):
        forest.reset_tree(t, t)
    seen, differs = set(), 0
    for rnd in range(2):
        counts = rng.integers(1, 4, T)
        off = np.concatenate([[0], np.cumsum(counts)])
        B = int(off[-1])
        tree_of_row = np.searchsorted(off, np.arange(B), "right") - 1
        samples = np.zeros((B, 6))
        for b, t in enumerate(tree_of_row):
            H, W = mazes[t].shape
            samples[b, :2] = rng.uniform(-W / 2, W / 2), rng.uniform(-H / 2, H / 2)
        acts = np.zeros((B, 1, forest.P, 2))
        acts[:, 0, :8] = np.stack([rng.uniform(-12, 12, (B, 8)), rng.uniform(-3, 3, (B, 8))], axis=2)
        xy = forest.tree.xy.cpu().numpy()
        state = forest.tree.state.cpu().numpy()
        sizes = [int(v) for v in forest.n_nodes_host]
        forest.expand_round(dev(samples), dev(samples[:, :2]), inject_actions=dev(acts), counts_per_tree=counts)
        rb = forest.rb
        parent = rb.parent[:B].cpu().numpy()
        assert np.array_equal(parent, nn_ref(xy, samples[:, :2], off, Cap, sizes))
        status, steps = rb.status[:B].cpu().numpy(), rb.chunk_steps[:B, 0].cpu().numpy()
        states, end = rb.states[:B, 0].cpu().numpy(), rb.end_state[:B].cpu().numpy()
        for t in range(T):
            rows = slice(off[t], off[t + 1])
            env_goal = forest.scene_env_goals[t]
            exp = G.rollout_chunk(state[parent[rows]], acts[rows, 0, :8], mazes[t], env_goal, 8)
            assert np.array_equal(status[rows] & 0xff, exp["status"]), t
            assert np.array_equal((status[rows] & 0x100) != 0, exp["goal_at_collision"]), t
            assert np.array_equal(steps[rows], exp["n_steps"]), t
            assert np.abs(states[rows] - exp["states"]).max() < 1e-9, t
            assert np.abs(end[rows] - exp["end_state"]).max() < 1e-9, t
            seen.update(exp["status"].tolist())
            if t > 0:                                             # scene 0's record for this row would give another outcome
                e0 = G.rollout_chunk(state[parent[rows]], acts[rows, 0, :8], mazes[0], forest.scene_env_goals[0], 8)
                differs += int((e0["status"] != exp["status"]).any() or (e0["n_steps"] != exp["n_steps"]).any())
    assert seen == {G.STATUS_OK, G.STATUS_GOAL, G.STATUS_COLLIDED} and differs >= 20, (seen, differs)
