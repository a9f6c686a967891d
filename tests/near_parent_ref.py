"""The planner's ``near_radius`` parent choice (include/ditree.h "near parent") written out sequentially in plain numpy /
Python, from the rule and not from the kernels.  Test infrastructure only: no device code.

The rule, for a query q over the candidates C = nodes lo .. hi-1 (with a mask: only those with key[n] < U):
  1. d2(n) = dx*dx + dy*dy; n* = the nearest node of C: strict '<', the lowest index on a tie, a NaN distance never wins.
  2. t = sqrt(d2(n*)) + radius, tau2 = t*t.  Near set N = {n*} + {n in C : d2(n) <= tau2}.
  3. g(n) = float(cost[n]) + sqrt(d2(n)) / reach.  The parent is the member of N with the smallest g; ties go to the smaller d2,
     then to the lower index.
  4. No node of C wins a '<' against +inf: ``lo`` (node 0, a forest tree's root).
All arithmetic is IEEE f64 with correctly rounded sqrt and division, which is what ``math.sqrt`` / ``np.sqrt`` and ``/`` give."""
import math

import numpy as np

NO_BOUND = 2 ** 31 - 1


def nearest_ref(q, xy, lo, hi, key=None, U=NO_BOUND):
    """Step 1 for one query -> (n*, d2(n*)), or (None, inf) when no candidate wins."""
    best, arg = math.inf, None
    for n in range(lo, hi):
        if key is not None and not key[n] < U:
            continue
        dx, dy = q[0] - xy[n, 0], q[1] - xy[n, 1]
        d = dx * dx + dy * dy
        if d < best:
            best, arg = d, n
    return arg, best


def near_parent_ref(queries, xy, cost, radius, reach, lo=0, hi=None, key=None, U=NO_BOUND, detail=False):
    """The loop form.  -> parents (B,) int64; ``detail``: also the nearest nodes (``lo`` where there is none) and the sizes of
    the near sets."""
    hi = len(xy) if hi is None else hi
    out = np.empty(len(queries), dtype=np.int64)
    nearest = np.empty(len(queries), dtype=np.int64)
    sizes = np.zeros(len(queries), dtype=np.int64)
    for i, q in enumerate(queries):
        q = (float(q[0]), float(q[1]))
        star, dstar = nearest_ref(q, xy, lo, hi, key, U)
        if star is None:
            out[i] = nearest[i] = lo
            continue
        t = math.sqrt(dstar) + radius
        tau2 = t * t
        win = None                                             # (g, d2, n) of the best member so far
        for n in range(lo, hi):
            if key is not None and not key[n] < U:
                continue
            dx, dy = q[0] - float(xy[n, 0]), q[1] - float(xy[n, 1])
            d = dx * dx + dy * dy
            if not (d <= tau2 or n == star):
                continue
            sizes[i] += 1
            g = float(cost[n]) + math.sqrt(d) / reach
            if win is None or g < win[0] or (g == win[0] and d < win[1]):      # n rises: an equal (g, d2) keeps the lower index
                win = (g, d, n)
        out[i], nearest[i] = win[2], star
    return (out, nearest, sizes) if detail else out


def near_parent_fast(queries, xy, cost, radius, reach, lo=0, hi=None, key=None, U=NO_BOUND, detail=False, block=256):
    """``near_parent_ref`` in array form (the large cases), ``block`` queries at a time."""
    hi = len(xy) if hi is None else hi
    B = len(queries)
    out = np.full(B, lo, dtype=np.int64)
    nearest = np.full(B, lo, dtype=np.int64)
    sizes = np.zeros(B, dtype=np.int64)
    if hi <= lo or B == 0:
        return (out, nearest, sizes) if detail else out
    nodes = np.asarray(xy[lo:hi], dtype=np.float64)
    c = np.asarray(cost[lo:hi]).astype(np.float64)
    closed = None if key is None else ~(np.asarray(key[lo:hi]) < U)
    idx = np.arange(hi - lo)
    block = max(1, min(block, 4_000_000 // (hi - lo)))             # a few (block, nodes) f64 temporaries at a time
    for b0 in range(0, B, block):
        q = np.asarray(queries[b0:b0 + block], dtype=np.float64)
        rows = np.arange(len(q))
        with np.errstate(invalid="ignore", over="ignore"):
            dx, dy = q[:, None, 0] - nodes[None, :, 0], q[:, None, 1] - nodes[None, :, 1]
            d = dx * dx + dy * dy
            cand = ~np.isnan(d)
            if closed is not None:
                cand &= ~closed[None, :]
            d1 = np.where(cand, d, np.inf)
            star = np.argmin(d1, axis=1)                           # first occurrence: the lowest index
            dstar = d1[rows, star]
            found = dstar < np.inf                                 # +inf never wins a strict '<' against the start value
            t = np.sqrt(dstar) + radius
            tau2 = t * t
            member = cand & ((d <= tau2[:, None]) | (idx[None, :] == star[:, None])) & found[:, None]
            g = np.where(member, c[None, :] + np.sqrt(np.where(member, d, 0.0)) / reach, np.inf)
            gmin = g.min(axis=1)
            tie = member & (g == gmin[:, None])
            d2 = np.where(tie, d, np.inf)
            dmin = d2.min(axis=1)
            pick = np.argmax(tie & (d2 == dmin[:, None]), axis=1)  # first occurrence: the lowest index
        sl = slice(b0, b0 + len(q))
        out[sl] = np.where(found, pick + lo, lo)
        nearest[sl] = np.where(found, star + lo, lo)
        sizes[sl] = member.sum(axis=1)
    return (out, nearest, sizes) if detail else out


# ---------------------------------------------------------------------- the rule inside the restated planner
_RUNS = {}


def near_run(solution, radius, near_speed=5.0, seed=None, rounds=None, scenario=None):
    """The restated planner of tests/accept_best_ref.py ("best_of_round", "anytime") or tests/anytime_pruned_ref.py
    ("anytime_pruned") on their shared scenario, with this rule as its parent choice (computed once per setting, shared, left
    unchanged) -> the oracle with ``path``, ``actions``, the ``RandomTape`` it left (``tape``) and, per round, ``nearest``: the
    plain nearest node of every candidate among the same candidates.  ``scenario``: another one, as (name, a function that
    returns a fresh ``OraclePlanner``, batch)."""
    from oracle import rrt as ORRT
    from tests import anytime_pruned_ref as APR
    from tests.accept_best_ref import SolutionOracle
    seed = APR.SEED if seed is None else seed
    rounds = APR.ROUNDS if rounds is None else rounds
    name, make_planner, batch = ("boxes", APR.scenario_planner, APR.BATCH) if scenario is None else scenario
    k = (solution, float(radius), float(near_speed), seed, rounds, name)
    if k in _RUNS:
        return _RUNS[k]
    reach = near_speed * APR.ENV_DT
    nearest = []
    if solution == "anytime_pruned":
        o = APR.PrunedOracle(make_planner(), 5.0 * APR.ENV_DT)

        def masked(q, xy, key, U):
            p, star, _ = near_parent_ref(q, xy, o.cost, radius, reach, key=key, U=U, detail=True)
            nearest.append(star)
            return p
        saved, APR.masked_nn_ref = APR.masked_nn_ref, masked
        ctx = None
    else:
        o = SolutionOracle(make_planner(), solution)

        def plain(q, xy):
            p, star, _ = near_parent_ref(q, xy, o.cost, radius, reach, detail=True)
            nearest.append(star)
            return p.astype(np.int32)
        ctx = APR._nearest(plain)
        ctx.__enter__()
    try:
        o.tape = ORRT.RandomTape(seed)
        o.path, o.actions = o.plan(o.tape, rounds * batch, batch)
    finally:
        if ctx is None:
            APR.masked_nn_ref = saved
        else:
            ctx.__exit__(None, None, None)
    assert len(nearest) == len(o.rounds)
    for r, star in zip(o.rounds, nearest):
        r["nearest"] = star
    _RUNS[k] = o
    return o
