"""The planner's ``solution="anytime_pruned"`` mode (include/ditree.h "branch and bound") written out sequentially in plain
numpy / Python: the heuristic, the masked nearest node, the bounded accept on host arrays, and a round-level wrapper that
applies the rule to ``oracle.rrt.OraclePlanner`` rounds.  Written from the rule, not from the kernels.  Test infrastructure
only: no device code.

The rule, in integer path rows: h(x, y) = 0 unless q = (norm(xy - goal) - goal_radius) / reach > 0, else min(ceil(q), 2^30);
key[n] = cost[n] + h(xy[n]); U = cost[incumbent] as of the round's start (INT32_MAX without one); a candidate's parent is the
nearest node among those with key < U; a candidate that did not collide gets a node only if cost + h(end) < U; the tree is
exhausted when key[root] >= U after an accept."""
import math
from contextlib import contextmanager

import numpy as np

from oracle import geometry as G
from oracle import rrt as ORRT

OK, GOAL, COLLIDED = 0, 1, 2
NO_BOUND = 2 ** 31 - 1
H_MAX = 2 ** 30


def h_ref(x, y, goal, goal_radius, reach):
    """Rows a path from (x, y) still needs at best."""
    d = float(G.norm2(x - goal[0], y - goal[1]))
    q = (d - goal_radius) / reach
    if not q > 0.0:                                       # inside the disc, or a NaN distance
        return 0
    return H_MAX if q >= H_MAX else min(int(math.ceil(q)), H_MAX)


def masked_nn_ref(queries, xy, key, U, lo=0, hi=None):
    """For every query the nearest node of xy[lo:hi] among the open ones (key < U): squared distance, the lowest index on a
    tie, a NaN distance never wins; no winner at all -> ``lo``."""
    hi = len(xy) if hi is None else hi
    out = np.empty(len(queries), dtype=np.int64)
    for i, q in enumerate(queries):
        best, arg = math.inf, lo
        for n in range(lo, hi):
            if not key[n] < U:
                continue
            dx, dy = q[0] - xy[n, 0], q[1] - xy[n, 1]
            d = dx * dx + dy * dy
            if d < best:
                best, arg = d, n
        out[i] = arg
    return out


def masked_nn_fast(queries, xy, key, U, lo=0, hi=None):
    """``masked_nn_ref`` in array form (the large cases): closed nodes and NaN distances count as +inf, argmin takes the first."""
    hi = len(xy) if hi is None else hi
    if hi <= lo:
        return np.full(len(queries), lo, dtype=np.int64)
    q, n = np.asarray(queries, dtype=np.float64), np.asarray(xy[lo:hi], dtype=np.float64)
    dx, dy = q[:, None, 0] - n[None, :, 0], q[:, None, 1] - n[None, :, 1]
    d = dx * dx + dy * dy
    d[np.isnan(d)] = np.inf
    d[:, ~(np.asarray(key[lo:hi]) < U)] = np.inf
    arg = np.argmin(d, axis=1)
    arg[np.isinf(d[np.arange(len(q)), arg])] = 0
    return arg + lo


def accept_bounded_ref(host, rnd, cnt, stats, lo, hi, base, cap, goal, goal_radius, reach):
    """Rows [lo, hi) of the round ``rnd`` on the tree whose counter row is ``cnt`` (8,), stats row ``stats`` (4,) and node slots
    [base, base + cap) of the arrays in ``host`` (those of tests/accept_best_ref.py plus ``key``).  An empty range leaves
    everything untouched."""
    if hi == lo:
        return
    S, D = host["state"].shape[1], host["last_action"].shape[1]
    U = NO_BOUND if cnt[1] < 0 else int(host["cost"][cnt[1]])
    rnd["node_id"][lo:hi] = -1
    cnt[7] = -1
    n = int(cnt[0])
    pruned = 0
    for b in range(lo, hi):
        par, run, st = int(rnd["parent"][b]), int(rnd["chunks_run"][b]), int(rnd["status"][b])
        cnt[4] += 1
        cnt[3] += run
        host["num_visit"][par] += 1
        if st & 0xff == COLLIDED:
            continue
        es, ea = rnd["states"][b, :run].reshape(-1, S), rnd["actions"][b, :run].reshape(-1, D)
        es, ea = es[~(es == 0).all(axis=1)], ea[~(ea == 0).all(axis=1)]
        c = int(host["cost"][par]) + len(es) + 1
        hh = h_ref(rnd["end_state"][b, 0], rnd["end_state"][b, 1], goal, goal_radius, reach)
        if not c + hh < U:
            pruned += 1
            continue
        if n >= cap:
            cnt[6] = 1
            continue
        k = base + n
        n += 1
        host["state"][k], host["xy"][k], host["parent"][k] = rnd["end_state"][b], rnd["end_state"][b, :2], par
        host["has_prev"][k], host["num_visit"][k] = 1, 0
        host["edge_states"][k, :len(es)], host["edge_nstates"][k] = es, len(es)
        host["edge_actions"][k, :len(ea)], host["edge_nactions"][k] = ea, len(ea)
        host["last_action"][k] = ea[-1] if len(ea) else 0.0
        host["cost"][k], host["key"][k] = c, c + hh
        rnd["node_id"][b] = k
    cnt[0] = n
    best = None
    for b in range(lo, hi):
        k = int(rnd["node_id"][b])
        if int(rnd["status"][b]) & 0xff == GOAL and k >= 0 and (best is None or host["cost"][k] < host["cost"][best]):
            best = k
    if best is not None and (cnt[1] < 0 or host["cost"][best] < host["cost"][cnt[1]]):
        cnt[1] = best
    u = NO_BOUND if cnt[1] < 0 else int(host["cost"][cnt[1]])
    stats[0], stats[1], stats[2], stats[3] = u, stats[1] + pruned, int(host["key"][base] >= u), pruned


@contextmanager
def _nearest(fn):
    """``OraclePlanner.expand_round`` searches through ``oracle.geometry.nn_argmin``: inside the block it searches with ``fn``."""
    saved = ORRT.G.nn_argmin
    ORRT.G.nn_argmin = fn
    try:
        yield
    finally:
        ORRT.G.nn_argmin = saved


class PrunedOracle:
    """``OraclePlanner`` rounds under ``solution="anytime_pruned"``: per node the cost and the key, per round a record
    (the bound, the open nodes, the parents and what the unmasked search would have given, node ids, pruned candidates, goal
    candidates that got a node, the incumbent after it, exhaustion).  ``plan`` is the planner's loop on a ``RandomTape``."""

    def __init__(self, planner, reach, goal_radius=0.5):
        assert not planner.sticky and len(planner.schedule) == 1
        self.pl, self.reach, self.goal_radius = planner, float(reach), float(goal_radius)
        s = planner.start_state
        self.cost = [1]
        self.key = [1 + self.h(s[0], s[1])]
        self.incumbent = None
        self.solutions = 0
        self.pruned = 0
        self.first_solution_candidates = None
        self.exhausted = False
        self.rounds = []

    def h(self, x, y):
        return h_ref(x, y, self.pl.env_goal, self.goal_radius, self.reach)

    def bound(self):
        return NO_BOUND if self.incumbent is None else self.cost[self.incumbent]

    def closed_nodes(self):
        u = self.bound()
        return 0 if u == NO_BOUND else sum(1 for k in self.key if k >= u)

    def round(self, samples, cond_goals):
        pl, t = self.pl, self.pl.tree
        B = len(samples)
        U = self.bound()
        key = np.array(self.key)
        assert (key < U).any(), "a round is never drawn on an exhausted tree"
        unmasked = G.nn_argmin(np.asarray(samples)[:, :2], t.xy())
        lists = ("states", "parents", "last_action", "has_prev", "num_visit", "edge_states", "edge_actions")
        keep = {k: list(getattr(t, k)) for k in lists}
        scalars = (pl.candidates, pl.iterations, pl.goal_node)
        with _nearest(lambda q, xy: masked_nn_ref(q, xy, key, U).astype(np.int32)):
            r = pl.expand_round(samples, cond_goals)
        for k, v in keep.items():                                 # take back that call's own first-goal accept
            setattr(t, k, v)
        pl.candidates, pl.iterations, pl.goal_node = scalars
        pl.env_done_latched = False
        node_id = np.full(B, -1, dtype=np.int64)
        goals, pruned = [], []
        for b in range(B):
            pl.candidates += 1
            t.num_visit[r["parent"][b]] += 1
            pl.iterations += int(r["chunks_run"][b])
            if r["status"][b] == G.STATUS_COLLIDED:
                continue
            run = int(r["chunks_run"][b])
            es, ea = r["states"][b, :run].reshape(-1, 6), r["actions"][b, :run].reshape(-1, 2)
            es, ea = es[~(es == 0).all(axis=1)], ea[~(ea == 0).all(axis=1)]
            c = self.cost[int(r["parent"][b])] + len(es) + 1
            f = c + self.h(r["end_state"][b, 0], r["end_state"][b, 1])
            if not f < U:
                pruned.append(b)
                continue
            node_id[b] = pl._append(r["end_state"][b].copy(), r["parent"][b], es, ea)
            self.cost.append(c)
            self.key.append(f)
            if r["status"][b] == G.STATUS_GOAL:
                goals.append(b)
        replaced = False
        if goals:
            self.solutions += len(goals)
            if self.first_solution_candidates is None:
                self.first_solution_candidates = scalars[0] + B
            best = min(goals, key=lambda b: (self.cost[node_id[b]], b))
            if self.incumbent is None or self.cost[node_id[best]] < self.cost[self.incumbent]:
                replaced = self.incumbent is not None
                self.incumbent = int(node_id[best])
        self.pruned += len(pruned)
        pl.goal_node = self.incumbent
        self.exhausted = self.key[0] >= self.bound()
        rec = dict(r, node_id=node_id, goals=goals, pruned=pruned, incumbent=self.incumbent, replaced=replaced, U=U,
                   closed_before=int((key >= U).sum()), nodes_before=len(key), unmasked_parent=unmasked,
                   exhausted=self.exhausted, nodes_after=len(self.key))
        self.rounds.append(rec)
        return rec

    def plan(self, tape, n_candidates, batch):
        """-> (path, actions) of the incumbent, else of the fallback node (planners/RRT.py:227-254)."""
        pl = self.pl
        H, W = pl.maze.shape
        while pl.candidates < n_candidates and not self.exhausted:
            B = min(batch, n_candidates - pl.candidates)
            s, c = tape.draw_round(B, W, H, pl.goal_state, goal_sample_rate=pl.gsr, goal_conditioning_bias=pl.gcb)
            self.round(s, c)
        node = self.incumbent if self.incumbent is not None else pl.fallback_node()
        return pl.path_to(node) if node is not None else (None, None)


# ---------------------------------------------------------------------- the shared scenario of the mode's tests
SEED, TAPE, BATCH, ROUNDS = 13, 5, 64, 4           # the scenario of tests/test_gpu_solution_modes.py
ENV_DT = 1.0 / 50.0                                 # car_env.py: one path row is one env step
_RUNS = {}


def scenario_planner(**kw):
    """A fresh ``OraclePlanner`` on boxes, (18, 13) -> (18, 17), edge length 32, action tape 5."""
    from oracle.tapes import ActionTape
    from tests.util import load_maze
    maze = load_maze("boxes")
    start = np.array([*G.cell_rowcol_to_xy([18, 13], maze), 0.0, 0, 0, 0])
    goal = np.array([*G.cell_rowcol_to_xy([18, 17], maze), 0, 0, 0, 0])
    return ORRT.OraclePlanner(maze, start, goal, ActionTape(TAPE).sampler(), edge_length=32, emulate_sticky_done=False, **kw)


def scenario_run(seed=SEED, bound_speed=5.0, rounds=ROUNDS):
    """The restatement's plan of the scenario (computed once per setting, shared, left unchanged) -> the ``PrunedOracle`` with
    ``path``, ``actions`` and the ``RandomTape`` it left (``tape``)."""
    k = (seed, float(bound_speed), rounds)
    if k not in _RUNS:
        po = PrunedOracle(scenario_planner(), bound_speed * ENV_DT)
        po.tape = ORRT.RandomTape(seed)
        po.path, po.actions = po.plan(po.tape, rounds * BATCH, BATCH)
        _RUNS[k] = po
    return _RUNS[k]
