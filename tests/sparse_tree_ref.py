"""The planner's ``sparse_cell`` (include/ditree.h "sparse tree": the witness pruning of SST on a grid) written out sequentially in
plain numpy / Python, from the rule and not from the kernels: the cell function, the active nodes of a tree from scratch, the
accept on host arrays, and a round-level wrapper that applies the rule to ``oracle.rrt.OraclePlanner`` rounds.  Test
infrastructure only: no device code.

The rule.  The cell of a state (x, y, psi, ..) on a map of W x L metres: ix = clamp(floor((x + W/2) / cell), 0, nx-1), iy the same
with y and L, a = psi - 2pi*floor(psi / 2pi), ih = clamp(floor(a / w), 0, nh-1), w = 2pi / nh, 2pi = 2.0 * pi; nx = ceil(W / cell),
ny = ceil(L / cell); a state with a non-finite x, y or psi has no cell.  A node is ACTIVE iff it has a cell and (cost, id) is the
lexicographic minimum over the nodes of its tree in that cell.  The accept of a round, behind the mode's own tests (collided: no
node; with a bound: f >= U, no node): the contender of a cell is the remaining candidate with the smallest (c, b); it wins iff the
cell holds no node or c < the representative's cost; a winner gets a node, a goal-reaching candidate gets one in any case, a
candidate without a cell gets one and is never active, every other candidate is dominated; ids go out in candidate order; a
winner past the capacity gets no node and does not become the representative."""
import math

import numpy as np

from tests.anytime_pruned_ref import NO_BOUND, h_ref

OK, GOAL, COLLIDED = 0, 1, 2
TWO_PI = 2.0 * math.pi
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
MAX_CELLS = 2 ** 22


def grid_ref(rows, cols, s_global, cell, headings):
    """The grid of a map of ``rows x cols`` cells scaled by ``s_global`` -> dict(W, L, nx, ny, nh, cell, w, cells)."""
    W, L = float(s_global) * cols, float(s_global) * rows
    nx, ny = int(math.ceil(W / cell)), int(math.ceil(L / cell))
    return dict(W=W, L=L, nx=nx, ny=ny, nh=int(headings), cell=float(cell), w=TWO_PI / int(headings), cells=nx * ny * int(headings))


def cell_ref(grid, states):
    """The cell of every row of ``states`` (.., >= 3) -> int64, -1 for a state without one."""
    s = np.asarray(states, dtype=np.float64).reshape(-1, np.shape(states)[-1])
    x, y, psi = s[:, 0], s[:, 1], s[:, 2]
    ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(psi)
    x, y, psi = np.where(ok, x, 0.0), np.where(ok, y, 0.0), np.where(ok, psi, 0.0)
    with np.errstate(over="ignore"):
        fx = np.clip(np.floor((x + grid["W"] / 2.0) / grid["cell"]), 0, grid["nx"] - 1)
        fy = np.clip(np.floor((y + grid["L"] / 2.0) / grid["cell"]), 0, grid["ny"] - 1)
        a = psi - TWO_PI * np.floor(psi / TWO_PI)
        fh = np.clip(np.floor(a / grid["w"]), 0, grid["nh"] - 1)
    c = (fy.astype(np.int64) * grid["nx"] + fx.astype(np.int64)) * grid["nh"] + fh.astype(np.int64)
    return np.where(ok, c, -1)


def table_key(cost, node):
    return np.uint64((int(cost) << 32) | int(node))


def active_ref(states, cost, grid, base=0, stride=None):
    """From scratch, for the nodes ``states`` / ``cost`` of one tree whose first node is the global slot ``base``
    -> (active (n,) uint8, table (stride,) uint64: (cost << 32) | global slot of every cell's active node, all ones where
    there is none)."""
    n = len(states)
    cells = cell_ref(grid, states) if n else np.zeros(0, dtype=np.int64)
    best = {}
    for k in range(n):
        c = int(cells[k])
        if c < 0:
            continue
        if c not in best or (int(cost[k]), k) < (int(cost[best[c]]), best[c]):
            best[c] = k
    active = np.zeros(n, dtype=np.uint8)
    table = np.full(grid["cells"] if stride is None else stride, EMPTY, dtype=np.uint64)
    for c, k in best.items():
        active[k] = 1
        table[c] = table_key(cost[k], base + k)
    return active, table


def sparse_accept_ref(host, rnd, cnt, sstats, table, lo, hi, base, cap, grid, bound=None):
    """Rows [lo, hi) of the round ``rnd`` on the tree whose counter row is ``cnt`` (8,), sparse stats row ``sstats`` (4,), table
    row ``table`` and node slots [base, base + cap) of the arrays in ``host`` (those of tests/accept_best_ref.py plus ``active``;
    with ``bound`` = dict(goal, radius, reach, stats) also ``key``).  An empty range leaves everything untouched."""
    if hi == lo:
        return
    S, D = host["state"].shape[1], host["last_action"].shape[1]
    U = NO_BOUND
    if bound is not None:
        U = NO_BOUND if cnt[1] < 0 else int(host["cost"][cnt[1]])
    rnd["node_id"][lo:hi] = -1
    cnt[7] = -1
    # what every candidate would cost, where it would land, and who contends for each cell
    info = {}
    contender = {}
    pruned = 0
    for b in range(lo, hi):
        par, run, st = int(rnd["parent"][b]), int(rnd["chunks_run"][b]), int(rnd["status"][b])
        if st & 0xff == COLLIDED:
            continue
        es, ea = rnd["states"][b, :run].reshape(-1, S), rnd["actions"][b, :run].reshape(-1, D)
        es, ea = es[~(es == 0).all(axis=1)], ea[~(ea == 0).all(axis=1)]
        c = int(host["cost"][par]) + len(es) + 1
        f = c
        if bound is not None:
            f = c + h_ref(rnd["end_state"][b, 0], rnd["end_state"][b, 1], bound["goal"], bound["radius"], bound["reach"])
            if not f < U:
                pruned += 1
                continue
        cell = int(cell_ref(grid, rnd["end_state"][b][None])[0])
        info[b] = (c, f, cell, es, ea)
        if cell >= 0 and (cell not in contender or (c, b) < contender[cell]):
            contender[cell] = (c, b)
    n = int(cnt[0])
    dominated = retired = fresh = 0
    for b in range(lo, hi):
        par, run = int(rnd["parent"][b]), int(rnd["chunks_run"][b])
        cnt[4] += 1
        cnt[3] += run
        host["num_visit"][par] += 1
        if b not in info:
            continue
        c, f, cell, es, ea = info[b]
        won = False
        if cell >= 0 and contender[cell] == (c, b):
            won = table[cell] == EMPTY or c < int(table[cell] >> np.uint64(32))
        if cell >= 0 and not won and int(rnd["status"][b]) & 0xff != GOAL:
            dominated += 1
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
        host["cost"][k] = c
        if bound is not None:
            host["key"][k] = f
        host["active"][k] = 1 if won else 0
        if won:
            if table[cell] != EMPTY:
                host["active"][int(table[cell] & np.uint64(0xFFFFFFFF))] = 0
                retired += 1
            else:
                fresh += 1
            table[cell] = table_key(c, k)
        rnd["node_id"][b] = k
    cnt[0] = n
    best = None
    for b in range(lo, hi):
        k = int(rnd["node_id"][b])
        if int(rnd["status"][b]) & 0xff == GOAL and k >= 0 and (best is None or host["cost"][k] < host["cost"][best]):
            best = k
    if best is not None and (cnt[1] < 0 or host["cost"][best] < host["cost"][cnt[1]]):
        cnt[1] = best
    sstats[0], sstats[1], sstats[2], sstats[3] = sstats[0] + dominated, sstats[1] + retired, sstats[2] + fresh, dominated
    if bound is not None:
        u = NO_BOUND if cnt[1] < 0 else int(host["cost"][cnt[1]])
        bs = bound["stats"]
        bs[0], bs[1], bs[2], bs[3] = u, bs[1] + pruned, int(host["key"][base] >= u), pruned


def masked_nearest(queries, xy, mask):
    """The nearest node of every query among the nodes with ``mask`` set: squared distance, strict '<' in rising index (the lowest
    index on a tie), a NaN distance never wins; no winner -> node 0."""
    q, n = np.asarray(queries, dtype=np.float64), np.asarray(xy, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy = q[:, None, 0] - n[None, :, 0], q[:, None, 1] - n[None, :, 1]
        d = dx * dx + dy * dy
    d[np.isnan(d)] = np.inf
    d[:, ~np.asarray(mask, dtype=bool)] = np.inf
    arg = np.argmin(d, axis=1)
    arg[np.isinf(d[np.arange(len(q)), arg])] = 0
    return arg


# ---------------------------------------------------------------------- the rule inside the restated planner
class SparseOracle:
    """``OraclePlanner`` rounds under ``sparse_cell`` in one of the modes "best_of_round", "anytime" and "anytime_pruned"
    (``reach``: its metres per path row), with or without the near-parent rule (``near`` = (radius, reach)).  Keeps per node the
    cost, the key (pruned) and the active flag, per cell its representative, per round a record: the parents and what the search
    over ALL nodes of the mode would have given (``dense_parent``), node ids, dominated and bound-pruned candidates, the nodes
    retired."""

    def __init__(self, planner, solution, cell, headings=8, reach=None, near=None, goal_radius=0.5):
        assert solution in ("best_of_round", "anytime", "anytime_pruned") and not planner.sticky and len(planner.schedule) == 1
        self.pl, self.solution, self.near = planner, solution, near
        self.bounded = solution == "anytime_pruned"
        self.reach, self.goal_radius = reach, float(goal_radius)
        rows, cols = planner.maze.shape
        self.grid = grid_ref(rows, cols, 1.0, cell, headings)
        s = planner.start_state
        self.cost = [1]
        self.key = [1 + self.h(s[0], s[1])] if self.bounded else None
        self.active = [1]
        self.rep = {int(cell_ref(self.grid, np.asarray(s)[None])[0]): 0}
        self.incumbent = None
        self.solutions = self.dominated = self.retired = self.pruned = 0
        self.first_solution_candidates = None
        self.exhausted = False
        self.rounds = []

    def h(self, x, y):
        return h_ref(x, y, self.pl.env_goal, self.goal_radius, self.reach)

    def bound(self):
        return NO_BOUND if (self.incumbent is None or not self.bounded) else self.cost[self.incumbent]

    def search(self, queries, xy, mask):
        """The mode's parent choice among the nodes of ``mask``."""
        if self.near is None:
            return masked_nearest(queries, xy, mask)
        from tests.near_parent_ref import near_parent_ref
        return near_parent_ref(queries, xy, self.cost, self.near[0], self.near[1], key=np.where(mask, 0, 1), U=1)

    def round(self, samples, cond_goals):
        from tests.anytime_pruned_ref import _nearest
        from oracle import geometry as G
        pl, t = self.pl, self.pl.tree
        B = len(samples)
        U = self.bound()
        is_open = np.array(self.key) < U if self.bounded else np.ones(len(self.cost), dtype=bool)
        mask = is_open & (np.array(self.active) != 0)
        assert mask.any(), "a round is never drawn on a tree without a candidate parent"
        dense = self.search(np.asarray(samples)[:, :2], t.xy(), is_open)
        lists = ("states", "parents", "last_action", "has_prev", "num_visit", "edge_states", "edge_actions")
        keep = {k: list(getattr(t, k)) for k in lists}
        scalars = (pl.candidates, pl.iterations, pl.goal_node)
        with _nearest(lambda q, xy: self.search(q, xy, mask).astype(np.int32)):
            r = pl.expand_round(samples, cond_goals)
        for k, v in keep.items():                                 # take back that call's own first-goal accept
            setattr(t, k, v)
        pl.candidates, pl.iterations, pl.goal_node = scalars
        pl.env_done_latched = False
        info, contender, pruned = {}, {}, []
        for b in range(B):
            if r["status"][b] == G.STATUS_COLLIDED:
                continue
            run = int(r["chunks_run"][b])
            es, ea = r["states"][b, :run].reshape(-1, 6), r["actions"][b, :run].reshape(-1, 2)
            es, ea = es[~(es == 0).all(axis=1)], ea[~(ea == 0).all(axis=1)]
            c = self.cost[int(r["parent"][b])] + len(es) + 1
            f = c + self.h(r["end_state"][b, 0], r["end_state"][b, 1]) if self.bounded else c
            if self.bounded and not f < U:
                pruned.append(b)
                continue
            cell = int(cell_ref(self.grid, r["end_state"][b][None])[0])
            info[b] = (c, f, cell, es, ea)
            if cell >= 0 and (cell not in contender or (c, b) < contender[cell]):
                contender[cell] = (c, b)
        node_id = np.full(B, -1, dtype=np.int64)
        goals, dominated, retired = [], [], []
        for b in range(B):
            pl.candidates += 1
            t.num_visit[r["parent"][b]] += 1
            pl.iterations += int(r["chunks_run"][b])
            if b not in info:
                continue
            c, f, cell, es, ea = info[b]
            won = cell >= 0 and contender[cell] == (c, b) and (cell not in self.rep or c < self.cost[self.rep[cell]])
            if cell >= 0 and not won and r["status"][b] != G.STATUS_GOAL:
                dominated.append(b)
                continue
            k = node_id[b] = pl._append(r["end_state"][b].copy(), r["parent"][b], es, ea)
            self.cost.append(c)
            if self.bounded:
                self.key.append(f)
            self.active.append(1 if won else 0)
            if won:
                if cell in self.rep:
                    self.active[self.rep[cell]] = 0
                    retired.append(self.rep[cell])
                self.rep[cell] = int(k)
            if r["status"][b] == G.STATUS_GOAL:
                goals.append(b)
        if goals:
            self.solutions += len(goals)
            if self.first_solution_candidates is None:
                self.first_solution_candidates = scalars[0] + B
            best = min(goals, key=lambda b: (self.cost[node_id[b]], b))
            if self.incumbent is None or self.cost[node_id[best]] < self.cost[self.incumbent]:
                self.incumbent = int(node_id[best])
        self.dominated += len(dominated)
        self.retired += len(retired)
        self.pruned += len(pruned)
        pl.goal_node = self.incumbent
        self.exhausted = self.bounded and self.key[0] >= self.bound()
        rec = dict(r, node_id=node_id, goals=goals, dominated=dominated, retired=retired, pruned=pruned, dense_parent=dense,
                   incumbent=self.incumbent, nodes_after=len(self.cost), cost_after=list(self.cost), active_after=list(self.active))
        self.rounds.append(rec)
        return rec

    def active_nodes(self):
        return int(sum(self.active))

    def plan(self, tape, n_candidates, batch):
        """-> (path, actions) of the incumbent, else of the fallback node (planners/RRT.py:227-254)."""
        pl = self.pl
        H, W = pl.maze.shape
        while pl.candidates < n_candidates and not self.exhausted and \
                (self.incumbent is None or self.solution != "best_of_round"):
            B = min(batch, n_candidates - pl.candidates)
            s, c = tape.draw_round(B, W, H, pl.goal_state, goal_sample_rate=pl.gsr, goal_conditioning_bias=pl.gcb)
            self.round(s, c)
        node = self.incumbent if self.incumbent is not None else pl.fallback_node()
        return pl.path_to(node) if node is not None else (None, None)


_RUNS = {}


def sparse_run(solution, cell, headings=8, near_radius=None, seed=None, rounds=None, batch=None, near_speed=5.0, bound_speed=5.0):
    """The restated planner on the scenario of tests/anytime_pruned_ref.py under ``sparse_cell`` (computed once per setting,
    shared, left unchanged) -> the ``SparseOracle`` with ``path``, ``actions`` and the ``RandomTape`` it left (``tape``)."""
    from oracle import rrt as ORRT
    from tests import anytime_pruned_ref as APR
    seed = APR.SEED if seed is None else seed
    rounds = APR.ROUNDS if rounds is None else rounds
    batch = APR.BATCH if batch is None else batch
    k = (solution, float(cell), headings, near_radius, seed, rounds, batch, near_speed, bound_speed)
    if k not in _RUNS:
        near = None if near_radius is None else (float(near_radius), near_speed * APR.ENV_DT)
        o = SparseOracle(APR.scenario_planner(), solution, cell, headings, reach=bound_speed * APR.ENV_DT, near=near)
        o.tape = ORRT.RandomTape(seed)
        o.path, o.actions = o.plan(o.tape, rounds * batch, batch)
        _RUNS[k] = o
    return _RUNS[k]


# ---------------------------------------------------------------------- synthetic trees and rounds (kernel-level tests)
def synthetic_states(rng, n, grid, special=True):
    """n car states spread over the grid and past its borders, headings in [-7, 7]; ``special``: a few rows without a cell
    (NaN / inf in x, y or psi) and a few on exact cell and bin borders."""
    s = rng.uniform(1, 2, (n, 6))
    s[:, 0] = rng.uniform(-grid["W"] / 2 - 0.3, grid["W"] / 2 + 0.3, n)
    s[:, 1] = rng.uniform(-grid["L"] / 2 - 0.3, grid["L"] / 2 + 0.3, n)
    s[:, 2] = rng.uniform(-7.0, 7.0, n)
    if special and n >= 16:
        k = rng.choice(n, 8, replace=False)
        s[k[0], 0], s[k[1], 1], s[k[2], 2] = np.nan, np.inf, -np.inf
        s[k[3], 0], s[k[4], 0] = -grid["W"] / 2, grid["W"] / 2
        s[k[5], 2], s[k[6], 2], s[k[7], 2] = 0.0, -grid["w"], TWO_PI * 2
    return s


def synthetic_tree(rng, host, base, n0, grid, stride, cost_hi=400):
    """Nodes [base, base + n0) of the host arrays get states over the grid and random costs (the root: 1); their active flags
    and the table row follow from ``active_ref``.  -> the table row."""
    st = synthetic_states(rng, n0, grid)
    st[0, :3] = [0.1, 0.2, 0.3]
    host["state"][base:base + n0] = st
    host["xy"][base:base + n0] = st[:, :2]
    host["cost"][base:base + n0] = rng.integers(2, cost_hi, n0)
    host["cost"][base] = 1
    act, table = active_ref(st, host["cost"][base:base + n0], grid, base=base, stride=stride)
    host["active"][base:base + n0] = act
    return table
