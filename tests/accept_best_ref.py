"""The accept step of the planner's ``solution`` modes "best_of_round" / "anytime" (include/ditree.h ditree_accept_best) written
out sequentially: scan, commit and pick on host arrays, one candidate after the other, and a round-level wrapper that applies
the rule to ``oracle.rrt.OraclePlanner`` rounds.  Test infrastructure only: plain numpy / Python, no device code."""
import numpy as np

from oracle import geometry as G

OK, GOAL, COLLIDED, GAC = 0, 1, 2, 0x100


def accept_best_ref(host, rnd, cnt, lo, hi, base, cap):
    """Rows [lo, hi) of the round ``rnd`` on the tree whose counter row is ``cnt`` (8,) and whose node slots are
    [base, base + cap) of the arrays in ``host`` (state, xy, parent, last_action, has_prev, num_visit, edge_states,
    edge_actions, edge_nstates, edge_nactions, cost).  Every candidate counts, adds its chunks and visits its parent; a
    candidate that did not collide becomes a node (end state, parent, edge without all-zero rows, last kept action, cost =
    parent's cost + kept edge states + 1) -- nothing ends the range; a node past the tree's slots is dropped (node id -1,
    overflow flag, n = cap).  Then the goal candidates that hold a node compete by (cost, row): the winner replaces the
    incumbent cnt[1] when there is none or its cost is strictly smaller.  An empty range leaves everything untouched."""
    if hi == lo:
        return
    S, D = host["state"].shape[1], host["last_action"].shape[1]
    rnd["node_id"][lo:hi] = -1
    cnt[7] = -1
    n = int(cnt[0])
    for b in range(lo, hi):
        par, run, st = int(rnd["parent"][b]), int(rnd["chunks_run"][b]), int(rnd["status"][b])
        cnt[4] += 1
        cnt[3] += run
        host["num_visit"][par] += 1
        if st & 0xff == COLLIDED:
            continue
        if n >= cap:
            cnt[6] = 1
            continue
        k = base + n
        n += 1
        es, ea = rnd["states"][b, :run].reshape(-1, S), rnd["actions"][b, :run].reshape(-1, D)
        es, ea = es[~(es == 0).all(axis=1)], ea[~(ea == 0).all(axis=1)]
        host["state"][k], host["xy"][k], host["parent"][k] = rnd["end_state"][b], rnd["end_state"][b, :2], par
        host["has_prev"][k], host["num_visit"][k] = 1, 0
        host["edge_states"][k, :len(es)], host["edge_nstates"][k] = es, len(es)
        host["edge_actions"][k, :len(ea)], host["edge_nactions"][k] = ea, len(ea)
        host["last_action"][k] = ea[-1] if len(ea) else 0.0
        host["cost"][k] = host["cost"][par] + len(es) + 1
        rnd["node_id"][b] = k
    cnt[0] = n
    best = None
    for b in range(lo, hi):
        k = int(rnd["node_id"][b])
        if int(rnd["status"][b]) & 0xff == GOAL and k >= 0 and (best is None or host["cost"][k] < host["cost"][best]):
            best = k                                                  # strict: the lowest row wins a tie
    if best is not None and (cnt[1] < 0 or host["cost"][best] < host["cost"][cnt[1]]):
        cnt[1] = best


class SolutionOracle:
    """``OraclePlanner`` rounds under a ``solution`` mode.  ``round`` expands one round through
    ``OraclePlanner.expand_round`` (nearest nodes and rollouts against the tree as of the round's start), takes back what that
    call's own first-goal accept did to the tree, and applies the mode's accept instead; ``plan`` is the planner's loop on a
    ``RandomTape``.  Keeps per node the path cost, per round a record (node ids, statuses, the incumbent after it)."""

    def __init__(self, planner, solution):
        assert solution in ("first", "best_of_round", "anytime") and not planner.sticky
        self.pl, self.solution = planner, solution
        self.cost = [1]
        self.incumbent = None
        self.solutions = 0
        self.first_solution_candidates = None
        self.rounds = []

    def round(self, samples, cond_goals):
        pl, t = self.pl, self.pl.tree
        B = len(samples)
        lists = ("states", "parents", "last_action", "has_prev", "num_visit", "edge_states", "edge_actions")
        keep = {k: list(getattr(t, k)) for k in lists}
        scalars = (pl.candidates, pl.iterations, pl.goal_node)
        r = pl.expand_round(samples, cond_goals)
        for k, v in keep.items():
            setattr(t, k, v)
        pl.candidates, pl.iterations, pl.goal_node = scalars
        pl.env_done_latched = False
        node_id = np.full(B, -1, dtype=np.int64)
        goals = []
        for b in range(B):
            pl.candidates += 1
            t.num_visit[r["parent"][b]] += 1
            pl.iterations += int(r["chunks_run"][b])
            if r["status"][b] == G.STATUS_COLLIDED:
                continue
            run = int(r["chunks_run"][b])
            es, ea = r["states"][b, :run].reshape(-1, 6), r["actions"][b, :run].reshape(-1, 2)
            es, ea = es[~(es == 0).all(axis=1)], ea[~(ea == 0).all(axis=1)]
            node_id[b] = pl._append(r["end_state"][b].copy(), r["parent"][b], es, ea)
            self.cost.append(self.cost[int(r["parent"][b])] + len(es) + 1)
            if r["status"][b] == G.STATUS_GOAL:
                goals.append(b)
                if self.solution == "first":                          # RRT.py:213-217: the rest of the round is dropped
                    break
        replaced = False
        if goals:
            self.solutions += len(goals)
            if self.first_solution_candidates is None:
                self.first_solution_candidates = scalars[0] + B       # whole rounds, as the planner counts what it drew
            best = min(goals, key=lambda b: (self.cost[node_id[b]], b))
            if self.incumbent is None or self.cost[node_id[best]] < self.cost[self.incumbent]:
                replaced = self.incumbent is not None
                self.incumbent = int(node_id[best])
        pl.goal_node = self.incumbent
        rec = dict(r, node_id=node_id, goals=goals, incumbent=self.incumbent, replaced=replaced)
        self.rounds.append(rec)
        return rec

    def plan(self, tape, n_candidates, batch):
        """-> (path, actions) of the incumbent, else of the fallback node (planners/RRT.py:227-254)."""
        pl = self.pl
        H, W = pl.maze.shape
        while pl.candidates < n_candidates and (self.incumbent is None or self.solution == "anytime"):
            B = min(batch, n_candidates - pl.candidates)
            s, c = tape.draw_round(B, W, H, pl.goal_state, goal_sample_rate=pl.gsr, goal_conditioning_bias=pl.gcb)
            self.round(s, c)
        node = self.incumbent if self.incumbent is not None else pl.fallback_node()
        return pl.path_to(node) if node is not None else (None, None)
