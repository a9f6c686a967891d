"""Host side of ``RRT_Planner(reuse_tree=True)``: where on its remembered plan does the car stand?  numpy only, no device.

A plan is remembered as the chain of tree nodes it runs through: per node the f64 rows ``tree_path`` strings together -- the
node's edge states, then its own state (the root: its state alone).  An edge is the chunks its candidate ran: a chunk
contributes ``A + 1`` state rows, its start state included, and ``A`` action rows; action ``i`` of a chunk leads from its row
``i`` to its row ``i + 1``.  So a chunk's last row and the next chunk's first row are the same state, as are an edge's last
row and its node's state, and a node's state and the first row of every child's edge.  Of such equal rows the LAST one on
the plan is the car's: what lies behind it is what the car has still to drive.
"""
from __future__ import annotations

import numpy as np


class RememberedPlan:
    """The chain of a returned plan: node ids, edge row counts (states, actions), the rows per node, and the goal the tree was
    grown for.  ``phase``: per node the (state rows, action rows) an earlier re-base already took off the FRONT of its edge --
    the one node behind a fresh root has such an edge --, (0, 0) for every other."""

    def __init__(self, chain, ns, na, rows, goal_state, phase=None):
        self.chain, self.ns, self.na, self.rows = list(chain), list(ns), list(na), rows
        self.phase = [(0, 0)] * len(self.chain) if phase is None else [tuple(p) for p in phase]
        self.goal_state = np.asarray(goal_state, dtype=np.float64).copy()


def locate(plan, state, tol, A):
    """-> ``(anchor, drop_states, drop_actions)`` for ``ExpansionEngine.rebase``, or None when the tree cannot be kept.

    The car's row is the last row of the plan whose x, y, heading and speed (m, m, rad, m/s) all lie within ``tol`` of
    ``state`` -- among them the last one that equals ``state`` in every component, where there is one.  On a node's own
    state, or on the first row of an edge where that row is the parent's state, the car stands on a node: ``(node, 0, 0)``.
    Inside an edge, at row ``r`` = chunk ``j``, step ``i`` of the edge as the round made it (rows an earlier re-base took off
    its front counted in), it has driven the rows up to ``r`` and ``j * A + i`` actions of that edge: ``(node, r + 1,
    j * A + i)``, less what is off already.  That count of actions holds only for an edge the zero-row filter left whole, or
    cut at its end alone (a goal reached in mid-chunk): any other edge gives None."""
    full = np.asarray(state, dtype=np.float64)
    s = full[:4]
    hit = exact = None
    for k, rows in enumerate(plan.rows):
        near = np.flatnonzero((np.abs(rows[:, :4] - s) <= tol).all(axis=1))
        if near.size:
            hit = (k, int(near[-1]))
            same = [int(r) for r in near if rows.shape[1] == full.shape[0] and np.array_equal(rows[r], full)]
            if same:
                exact = (k, same[-1])
    if hit is None:
        return None
    # A car that starts from rest keeps x, y, heading and speed over its first step (only throttle and steering move), so the
    # rows behind a standing car lie within any tolerance of it.  A state that IS a row of the plan, every component bit for
    # bit -- the reset at the root's own state that online.plan_path makes after every plan -- stands on the last such row.
    k, r = hit if exact is None else exact
    ns, na = plan.ns[k], plan.na[k]
    if r == ns:
        return plan.chain[k], 0, 0
    if r == 0 and np.array_equal(plan.rows[k][0], plan.rows[k - 1][-1]):
        return plan.chain[k - 1], 0, 0
    off_s, off_a = plan.phase[k]
    whole, tail = divmod(ns + off_s, A + 1)
    if na + off_a != whole * A + max(tail - 1, 0):
        return None
    j, i = divmod(r + off_s, A + 1)
    drop_states, drop_actions = r + 1, j * A + i - off_a
    if not (drop_states < ns and 0 <= drop_actions < na):
        return None
    return plan.chain[k], drop_states, drop_actions
