"""numpy restatement of ditree_tree_rebase (include/ditree.h "re-planning on a kept tree") with plain loops: descendants by
walking parents, blocked nodes by the oracle's car collision test on the rows, compaction, the cost rule and the counters.
It shares no code with the product.  ``tree``: a dict of host arrays named like the fields of the device tree."""
import numpy as np

from oracle import geometry as G

NODE_FIELDS = ("state", "xy", "parent", "last_action", "has_prev", "num_visit", "edge_nstates", "edge_nactions")
E_DROP, E_ANCHOR = -1, -2


def maze8():
    """8 x 8, a border and two inner walls."""
    m = np.zeros((8, 8))
    m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = 1
    m[2, 2] = m[2, 3] = 1
    m[4, 5] = m[5, 5] = 1
    return m


def cell_state(maze, row, col, psi=0.0, dx=0.0, dy=0.0):
    x, y = G.cell_rowcol_to_xy([row, col], maze)
    return np.array([x + dx, y + dy, psi, 0.5, 0.1, 0.0])


def descendants(parent, n, anchor):
    """Nodes of [0, n) whose chain of parents reaches ``anchor`` (``anchor`` itself included)."""
    out = []
    for m in range(n):
        k = m
        while k >= 0 and k != anchor:
            k = int(parent[k])
        if k == anchor:
            out.append(m)
    return out


def row_collides(row, maze):
    with np.errstate(invalid="ignore"):                  # a NaN row: numpy's cast warns and lands out of the map
        return bool(G.is_colliding_car(np.asarray(row, dtype=np.float64), maze))


def collision_table(tree, n, maze):
    """Per-row collision answers for ``rebase_ref(..., collides=)``: ``edge_states`` (n, rows) and ``state`` (n,) booleans from
    one vectorised oracle call over all rows of the first n nodes (rows past a node's edge_nstates are answered too and never
    looked at).  The caller checks it against ``row_collides``."""
    def ask(rows):
        with np.errstate(invalid="ignore"):
            return np.asarray(G.is_colliding_car(np.asarray(rows, dtype=np.float64), maze), dtype=bool)
    return dict(edge_states=ask(tree["edge_states"][:n]), state=ask(tree["state"][:n]))


def node_blocked(tree, m, maze, first_row, collides=None):
    if collides is not None:
        return bool(collides["edge_states"][m, first_row:int(tree["edge_nstates"][m])].any() or collides["state"][m])
    rows = [tree["edge_states"][m, r] for r in range(first_row, int(tree["edge_nstates"][m]))] + [tree["state"][m]]
    for row in rows:
        if row_collides(row, maze):
            return True
    return False


def rebase_ref(tree, counters, maze, anchor, root_state=None, drop_states=0, drop_actions=0, collides=None):
    """``collides``: the rows' collision answers looked up in a ``collision_table`` instead of asked row by row (the default).
    -> dict: ``status`` (0, or the word a refused call leaves in dst's counters[0]); and for status 0 ``n`` nodes, the node
    fields over [0, n), ``edge_states`` / ``edge_actions`` as lists of the kept rows per node, ``cost`` (where ``tree`` has
    one), ``obstacle_ahead`` (where it has one), the 8 ``counters`` and ``new_id`` of every old node (-1: dropped)."""
    n = int(counters[0])
    fresh = root_state is not None
    if anchor >= n:
        return dict(status=E_ANCHOR)
    ns_a, na_a = int(tree["edge_nstates"][anchor]), int(tree["edge_nactions"][anchor])
    if fresh and not (0 < drop_states < ns_a and 0 <= drop_actions < na_a):
        return dict(status=E_DROP)
    blocked = {}
    for m in descendants(tree["parent"], n, anchor):
        first = 0
        if m == anchor:
            first = drop_states if fresh else ns_a       # as the root it keeps no edge row
        blocked[m] = node_blocked(tree, m, maze, first, collides)
    kept = []
    for m in sorted(blocked):
        k, clear = m, True
        while True:
            clear = clear and not blocked[k]
            if k == anchor:
                break
            k = int(tree["parent"][k])
        if clear or (m == anchor and not fresh):         # the anchor as the root stays, whatever stands on it
            kept.append(m)
    new_id = np.full(n, -1, dtype=np.int64)
    for i, m in enumerate(kept):
        new_id[m] = i + (1 if fresh else 0)
    n_new = len(kept) + (1 if fresh else 0)
    S, D = tree["state"].shape[1], tree["last_action"].shape[1]
    out = dict(status=0, n=n_new, new_id=new_id, state=np.zeros((n_new, S)), xy=np.zeros((n_new, 2)),
               parent=np.full(n_new, -1, dtype=np.int64), last_action=np.zeros((n_new, D)),
               has_prev=np.zeros(n_new, dtype=np.int64), num_visit=np.zeros(n_new, dtype=np.int64),
               edge_nstates=np.zeros(n_new, dtype=np.int64), edge_nactions=np.zeros(n_new, dtype=np.int64),
               edge_states=[np.zeros((0, S))] * n_new, edge_actions=[np.zeros((0, D))] * n_new)
    has_cost, has_flag = tree.get("cost") is not None, tree.get("obstacle_ahead") is not None
    if has_cost:
        out["cost"] = np.ones(n_new, dtype=np.int64)
    if has_flag:
        out["obstacle_ahead"] = np.zeros(n_new, dtype=np.int64)
    if fresh:
        out["state"][0] = root_state
        out["xy"][0] = np.asarray(root_state)[:2]
    cost_anchor = 1 + (ns_a - drop_states) + 1 if fresh else 1
    for m in kept:
        i = int(new_id[m])
        out["state"][i], out["xy"][i] = tree["state"][m], tree["xy"][m]
        out["num_visit"][i] = tree["num_visit"][m]
        if m == anchor and not fresh:
            continue                                     # the root: no parent, no edge, no previous action, cost 1, flag 0
        s0, a0 = (drop_states, drop_actions) if m == anchor else (0, 0)
        out["parent"][i] = 0 if m == anchor else new_id[int(tree["parent"][m])]
        out["last_action"][i], out["has_prev"][i] = tree["last_action"][m], tree["has_prev"][m]
        out["edge_states"][i] = tree["edge_states"][m, s0:int(tree["edge_nstates"][m])].copy()
        out["edge_actions"][i] = tree["edge_actions"][m, a0:int(tree["edge_nactions"][m])].copy()
        out["edge_nstates"][i], out["edge_nactions"][i] = len(out["edge_states"][i]), len(out["edge_actions"][i])
        if has_cost:
            out["cost"][i] = cost_anchor if m == anchor else int(tree["cost"][m]) - int(tree["cost"][anchor]) + cost_anchor
        if has_flag:
            out["obstacle_ahead"][i] = int(bool(G.check_obstacle_ahead(tree["state"][m], maze)))
    goal = int(counters[1])
    out["counters"] = np.array([n_new, new_id[goal] if 0 <= goal < n else -1, 0, 0, 0, 0, 0, -1], dtype=np.int64)
    return out


def path_rows(out, node):
    """The f64 rows and actions of the path root .. ``node`` in a restated tree, strung together as the planner's path is:
    per node below the root its edge states, then its state."""
    chain = []
    k = int(node)
    while k >= 0:
        chain.append(k)
        k = int(out["parent"][k])
    rows, acts = [], []
    for k in chain[::-1]:
        rows.extend(out["edge_states"][k])
        rows.append(out["state"][k])
        acts.extend(out["edge_actions"][k])
    return np.array(rows), np.array(acts).reshape(-1, out["last_action"].shape[1])
