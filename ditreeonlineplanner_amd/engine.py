"""Device-resident tree + round driver of the DiTree expansion engine.

The reference keeps a Python list of ``Node`` objects (planners/base_planner.py:24-34)
and expands one candidate at a time (planners/RRT.py:131-219).  Here the tree is a
struct of arrays in HBM and a *round* expands B candidates against the tree snapshot:
nearest node -> n_chunks x [local map -> conditioning -> denoiser -> 8-step rollout with
goal / collision tests] -> accept in candidate order.  B = 1 is the reference loop.

With ``world_size > 1`` (one process per GPU, torch.distributed / RCCL) each rank expands
a contiguous block of the round's candidates and the candidate records are all-gathered
before the (replicated, deterministic) accept step, so every rank holds the same tree.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, NamedTuple

import numpy as np
import torch

from . import _lib
from ._lib import Bound, Near, Round, RoundParams, Sparse, Tree, check, lib
from .ops import CAR_NORM, Context, _dbl, _flt, _ptr, local_axis

CNT_NODES, CNT_GOAL, CNT_LATCH, CNT_ITERS, CNT_CANDS, CNT_STICKY, CNT_OVERFLOW, CNT_PHANTOM = range(8)
# include/ditree.h ditree_bound.stats: the bound after the last accept, candidates pruned since the reset, no open node left,
# candidates pruned by the last accept
ST_BOUND, ST_PRUNED, ST_EXHAUSTED, ST_PRUNED_ROUND = range(4)
NO_BOUND = 2 ** 31 - 1
STATS_ROOT = np.array([NO_BOUND, 0, 0, 0], dtype=np.int32)
# include/ditree.h ditree_sparse.stats: candidates dominated and nodes retired since the rebuild, active nodes, candidates
# dominated by the last accept; a tree that holds its root alone has one active node
SP_DOMINATED, SP_RETIRED, SP_ACTIVE, SP_DOMINATED_ROUND = range(4)
SPARSE_ROOT = np.array([0, 0, 1, 0], dtype=np.int32)
SPARSE_MAX_CELLS = 2 ** 22


class DeviceTree:
    """planners/base_planner.py:24-34 ``Node`` as a struct of arrays in HBM (include/ditree.h ditree_tree).  ``state_dim`` /
    ``action_dim``: 6 / 2 for the car, 29 / 8 for the ant; ``hist``: keep the last three rows of every node's edge (what the
    first sampler call of a child sees with obs_history 3 -- the ant); ``cost``: keep every node's path cost (the rows
    ``tree_path`` returns for it), which the ``solution`` modes other than "first" rank goal nodes by; ``key``: keep beside it
    every node's key = cost + the rows it still needs at best (include/ditree.h "branch and bound": "anytime_pruned"), and a
    stats row behind the counters, in the same small buffer, so that one copy reads both; ``active``: keep every node's active
    flag of the sparse tree (include/ditree.h "sparse tree"), and its stats row in that buffer too."""

    def __init__(self, ctx: Context, capacity: int, n_chunks: int, A: int, track_obstacle_ahead: bool = False,
                 state_dim: int = 6, action_dim: int = 2, hist: bool = False, cost: bool = False, key: bool = False,
                 active: bool = False):
        dev = ctx.device
        self.capacity, self.n_chunks, self.A = capacity, n_chunks, A
        self.S, self.D = S, D = int(state_dim), int(action_dim)
        f64, i32, u8 = torch.float64, torch.int32, torch.uint8
        self.state = torch.zeros(capacity, S, dtype=f64, device=dev)
        self.xy = torch.zeros(capacity, 2, dtype=f64, device=dev)
        self.parent = torch.full((capacity,), -1, dtype=i32, device=dev)
        self.last_action = torch.zeros(capacity, D, dtype=f64, device=dev)
        self.has_prev = torch.zeros(capacity, dtype=u8, device=dev)
        self.num_visit = torch.zeros(capacity, dtype=i32, device=dev)
        self.edge_states = torch.zeros(capacity, n_chunks * (A + 1), S, dtype=f64, device=dev)
        self.edge_actions = torch.zeros(capacity, n_chunks * A, D, dtype=f64, device=dev)
        self.edge_nstates = torch.zeros(capacity, dtype=i32, device=dev)
        self.edge_nactions = torch.zeros(capacity, dtype=i32, device=dev)
        # counters [+ the bound's stats row] [+ the sparse tree's stats row]
        self._cnt_buf = torch.zeros(8 + (4 if key else 0) + (4 if active else 0), dtype=i32, device=dev)
        self.counters = self._cnt_buf[:8]
        self.stats = self._cnt_buf[8:12] if key else None
        self.stats_host = STATS_ROOT.copy() if key else None
        self.sparse_stats = self._cnt_buf[-4:] if active else None
        self.sparse_host = SPARSE_ROOT.copy() if active else None
        # RRT.py:202-205: per-node check_obstacle_ahead flag, kept only for run_type > 0
        self.obstacle_ahead = torch.zeros(capacity, dtype=u8, device=dev) if track_obstacle_ahead else None
        # rank holding each node's edge rows (sharded rounds keep trajectories on the producing rank); -1 = every rank
        self.edge_owner = torch.full((capacity,), -1, dtype=i32, device=dev)
        self.hist = torch.zeros(capacity, 3, S, dtype=f64, device=dev) if hist else None
        self.hist_n = torch.zeros(capacity, dtype=i32, device=dev) if hist else None
        self.cost = torch.zeros(capacity, dtype=i32, device=dev) if cost or key or active else None   # not part of the descriptor
        self.key = torch.zeros(capacity, dtype=i32, device=dev) if key else None             # nor this (ditree_bound)
        self.active = torch.zeros(capacity, dtype=u8, device=dev) if active else None        # nor this (ditree_sparse)
        self.desc = Tree(capacity, n_chunks, A, S, D, *[None if t is None else t.data_ptr() for t in (
            self.state, self.xy, self.parent, self.last_action, self.has_prev, self.num_visit,
            self.edge_states, self.edge_actions, self.edge_nstates, self.edge_nactions, self.obstacle_ahead,
            self.edge_owner, self.hist, self.hist_n, self.counters)])
        self.record_doubles = int(lib().ditree_record_doubles(C.byref(self.desc)))
        self.n_nodes_host = 0

    def write_root(self, slot, span, start_state):
        """The root row of a tree that owns the ``span`` slots from ``slot`` (the whole tree, or one tree of a forest)."""
        r = int(slot)
        s = torch.as_tensor(np.asarray(start_state, dtype=np.float64), device=self.state.device)
        self.state[r] = s
        self.xy[r] = s[:2]
        self.parent[r] = -1
        self.last_action[r] = 0
        self.has_prev[r] = 0
        self.num_visit[r:r + span].zero_()
        self.edge_nstates[r] = 0
        self.edge_nactions[r] = 0
        self.edge_owner[r] = -1
        if self.hist is not None:                       # RRT.py:146: the root's child sees curr_state[None, None, :]
            self.hist[r].zero_()
            self.hist[r, 2] = s
            self.hist_n[r] = 1
        if self.cost is not None:
            self.cost[r] = 1                            # the root's path is its own state row

    def reset(self, start_state):
        self.write_root(0, self.capacity, start_state)
        if self.obstacle_ahead is not None:
            self.obstacle_ahead.zero_()
        self.counters.zero_()
        self.counters[CNT_NODES] = 1
        self.counters[CNT_GOAL] = -1
        self.counters[CNT_PHANTOM] = -1
        if self.stats is not None:                      # the root's key is the engine's to set: it knows the goal
            self.stats.copy_(torch.as_tensor(STATS_ROOT))
            self.stats_host = STATS_ROOT.copy()
        if self.sparse_stats is not None:               # the table and the flags are the engine's to rebuild: it knows the map
            self.sparse_host = SPARSE_ROOT.copy()
        self.n_nodes_host = 1

    def read_counters(self):
        c = self._cnt_buf.cpu().numpy()                 # one small copy: the counters and, where kept, the stats rows
        self.n_nodes_host = int(c[CNT_NODES])
        if self.stats is not None:
            self.stats_host = c[8:12]
        if self.sparse_stats is not None:
            self.sparse_host = c[-4:]
        return c[:8]


class RoundBuffers:
    def __init__(self, ctx: Context, B: int, n_chunks: int, A: int, state_dim: int = 6, action_dim: int = 2, hist: bool = False,
                 record_doubles: int = _lib.RECORD_DOUBLES):
        dev = ctx.device
        self.B = B
        self.S, self.D, self.with_hist, self.R = int(state_dim), int(action_dim), bool(hist), int(record_doubles)
        S, D = self.S, self.D
        f64, i32 = torch.float64, torch.int32
        self.parent = torch.zeros(B, dtype=i32, device=dev)
        self.status = torch.zeros(B, dtype=i32, device=dev)
        self.chunks_run = torch.zeros(B, dtype=i32, device=dev)
        self.end_state = torch.zeros(B, S, dtype=f64, device=dev)
        self.states = torch.zeros(B, n_chunks, A + 1, S, dtype=f64, device=dev)
        self.actions = torch.zeros(B, n_chunks, A, D, dtype=f64, device=dev)
        self.chunk_steps = torch.zeros(B, n_chunks, dtype=i32, device=dev)
        self.node_id = torch.full((B,), -1, dtype=i32, device=dev)
        # sharded rounds only (allocated on first use): exchanged records (96 bytes for the car) and what they carry beyond
        # the SoA above
        self.records = self.last_action = self.first_action = self.hist = self.hist_n = None

    def ensure_exchange(self, rows):
        if self.records is None or self.records.shape[0] < rows:
            dev = self.parent.device
            n = max(rows, self.B)
            self.records = torch.zeros(rows, self.R, dtype=torch.float64, device=dev)
            self.last_action = torch.zeros(n, self.D, dtype=torch.float64, device=dev)
            self.first_action = torch.zeros(n, self.D, dtype=torch.float64, device=dev)
            if self.with_hist:
                self.hist = torch.zeros(n, 3, self.S, dtype=torch.float64, device=dev)
                self.hist_n = torch.zeros(n, dtype=torch.int32, device=dev)

    def fields(self):
        return (self.parent, self.status, self.chunks_run, self.end_state, self.states, self.actions,
                self.chunk_steps, self.node_id)

    def desc(self, lo=0, n=None, own=None, shard=0):
        """Round descriptor of rows [lo, lo + n).  ``own`` = (own_lo, own_n) in the descriptor's row numbering and
        ``shard`` = candidates per rank for a sharded round (default: every row was produced here)."""
        n = self.B - lo if n is None else n
        ptrs = [t[lo:lo + n].data_ptr() if n > 0 else t.data_ptr() for t in self.fields()]
        la = fa = hs = hn = None
        if shard and self.last_action is not None:
            la, fa = self.last_action[lo:].data_ptr(), self.first_action[lo:].data_ptr()
            if self.hist is not None:
                hs, hn = self.hist[lo:].data_ptr(), self.hist_n[lo:].data_ptr()
        own_lo, own_n = (0, n) if own is None else own
        return Round(n, *ptrs, la, fa, own_lo, own_n, shard, hs, hn)


def allgather_round_fields(fields, per, rank, world, group=None):
    """One fixed-stride all-gather per candidate-record field.

    Every field is a tensor whose leading axis is the round's candidate index; rank r produced
    rows [r*per, (r+1)*per).  After the call all ranks hold all rows, so the replicated,
    deterministic accept step builds the same tree everywhere.  With the nccl backend (RCCL) the
    gather runs device-to-device over xGMI; with gloo (CPU tests, or several ranks sharing one
    GPU in a test) CUDA tensors are staged through the host.
    """
    import torch.distributed as dist
    backend = dist.get_backend(group)
    pairs = []
    for t in fields:
        if t.shape[0] < per * world:
            raise ValueError("round buffers must hold ceil(B / world) * world candidates")
        flat = t[: per * world]
        pairs.append((flat, flat[rank * per:(rank + 1) * per]))
    if backend == "gloo":
        for flat, mine in pairs:
            if flat.is_cuda:
                host = torch.empty(flat.shape, dtype=flat.dtype)
                dist.all_gather_into_tensor(host, mine.cpu().contiguous(), group=group)
                flat.copy_(host)
            else:
                dist.all_gather_into_tensor(flat, mine.clone(), group=group)
        return
    # RCCL: one collective per field -- ONE per round in the default exchange (the packed records), seven with
    # DITREE_GATHER_EDGES=1 (measured 0.4 ms of a 26 ms round on one MI355X).  With
    # DITREE_COALESCE=1 they are issued as one grouped launch through torch's coalescing manager
    # (no measurable gain on one GPU, so the plain, universally supported calls are the default).
    import os
    sends = [mine.clone() for _, mine in pairs]
    cm = getattr(dist, "_coalescing_manager", None) if os.environ.get("DITREE_COALESCE", "0") == "1" else None
    if cm is not None and not _COALESCE_BROKEN[0]:
        try:
            with cm(group=group, device=pairs[0][0].device, async_ops=False):
                for (flat, _), snd in zip(pairs, sends):
                    dist.all_gather_into_tensor(flat, snd, group=group)
            return
        except Exception:                              # pragma: no cover - depends on the torch build
            _COALESCE_BROKEN[0] = True
    for (flat, _), snd in zip(pairs, sends):
        dist.all_gather_into_tensor(flat, snd, group=group)


_COALESCE_BROKEN = [False]


def default_shard():
    """(rank, world_size, process_group) a facade shards over when the caller names none.  Sharding over the default
    torch.distributed group is OPT-IN -- DITREE_SHARD_DEFAULT_GROUP=1, which `python -m ditreeonlineplanner_amd.run` sets when
    it joins the group for a driver script -- because it is only sound when every rank plans the SAME scenario with identical
    RNG streams: a data-parallel harness whose ranks plan different scenarios would dead-lock or mix trees in the per-round
    collectives.  Everything else gets (0, 1, None); explicit ``rank`` / ``world_size`` / ``process_group`` always win."""
    import os
    import torch.distributed as dist
    if os.environ.get("DITREE_SHARD_DEFAULT_GROUP", "0") == "1" and dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size(), None
    return 0, 1, None


def env_goal_of(maze, goal_state):
    """env.goal after planner.reset -> env.reset(options): the centre of the goal cell (car_env.py:189-201,225-226)."""
    H, W = np.asarray(maze).shape
    gi = np.floor((H / 2 - goal_state[1]) / 1.0)
    gj = np.floor((goal_state[0] + W / 2) / 1.0)
    return np.array([(gj + 0.5) * 1.0 - W / 2, H / 2 - (gi + 0.5) * 1.0])


def ant_cell_centre(maze, goal_state, s_global):
    """The centre of the cell ``goal_state[:2]`` lies in, in the map scaled by ``s_global``: an ant env's ``desired_goal``
    without its position noise."""
    H, W = np.asarray(maze).shape
    sg = float(s_global)
    gi = np.floor((H / 2 * sg - goal_state[1]) / sg)
    gj = np.floor((goal_state[0] + W / 2 * sg) / sg)
    return np.array([(gj + 0.5) * sg - W / 2 * sg, H / 2 * sg - (gi + 0.5) * sg])


def parent_chain(tr, node, n_nodes, base=0):
    """The walk from ``node`` up to the root over the stored parents, root first.  The tree is the ``n_nodes`` slots from
    ``base`` (a forest's tree; ``node`` is local to it, the stored parents are global).  -> (local ids, their slots on the
    tree's device)."""
    parents = tr.parent[base: base + n_nodes].cpu().numpy()
    chain = []
    k = int(node)
    while k >= 0:
        chain.append(k)
        p = int(parents[k])
        k = -1 if p < 0 else p - base
    chain = chain[::-1]
    return chain, torch.as_tensor(chain, device=tr.state.device, dtype=torch.long) + base


def tree_path(tr, node, n_nodes, base=0, edge_rows=None):
    """planners/base_planner.py:342-363 on a ``DeviceTree``: float32 path (edge states + node states) and actions from the
    root to ``node`` (``parent_chain``'s arguments).  ``edge_rows(idx, es, ea, ns, na)``: what a sharded engine does to the
    chain's edge rows first."""
    chain, idx = parent_chain(tr, node, n_nodes, base)
    st = tr.state[idx].cpu().numpy()
    rows = (tr.edge_states[idx], tr.edge_actions[idx], tr.edge_nstates[idx], tr.edge_nactions[idx])
    if edge_rows is not None:
        rows = edge_rows(idx, *rows)
    es, ea, ns, na = (x.cpu().numpy() for x in rows)
    path, actions = [], []
    for j, nd in enumerate(chain):
        if nd != 0:
            path.extend(es[j, : ns[j]])
            actions.extend(ea[j, : na[j]])
        path.append(st[j])
    path = np.array(path, dtype=np.float32) if path else None
    actions = np.array(actions, dtype=np.float32) if actions else None
    return path, actions


SOLUTIONS = ("first", "best_of_round", "anytime", "anytime_pruned")
ANYTIME = ("anytime", "anytime_pruned")           # the modes that plan on after the first goal-reaching round
CAR_GOAL_RADIUS = 0.5                             # car_env.py:346-351, the rollout's goal test
CAR_REACH = 5 * 0.02                              # planners/base_planner.py:87 max_v x the car env's dt: metres per path row


def check_reach(reach):
    """The metres a path row is assumed to cover at most ("anytime_pruned"): a positive finite number."""
    try:
        r = float(reach)
    except (TypeError, ValueError):
        r = float("nan")
    if not (np.isfinite(r) and r > 0.0):
        raise ValueError(f"reach must be a positive finite number of metres per path row, got {reach!r}")
    return r


def check_near(near_radius, near_reach, solution, ant=False, prop_duration=None):
    """The near-parent search (include/ditree.h "near parent") -> (radius [m], reach [m per path row]), or None when it is off.
    Its scope is the cost column's -- a ``solution`` other than "first", whose own scope ``check_solution`` holds: the car, one
    rank, run_type 0 -- and a single ``prop_duration`` entry (the chunk-budget search is the plain nearest node)."""
    if near_radius is None:
        if near_reach is not None:
            raise ValueError("near_reach belongs to near_radius (near_radius is None)")
        return None

    def positive(name, v, unit):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or v <= 0:
            raise ValueError(f"{name} must be a positive finite number of {unit}, got {v!r}")
        return float(v)
    radius = positive("near_radius", near_radius, "metres")
    reach = positive("near_reach", CAR_REACH if near_reach is None else near_reach, "metres per path row")
    if solution == "first":
        raise ValueError("near_radius needs a solution other than 'first' (the cost column belongs to 'best_of_round', 'anytime' "
                         "and 'anytime_pruned')")
    if ant:
        raise NotImplementedError("near_radius: the car only (the ant's tree has no cost column)")
    if prop_duration is not None and len(prop_duration) > 1:
        raise NotImplementedError("near_radius: a single prop_duration entry (the chunk-budget search is the plain nearest node)")
    return radius, reach


def sparse_grid(maze_shape, s_global, cell, headings):
    """The grid of the sparse tree on a map of ``rows x cols`` cells scaled by ``s_global`` (include/ditree.h "sparse tree") ->
    (W, L, nx, ny): the metres ``random_node_sample`` draws in, and ceil(W / cell), ceil(L / cell) cells."""
    rows, cols = (int(v) for v in maze_shape)
    W, L = float(s_global) * cols, float(s_global) * rows
    nx, ny = int(np.ceil(W / cell)), int(np.ceil(L / cell))
    if nx < 1 or ny < 1 or nx * ny * int(headings) > SPARSE_MAX_CELLS:
        raise ValueError(f"sparse_cell={cell!r} with sparse_headings={headings} gives {nx} x {ny} x {headings} cells on a map of "
                         f"{W} m x {L} m, more than {SPARSE_MAX_CELLS} per tree")
    return W, L, nx, ny


def check_sparse(sparse_cell, sparse_headings, solution, ant=False, prop_duration=None):
    """The sparse tree (include/ditree.h "sparse tree") -> (cell [m], heading bins), or None when it is off.  Its scope is the
    cost column's, as ``check_near``'s: a ``solution`` other than "first" (whose own scope ``check_solution`` holds: the car,
    one rank, run_type 0) and a single ``prop_duration`` entry."""
    if sparse_cell is None:
        if sparse_headings is not None:
            raise ValueError("sparse_headings belongs to sparse_cell (sparse_cell is None)")
        return None
    v = sparse_cell
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or v <= 0:
        raise ValueError(f"sparse_cell must be a positive finite number of metres, got {v!r}")
    h = 8 if sparse_headings is None else sparse_headings
    if isinstance(h, bool) or not isinstance(h, (int, np.integer)) or not 1 <= h <= 64:
        raise ValueError(f"sparse_headings must be an integer from 1 to 64, got {h!r}")
    if ant:
        raise NotImplementedError("sparse_cell: the car only (the ant's tree has no cost column)")
    if solution == "first":
        raise ValueError("sparse_cell needs a solution other than 'first' (the cost column belongs to 'best_of_round', 'anytime' "
                         "and 'anytime_pruned')")
    if prop_duration is not None and len(prop_duration) > 1:
        raise NotImplementedError("sparse_cell: a single prop_duration entry (a schedule's chunk budgets are not built for the "
                                  "rounds that mask their search)")
    return float(v), int(h)


def check_solution(solution, emulate_sticky_done, world_size=1, run_type=0):
    """The scope of the ``solution`` modes other than "first" (ditree_accept_best, ditree_accept_bounded): one rank, run_type 0,
    no sticky-done emulation (its phantom candidate belongs to the first-goal rule)."""
    if solution not in SOLUTIONS:
        raise ValueError(f"solution must be one of {SOLUTIONS}, got {solution!r}")
    if solution == "first":
        return
    if emulate_sticky_done:
        raise ValueError(f"solution={solution!r} needs emulate_sticky_done=False (the sticky-done emulation ends a plan at its "
                         "first goal)")
    if world_size > 1:
        raise NotImplementedError(f"solution={solution!r}: one rank (world_size {world_size})")
    if run_type != 0:
        raise NotImplementedError(f"solution={solution!r}: run_type 0 only (got {run_type})")


def bound_stats(pruned, row, key, base, n_nodes):
    """The "anytime_pruned" statistics of one tree, from its stats row as of the last accept and the keys of its ``n_nodes``
    slots from ``base``: (exhausted: no node can be open any more, key[root] >= the incumbent's cost; candidates pruned since
    the reset; closed_nodes(): the nodes whose key is at or past the incumbent's cost, 0 without an incumbent -- one
    reduction and one scalar copy, so it is a call)."""
    if not pruned:
        return False, 0, lambda: 0
    u = int(row[ST_BOUND])
    return (bool(row[ST_EXHAUSTED]), int(row[ST_PRUNED]),
            lambda: 0 if u == NO_BOUND else int((key[base: base + n_nodes] >= u).sum().item()))


class Entries(NamedTuple):
    """What an engine calls in the library, fixed at construction by three facts -- forest or single tree, scene table or
    single maze, ant or car -- and the ``solution`` mode: the names of its entry points, ``accept_tail(engine)`` = what its
    accept takes behind the round descriptor (the sticky-done flag, the cost column, the bound, or nothing), and the
    descriptors its calls take behind the tree's -- ``lead`` in every call (a forest's descriptor), ``scenes`` behind those
    in the expand call (a scene forest's descriptor; NULL for a plain forest's bounded round, whose entry point serves both
    kinds of forest).  ``near``: the rounds of an engine with ``near_radius`` go through ditree_[forest_]expand_round_near, which
    serves every mode (the bound or NULL) and both kinds of forest; the accept and the fallback stay the mode's own.
    ``sparse``: the rounds and the accepts of an engine with ``sparse_cell`` go through ditree_[forest_]expand_round_sparse (the
    bound or NULL, the near descriptor or NULL, the sparse one) and ditree_[forest_]accept_sparse (the cost column, the bound or
    NULL, the sparse descriptor)."""
    expand: str
    accept: str
    accept_tail: Callable
    fallback: str
    budget: str
    lead: tuple
    scenes: tuple

    @classmethod
    def of(cls, solution, ant, forest=None, scenes=None, near=False, sparse=False):
        f, a = ("forest_" if forest is not None else ""), ("_ant" if ant else "")
        lead = () if forest is None else (C.byref(forest),)
        sc = () if scenes is None else (C.byref(scenes),)
        if solution == "anytime_pruned":
            expand, accept, tail = f"ditree_{f}expand_round_bounded", f"ditree_{f}accept_bounded", lambda e: (C.byref(e.bound),)
            sc = sc or ((None,) if forest is not None else ())
        else:
            expand = f"ditree_{f}expand_round{a}" + ("_scenes" if scenes is not None else "")
            if solution != "first":
                accept, tail = f"ditree_{f}accept_best", lambda e: (e.tree.cost.data_ptr(),)
            elif ant and forest is not None:             # the ant env has no sticky-done latch
                accept, tail = "ditree_forest_accept_ant", lambda e: ()
            else:
                accept, tail = f"ditree_{f}accept", lambda e: (e.sticky,)
        if near:             # one expand entry for every mode and kind of forest: [scenes or NULL], ..., the bound or NULL, near
            expand = f"ditree_{f}expand_round_near"
            sc = sc or ((None,) if forest is not None else ())
        if sparse:           # as near: one expand entry, and one accept entry for the best and the bounded rule
            expand, accept = f"ditree_{f}expand_round_sparse", f"ditree_{f}accept_sparse"
            sc = sc or ((None,) if forest is not None else ())
            tail = lambda e: (e.tree.cost.data_ptr(), C.byref(e.bound) if e.pruned else None, C.byref(e._sparse_desc()))  # noqa: E731
        fallback = "ditree_fallback_select" if forest is None else \
            "ditree_forest_fallback" + ("_goals" if scenes is not None else "") + a
        return cls(expand, accept, tail, fallback, f"ditree_{f}chunk_budget", lead, sc)


class ExpansionEngine:
    """Batched RRT expansion on one GPU (optionally one shard of a multi-GPU round).  ``solution``: which goal-reaching
    candidate becomes the goal node -- "first" (the reference's: the lowest index, the rest of the round dropped), or, through
    ditree_accept_best, the cheapest one ("best_of_round", "anytime": every non-collided candidate of the round is appended
    and ``goal_node`` is the incumbent, which later rounds may replace).  "anytime_pruned" is "anytime" until the tree holds an
    incumbent and branch and bound from then on (include/ditree.h "branch and bound"): with ``reach`` metres per path row
    (an assumption about the dynamics, not a theorem -- a smaller value prunes more and may prune a branch that would have
    won), parents are chosen among the nodes that can still lead to a shorter path, candidates that cannot beat the incumbent
    get no node, and ``exhausted`` says that no node is open any more.  A single ``prop_duration`` entry only
    (ditree_chunk_budget runs its own, unmasked nearest-node search)."""
    STATE_DIM, ACTION_DIM, HIST = 6, 2, False

    def __init__(self, ctx: Context, maze, start_state, goal_state, edge_length=64, action_horizon=8,
                 pred_horizon=64, local_map_size=20, local_map_scale=0.2, s_global=1.0, batch=1024,
                 capacity=65536, k_steps=1, emulate_sticky_done=True, norm=CAR_NORM, rank=0, world_size=1,
                 process_group=None, early_exit=False, run_type=0, goal_scale=None, prop_duration=None, solution="first",
                 reach=None, near_radius=None, near_reach=None, sparse_cell=None, sparse_headings=None):
        check_solution(solution, emulate_sticky_done, world_size, run_type)
        self.solution = solution
        self.pruned = solution == "anytime_pruned"
        if reach is not None and not self.pruned:
            raise ValueError(f"reach belongs to solution='anytime_pruned' (got solution={solution!r})")
        self.reach = check_reach(CAR_REACH if reach is None else reach) if self.pruned else None
        if self.pruned and prop_duration is not None and len(prop_duration) > 1:
            raise NotImplementedError("solution='anytime_pruned': a single prop_duration entry (the chunk-budget search is not masked)")
        self.near = check_near(near_radius, near_reach, solution, self.HIST, prop_duration)
        self.sparse = check_sparse(sparse_cell, sparse_headings, solution, self.HIST, prop_duration)
        self.ctx = ctx
        self.maze = np.asarray(maze, dtype=np.float32)
        # planners/RRT.py:26,149-152: per-visit edge lengths; the tree's edge capacity is the longest entry
        self.schedule = [int(edge_length)] if prop_duration is None else [int(v) for v in prop_duration]
        if not self.schedule or any(v < action_horizon or v % action_horizon for v in self.schedule) or len(self.schedule) > 16:
            raise ValueError("prop_duration: 1..16 edge lengths, each a positive multiple of action_horizon")
        edge_length = max(self.schedule)
        self.H, self.A, self.P = edge_length, action_horizon, pred_horizon
        self.n_chunks = edge_length // action_horizon
        self.lm_n, self.lm_scale, self.s_global = local_map_size, local_map_scale, s_global
        # divisor of the goal offset inside tanh (fm_policy.py:125-143 uses the SAMPLER's local_map_size)
        self.goal_scale = float(local_map_size if goal_scale is None else goal_scale)
        self.batch = batch
        self.k_steps = k_steps
        self.sticky = int(bool(emulate_sticky_done))
        self.early_exit = int(bool(early_exit))    # skip later chunks of collided / finished candidates
        self.norm = np.ascontiguousarray(CAR_NORM if norm is None else norm, dtype=np.float64)
        self.rank, self.world, self.pg = rank, world_size, process_group
        self.ddpm = None                    # (timesteps (K,), coef (K, 5)): the sampler's DDPM branch instead of the flow steps
        self.force_allgather = False        # run the collective even with one rank (exercises the RCCL path on 1 GPU)
        self.exchange_events = None         # list -> one (start, end) event pair per round around pack + all-gather + unpack
        self.run_type = int(run_type)
        self.init_main_path = None          # (P, >=2) reference path of an earlier plan (run_type > 0)
        self.tree = DeviceTree(ctx, capacity, self.n_chunks, self.A, track_obstacle_ahead=self.run_type > 0,
                               state_dim=self.STATE_DIM, action_dim=self.ACTION_DIM, hist=self.HIST,
                               cost=solution != "first", key=self.pruned, active=self.sparse is not None)
        # sharded rounds exchange ceil(batch / world) fixed slots per rank: size the round buffers for whole slots, so a batch
        # that does not divide by the rank count is fine (the last rank's tail slots stay unused)
        per = (batch + world_size - 1) // world_size
        self.rb = RoundBuffers(ctx, per * world_size, self.n_chunks, self.A, state_dim=self.STATE_DIM,
                               action_dim=self.ACTION_DIM, hist=self.HIST, record_doubles=self.tree.record_doubles)
        self._budget = self._budget_parent = None
        if len(self.schedule) > 1:
            self._budget = torch.zeros(batch, dtype=torch.int32, device=ctx.device)
            self._budget_parent = torch.zeros(batch, dtype=torch.int32, device=ctx.device)
            self._sched_chunks = (C.c_int32 * len(self.schedule))(*[v // action_horizon for v in self.schedule])
        self.axis = local_axis(local_map_size, local_map_scale)
        from .common.fm_utils import get_timesteps
        t0, dt = get_timesteps("exp", k_steps, 4.0)
        self.t0, self.dt = t0.numpy().copy(), dt.numpy().copy()
        ctx.upload_maze(self.maze, owner=self)
        # a forest's descriptors exist by now (ForestTrees._init_forest, SceneTrees._init_scenes run before this constructor)
        fdesc = getattr(self, "fdesc", None)
        self.entries = Entries.of(solution, self.HIST, fdesc, getattr(self, "sdesc", None), near=self.near is not None,
                                  sparse=self.sparse is not None)
        if self.pruned:
            if fdesc is None:
                self._init_bound(1, 0, self.tree.stats)
            else:
                self._init_bound(self.T, self.C, self.fstats)
        if self.sparse is not None:
            self._init_sparse()
        self.reset(start_state, goal_state)

    def _call(self, entry, *args):
        """One call of the library on this engine's tree: the handle, the tree's descriptor, ``args``, the stream."""
        check(self.ctx._h, getattr(lib(), entry)(self.ctx._h, C.byref(self.tree.desc), *args, self.ctx.stream),
              entry[len("ditree_"):])

    def round_settings(self):
        """The keyword arguments that rebuild this engine's round program in another engine of its kind (a forest)."""
        kw = dict(action_horizon=self.A, pred_horizon=self.P, local_map_size=self.lm_n, local_map_scale=self.lm_scale,
                  s_global=self.s_global, k_steps=self.k_steps, norm=self.norm, early_exit=bool(self.early_exit),
                  goal_scale=self.goal_scale)
        if self.HIST:
            kw.update(edge_length=self.H, dynamics=self.dynamics, model=self.model, ball_radius=self.ball_radius)
        else:
            kw.update(emulate_sticky_done=bool(self.sticky), prop_duration=self.schedule, solution=self.solution,
                      reach=self.reach, near_radius=self.near and self.near[0], near_reach=self.near and self.near[1],
                      sparse_cell=self.sparse and self.sparse[0], sparse_headings=self.sparse and self.sparse[1])
        return kw

    # ------------------------------------------------------------------ the bound of "anytime_pruned"
    def _init_bound(self, n_trees, tree_capacity, stats):
        """The ditree_bound descriptor: the tree's cost and key columns, one goal row per tree and the ``stats`` rows.
        ``tree_capacity``: the slots of each tree of a forest, 0 for a single tree (ditree_bound_keys)."""
        self._bound_goals = torch.zeros(n_trees, 2, dtype=torch.float64, device=self.ctx.device)
        self._bound_roots, self._bound_capacity = [], int(tree_capacity)
        self.bound = Bound(self.tree.cost.data_ptr(), self.tree.key.data_ptr(), self._bound_goals.data_ptr(), CAR_GOAL_RADIUS,
                           self.reach, stats.data_ptr())

    def _bound_goal_rows(self):
        return np.asarray(self.env_goal, dtype=np.float64)[None, :2]

    def _bound_sync(self):
        """Before a launch that reads the bound: the goal rows as they are now (a facade sets ``env_goal`` after ``reset``) and
        the key of every root reset since -- on the device, by the function that keys every other node."""
        if not self._bound_roots:
            return
        self._bound_goals.copy_(torch.as_tensor(np.ascontiguousarray(self._bound_goal_rows())))
        for r in self._bound_roots:
            self._call("ditree_bound_keys", C.byref(self.bound), int(r), 1, self._bound_capacity)
        self._bound_roots = []

    def _bound_stats(self):
        tr = self.tree
        return bound_stats(self.pruned, tr.stats_host, tr.key, 0, tr.n_nodes_host)

    @property
    def exhausted(self):
        """"anytime_pruned": no node of the tree can be open after the last accept (key[root] >= the incumbent's cost)."""
        return self._bound_stats()[0]

    @property
    def pruned_candidates(self):
        return self._bound_stats()[1]

    def closed_nodes(self):
        """Nodes whose key is at or past the incumbent's cost (0 without an incumbent); one reduction and one scalar copy."""
        return self._bound_stats()[2]()

    # ------------------------------------------------------------------ the sparse tree of ``sparse_cell``
    def _sparse_mazes(self):
        """The maps a tree of this engine may grow on: they size the table."""
        return [self.maze]

    def _sparse_maze_of(self, t):
        return self.maze

    def _init_sparse(self):
        """What the ditree_sparse descriptor points to, but for the tree's own arrays (the active column, the stats row: a
        re-base swaps the two trees): per tree the map extents and the grid dims, the table and the contender words, and the
        accept's candidate scratch."""
        cell, nh = self.sparse
        dev, T = self.ctx.device, getattr(self, "T", 1)
        self._sparse_stride = max(nx * ny * nh for _, _, nx, ny in (sparse_grid(m.shape, self.s_global, cell, nh)
                                                                    for m in self._sparse_mazes()))
        self._sparse_extent = torch.zeros(T, 2, dtype=torch.float64, device=dev)
        self._sparse_dims = torch.zeros(T, 2, dtype=torch.int32, device=dev)
        self._sparse_dims_host = (C.c_int32 * (2 * T))()
        self._sparse_table = torch.full((T, self._sparse_stride), -1, dtype=torch.int64, device=dev)       # all ones: no node
        self._sparse_scratch = torch.full((T, self._sparse_stride), -1, dtype=torch.int64, device=dev)
        self._sparse_cand = torch.zeros(2 * self.rb.B, dtype=torch.int32, device=dev)
        self._sparse_roots = []

    def _sparse_stats_rows(self):
        return self.tree.sparse_stats

    def _sparse_desc(self):
        cell, nh = self.sparse
        return Sparse(cell, 2.0 * np.pi / nh, nh, self._sparse_stride, self._sparse_extent.data_ptr(), self._sparse_dims.data_ptr(),
                      self._sparse_dims_host, self._sparse_table.data_ptr(), self._sparse_scratch.data_ptr(),
                      self.tree.active.data_ptr(), self._sparse_stats_rows().data_ptr(), self._sparse_cand.data_ptr())

    def _sparse_sync(self):
        """Before a launch that reads the sparse tree: the grid of every tree's map as it is now, and the table, the flags and
        the stats row of every tree reset or re-based since, rebuilt on the device from the tree itself (purity: the active
        nodes are a function of the tree)."""
        if not self._sparse_roots:
            return
        cell, nh = self.sparse
        T = getattr(self, "T", 1)
        grids = [sparse_grid(self._sparse_maze_of(t).shape, self.s_global, cell, nh) for t in range(T)]
        if max(nx * ny * nh for _, _, nx, ny in grids) > self._sparse_stride:      # a larger map since: every tree again
            self._init_sparse()
            self._sparse_roots = list(range(T))
        for t, (W, L, nx, ny) in enumerate(grids):
            self._sparse_dims_host[2 * t], self._sparse_dims_host[2 * t + 1] = nx, ny
        self._sparse_extent.copy_(torch.as_tensor(np.array([g[:2] for g in grids], dtype=np.float64)))
        self._sparse_dims.copy_(torch.as_tensor(np.array([g[2:] for g in grids], dtype=np.int32)))
        roots = sorted(set(self._sparse_roots))
        runs = [(0, T)] if len(roots) == T else [(t, 1) for t in roots]
        for first, n in runs:
            self._call("ditree_sparse_rebuild", *(self.entries.lead or (None,)), C.byref(self._sparse_desc()),
                       self.tree.cost.data_ptr(), first, n)
        self._sparse_roots = []

    def _sparse_row(self):
        return self.tree.sparse_host

    @property
    def dominated_candidates(self):
        """``sparse_cell``: candidates that took no node because a node at most as dear holds their cell, since the reset."""
        return int(self._sparse_row()[SP_DOMINATED])

    @property
    def retired_nodes(self):
        """``sparse_cell``: nodes a cheaper one displaced as its cell's representative, since the reset."""
        return int(self._sparse_row()[SP_RETIRED])

    @property
    def active_nodes(self):
        """``sparse_cell``: the nodes the searches look at, one per occupied cell."""
        return int(self._sparse_row()[SP_ACTIVE])

    # ------------------------------------------------------------------ state
    def reset(self, start_state, goal_state):
        self.start_state = np.asarray(start_state, dtype=np.float64).copy()
        self.goal_state = np.asarray(goal_state, dtype=np.float64).copy()
        if self.start_state.shape != (self.STATE_DIM,):
            raise ValueError(f"start_state must have {self.STATE_DIM} elements")
        self._derive_env_goal()
        self.tree.reset(self.start_state)
        if self.pruned:
            self._bound_roots = [0]
        if self.sparse is not None:
            self._sparse_roots = [0]
        self.generation = getattr(self, "generation", 0) + 1      # consumers caching per-tree data (node_list) key on it

    def _derive_env_goal(self):
        self.env_goal = env_goal_of(self.maze, self.goal_state)

    def update_maze(self, maze):
        self.maze = np.asarray(maze, dtype=np.float32)
        self.ctx.upload_maze(self.maze, owner=self)
        if self.sparse is not None:                   # the cells follow the map's extents: every tree's table again
            self._sparse_roots = list(range(getattr(self, "T", 1)))

    def ensure_maze(self):
        """The ctx's device maze must be THIS engine's before any launch that reads it (another planner, or a
        check_collision call, may have uploaded its own since)."""
        if self.ctx.maze_owner is not self:
            self.ctx.upload_maze(self.maze, owner=self)

    # ------------------------------------------------------------------ re-planning on a kept tree
    def rebase(self, anchor, root_state=None, drop_states=0, drop_actions=0):
        """Re-root the tree at the car instead of wiping it (include/ditree.h "re-planning on a kept tree"): the subtree of
        ``anchor`` that still clears this engine's maze, compacted to the front.  ``drop_states == 0``: the car stands on
        ``anchor``, which becomes the root (``root_state``, where given, replaces its state: the car's real one).
        ``drop_states > 0``: the car is inside ``anchor``'s edge -- ``root_state`` becomes a fresh root and ``anchor`` its only
        child, its edge without the first ``drop_states`` state rows and ``drop_actions`` action rows.  The goal is the one the
        tree was grown for.  Returns ``(kept, dropped)``: the nodes of the old tree that are in the new one, and the rest.
        The second tree is allocated on the first call and the two swap roles from then on."""
        if self.HIST:
            raise NotImplementedError("rebase: the car (the ant's tree keeps edge histories)")
        if type(self) is not ExpansionEngine:
            raise NotImplementedError(f"rebase: a single tree ({type(self).__name__} is not built)")
        if self.world > 1 or getattr(self, "_sharded", False):
            raise NotImplementedError(f"rebase: one rank (world_size {self.world}: a sharded tree keeps edge rows on other ranks)")
        if self.pruned:
            raise NotImplementedError("rebase: solution='anytime_pruned' is not built (key column, stats row, closed nodes)")
        fresh_root = int(drop_states) > 0
        if fresh_root and root_state is None:
            raise ValueError("rebase: drop_states > 0 needs the root_state")
        if not fresh_root and int(drop_actions) != 0:
            raise ValueError("rebase: drop_actions without drop_states")
        root = None if root_state is None else np.ascontiguousarray(root_state, dtype=np.float64)
        if root is not None and root.shape != (self.STATE_DIM,):
            raise ValueError(f"root_state must have {self.STATE_DIM} elements")
        self.ensure_maze()
        old = self.tree
        if getattr(self, "_spare_tree", None) is None:
            self._spare_tree = DeviceTree(self.ctx, old.capacity, self.n_chunks, self.A,
                                          track_obstacle_ahead=old.obstacle_ahead is not None, state_dim=self.STATE_DIM,
                                          action_dim=self.ACTION_DIM, hist=self.HIST, cost=old.cost is not None,
                                          active=old.active is not None)
            self._rebase_scratch = torch.zeros(3 * old.capacity, dtype=torch.int32, device=self.ctx.device)
        new = self._spare_tree
        n_old = old.n_nodes_host
        rs = root.ctypes.data_as(C.POINTER(C.c_double)) if fresh_root else None
        cost = (None, None) if old.cost is None else (old.cost.data_ptr(), new.cost.data_ptr())
        check(self.ctx._h, lib().ditree_tree_rebase(self.ctx._h, C.byref(old.desc), C.byref(new.desc), int(anchor), rs,
                                                    int(drop_states), int(drop_actions), cost[0], cost[1],
                                                    self._rebase_scratch.data_ptr(), self.ctx.stream), "tree_rebase")
        cnt = new.read_counters()                 # the one D2H: the new size, or the device's refusal
        if cnt[CNT_NODES] <= 0:
            new.n_nodes_host = 0
            raise ValueError(f"rebase: refused on the device ({'drop counts' if cnt[CNT_NODES] == -1 else 'anchor'} out of "
                             f"range: anchor {anchor}, drop_states {drop_states}, drop_actions {drop_actions}, {n_old} nodes)")
        self.tree, self._spare_tree = new, old    # every descriptor with tree pointers is the DeviceTree's own
        if root is not None:
            self.start_state = root.copy()
            if not fresh_root:
                s = torch.as_tensor(root, device=new.state.device)
                new.state[0] = s
                new.xy[0] = s[:2]
        self.rebase_ids = self._rebase_scratch[2 * old.capacity:]      # old id -> new id (-1: dropped) until the next rebase
        if self.sparse is not None:               # table, flags and stats of the re-based tree, from the tree itself
            self._sparse_roots = [0]
            self._sparse_sync()
            new.read_counters()
        self.generation += 1
        kept = int(cnt[CNT_NODES]) - (1 if fresh_root else 0)
        return kept, n_old - kept

    def chain_rows(self, node):
        """The chain root .. ``node`` with what the tree holds for it in f64: ids, per-node edge row counts (states, actions)
        and per node the rows ``tree_path`` strings together -- its edge states, then its state (the root: its state alone)."""
        chain, idx = parent_chain(self.tree, node, self.tree.n_nodes_host)
        st, es = self.tree.state[idx].cpu().numpy(), self.tree.edge_states[idx].cpu().numpy()
        ns, na = self.tree.edge_nstates[idx].cpu().numpy(), self.tree.edge_nactions[idx].cpu().numpy()
        ns[0] = na[0] = 0
        rows = [np.concatenate([es[j, :ns[j]], st[j][None]]) for j in range(len(chain))]
        return chain, ns.astype(int).tolist(), na.astype(int).tolist(), rows

    def shard(self, B):
        """Contiguous candidate block of this rank."""
        per = (B + self.world - 1) // self.world
        lo = min(self.rank * per, B)
        hi = min(lo + per, B)
        return lo, hi, per

    def agree(self, flag: bool) -> bool:
        """Rank 0's decision for every rank (the wall-clock budget of a plan is read on rank 0 only: ranks that disagreed
        about running another round would dead-lock in its collective).  One 4-byte broadcast; identity for one rank."""
        if self.world <= 1:
            return bool(flag)
        import torch.distributed as dist
        gloo = dist.get_backend(self.pg) == "gloo"
        t = torch.tensor([1 if flag else 0], dtype=torch.int32, device="cpu" if gloo else self.ctx.device)
        src = 0 if self.pg is None else dist.get_global_rank(self.pg, 0)
        dist.broadcast(t, src=src, group=self.pg)
        return bool(int(t.item()))

    def sum_over_ranks(self, value: int, op="sum") -> int:
        if self.world <= 1:
            return int(value)
        import torch.distributed as dist
        gloo = dist.get_backend(self.pg) == "gloo"
        t = torch.tensor([int(value)], dtype=torch.int64, device="cpu" if gloo else self.ctx.device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX if op == "max" else dist.ReduceOp.SUM, group=self.pg)
        return int(t.item())

    # ------------------------------------------------------------------ one round
    def _sampler_schedule(self, rp, keep, step_noise, lo, hi):
        """t0 / dt of the flow steps, or -- self.ddpm set -- the DDPM timesteps, coefficient table and this round's step noise."""
        if self.ddpm is None:
            for name, arr in (("t0", self.t0), ("dt", self.dt)):
                a, p = _flt(arr)
                keep.append(a)
                setattr(rp, name, p)
            rp.K = self.k_steps
            rp.ddpm_coef, rp.step_noise = None, None
            return
        ts, coef = self.ddpm
        a, rp.t0 = _flt(ts)
        b, rp.ddpm_coef = _flt(coef)
        keep += [a, b, step_noise]
        rp.dt = None
        rp.K = len(a)
        if step_noise is None:
            raise ValueError("the DDPM branch needs step_noise (B, n_chunks, K, P, D) f32")
        want = (self.n_chunks, rp.K, self.P, self.ACTION_DIM)
        if tuple(step_noise.shape[1:]) != want or step_noise.dtype != torch.float32 or not step_noise.is_contiguous():
            raise ValueError(f"step_noise must be a contiguous float32 (B, {want[0]}, {want[1]}, {want[2]}, {want[3]}) tensor")
        rp.step_noise = step_noise[lo:hi].data_ptr() if hi > lo else None

    def _round_params(self, rp, samples, cond_goal, noise, inject_actions, step_noise, lo, hi, goal_field="goal_xy"):
        """What every round type's parameter block shares, for rows [lo, hi) of the round: the sample, goal, noise and action
        pointers, the sampler schedule, norm / goal / axis, the local-map fields, early_exit and -- with a ``prop_duration``
        schedule -- the chunk budgets.  Returns the list that keeps the pointed-to arrays alive until the launch has been issued."""
        n = hi - lo
        rp.n_nodes = self.tree.n_nodes_host           # a forest round does not read it: each tree's size is in its counter row
        rp.samples = samples[lo:hi].data_ptr() if n else None
        rp.cond_goal = cond_goal[lo:hi].data_ptr() if n else None
        rp.noise = noise[lo:hi].data_ptr() if (noise is not None and n) else None
        rp.inject_actions = inject_actions[lo:hi].data_ptr() if (inject_actions is not None and n) else None
        rp.P = self.P
        keep = [samples, cond_goal, noise, inject_actions, step_noise]
        if self.ddpm is None or noise is None:
            self._flow_only(rp, keep)
        else:
            self._sampler_schedule(rp, keep, step_noise, lo, hi)
        for name, arr in (("norm", self.norm), (goal_field, self.env_goal), ("axis", self.axis)):
            a, ptr = _dbl(arr)
            keep.append(a)
            setattr(rp, name, ptr)
        rp.lm_n, rp.lm_size, rp.s_global = self.lm_n, self.goal_scale, float(self.s_global)
        rp.early_exit = self.early_exit
        if self._budget is not None:                  # else the field keeps its NULL
            # planners/RRT.py:149-152 -> ``self._budget``.  Every rank derives the budgets of the WHOLE round (a candidate's
            # place in its parent's visit order is global); a forest's trees carry their sizes in their counter rows
            e = self.entries
            self._call(e.budget, *e.lead, samples.data_ptr(), samples.shape[0], *(() if e.lead else (self.tree.n_nodes_host,)),
                       self._sched_chunks, len(self.schedule), self._budget_parent.data_ptr(), self._budget.data_ptr())
            rp.chunk_budget = self._budget[lo:hi].data_ptr() if n else None
        return keep

    def _params(self, samples, cond_goal, noise, inject_actions, lo, hi, step_noise=None):
        """-> (this engine's parameter block for rows [lo, hi) of the round, what it points to)."""
        rp = RoundParams()
        return rp, self._round_params(rp, samples, cond_goal, noise, inject_actions, step_noise, lo, hi)

    def _round_head(self, samples, cond_goal, counts_per_tree):
        """-> B, the candidates of the round (a forest: after setting the offsets of ``counts_per_tree``)."""
        return samples.shape[0]

    def _check_round_shapes(self, B, samples, cond_goal, noise, inject_actions, next_obs_tape=None, step_fn=None):
        """The car's shapes are the library's to check."""

    def expand_round(self, samples, cond_goal, noise=None, inject_actions=None, accept=True, step_noise=None):
        """samples (B,6) f64, cond_goal (B,2) f64 [device tensors, all candidates of the round];
        noise (B, n_chunks, P, 2) f32 or inject_actions (B, n_chunks, P, 2) f64 for this round; step_noise
        (B, n_chunks, K, P, 2) f32 with ``self.ddpm`` set (the sampler's DDPM branch)."""
        return self._round(samples, cond_goal, noise, inject_actions, step_noise, accept)

    def _round(self, samples, cond_goal, noise, inject_actions, step_noise, accept, counts_per_tree=None, step_fn=None,
               **ant):
        """One round of every engine: head (B; a forest's offsets), shape check, this engine's maze or scene table on the
        device, the parameter block of this rank's rows, the launch, and the tail (exchange, accept).  ``ant``: the ant
        rounds' own tensors (``next_obs_tape``, ``cond_out``); ``step_fn``: a host-stepped ant round's simulator."""
        B = self._round_head(samples, cond_goal, counts_per_tree)
        if B > self.batch:
            raise ValueError(f"round of {B} candidates exceeds engine batch {self.batch}")
        if B == 0 and counts_per_tree is not None:    # no tree has a candidate: nothing to expand or accept
            return self.cnt_host.copy() if accept else None
        self._check_round_shapes(B, samples, cond_goal, noise, inject_actions, ant.get("next_obs_tape"), step_fn)
        lo, hi, per = self.shard(B)
        self.ensure_maze()
        rp, keep = self._params(samples, cond_goal, noise, inject_actions, lo, hi, step_noise=step_noise, **ant)
        if hi > lo:                                   # a rank without rows still takes part in the exchange and the accept
            rd = self.rb.desc(lo, hi - lo)
            if step_fn is not None:
                self._host_stepped_round(rd, rp, lo, hi - lo, step_fn)
            else:
                self._launch_round(rd, rp)
        del keep                                      # alive until the launch has been issued
        self._B = B                                   # for ``accept()`` without an argument
        return self._finish_round(B, per, noise is not None, accept)

    def _launch_round(self, rd, rp):
        e = self.entries
        tail = ()
        if self.pruned:
            self._bound_sync()
            tail = (C.byref(self.bound),)
        if self.near is not None:                     # the bound or NULL, then the near descriptor on the cost column of the
            near = Near(self.tree.cost.data_ptr(), *self.near)      # tree as it is now (a re-base swaps the two trees)
            tail = (*(tail or (None,)), C.byref(near))
        if self.sparse is not None:                   # the bound or NULL, the near descriptor or NULL, then the sparse one
            self._sparse_sync()
            tail = (*tail, None, None)[:2] + (C.byref(self._sparse_desc()),)
        self._call(e.expand, *e.lead, *e.scenes, C.byref(rd), C.byref(rp), *tail)

    def _flow_only(self, rp, keep):
        """An action-tape round of an engine whose sampler is the DDPM branch: no sampler call, the schedule is irrelevant."""
        saved, self.ddpm = self.ddpm, None
        try:
            self._sampler_schedule(rp, keep, None, 0, 0)
        finally:
            self.ddpm = saved

    def _finish_round(self, B, per, used_denoiser, accept):
        """The part of a round behind the expansion: the record exchange (sharded rounds) and the replicated accept."""
        if self.world > 1 or self.force_allgather:
            ev = None
            if self.exchange_events is not None:
                # torch's collective runs on the backend's own stream, but the current stream waits for it (async_op=False):
                # events on the current stream bracket pack + collective + unpack
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev[0].record()
            self._allgather_round(B, per)
            if ev is not None:
                ev[1].record()
                self.exchange_events.append(ev)
        self._used_denoiser = bool(used_denoiser)
        if accept:
            return self.accept(B)
        return None

    def _allgather_round(self, B, per):
        """One collective per round: 96-byte candidate records (end state, last / first action, parent, status, chunks run;
        SURVEY.md 8(e)).  The edge trajectories stay on the rank that produced them (tree.edge_owner) and are only moved
        by ``path_to``.  DITREE_GATHER_EDGES=1 restores the round-1 behaviour (every field incl. trajectories)."""
        import os
        if os.environ.get("DITREE_GATHER_EDGES", "0") == "1":
            self._sharded = False
            allgather_round_fields(self.rb.fields()[:-1], per, self.rank, self.world, self.pg)
            return
        self._sharded = True
        rows = per * self.world
        rb = self.rb
        rb.ensure_exchange(rows)
        lo, hi, _ = self.shard(B)
        n = hi - lo
        mine = rb.records[self.rank * per:(self.rank + 1) * per]
        if n > 0:
            rd = rb.desc(lo, n)
            self._call("ditree_round_pack", C.byref(rd), mine.data_ptr())
        allgather_round_fields([rb.records], per, self.rank, self.world, self.pg)
        rd = rb.desc(0, B, shard=per)
        self._call("ditree_round_unpack", C.byref(rd), rb.records.data_ptr())

    def accept(self, B=None):
        """The replicated accept of the last round's first ``B`` candidates (default: all of them) -> the counters (a
        forest: every tree's row)."""
        B = self._B if B is None else int(B)
        self.ensure_maze()                        # run_type > 0: the commit kernel evaluates check_obstacle_ahead
        if getattr(self, "_sharded", False) and (self.world > 1 or self.force_allgather):
            lo, hi, per = self.shard(B)
            rd = self.rb.desc(0, B, own=(lo, hi - lo), shard=per)
        else:
            rd = self.rb.desc(0, B)
        e = self.entries
        if self.pruned:
            self._bound_sync()
        if self.sparse is not None:
            self._sparse_sync()
        self._call(e.accept, *e.lead, C.byref(rd), *e.accept_tail(self))
        cnt = self.read_counters()                # one small D2H per round: n_nodes / goal (a forest: every tree's row)
        self._range_guard()
        return cnt

    def read_counters(self):
        return self.tree.read_counters()

    def _range_guard(self):
        """The tail of every accept: a round that ran the denoiser raises if the f16 range guard clamped activations."""
        if not getattr(self, "_used_denoiser", False):
            return
        # the stream is drained already, one more tiny D2H.  Sharded: a rank whose shard saturated must not raise alone (the
        # others would wait in the next collective until the launcher kills them) -- the ranks agree on the worst count first
        # and then all raise.
        layers = self.ctx.denoise_status(clear=True)
        worst = self.sum_over_ranks(len(layers), op="max")
        if worst:
            if not layers:
                raise _lib.DitreeError(f"f16 range guard: another rank clamped activations in {worst} layer(s) of this round; "
                                       "bind the checkpoint with precision=PREC_BF16X3 or PREC_F32")
            self.ctx.raise_range_error(layers)

    # ------------------------------------------------------------------ results
    def round_solutions(self, B):
        """Device scalar: how many of the last round's first B candidates are goal nodes of the tree now."""
        rb = self.rb
        return (((rb.status[:B] & 0xFF) == _lib.ST_GOAL) & (rb.node_id[:B] >= 0)).sum()

    @property
    def goal_node(self):
        """counters[1]: the first goal node, or -- ``solution`` other than "first" -- the incumbent."""
        g = int(self.tree.counters[CNT_GOAL].item())
        return None if g < 0 else g

    def fallback_node(self):
        """planners/RRT.py:227-254.  run_type 0: among nodes 1.., the first one with the smallest
        np.linalg.norm(xy - goal_state xy) (ditree_fallback_select without obstacle flags: the norm, not the nearest-node
        kernel's squared distance -- two squares that differ in the last place can have equal norms, and np.argmin then
        returns the lower index).  run_type > 0:
        None when every node has an obstacle ahead; else nearest to the goal with +1e4 on flagged nodes, or --
        with a reference path -- the unflagged node whose nearest path point lies furthest along it."""
        n = self.tree.n_nodes_host
        if n < 2:
            return None
        out = torch.empty(1, dtype=torch.int32, device=self.tree.xy.device)
        g, gp = _dbl(self.goal_state[:2])
        if self.run_type > 0 and self.init_main_path is not None:
            pa, pp = _dbl(np.asarray(self.init_main_path)[:, :2])
            P = pa.shape[0]
        else:
            pa, pp, P = None, None, 0
        self._call(self.entries.fallback, n, gp, pp, P, out.data_ptr())
        node = int(out.item())
        return None if node < 0 else node

    def path_to(self, node):
        """planners/base_planner.py:342-363: float32 path (edge states + node states) and actions."""
        sharded = self.world > 1 and getattr(self, "_sharded", False)
        return tree_path(self.tree, node, self.tree.n_nodes_host, edge_rows=self._reduce_edge_rows if sharded else None)

    def _reduce_edge_rows(self, idx, es_t, ea_t, ns_t, na_t):
        """Collective (every rank walks the same chain): each edge comes from the rank that expanded it; rows a rank does not
        hold are zeroed, the sum over ranks is then exact (x + 0 + ... + 0)."""
        import torch.distributed as dist
        owner = self.tree.edge_owner[idx]
        mine = (owner == self.rank) | ((owner < 0) & (self.rank == 0))
        mask = mine.to(es_t.dtype)
        es_t = es_t * mask[:, None, None]
        ea_t = ea_t * mask[:, None, None]
        ns_t = torch.where(mine, ns_t, torch.zeros_like(ns_t))
        na_t = torch.where(mine, na_t, torch.zeros_like(na_t))
        gloo = dist.get_backend(self.pg) == "gloo"
        bufs = []
        for x in (es_t, ea_t, ns_t, na_t):
            y = x.cpu() if gloo else x.contiguous()
            dist.all_reduce(y, op=dist.ReduceOp.SUM, group=self.pg)
            bufs.append(y)
        return bufs

    def tree_snapshot(self):
        n = self.tree.n_nodes_host
        return dict(parents=self.tree.parent[:n].cpu().numpy(), states=self.tree.state[:n].cpu().numpy(),
                    counters=self.tree.counters.cpu().numpy())


class AntExpansionEngine(ExpansionEngine):
    """The expansion rounds of BASELINE config 3 (cfgs/antmaze.yaml: 29-d states, 8-d actions, action_horizon 2, edge length
    48, obs_history 3, local map 16 @ 0.8, s_global 4): nearest node -> 24 chunks x [local map -> ant conditioning vector ->
    denoiser -> 2 env steps with the reference's goal (planners/base_planner.py:296-297) and collision tests
    (common/map_utils.py:126-219)] -> accept (planners/RRT.py:195-217), on a tree that also keeps every node's last three
    edge rows (the history a child's first sampler call sees).

    THE ENV STEP is MuJoCo in the reference (third party, no oracle here) and is NOT implemented.  ``dynamics``:
      "tape"   ``expand_round(..., next_obs_tape=(B, n_chunks, A, 29))``: observations given from outside;
      "model"  the build's stand-in crawler model (include/ditree.h ditree_ant_model; not MuJoCo, parity unpinned);
      "host"   ``expand_round(..., step_fn=...)``: the caller's simulator, ``step_fn(chunk, start_states (n, 29), actions
               (n, A, 8), rows (n,)) -> (n, A, 29)`` observations, called once per chunk for the candidates still alive.
    """
    STATE_DIM, ACTION_DIM, HIST = 29, 8, True

    def __init__(self, ctx: Context, maze, start_state, goal_state, desired_goal=None, norm=None, edge_length=48,
                 action_horizon=2, pred_horizon=16, local_map_size=16, local_map_scale=0.8, s_global=4.0, batch=4096,
                 capacity=65536, k_steps=1, rank=0, world_size=1, process_group=None, early_exit=False, goal_scale=None,
                 dynamics="tape", model=None, ball_radius=1.2, goal_factor=0.45):
        if norm is None:
            raise ValueError("AntExpansionEngine: norm = obs_mean[27] + obs_std[27] + act_mean[8] + act_std[8] (metadata/antmaze.pt)")
        if dynamics not in ("tape", "model", "host"):
            raise ValueError("dynamics must be 'tape', 'model' or 'host'")
        self.dynamics = dynamics
        self.model = _lib.AntModel.default() if model is None else model
        self.ball_radius = float(ball_radius)
        self.goal_radius = float(goal_factor) * float(s_global)          # planners/base_planner.py:297
        self._desired_arg = None if desired_goal is None else np.asarray(desired_goal, dtype=np.float64)[:2].copy()
        super().__init__(ctx, maze, start_state, goal_state, edge_length=edge_length, action_horizon=action_horizon,
                         pred_horizon=pred_horizon, local_map_size=local_map_size, local_map_scale=local_map_scale,
                         s_global=s_global, batch=batch, capacity=capacity, k_steps=k_steps, emulate_sticky_done=False,
                         norm=np.asarray(norm, dtype=np.float64), rank=rank, world_size=world_size, process_group=process_group,
                         early_exit=early_exit, run_type=0, goal_scale=goal_scale)
        if self.norm.size != 70:
            raise ValueError("norm: 27 + 27 + 8 + 8 doubles")

    def _derive_env_goal(self):
        # obs['desired_goal'] of the env (the goal cell's centre plus the env's position noise): given by the caller, else
        # the centre of the goal cell in the scaled map
        if self._desired_arg is not None:
            self.env_goal = self._desired_arg.copy()
            return
        self.env_goal = ant_cell_centre(self.maze, self.goal_state, self.s_global)

    def _params(self, samples, cond_goal, noise, inject_actions, lo, hi, next_obs_tape=None, cond_out=None, step_noise=None):
        n = hi - lo
        rp = _lib.AntRoundParams()
        keep = self._round_params(rp, samples, cond_goal, noise, inject_actions, step_noise, lo, hi, goal_field="desired_goal")
        keep += [next_obs_tape, cond_out]
        rp.goal_radius, rp.ball_radius = self.goal_radius, self.ball_radius
        rp.dynamics = _lib.ANT_DYN_MODEL if self.dynamics == "model" else _lib.ANT_DYN_TAPE
        rp.next_obs_tape = next_obs_tape[lo:hi].data_ptr() if (next_obs_tape is not None and n) else None
        rp.model = C.pointer(self.model)
        rp.cond_out = cond_out[lo:hi].data_ptr() if (cond_out is not None and n) else None
        return rp, keep

    def _check_round_shapes(self, B, samples, cond_goal, noise, inject_actions, next_obs_tape=None, step_fn=None):
        if tuple(samples.shape) != (B, 29) or tuple(cond_goal.shape) != (B, 2):
            raise ValueError("samples must be (B, 29), cond_goal (B, 2)")
        shape = (B, self.n_chunks, self.P, 8)
        for nm, t in (("noise", noise), ("inject_actions", inject_actions)):
            if t is not None and tuple(t.shape) != shape:
                raise ValueError(f"{nm} must be {shape}, got {tuple(t.shape)}")
        if self.dynamics == "tape" and (next_obs_tape is None or tuple(next_obs_tape.shape) != (B, self.n_chunks, self.A, 29)):
            raise ValueError(f"dynamics='tape': next_obs_tape must be ({B}, {self.n_chunks}, {self.A}, 29)")
        if self.dynamics == "host" and step_fn is None:
            raise ValueError("dynamics='host': step_fn is required")

    def expand_round(self, samples, cond_goal, noise=None, inject_actions=None, accept=True, next_obs_tape=None, step_fn=None,
                     cond_out=None, step_noise=None):
        """samples (B, 29) f64, cond_goal (B, 2) f64, noise (B, n_chunks, P, 8) f32 or inject_actions (B, n_chunks, P, 8) f64
        [device tensors, all candidates of the round]; next_obs_tape (B, n_chunks, A, 29) f64 for dynamics='tape'; step_fn for
        dynamics='host'; cond_out (B, n_chunks, 97) f32: receives every sampler call's conditioning vector (tests)."""
        return self._round(samples, cond_goal, noise, inject_actions, step_noise, accept, next_obs_tape=next_obs_tape,
                           cond_out=cond_out, step_fn=step_fn if self.dynamics == "host" else None)

    def _host_stepped_round(self, rd, rp, lo, n, step_fn):
        """The caller's simulator between the two halves of every chunk (include/ditree.h ditree_ant_round_begin / _chunk_sample
        / _chunk_step): per chunk one D2H of the alive candidates' start states and actions, one H2D of their observations."""
        rb = self.rb
        self._call("ditree_ant_round_begin", C.byref(rd), C.byref(rp))
        obs = torch.zeros(n, self.A, 29, dtype=torch.float64, device=self.ctx.device)
        for j in range(self.n_chunks):
            self._call("ditree_ant_chunk_sample", C.byref(rd), C.byref(rp), j)
            alive = torch.nonzero(rb.status[lo:lo + n] == _lib.ST_OK).flatten()
            if alive.numel() == 0:
                break
            rows = alive.cpu().numpy()
            acts = rb.actions[lo:lo + n, j][alive].cpu().numpy()            # (n_alive, A, 8): what chunk_sample just wrote
            start = rb.end_state[lo:lo + n][alive].cpu().numpy()
            o = np.asarray(step_fn(j, start, acts, rows), dtype=np.float64)
            if o.shape != (rows.size, self.A, 29):
                raise ValueError(f"step_fn returned {o.shape}, need {(rows.size, self.A, 29)}")
            obs[alive] = torch.as_tensor(o, device=obs.device)
            self._call("ditree_ant_chunk_step", C.byref(rd), C.byref(rp), j, obs.data_ptr())
