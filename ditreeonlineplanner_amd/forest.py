"""Many independent runs in one round: a forest of T trees in one device tree (include/ditree.h "forests").

The reference's benchmark is a loop of independent runs (run_scenarios.py:336-343: ``planner.reset(); planner.plan()`` on the
same maze, start and goal, only the random stream differs).  A round of a few candidates costs as much as a round of a few
hundred, so runs one after another leave the GPU idle.  Here T runs are T trees of C node slots in one
``ditree_tree`` of capacity T * C -- tree t owns slots [t*C, (t+1)*C), its root at t*C, parents stay global -- and one round
expands the candidates of every active run, grouped by tree.  Only what knows about "the tree" has a per-tree form: the
nearest-node search (segmented by tree), accept / commit (one work-group per tree, a (T, 8) counter block), the chunk-budget
visit count and the fallback choice.  Every per-candidate kernel is the single-tree round's, and its result does not depend on
the batch, so each tree grows exactly as it would in its own ``ExpansionEngine`` fed the same rows.

Scope: run_type 0, one GPU.  The car: one maze / start / goal for every tree -- or, in a ``SceneForestEngine``, each tree on
its own scene (maze, start, goal) of a scenario set (run_scenarios.py:203-250), the mazes in one scene table on the device.
The ant (BASELINE config 3): ``AntForestEngine``, one maze / start / goal -- or, in an ``AntSceneForestEngine``, each tree on its
own scene of the ant scenario set (run_scenarios.py:202-233) -- tape or model dynamics (a host-stepped simulator steps one
candidate at a time and has no forest form).  ``ForestTrees`` holds what the forests share, ``SceneTrees`` what the two scene
forests share.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from ._lib import MAX_ATLAS_CELLS, MAX_SCENES, ST_GOAL, Forest, ForestScenes
from .engine import (CNT_GOAL, CNT_NODES, CNT_PHANTOM, SP_ACTIVE, SP_DOMINATED, SP_RETIRED, SPARSE_ROOT, STATS_ROOT,
                     AntExpansionEngine, ExpansionEngine, ant_cell_centre, bound_stats, env_goal_of, tree_path)
from .ops import CAR_NORM, Context, _dbl


class ForestTrees:
    """The per-tree bookkeeping of a forest, mixed in over a single-tree engine (``ExpansionEngine`` for the car,
    ``AntExpansionEngine`` for the ant): the (T, 8) counter block and the candidate offsets, ``reset`` / ``reset_tree``, the
    accept and the per-tree results.  Node numbers in its results (``goal_node``, ``fallback_node``, ``path_to``,
    ``tree_snapshot``) are LOCAL to their tree (root = 0), as a single-tree engine reports them; the device arrays
    (``tree.parent``, ``counters``' goal node, the round's ``node_id``) hold global slot numbers.  The round, the accept and the
    entry points are the single-tree engine's (``ExpansionEngine._round``, ``engine.Entries``): a forest adds the head of a
    round -- the candidate offsets -- and is one rank."""

    def _init_forest(self, ctx, n_trees, tree_capacity):
        """Before the engine's own constructor (which ends in ``reset``): -> the capacity of the one device tree."""
        T, Cap = int(n_trees), int(tree_capacity)
        if T < 1 or Cap < 1:
            raise ValueError("a forest needs n_trees >= 1 and tree_capacity >= 1")
        if T * Cap >= 2 ** 31:
            raise ValueError(f"n_trees * tree_capacity = {T * Cap} does not fit the int32 node numbering")
        self.T, self.C = T, Cap
        dev = ctx.device
        # every tree's counter row and, behind them, every tree's stats row of the "anytime_pruned" bound and of the sparse tree:
        # one small buffer, so that one copy per round reads them all
        self._fcnt_buf = torch.zeros(T * 16, dtype=torch.int32, device=dev)
        self.fcounters = self._fcnt_buf[:T * 8].view(T, 8)
        self.fstats = self._fcnt_buf[T * 8:T * 12].view(T, 4)
        self.fsparse = self._fcnt_buf[T * 12:].view(T, 4)
        self.stats_host = np.tile(STATS_ROOT, (T, 1))
        self.sparse_host = np.tile(SPARSE_ROOT, (T, 1))
        self.off_host = (C.c_int32 * (T + 1))()
        self.off_dev = torch.zeros(T + 1, dtype=torch.int32, device=dev)
        self.n_nodes_host = np.ones(T, dtype=np.int64)
        self.cnt_host = np.zeros((T, 8), dtype=np.int32)
        self.fdesc = Forest(T, Cap, self.fcounters.data_ptr(), self.off_dev.data_ptr(), self.off_host)
        return T * Cap

    # ------------------------------------------------------------------ state
    def reset(self, start_state, goal_state):
        """Every tree back to its root (the shared start and goal)."""
        self.start_state = np.asarray(start_state, dtype=np.float64).copy()
        self.goal_state = np.asarray(goal_state, dtype=np.float64).copy()
        if self.start_state.shape != (self.STATE_DIM,):
            raise ValueError(f"start_state must have {self.STATE_DIM} elements")
        self._derive_env_goal()
        self.tree.reset(self.start_state)            # slot 0, num_visit, the (unused) single-tree counters
        for t in range(self.T):
            self.reset_tree(t)
        self.generation = getattr(self, "generation", 0) + 1

    def reset_tree(self, t, start_state=None):
        """Tree t back to its root, so a finished run's slot can take the next run (DeviceTree.reset for one tree).
        ``start_state``: the root's state (default: the forest's start)."""
        t = self._tree_index(t)
        r = t * self.C
        self.tree.write_root(r, self.C, self.start_state if start_state is None else start_state)
        if self.pruned:                               # the root's key follows on the device before the next launch (_bound_sync)
            self.fstats[t] = self._stats_row
            self.stats_host[t] = STATS_ROOT
            self._bound_roots.append(r)
        if self.sparse is not None:                   # its table, flags and stats row follow on the device (_sparse_sync)
            self.sparse_host[t] = SPARSE_ROOT
            self._sparse_roots.append(t)
        self.fcounters[t] = self._root_row
        self.cnt_host[t] = self._ROOT
        self.n_nodes_host[t] = 1

    _ROOT = np.array([1, -1, 0, 0, 0, 0, 0, -1], dtype=np.int32)

    @property
    def _root_row(self):
        row = getattr(self, "_root_row_dev", None)
        if row is None:
            row = self._root_row_dev = torch.as_tensor(self._ROOT, device=self.fcounters.device)
        return row

    @property
    def _stats_row(self):
        row = getattr(self, "_stats_row_dev", None)
        if row is None:
            row = self._stats_row_dev = torch.as_tensor(STATS_ROOT, device=self.fcounters.device)
        return row

    def _bound_goal_rows(self):                       # one goal row per tree
        return np.tile(np.asarray(self.env_goal, dtype=np.float64)[None, :2], (self.T, 1))

    def _bound_stats(self, t):
        t = self._tree_index(t)
        return bound_stats(self.pruned, self.stats_host[t], self.tree.key, t * self.C, int(self.n_nodes_host[t]))

    def exhausted(self, t):
        """"anytime_pruned": no node of tree t can be open after the last accept."""
        return self._bound_stats(t)[0]

    def pruned_candidates(self, t):
        return self._bound_stats(t)[1]

    def closed_nodes(self, t):
        """Nodes of tree t whose key is at or past its incumbent's cost (0 without an incumbent)."""
        return self._bound_stats(t)[2]()

    def _sparse_stats_rows(self):
        return self.fsparse

    def dominated_candidates(self, t):
        """``sparse_cell``: candidates of tree t that took no node because a node at most as dear holds their cell."""
        return int(self.sparse_host[self._tree_index(t), SP_DOMINATED])

    def retired_nodes(self, t):
        return int(self.sparse_host[self._tree_index(t), SP_RETIRED])

    def active_nodes(self, t):
        return int(self.sparse_host[self._tree_index(t), SP_ACTIVE])

    def _tree_index(self, t):
        t = int(t)
        if not 0 <= t < self.T:
            raise IndexError(f"tree {t} of a forest of {self.T}")
        return t

    # ------------------------------------------------------------------ one round
    def _set_offsets(self, counts_per_tree):
        counts = np.asarray(counts_per_tree, dtype=np.int64).reshape(-1)
        if counts.shape != (self.T,):
            raise ValueError(f"counts_per_tree must have one entry per tree ({self.T})")
        if (counts < 0).any():
            raise ValueError("counts_per_tree must be >= 0")
        off = np.zeros(self.T + 1, dtype=np.int64)
        np.cumsum(counts, out=off[1:])
        for i, v in enumerate(off):
            self.off_host[i] = int(v)
        self.off_dev.copy_(torch.from_numpy(off.astype(np.int32)))
        return off

    def _round_head(self, samples, cond_goal, counts_per_tree):
        """The head of every forest round: the offsets of ``counts_per_tree`` on the host and the device -> B = their sum."""
        if counts_per_tree is None:
            raise ValueError("counts_per_tree is required (T entries, the candidates of each tree this round)")
        off = self._set_offsets(counts_per_tree)
        B = int(off[-1])
        if samples.shape[0] != B or cond_goal.shape[0] != B:
            raise ValueError(f"samples / cond_goal must have sum(counts_per_tree) = {B} rows")
        return B

    def read_counters(self):
        """-> the (T, 8) counter block, the caller's own copy (``cnt_host`` follows ``reset_tree``)."""
        buf = self._fcnt_buf.cpu().numpy()            # one small copy: the counter rows and the stats rows
        self.cnt_host = buf[:self.T * 8].reshape(self.T, 8)
        self.stats_host = buf[self.T * 8:self.T * 12].reshape(self.T, 4)
        self.sparse_host = buf[self.T * 12:].reshape(self.T, 4)
        self.n_nodes_host = self.cnt_host[:, CNT_NODES].astype(np.int64)
        return self.cnt_host.copy()

    # ------------------------------------------------------------------ results (local node numbers)
    def counters(self, t):
        """Tree t's counter row as of the last accept (goal node and phantom in the global numbering, as on the device)."""
        return self.cnt_host[self._tree_index(t)].copy()

    def goal_node(self, t):
        """Tree t's goal node (``solution`` other than "first": its incumbent) as of the last accept, local to the tree."""
        t = self._tree_index(t)
        g = int(self.cnt_host[t, CNT_GOAL])
        return None if g < 0 else g - t * self.C

    def round_solutions(self, B):
        """Device (T,) int64: how many of the last round's B candidates are goal nodes of each tree now."""
        rb = self.rb
        is_goal = ((rb.status[:B] & 0xFF) == ST_GOAL) & (rb.node_id[:B] >= 0)
        tree_of = torch.div(rb.node_id[:B].clamp(min=0), self.C, rounding_mode="floor").long()
        return torch.zeros(self.T, dtype=torch.int64, device=is_goal.device).index_add_(0, tree_of, is_goal.long())

    def phantom(self, t):
        """The round row of tree t's sticky-done phantom in the last round, or None."""
        p = int(self.cnt_host[self._tree_index(t), CNT_PHANTOM])
        return None if p < 0 else p

    def fallback_nodes(self):
        """planners/RRT.py:227-254 (run_type 0) for every tree in one launch: local node nearest to the goal among nodes 1..,
        None for a tree that holds only its root."""
        return self._fallback_launch(self.goal_state[:2])

    def _fallback_launch(self, goals):
        """The engine's forest fallback call on its goal array (one goal, or one per tree) -> each tree's local node id or
        None."""
        out = torch.empty(self.T, dtype=torch.int32, device=self.tree.xy.device)
        ga, gp = _dbl(goals)
        self._call(self.entries.fallback, *self.entries.lead, gp, out.data_ptr())
        del ga
        ids = out.cpu().numpy()
        return [None if v < 0 else int(v) - t * self.C for t, v in enumerate(ids)]

    def fallback_node(self, t):
        return self.fallback_nodes()[self._tree_index(t)]

    def path_to(self, t, node):
        """planners/base_planner.py:342-363 for tree t's local ``node``: float32 path and actions."""
        t = self._tree_index(t)
        return tree_path(self.tree, node, int(self.n_nodes_host[t]), base=t * self.C)

    def tree_snapshot(self, t):
        """Tree t as a single-tree engine reports it: local parents (root -1), states, its counter row."""
        t = self._tree_index(t)
        base, n = t * self.C, int(self.n_nodes_host[t])
        par = self.tree.parent[base: base + n].cpu().numpy()
        return dict(parents=np.where(par < 0, par, par - base), states=self.tree.state[base: base + n].cpu().numpy(),
                    counters=self.counters(t))

    def shard(self, B):                               # one rank
        return 0, B, B


class ForestEngine(ForestTrees, ExpansionEngine):
    """T independent car trees of ``tree_capacity`` node slots, expanded together (per-tree surface: ``ForestTrees``)."""

    def __init__(self, ctx: Context, maze, start_state, goal_state, n_trees, tree_capacity, edge_length=64, action_horizon=8,
                 pred_horizon=64, local_map_size=20, local_map_scale=0.2, s_global=1.0, batch=1024, k_steps=1,
                 emulate_sticky_done=True, norm=CAR_NORM, early_exit=False, goal_scale=None, prop_duration=None, solution="first",
                 reach=None, near_radius=None, near_reach=None, sparse_cell=None, sparse_headings=None):
        capacity = self._init_forest(ctx, n_trees, tree_capacity)
        super().__init__(ctx, maze, start_state, goal_state, edge_length=edge_length, action_horizon=action_horizon,
                         pred_horizon=pred_horizon, local_map_size=local_map_size, local_map_scale=local_map_scale,
                         s_global=s_global, batch=batch, capacity=capacity, k_steps=k_steps,
                         emulate_sticky_done=emulate_sticky_done, norm=norm, early_exit=early_exit, run_type=0,
                         goal_scale=goal_scale, prop_duration=prop_duration, solution=solution, reach=reach,
                         near_radius=near_radius, near_reach=near_reach, sparse_cell=sparse_cell,
                         sparse_headings=sparse_headings)

    def expand_round(self, samples, cond_goal, noise=None, inject_actions=None, counts_per_tree=None, step_noise=None,
                     accept=True):
        """samples (B, 6) f64, cond_goal (B, 2) f64, noise (B, n_chunks, P, 2) f32 or inject_actions (B, n_chunks, P, 2) f64,
        step_noise (B, n_chunks, K, P, 2) f32 with ``self.ddpm`` [device tensors]: the rows of tree t are
        [off[t], off[t+1]), off = the running sum of ``counts_per_tree`` (T,), each tree's rows in its run's own order.
        Returns the (T, 8) counter block after the accept."""
        return self._round(samples, cond_goal, noise, inject_actions, step_noise, accept, counts_per_tree)


class AntForestEngine(ForestTrees, AntExpansionEngine):
    """T independent ant trees (BASELINE config 3: 29-d states, 8-d actions, every node's three history rows) of
    ``tree_capacity`` node slots, expanded together: ``AntExpansionEngine``'s round settings and dynamics ("tape" | "model")
    with ``ForestTrees``' per-tree surface.  Each tree grows exactly as in its own ``AntExpansionEngine`` fed the same rows.
    The ant env has no sticky-done latch, so no tree ever has a phantom candidate."""

    def __init__(self, ctx: Context, maze, start_state, goal_state, n_trees, tree_capacity, desired_goal=None, norm=None,
                 edge_length=48, action_horizon=2, pred_horizon=16, local_map_size=16, local_map_scale=0.8, s_global=4.0,
                 batch=4096, k_steps=1, early_exit=False, goal_scale=None, dynamics="tape", model=None, ball_radius=1.2,
                 goal_factor=0.45):
        if dynamics not in ("tape", "model"):
            raise ValueError("an ant forest's dynamics must be 'tape' or 'model' (a host-stepped round has no forest form)")
        capacity = self._init_forest(ctx, n_trees, tree_capacity)
        super().__init__(ctx, maze, start_state, goal_state, desired_goal=desired_goal, norm=norm, edge_length=edge_length,
                         action_horizon=action_horizon, pred_horizon=pred_horizon, local_map_size=local_map_size,
                         local_map_scale=local_map_scale, s_global=s_global, batch=batch, capacity=capacity, k_steps=k_steps,
                         early_exit=early_exit, goal_scale=goal_scale, dynamics=dynamics, model=model, ball_radius=ball_radius,
                         goal_factor=goal_factor)

    def expand_round(self, samples, cond_goal, noise=None, inject_actions=None, counts_per_tree=None, step_noise=None,
                     accept=True, next_obs_tape=None, cond_out=None):
        """samples (B, 29) f64, cond_goal (B, 2) f64, noise (B, n_chunks, P, 8) f32 or inject_actions (B, n_chunks, P, 8) f64,
        step_noise (B, n_chunks, K, P, 8) f32 with ``self.ddpm``, next_obs_tape (B, n_chunks, A, 29) f64 for
        dynamics='tape', cond_out (B, n_chunks, 97) f32 (tests) [device tensors]: the rows of tree t are [off[t], off[t+1]),
        off = the running sum of ``counts_per_tree`` (T,), each tree's rows in its run's own order.  Returns the (T, 8)
        counter block after the accept."""
        return self._round(samples, cond_goal, noise, inject_actions, step_noise, accept, counts_per_tree,
                           next_obs_tape=next_obs_tape, cond_out=cond_out)


# ---------------------------------------------------------------------- scene forests
def cell_codes(maze):
    """The u8 cell codes the device stores for a maze (ditree_upload_maze's rule: integral values 0..255, else 255)."""
    m = np.asarray(maze, dtype=np.float32)
    c = m.astype(np.int64)
    ok = (m == c.astype(np.float32)) & (c >= 0) & (c < 256)
    return np.where(ok, c, 255).astype(np.uint8)


def atlas_layout(mazes):
    """The atlas ditree_upload_scenes builds: a map equal to an earlier scene's (dims and cell codes) shares its bytes.
    -> (offsets (n,), dims (n, 2), atlas cells)."""
    offsets, dims, seen, used = [], [], [], 0
    for m in mazes:
        codes = cell_codes(m)
        off = next((o for o, k in seen if k.shape == codes.shape and np.array_equal(k, codes)), None)
        if off is None:
            off = used
            seen.append((off, codes))
            used += codes.size
        offsets.append(off)
        dims.append(codes.shape)
    return np.array(offsets, dtype=np.int64), np.array(dims, dtype=np.int64).reshape(-1, 2), used


class SceneTrees:
    """The scene bookkeeping of a scene forest, mixed in over a forest engine (``ForestEngine`` for the car, ``AntForestEngine``
    for the ant): the scene lists, the atlas and the scene table's upload, the scene id of every tree, ``reset`` /
    ``reset_tree(t, scene)`` and the per-tree fallback goals.  ``scenes``: a list of ``(maze, start_state, goal_state, goal)``;
    ``goal`` is what the scene table's goal column holds -- what the rollout's goal test reads: the car's ``env.goal``, the
    ant's ``desired_goal`` -- and the engine class derives it when it is None or left out (``_scene_goal``)."""

    def _init_scenes(self, ctx, scenes, n_trees):
        """Before the forest's own constructor (which ends in ``reset``)."""
        scenes = list(scenes)
        if not 1 <= len(scenes) <= MAX_SCENES:
            raise ValueError(f"a scene forest holds 1..{MAX_SCENES} scenes, got {len(scenes)}")
        self.scene_mazes, self.scene_starts, self.scene_goals, self.scene_env_goals = [], [], [], []
        for sc in scenes:
            maze, start, goal = sc[0], sc[1], sc[2]
            env_goal = sc[3] if len(sc) > 3 else None
            maze = np.asarray(maze, dtype=np.float32)
            goal = np.asarray(goal, dtype=np.float64).copy()
            self.scene_mazes.append(maze)
            self.scene_starts.append(np.asarray(start, dtype=np.float64).copy())
            self.scene_goals.append(goal)
            self.scene_env_goals.append(np.asarray(self._scene_goal(maze, goal) if env_goal is None else env_goal, dtype=np.float64)[:2].copy())
        cells = sum(m.size for m in self.scene_mazes)
        if cells > MAX_ATLAS_CELLS:
            raise ValueError(f"the scenes' mazes hold {cells} cells, more than the atlas's {MAX_ATLAS_CELLS}")
        self.atlas_offsets, self.atlas_dims, self.atlas_cells = atlas_layout(self.scene_mazes)
        T = int(n_trees)
        self.tree_scene_host = (C.c_int32 * max(T, 1))()
        self.tree_scene_dev = torch.zeros(max(T, 1), dtype=torch.int32, device=ctx.device)
        self.sdesc = ForestScenes(self.tree_scene_dev.data_ptr(), self.tree_scene_host)
        self.ctx = ctx
        self.upload_scenes()

    def upload_scenes(self):
        self.ctx.upload_scenes(self.scene_mazes, np.stack(self.scene_env_goals), owner=self)

    def ensure_maze(self):
        """The ctx's scene table must be this forest's before any launch (the single maze is not read)."""
        if self.ctx.scenes_owner is not self:
            self.upload_scenes()

    def update_maze(self, maze):
        raise NotImplementedError("a scene forest's mazes are fixed at construction")

    @property
    def n_scenes(self):
        return len(self.scene_mazes)

    def reset(self, start_state=None, goal_state=None):
        """Every tree back to the root of its scene (start_state / goal_state are not read: each scene has its own)."""
        self.start_state, self.goal_state = self.scene_starts[0].copy(), self.scene_goals[0].copy()
        self.env_goal = self.scene_env_goals[0].copy()
        self.tree.reset(self.start_state)
        for t in range(self.T):
            self.reset_tree(t, self.tree_scene_host[t])
        self.generation = getattr(self, "generation", 0) + 1

    def reset_tree(self, t, scene=None):
        """Tree t back to a root: the start of ``scene`` (default: the tree's current scene), which the tree then grows on
        (the ant: with the root's history rows restored from that start, as ``ForestTrees.reset_tree`` leaves them)."""
        t = self._tree_index(t)
        scene = int(self.tree_scene_host[t] if scene is None else scene)
        if not 0 <= scene < self.n_scenes:
            raise IndexError(f"scene {scene} of {self.n_scenes}")
        self.tree_scene_host[t] = scene
        self.tree_scene_dev[t] = scene
        super().reset_tree(t, self.scene_starts[scene])

    def tree_scene(self, t):
        return int(self.tree_scene_host[self._tree_index(t)])

    def _sparse_mazes(self):                          # the sparse tree's table is sized for the largest scene
        return self.scene_mazes

    def _sparse_maze_of(self, t):
        return self.scene_mazes[self.tree_scene(t)]

    def fallback_nodes(self):
        """planners/RRT.py:227-254 (run_type 0) for every tree, each against its own scene's goal_state[:2]."""
        return self._fallback_launch(np.stack([self.scene_goals[self.tree_scene(t)][:2] for t in range(self.T)]))


class SceneForestEngine(SceneTrees, ForestEngine):
    """A forest whose trees belong to different scenes of a scenario set.  ``scenes``: a list of ``(maze, start_state,
    goal_state, env_goal)`` (env_goal None: the goal cell's centre, as env.reset sets it).  Tree t grows on scene
    ``tree_scene(t)``: its root is that scene's start, its local map, collision and goal tests use that scene's maze and goal,
    and its fallback is the node nearest to that scene's goal -- exactly as its own ``ExpansionEngine`` on that scene.  All
    mazes sit in one scene table on the device (include/ditree.h "scene forests"); no single maze is read.  The scene
    bookkeeping is ``SceneTrees``'."""
    _scene_goal = staticmethod(env_goal_of)

    def __init__(self, ctx: Context, scenes, n_trees, tree_capacity, **kw):
        self._init_scenes(ctx, scenes, n_trees)
        super().__init__(ctx, self.scene_mazes[0], self.scene_starts[0], self.scene_goals[0], n_trees, tree_capacity, **kw)

    def _bound_goal_rows(self):                       # each tree's own scene's goal
        return np.stack([self.scene_env_goals[self.tree_scene(t)] for t in range(self.T)])


class AntSceneForestEngine(SceneTrees, AntForestEngine):
    """An ant forest whose trees belong to different scenes of the antmaze scenario set (run_scenarios.py:202-233).
    ``scenes``: a list of ``(maze, start_state (29,), goal_state (29,), desired_goal (2,))`` (desired_goal None: the goal cell's
    centre); ``**ant_kw``: ``AntForestEngine``'s keyword arguments.  Tree t grows on scene ``tree_scene(t)``: its root (state and
    history rows) is that scene's start, its local map, collision test and goal test use that scene's maze and
    ``desired_goal`` -- the scene table's goal column -- and its fallback is the node nearest to that scene's
    ``goal_state[:2]``: exactly as its own ``AntExpansionEngine`` on that scene.  ``goal_radius``, ``ball_radius`` and
    ``s_global`` hold for all scenes.  All mazes sit in one scene table on the device (include/ditree.h "ant scene forests");
    no single maze is read."""
    def __init__(self, ctx: Context, scenes, n_trees, tree_capacity, **ant_kw):
        if "desired_goal" in ant_kw:
            raise TypeError("AntSceneForestEngine: every scene carries its own desired_goal")
        self._scene_s_global = float(ant_kw.get("s_global", 4.0))
        self._init_scenes(ctx, scenes, n_trees)
        super().__init__(ctx, self.scene_mazes[0], self.scene_starts[0], self.scene_goals[0], n_trees, tree_capacity,
                         desired_goal=self.scene_env_goals[0], **ant_kw)

    def _scene_goal(self, maze, goal_state):
        return ant_cell_centre(maze, goal_state, self._scene_s_global)
