"""RRT_Planner facade (reference: planners/RRT.py:18-257) -- the expand loop as wide rounds on the GPU.

Constructor kwargs, ``plan() -> (path f32 (P,6)|None, actions f32 (A,2)|None)``, ``reset``,
``update_maze``, ``results`` and ``node_list`` follow the reference.  Extra kwargs:
  ``batch``            candidates per round (default 512 = one full wave of 256-row tiles on the 256 CUs for the `large`
                       denoiser: rounds of 128 and 256 take the same time as each other, multiples of 512 fill whole waves; 1 = the
                       reference's sequential order),
  ``max_candidates``   deterministic budget instead of / in addition to the wall-clock budget,
  ``early_exit``       (default True) later chunks of collided / finished candidates are skipped, as the
                       reference abandons a collided edge; results are identical either way,
  ``prop_duration``    the reference's per-visit edge-length schedule (RRT.py:26,149-152): in a round the candidates of
                       one parent are its visits in candidate order,
  ``rank`` / ``world_size`` / ``process_group``   shard every round over the ranks of a torch.distributed group (default:
                       the initialised default group, i.e. what `torch.distributed.run` set up; one rank otherwise).  All
                       ranks must draw the same samples and noise -- the reference's scripts seed every RNG with 42
                       (run_scenarios.py:86-90) -- and all ranks return the same path.
  ``solution``         which goal-reaching candidate a plan returns.  "first" (default): the lowest-index one of the first
                       goal-reaching round, the rest of that round dropped -- the reference's loop.  "best_of_round": the plan
                       still ends with that round, but every non-collided candidate of it is appended and the goal node is the
                       one with the shortest path (rows of ``path``; ties to the lowest index).  "anytime": rounds go on until
                       ``time_budget`` / ``max_candidates`` ends and the shortest goal path found is returned (a later node
                       replaces the incumbent only when strictly shorter).  The two new modes need
                       ``emulate_sticky_done=False`` (its default then) and cover the car, one rank, run_type 0.
                       ``results`` gains ``solutions`` (goal nodes appended) and ``first_solution_candidates`` (candidates
                       processed up to and including the first goal-reaching round, or None).
                       "anytime_pruned": "anytime" until a plan holds an incumbent, branch and bound from then on -- a parent
                       is chosen only among the nodes whose key (path rows so far + rows still needed at best) is below the
                       incumbent's rows, a candidate that cannot beat the incumbent gets no node, and the plan ends as soon
                       as no node is open, before the budgets do.  ``bound_speed`` (this mode only; default ``max_v`` = 5, the
                       reference's velocity range) sets the metres a path row is assumed to cover at most, ``bound_speed *
                       env_dt`` (0.1 m for the car).  The dynamics have no hard speed limit, so this bound is a setting and
                       not a theorem: a smaller ``bound_speed`` prunes more and may prune a branch that would have won.
                       Same scope as "anytime", and a single ``prop_duration`` entry.  ``results`` gains
                       ``pruned_candidates``, ``closed_nodes`` (nodes whose key is at or past the final incumbent's rows,
                       counted once at the end) and ``bound_exhausted``.
  ``reuse_tree``       (default False) ``reset(start_state=...)`` keeps the tree of the last plan where the car still stands on
                       that plan and the goal is unchanged: it is re-rooted at the car, the branches the current maze blocks
                       are dropped with everything behind them, and the rest is compacted on the device
                       (``ExpansionEngine.rebase``).  ``reuse_tol`` (default 1e-3: m, m, rad, m/s; 1 % of the collision ball's
                       0.1 m radius) is how close ``start_state`` must be to a row of the plan.  Anything else -- no plan yet,
                       the car off its plan, another goal -- is the reset as ever.  ``plan()`` on a tree that kept its goal node
                       returns that node's path at once ("first", "best_of_round") or plans on with it as the incumbent
                       ("anytime").  ``results`` gains ``reused_nodes`` / ``dropped_nodes`` (0 after a fresh reset), and
                       ``number_of_nodes`` counts the reused nodes.  The car, one rank, not "anytime_pruned".
  ``near_radius``      (default None: off, the planner as it is without the kwarg) metres.  A sample's parent is not its nearest
                       node but, among the nodes within ``near_radius`` of that nearest distance, the one through which the
                       sample is reached in the fewest path rows: cost[n] + distance(n, sample) / (``near_speed * env_dt``)
                       (include/ditree.h "near parent" -- the choose-parent step of RRT*, no rewiring).  ``near_speed``
                       (default ``max_v``, as ``bound_speed``) is the speed a path row is assumed to cover; a setting, not a
                       theorem.  No random stream moves: the samples are those of the same run without the kwarg.  Scope: that
                       of the cost column -- ``solution`` "best_of_round", "anytime" or "anytime_pruned" (then among the open
                       nodes), the car, one rank, run_type 0, a single ``prop_duration`` entry; ``plan_runs``,
                       ``plan_scenario_runs`` and ``reuse_tree`` included.
  ``sparse_cell``      (default None: off, the planner as it is without the kwarg) metres.  The witness pruning of SST (Li,
                       Littlefield, Bekris 2016) on a grid of ``sparse_cell`` x ``sparse_cell`` metres x ``sparse_headings``
                       heading bins (an integer from 1 to 64, default 8) over the map (include/ditree.h "sparse tree"): of the
                       nodes that end in one cell only the cheapest -- the cell's active node -- is looked at by the parent
                       search (nearest node, ``near_radius``, with "anytime_pruned" among the open ones), and a candidate that
                       lands in a cell whose node is at most as dear takes no node.  A goal-reaching candidate always gets its
                       node, so the solutions and the incumbent rule are untouched; a displaced node stays in the tree with its
                       subtree and its place in the fallback.  No random stream moves.  The tree stays small -- and may lose
                       goals that the dense tree finds: large cells throw away the nodes that would have squeezed through.
                       ``results`` gains ``dominated_candidates``, ``retired_nodes`` and ``active_nodes``.  Scope: that of
                       ``near_radius``, with or without it; with ``reuse_tree`` the active nodes are derived again from the
                       re-based tree.
All of the reference's ``run_type`` values: 0 "Original"; 1 "Original+Ref" (obstacle-ahead flags per node, sampling
biased to the part of ``init_main_path`` behind the obstacle, furthest-along-path fallback); 2 "OM+Ref" (sample
positions drawn from the EDT prior); 3 "OM+LB+Ref" (prior log-blended with the start -> goal Gaussian, refreshed at
every plan); 4 adds the driver's forced re-plan and is the same as 3 inside the planner.
"""
from __future__ import annotations

import random
import time

import numpy as np
import torch

from ..engine import ANYTIME, CNT_GOAL, CNT_ITERS, AntExpansionEngine, ExpansionEngine, default_shard
from .base_planner import BasePlanner, Node


class RRT_Planner(BasePlanner):
    def __init__(self, start_state, goal_state, environment, sampler, **kwargs):
        super().__init__(start_state, goal_state, environment, sampler, **kwargs)
        self.kd_tree_dim = 2
        self.goal_sample_rate = 0.15
        self.goal_conditioning_bias = kwargs.get("goal_conditioning_bias", 0.85)
        self.prop_duration_schedule = list(kwargs.get("prop_duration", [64]))
        # plan() runs fused rounds (ditree_expand_round): K flow-matching Euler steps inside the library, or -- a sampler built
        # with policy='diffusion' and a DDPM scheduler of the reference's configuration (run_scenarios.py:157-158) -- the K
        # DDPM reverse steps (fm_policy.py:164-182; ditree_denoise_ddpm).  Any other scheduler object can only drive
        # DiffusionSampler.forward itself: refuse instead of sampling with the wrong rule.
        self._ddpm = None
        if getattr(sampler, "policy", "flow_matching") == "diffusion":
            self._ddpm = sampler.ddpm_tables() if hasattr(sampler, "ddpm_tables") else None
            if self._ddpm is None:
                raise NotImplementedError("RRT_Planner.plan with policy='diffusion' needs a DDPM scheduler with epsilon prediction, "
                                          "clip_sample and fixed_small variance (the reference's configuration); other schedulers "
                                          "are only available through DiffusionSampler.forward")
        elif getattr(sampler, "policy", "flow_matching") != "flow_matching":
            raise NotImplementedError(f"policy={getattr(sampler, 'policy', None)!r}")
        self.offline_time_budget = kwargs.get("offline_time_budget", 60)
        self.plan_count = 0
        self.init_main_path = None
        self.run_type = kwargs.get("run_type", 0)
        self.env.run_type = self.run_type
        self.batch = int(kwargs.get("batch", 512))
        self.max_candidates = kwargs.get("max_candidates", None)
        self.capacity = int(kwargs.get("capacity", 65536))
        self.solution = kwargs.get("solution", "first")
        self._check_near(kwargs)
        self._check_sparse(kwargs)
        self._check_solution(kwargs)
        self._check_reuse(kwargs)
        sticky = kwargs.get("emulate_sticky_done", self.solution == "first")
        lm = self.local_map_size if isinstance(self.local_map_size, (int, float)) else self.local_map_size[0]
        d_rank, d_world, d_pg = default_shard()
        self.world_size = int(kwargs.get("world_size", d_world))
        self.rank = int(kwargs.get("rank", d_rank if self.world_size == d_world else 0))
        self.process_group = kwargs.get("process_group", d_pg)
        from concurrent.futures import ThreadPoolExecutor
        self._draw_pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="ditree-draw")
        if self.is_ant:
            self._init_ant_engine(sampler, kwargs, int(lm))
            return
        self._engine = ExpansionEngine(
            self.ctx, self.maze, self.start_node.state, self.goal_state, edge_length=max(self.prop_duration_schedule),
            prop_duration=self.prop_duration_schedule,
            action_horizon=self.action_horizon, pred_horizon=getattr(sampler, "pred_horizon", 64),
            local_map_size=int(lm), local_map_scale=self.local_map_scale, s_global=self.s_global, batch=self.batch,
            capacity=self.capacity, k_steps=getattr(sampler, "num_diffusion_iters", 1),
            norm=getattr(sampler, "norm", None) if getattr(sampler, "norm", None) is not None else None,
            emulate_sticky_done=sticky, early_exit=kwargs.get("early_exit", True),
            run_type=self.run_type, goal_scale=getattr(sampler, "local_map_size", None),
            rank=self.rank, world_size=self.world_size, process_group=self.process_group, solution=self.solution,
            reach=self.bound_reach, near_radius=self.near_radius, near_reach=self.near_reach, sparse_cell=self.sparse_cell,
            sparse_headings=self.sparse_headings)
        self._engine.env_goal = np.asarray(self.env.goal, dtype=np.float64)
        self._engine.ddpm = self._ddpm

    def _check_solution(self, kwargs):
        """The ``solution`` modes other than "first": refused by name where they are not built, before the device is touched."""
        from ..engine import SOLUTIONS
        sol = self.solution
        if sol not in SOLUTIONS:
            raise ValueError(f"solution must be one of {SOLUTIONS}, got {sol!r}")
        self.bound_speed = self.bound_reach = None
        if "bound_speed" in kwargs and sol != "anytime_pruned":
            raise ValueError(f"bound_speed belongs to solution='anytime_pruned' (got solution={sol!r})")
        if sol == "first":
            return
        if kwargs.get("emulate_sticky_done", False):
            raise ValueError(f"solution={sol!r} and emulate_sticky_done=True do not go together: the sticky-done emulation ends "
                             "a plan at its first goal")
        if self.is_ant:
            raise NotImplementedError(f"solution={sol!r}: the car only (env_id='antmaze' keeps solution='first')")
        world = int(kwargs.get("world_size", default_shard()[1]))
        if world > 1:
            raise NotImplementedError(f"solution={sol!r}: one rank (world_size {world}; a sharded round keeps solution='first')")
        if self.run_type != 0:
            raise NotImplementedError(f"solution={sol!r}: run_type 0 only (run_type {self.run_type} keeps solution='first')")
        if sol != "anytime_pruned":
            return
        if len(self.prop_duration_schedule) > 1:
            raise NotImplementedError(f"solution={sol!r}: a single prop_duration entry (the chunk-budget search of a schedule is "
                                      "not masked by the bound)")
        v = kwargs.get("bound_speed", self.max_v)
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or v <= 0:
            raise ValueError(f"bound_speed must be a positive finite number, got {v!r}")
        self.bound_speed = float(v)
        self.bound_reach = self.bound_speed * float(self.env_dt)      # metres a path row is assumed to cover at most

    def _check_near(self, kwargs):
        """``near_radius`` / ``near_speed``: refused by name where they are not built, before the device is touched."""
        r = kwargs.get("near_radius")
        self.near_radius = self.near_speed = self.near_reach = None
        if r is None:
            if kwargs.get("near_speed") is not None:
                raise ValueError("near_speed belongs to near_radius (near_radius is None)")
            return
        v = kwargs.get("near_speed")
        v = self.max_v if v is None else v
        for name, x in (("near_radius", r), ("near_speed", v)):
            if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or not np.isfinite(x) or x <= 0:
                raise ValueError(f"{name} must be a positive finite number, got {x!r}")
        if self.solution == "first":
            raise ValueError("near_radius needs solution='best_of_round', 'anytime' or 'anytime_pruned' (solution='first' keeps no "
                             "cost column)")
        if self.is_ant:
            raise NotImplementedError("near_radius: the car only (env_id='antmaze' keeps no cost column)")
        world = int(kwargs.get("world_size", default_shard()[1]))
        if world > 1:
            raise NotImplementedError(f"near_radius: one rank (world_size {world})")
        if self.run_type != 0:
            raise NotImplementedError(f"near_radius: run_type 0 only (got run_type {self.run_type})")
        if len(self.prop_duration_schedule) > 1:
            raise NotImplementedError("near_radius: a single prop_duration entry (the chunk-budget search of a schedule is the plain "
                                      "nearest node)")
        self.near_radius, self.near_speed = float(r), float(v)
        self.near_reach = self.near_speed * float(self.env_dt)        # metres a path row is assumed to cover

    def _check_sparse(self, kwargs):
        """``sparse_cell`` / ``sparse_headings``: refused by name where they are not built, before the device is touched."""
        from ..engine import check_sparse, sparse_grid
        self.sparse_cell = self.sparse_headings = None
        if kwargs.get("sparse_cell") is None:
            check_sparse(None, kwargs.get("sparse_headings"), self.solution)
            return
        cell, headings = check_sparse(kwargs["sparse_cell"], kwargs.get("sparse_headings"), self.solution, self.is_ant,
                                      self.prop_duration_schedule)
        world = int(kwargs.get("world_size", default_shard()[1]))
        if world > 1:
            raise NotImplementedError(f"sparse_cell: one rank (world_size {world})")
        if self.run_type != 0:
            raise NotImplementedError(f"sparse_cell: run_type 0 only (got run_type {self.run_type})")
        self.sparse_cell, self.sparse_headings = cell, headings
        sparse_grid(np.asarray(self.maze).shape, self.s_global, self.sparse_cell, self.sparse_headings)     # the table's size

    def _check_reuse(self, kwargs):
        """``reuse_tree``: refused by name where it is not built, before the device is touched."""
        self.reuse_tree = bool(kwargs.get("reuse_tree", False))
        self.reuse_tol = float(kwargs.get("reuse_tol", 1e-3))
        self._remembered = None                      # _reuse.RememberedPlan of the last returned plan
        self._edge_phase = {}                        # node id -> (state rows, action rows) re-bases took off its edge's front
        if not self.reuse_tree:
            return
        if not (np.isfinite(self.reuse_tol) and self.reuse_tol >= 0):
            raise ValueError(f"reuse_tol must be a finite number >= 0, got {kwargs.get('reuse_tol')!r}")
        if self.is_ant:
            raise NotImplementedError("reuse_tree=True: the car only (env_id='antmaze' resets its tree)")
        world = int(kwargs.get("world_size", default_shard()[1]))
        if world > 1:
            raise NotImplementedError(f"reuse_tree=True: one rank (world_size {world}; a sharded tree keeps edge rows on other ranks)")
        if self.solution == "anytime_pruned":
            raise NotImplementedError("reuse_tree=True: solution='anytime_pruned' is not built (key column, stats row, closed nodes)")

    # ------------------------------------------------------------------ ant (BASELINE config 3)
    def _init_ant_engine(self, sampler, kwargs, lm):
        """env_id = 'antmaze' (cfgs/antmaze.yaml, run_scenarios.py:123-132,225-233): 29-d states, 8-d actions, action_horizon 2,
        local map 16 @ 0.8, global_map_scale 4.  Everything of the expand loop runs on the device -- sampling glue, denoiser,
        the reference's collision and goal tests on every observation, accept -- EXCEPT the env step, which is MuJoCo in the
        reference and is not part of this build: ``ant_dynamics``
          "host" (default)  the planner steps the CALLER's env (``environment.ant_env.set_state(qpos, qvel)`` +
                            ``environment.step(action)`` per candidate and step, planners/base_planner.py:278-279,290) between
                            the two halves of every chunk,
          "model"           the build's stand-in crawler model on the device (NOT MuJoCo; parity unpinned),
          "tape"            observations from ``next_obs_tape_fn(first_candidate, B) -> (B, n_chunks, A, 29)`` (tests)."""
        if self.run_type != 0:
            raise NotImplementedError("antmaze: run_type 0 (the reference's check_obstacle_ahead / sampling maps are the car's)")
        if len(self.prop_duration_schedule) != 1:
            raise NotImplementedError("antmaze: a single prop_duration entry")
        self.ant_dynamics = kwargs.get("ant_dynamics", "host")
        self._tape_fn = kwargs.get("next_obs_tape_fn")
        norm = getattr(sampler, "norm", None)
        if norm is None:                                        # a non-network sampler: the packaged copy of metadata/antmaze.pt
            from ..policies.fm_policy import load_metadata
            md = load_metadata("antmaze")
            norm = np.concatenate([md["Observations_mean"], md["Observations_std"], md["Actions_mean"], md["Actions_std"]])
        desired = kwargs.get("desired_goal")
        out = getattr(self, "_reset_out", None)
        if desired is None and isinstance(out, tuple) and isinstance(out[0], dict) and "desired_goal" in out[0]:
            desired = out[0]["desired_goal"]                    # the env's goal incl. its position noise (base_planner.py:296)
        if self.ant_dynamics == "host" and self.world_size > 1:
            raise NotImplementedError("antmaze with a host-side simulator: one rank (the env object is not sharded)")
        self._engine = AntExpansionEngine(
            self.ctx, self.maze, self.start_node.state, self.goal_state, desired_goal=desired, norm=norm,
            edge_length=self.prop_duration_schedule[0], action_horizon=self.action_horizon,
            pred_horizon=getattr(sampler, "pred_horizon", 16), local_map_size=lm, local_map_scale=self.local_map_scale,
            s_global=self.s_global, batch=self.batch, capacity=self.capacity, k_steps=getattr(sampler, "num_diffusion_iters", 1),
            early_exit=kwargs.get("early_exit", True), goal_scale=getattr(sampler, "local_map_size", None),
            dynamics=self.ant_dynamics, model=kwargs.get("ant_model"), rank=self.rank, world_size=self.world_size,
            process_group=self.process_group)
        self._engine.ddpm = self._ddpm

    def _ant_env_step(self, chunk, start, actions, rows):
        """planners/base_planner.py:278-279,290,298 for the alive candidates of one chunk, on the caller's env."""
        A = actions.shape[1]
        out = np.zeros((len(rows), A, 29))
        for k in range(len(rows)):
            self.env.ant_env.set_state(start[k, :15], start[k, 15:])
            for i in range(A):
                out[k, i], _ = self.ant_obs(self.env.step(actions[k, i]))
        return out

    # ------------------------------------------------------------------ reference surface
    def reset(self, start_state=None, goal_state=None, reset_main_path=False):
        if reset_main_path:
            self.init_main_path = None
        if start_state is not None:
            self.start_node = Node(np.asarray(start_state, dtype=np.float64))
            self.goal_state = np.asarray(goal_state, dtype=np.float64)
            to_rc = self.env.maze_data.cell_xy_to_rowcol if self.is_ant else self.env.cell_xy_to_rowcol
            self.options["reset_cell"] = to_rc(start_state[:2])
            if not self.is_ant:
                self.options["reset_deg"] = np.rad2deg(start_state[2])
            self.options["goal_cell"] = to_rc(goal_state[:2])
        self.failed_node_list = []
        self.results = {"iterations": 0, "time": 0, "path": None, "actions": None, "number_of_nodes": 0, "solutions": 0,
                        "first_solution_candidates": None}
        if self.solution == "anytime_pruned":
            self.results.update(pruned_candidates=0, closed_nodes=0, bound_exhausted=False)
        if self.reuse_tree:
            self.results.update(reused_nodes=0, dropped_nodes=0)
        if self.sparse_cell is not None:
            self.results.update(dominated_candidates=0, retired_nodes=0, active_nodes=1)
        out = self.env.reset(options=self.options)
        if self.is_ant:
            if isinstance(out, tuple) and isinstance(out[0], dict) and "desired_goal" in out[0]:
                self._engine._desired_arg = np.asarray(out[0]["desired_goal"], dtype=np.float64)[:2].copy()
            self._engine.reset(self.start_node.state, self.goal_state)
            return
        if not (self.reuse_tree and start_state is not None and self._reuse_reset()):
            self._remembered, self._edge_phase = None, {}
            self._engine.reset(self.start_node.state, self.goal_state)
        self._engine.env_goal = np.asarray(self.env.goal, dtype=np.float64)

    def _reuse_reset(self):
        """``reset(start_state=...)`` with ``reuse_tree``: re-base the tree at the car where it stands on the remembered plan
        (planners/_reuse.py), grown for this goal.  False: nothing to keep -- the caller resets as ever."""
        from ._reuse import locate
        plan, eng = self._remembered, self._engine
        if plan is None or not np.array_equal(plan.goal_state, self.goal_state):
            return False
        where = locate(plan, self.start_node.state, self.reuse_tol, eng.A)
        if where is None:
            return False
        anchor, drop_states, drop_actions = where
        kept, dropped = eng.rebase(anchor, root_state=self.start_node.state, drop_states=drop_states, drop_actions=drop_actions)
        self.results.update(reused_nodes=kept, dropped_nodes=dropped)
        # what is left of the plan, under the new ids: the chain from the anchor to its last kept node
        tail = plan.chain[plan.chain.index(anchor):]
        ids = eng.rebase_ids[torch.as_tensor(tail, device=self.ctx.device, dtype=torch.long)].cpu().numpy()
        last = 0
        for v in ids:
            if v < 0:
                break
            last = int(v)
        # the rows that re-bases have taken off the front of an edge stay known under the node's new id: behind a fresh root it
        # is the anchor's edge that lost rows (again); an anchor that became the root has no edge any more
        old = self._edge_phase
        self._edge_phase = {}
        if old:
            keys = list(old)
            new = eng.rebase_ids[torch.as_tensor(keys, device=self.ctx.device, dtype=torch.long)].cpu().numpy()
            self._edge_phase = {int(v): old[k] for k, v in zip(keys, new) if v > 0}
        if drop_states > 0 and int(ids[0]) == 1:
            s0, a0 = old.get(anchor, (0, 0))
            self._edge_phase[1] = (s0 + drop_states, a0 + drop_actions)
        self._remembered = self._remember(last)
        return True

    def _remember(self, node):
        """The chain root .. ``node`` in the tree's f64 (``path`` is float32), for the next ``reset(start_state=...)``."""
        from ._reuse import RememberedPlan
        chain, ns, na, rows = self._engine.chain_rows(node)
        return RememberedPlan(chain, ns, na, rows, self.goal_state, [self._edge_phase.get(c, (0, 0)) for c in chain])

    def handle_goal_reached(self, node_index, iterations, start_time):
        out = super().handle_goal_reached(node_index, iterations, start_time)
        if self.reuse_tree:
            self._remembered = self._remember(node_index)
        return out

    def update_maze(self, new_maze):
        self.maze = np.float32(new_maze)
        if not self.is_ant:
            self.env.maze_map = new_maze
        self._engine.update_maze(self.maze)

    def adopt_maze(self, new_maze):
        """Take a known maze whose device copy is already current (online.follow_plan refreshes it in its own
        launch): same bookkeeping as ``update_maze`` without the upload."""
        self.maze = np.float32(new_maze)
        self.env.maze_map = new_maze
        self._engine.maze = self.maze

    @property
    def node_list(self):
        """``Node`` objects of the device tree (RRT.py:42, base_planner.py:24-34).  The tree only grows between two
        ``reset`` calls, so the list is kept and extended by the rows appended since the last access (one D2H of the new
        rows + the visit counters), not rebuilt: scripts that poll ``len(planner.node_list)`` pay O(new nodes)."""
        t = self._engine.tree
        n = t.n_nodes_host
        gen = getattr(self._engine, "generation", 0)
        cache = getattr(self, "_node_cache", None)
        if cache is None or cache[0] != gen or len(cache[1]) > n:
            cache = (gen, [])
        nodes = cache[1]
        k = len(nodes)
        if k < n:
            states = t.state[k:n].cpu().numpy()
            parents = t.parent[k:n].cpu().numpy()
            es, ea = t.edge_states[k:n].cpu().numpy(), t.edge_actions[k:n].cpu().numpy()
            ns, na = t.edge_nstates[k:n].cpu().numpy(), t.edge_nactions[k:n].cpu().numpy()
            for i in range(k, n):
                j = i - k
                if i == 0:
                    nodes.append(Node(states[0]))
                else:
                    nodes.append(Node(states[j], ea[j, : na[j]], es[j, : ns[j]][None], parent=nodes[parents[j]]))
        nv = t.num_visit[:n].cpu().numpy()
        for i in range(n):
            nodes[i].num_visit = int(nv[i])
        self._node_cache = cache
        return nodes

    def nearest_node(self, sample):
        t = self._engine.tree
        q = torch.as_tensor(np.ascontiguousarray(np.asarray(sample, dtype=np.float64)[:, :2]), device=self.ctx.device)
        idx = self.ctx.nn_argmin(q, t.xy, n_nodes=t.n_nodes_host)
        return self.node_list[int(idx[0].item())]          # cached list: O(nodes appended since the last call)

    def check_obstacle_ahead(self, state):
        """RRT.py:61-81 through the device op (the accept kernel evaluates the same function per new node)."""
        self.ctx.upload_maze(np.asarray(self.maze, dtype=np.float32), owner=None)
        st = torch.as_tensor(np.asarray(state, dtype=np.float64).reshape(1, -1), device=self.ctx.device)
        return bool(self.ctx.obstacle_ahead(st)[0].item())

    def extract_path_after_obstacle(self):
        """RRT.py:83-111: xy of ``init_main_path`` from the point nearest to the env state onwards, cut to what lies behind
        the first blocked stretch.  On the device (ditree_path_after_obstacle: nearest point, cell lookup and the two
        searches in one launch on the known maze).  The nearest-point distances are formed in the dtype numpy gives
        ``env.state[:2] - path`` (float64 unless the env state is float32, as right after env.reset), the cells in the
        path's float32."""
        import ctypes as C
        from .._lib import check, lib
        eng = self._engine
        eng.ensure_maze()
        path = np.ascontiguousarray(self.init_main_path, dtype=np.float32)
        p_dev = torch.as_tensor(path, device=self.ctx.device)
        out = torch.zeros(2, dtype=torch.int32, device=self.ctx.device)
        st = np.asarray(self.env.state)
        cur = (C.c_double * 2)(*[float(v) for v in st[:2]])
        check(self.ctx._h, lib().ditree_path_after_obstacle(self.ctx._h, p_dev.data_ptr(), int(path.shape[1]), int(path.shape[0]),
                                                            cur, int(st.dtype == np.float32), out.data_ptr(), self.ctx.stream),
              "path_after_obstacle")
        c, k = (int(v) for v in out.cpu().numpy())
        return self.init_main_path[c:, :2].copy()[k:]

    def draw_round(self, B, remain_init_path=None):
        """B x [sample -> conditioning goal], element for element what the reference's loop draws and leaving both global
        generators where it leaves them -- in bulk (planners/_draw.py: the raw generator output of the whole round is pulled
        once; 8192 candidates in a few ms instead of 76), falling back to the loop itself for anything the bulk path does not
        cover."""
        from ._draw import draw_round_bulk
        out = draw_round_bulk(self, B, remain_init_path)
        return out if out is not None else self._draw_round_loop(B, remain_init_path)

    def _draw_round_loop(self, B, remain_init_path=None):
        """B x [sample -> conditioning goal] in the reference's RNG call order (base_planner.py:162-207,
        RRT.py:134-140,153-156).  run_type 0: random_node_sample, then the goal-conditioning coin.
        run_type > 0: with a remaining reference path, np.random.choice of one of its points kept with
        probability 0.6 (else random_node_sample); the conditioning goal is the sample itself."""
        s = np.zeros((B, self.start_node.state.shape[0]))
        c = np.zeros((B, 2))
        for i in range(B):
            if remain_init_path is not None:
                k = np.random.choice(np.arange(len(remain_init_path)))
                smp = self.random_node_sample() if random.random() < 0.4 else remain_init_path[k][np.newaxis]
            else:
                smp = self.random_node_sample()
            s[i, : smp.shape[1]] = smp[0]
            if self.run_type == 0:
                c[i] = smp[0, :2] if random.random() > self.goal_conditioning_bias else self.goal_state[:2]
            else:
                c[i] = smp[0, :2]
        return s, c

    # ------------------------------------------------------------------ plan
    def _host_actions(self, first, B):
        """A sampler that is not the network (no ``ensure_bound``): the action sequences of a round come from the host
        and by-pass the denoiser (``inject_actions``).  Protocols, in this order:
          ``sampler.sample_round(first_candidate, B, n_chunks, pred_horizon) -> (B, n_chunks, P, 2)``  (tapes: a pure
          function of the global candidate index, so results do not depend on the round size), or a plain callable in
          the reference's shape, ``sampler(obs, prev_actions, goal, local_map)``, called once per (candidate, chunk) in
          candidate-major order with ``obs = prev_actions = local_map = None`` (it cannot see the state: the rounds are
          expanded on the device) and returning (1, P, 2), (P, 2), or one action (1, 2) / (2,) held for the chunk
          -- the shape policies/uniform_policy.py:7-8 returns."""
        eng = self._engine
        if hasattr(self.sampler, "sample_round"):
            a = np.asarray(self.sampler.sample_round(first, B, eng.n_chunks, eng.P), dtype=np.float64)
        else:
            D = eng.ACTION_DIM
            a = np.empty((B, eng.n_chunks, eng.P, D))
            for b in range(B):
                for j in range(eng.n_chunks):
                    v = np.asarray(self.sampler(None, None, self.goal_state[:2], None), dtype=np.float64)
                    a[b, j] = v.reshape(-1, D) if v.size == eng.P * D else v.reshape(1, D)
        if a.shape != (B, eng.n_chunks, eng.P, eng.ACTION_DIM):
            raise ValueError(f"sampler returned actions of shape {a.shape}, need {(B, eng.n_chunks, eng.P, eng.ACTION_DIM)}")
        return torch.as_tensor(np.ascontiguousarray(a), device=self.ctx.device)

    def plan(self):
        eng = self._engine
        dev = self.ctx.device
        # a re-based tree (reuse_tree) may still hold its goal node: the modes that end at their first goal return its path at
        # once -- no round, no draw from any generator --, the anytime mode plans on with it as the incumbent
        kept_goal = eng.goal_node if self.reuse_tree and self.results.get("reused_nodes", 0) > 0 else None
        if kept_goal is not None and self.solution not in ANYTIME:
            self.results.update(solutions=1, first_solution_candidates=0)
            self.env.done = True
            return self.handle_goal_reached(kept_goal, 0, time.time())
        network = hasattr(self.sampler, "ensure_bound")
        if network:
            self.sampler.ensure_bound(eng.shard(self.batch)[2])
        start_time = time.time()
        drawn = 0
        goal = kept_goal
        has_pm = hasattr(self.env, "prob_map")               # the gym ant env has none (the reference reads it: RRT.py:122)
        orig_prob_map = self.env.prob_map.copy() if has_pm else None
        if self.run_type >= 3:
            self.env.update_prob_map_by_loc()
        remain = None
        if self.run_type > 0 and self.init_main_path is not None:
            remain = self.extract_path_after_obstacle()
        eng.init_main_path = self.init_main_path if self.run_type > 0 else None
        # The samples of round r+1 are drawn (host RNGs, reference call order) by a helper thread while round r runs
        # on the GPU: the C-ABI call releases the GIL, and the draws do not depend on the tree.  The global RNG states
        # are snapshotted before every draw-ahead and restored when the pre-drawn round turns out not to be used (goal
        # reached, budget over), so `random` / `np.random` leave plan() exactly where a run without draw-ahead leaves
        # them.  With batch = 1 nothing is drawn ahead.
        def round_size(already):
            return self.batch if self.max_candidates is None else min(self.batch, self.max_candidates - already)

        ahead = self.batch > 1
        pool = self._draw_pool if ahead else None
        pending = rng_before = None
        cnt = None
        steps_dev = torch.zeros((), dtype=torch.int64, device=dev)     # env steps = two-ball collision tests (cc_calls)
        first = self.solution == "first"
        solutions_dev = None if first else torch.zeros((), dtype=torch.int64, device=dev)
        first_at = None if kept_goal is None else 0                    # candidates drawn when the first goal node appeared
        while eng.agree((time.time() - start_time) < self.time_budget):
            if self.max_candidates is not None and drawn >= self.max_candidates:
                break
            B = round_size(drawn)
            s, c = pending.result() if pending is not None else self.draw_round(B, remain)
            pending = None
            nxt = drawn + B
            if ahead and (self.max_candidates is None or nxt < self.max_candidates):
                rng_before = (random.getstate(), np.random.get_state())
                pending = pool.submit(self.draw_round, round_size(nxt), remain)
            if network:
                # every rank draws the noise of the WHOLE round (same generator state everywhere) and uses its slice
                noise, acts = torch.randn((B, eng.n_chunks, eng.P, eng.ACTION_DIM), device=dev), None
            else:
                noise, acts = None, self._host_actions(drawn, B)
            extra = {}
            if network and eng.ddpm is not None:       # the z of every reverse step, drawn like the start noise (whole round, every rank)
                extra["step_noise"] = torch.randn((B, eng.n_chunks, len(eng.ddpm[0]), eng.P, eng.ACTION_DIM), device=dev)
            if self.is_ant:
                if self.ant_dynamics == "host":
                    extra["step_fn"] = self._ant_env_step
                elif self.ant_dynamics == "tape":
                    extra["next_obs_tape"] = torch.as_tensor(np.ascontiguousarray(self._tape_fn(drawn, B)), device=dev)
            cnt = eng.expand_round(torch.as_tensor(s, device=dev), torch.as_tensor(c, device=dev), noise=noise,
                                   inject_actions=acts, **extra)
            drawn += B
            lo, hi, _ = eng.shard(B)
            steps_dev += eng.rb.chunk_steps[lo:hi].sum()
            if not first:
                solutions_dev += eng.round_solutions(B)
            goal = int(cnt[CNT_GOAL]) if int(cnt[CNT_GOAL]) >= 0 else None      # the incumbent, for the modes that keep one
            if goal is not None:
                if first_at is None:
                    first_at = drawn
                if self.solution not in ANYTIME:
                    break
                if eng.exhausted:                # "anytime_pruned": no node is open any more, the plan ends before its budgets
                    break
        if pending is not None:
            pending.result()                     # never leave the helper running on the global RNGs
            random.setstate(rng_before[0])       # the pre-drawn round is dropped: un-draw it
            np.random.set_state(rng_before[1])
        iters = int(cnt[CNT_ITERS]) if cnt is not None else 0
        from ..common import map_utils as _mu
        if not self.is_ant:                                  # is_colliding_ant does not count its calls (map_utils.py:126-136)
            _mu.add_cc_calls(eng.sum_over_ranks(int(steps_dev.item())))   # the counter the drivers read (run_scenarios.py:338,343)
        if has_pm:
            self.env.prob_map = orig_prob_map
        self.results["solutions"] = (0 if goal is None else 1) if first else int(solutions_dev.item())
        self.results["first_solution_candidates"] = first_at
        if self.solution == "anytime_pruned":
            self.results.update(pruned_candidates=eng.pruned_candidates, closed_nodes=eng.closed_nodes(),
                                bound_exhausted=bool(eng.exhausted))
        if self.sparse_cell is not None:
            self.results.update(dominated_candidates=eng.dominated_candidates, retired_nodes=eng.retired_nodes,
                                active_nodes=eng.active_nodes)
        if goal is not None:
            if not self.is_ant:
                self.env.done = True
            return self.handle_goal_reached(goal, iters, start_time)
        node = eng.fallback_node()                          # RRT.py:227-254
        if node is None:
            return self.handle_goal_not_reached(iters, start_time)
        return self.handle_goal_reached(node, iters, start_time)

    # ------------------------------------------------------------------ polish the plan found
    def polish(self, **settings):
        """Shorten the last plan's action tape by sampled roll-outs on the device (polish.polish_plans; include/ditree.h "plan
        polishing") against the planner's current maze, start and goal.  ``settings``: ``rollouts``, ``iterations``, ``sigma``,
        ``hold``, ``seed`` (defaults: polish.DEFAULTS -- settings picked from a sweep, not tuned truths).

        Replaces ``results["path"]`` (float32 (rows + 1, 6): the start state plus one state per action -- no node row appears
        twice), ``results["actions"]`` and ``results["path_time"]`` (``len(path) * env_dt`` on the new path), adds
        ``results["polish"]`` (``status``, ``rows_in``, ``rows_out``, ``arrival_in``, ``arrival_out``, ``trace``) and returns
        ``(path, actions)``.  A plan without a goal node (``status`` "no_goal": a fallback path, or no path) or one whose
        actions do not replay to the goal from the start state ("no_arrival", "collides", "start_in_goal") comes back
        unchanged.  The car, one rank; ``plan()`` itself is untouched."""
        if self.is_ant:
            raise NotImplementedError("polish: the car (env_id='carmaze') only; the ant's plans are not polished")
        from ..polish import polish_plans
        res = self.results
        if res.get("actions") is None or self._engine.goal_node is None:
            res["polish"] = _polish_report(None, res.get("actions"))
            return res.get("path"), res.get("actions")
        r = polish_plans(self.ctx, self.maze, self.start_node.state[None, :6], np.asarray(self.env.goal, dtype=np.float64)[None, :2],
                         [res["actions"]], **settings)[0]
        _apply_polish(res, r, self.env_dt)
        return res["path"], res["actions"]

    # ------------------------------------------------------------------ many seeded runs at once
    def _forest_engine(self, T, tree_capacity, batch):
        """The ForestEngine (ant: AntForestEngine) of ``plan_runs`` (kept between calls of the same shape): the single-tree
        engine's settings."""
        from ..forest import AntForestEngine, ForestEngine
        e = self._engine
        key = (T, tree_capacity, batch)
        f = getattr(self, "_forest", None)
        if f is None or self._forest_key != key:
            self._forest = f = None                      # free the previous forest's slots first
            cls, kw = (AntForestEngine, {"desired_goal": e.env_goal}) if self.is_ant else (ForestEngine, {})
            f = _forest_like(cls, e, self.maze, self.start_node.state, self.goal_state, T, tree_capacity, batch=batch, **kw)
            self._forest, self._forest_key = f, key
        f.ddpm = e.ddpm
        f.update_maze(self.maze)
        return f

    def plan_runs(self, seeds, concurrent=None, tree_capacity=None):
        """N independent seeded runs of this scenario, expanded together as a forest of trees on one GPU (forest.py).

        Run i returns what ``random.seed(s); np.random.seed(s); torch.manual_seed(s); planner.reset(); planner.plan()`` leaves
        in ``results``, s = seeds[i] -- the same tree, path and actions -- as one dict per seed with ``seed``, ``success`` (a
        path came back: run_scenarios.py:350-353), ``goal_reached``, ``iterations``, ``time``, ``path``, ``actions``,
        ``number_of_nodes``, ``path_time`` (None without a path) and ``cc_calls``.  At most ``concurrent`` runs are in flight
        (default: all); a finished run's tree takes the next seed.  Each round gives every active run min(batch, what is left
        of its max_candidates) candidates; ``time_budget`` counts from a run's own start, so ``time`` is wall time inside a
        shared forest.  ``tree_capacity``: node slots per run (default: max_candidates + 1, at most ``capacity``).  The
        caller's ``random`` / ``np.random`` / torch generator states are left as they were; the summed collision-check count
        is added to ``common.map_utils.cc_calls`` once.  Scope: run_type 0, one rank, a network sampler or one with
        ``sample_round`` (a plain callable draws from its own generator and cannot be split per run); the car, or the ant
        (env_id 'antmaze') with ``ant_dynamics`` "model" or "tape".

        The ant: the forest is an ``AntForestEngine``; ``ant_dynamics="host"`` is refused (the caller's simulator steps one
        candidate at a time on the host, so it bounds such a run and a forest buys nothing).  ``reset()`` is called ONCE and
        all runs share that reset's ``desired_goal``: equality with the sequential runs holds for an env whose ``reset``
        returns the same ``desired_goal`` every time -- a gym env that adds position noise per reset gives one draw for all
        runs here, a fresh one per run in the loop.  ``is_colliding_ant`` does not count its calls, so ant runs report
        ``cc_calls`` 0 and leave ``common.map_utils.cc_calls`` as it is, as ``plan()`` does."""
        from ._runs import Job, check_forest_scope, run_jobs
        check_forest_scope(self, "plan_runs")
        seeds = [int(s) for s in seeds]
        if not seeds:
            return []
        T = len(seeds) if concurrent is None else max(1, min(int(concurrent), len(seeds)))
        if tree_capacity is None:
            tree_capacity = _default_tree_capacity([self])
        eng = self._forest_engine(T, int(tree_capacity), T * self.batch)
        self.reset()                                        # env.reset(options) as before every sequential plan()
        if self.is_ant:
            eng._desired_arg = self._engine.env_goal.copy()  # the desired_goal this reset left: one for all runs
            eng.reset(self.start_node.state, self.goal_state)
        else:
            eng.reset(self.start_node.state, self.goal_state)
            eng.env_goal = np.asarray(self.env.goal, dtype=np.float64)
        if hasattr(self.sampler, "ensure_bound"):
            self.sampler.ensure_bound(T * self.batch)
        results = [None] * len(seeds)
        run_jobs(eng, [Job(self, s, (results, i)) for i, s in enumerate(seeds)], self.batch, self.ctx.device)
        return results


def _polish_report(r, actions):
    """``results["polish"]`` from one polish_plans result (None: the plan has no goal node and nothing was run)."""
    if r is None:
        n = 0 if actions is None else len(actions)
        return dict(status="no_goal", rows_in=n, rows_out=n, arrival_in=None, arrival_out=None, trace=None)
    return {k: r[k] for k in ("status", "rows_in", "rows_out", "arrival_in", "arrival_out", "trace")}


def _apply_polish(res, r, env_dt):
    """Write one polish_plans result into a ``results`` dict; a refused plan keeps its path and actions."""
    res["polish"] = _polish_report(r, res.get("actions"))
    if r["status"] == "ok":
        res["path"], res["actions"] = r["path"], r["actions"]
        res["path_time"] = len(r["path"]) * env_dt


def polish_runs(planners, results, **settings):
    """Polish every goal-reaching run of a ``plan_runs`` result (``planners``: that planner, ``results``: its list of run
    dicts) or of a ``plan_scenario_runs`` result (a list of planners and one list of run dicts per planner) in ONE
    ``polish_plans`` call: each run against its planner's maze, start and goal, with the same ``settings`` -- so a run ends
    as ``RRT_Planner.polish`` leaves the same plan.  The run dicts are updated in place (``path``, ``actions``,
    ``path_time``, ``polish``) and ``results`` is returned; a run without a goal node gets ``polish`` with status "no_goal"."""
    from ..polish import polish_plans
    single = isinstance(planners, RRT_Planner)
    pls = [planners] if single else list(planners)
    per = [results] if single else list(results)
    if len(per) != len(pls):
        raise ValueError(f"polish_runs: one list of runs per planner ({len(pls)}), got {len(per)}")
    for pl in pls:
        if pl.is_ant:
            raise NotImplementedError("polish_runs: the car (env_id='carmaze') only; the ant's plans are not polished")
        if pl.ctx is not pls[0].ctx:
            raise ValueError("polish_runs: all planners must share one ctx")
    jobs = []
    for pl, runs in zip(pls, per):
        for run in runs:
            if run.get("goal_reached") and run.get("actions") is not None:
                jobs.append((pl, run))
            else:
                run["polish"] = _polish_report(None, run.get("actions"))
    if jobs:
        mazes = pls[0].maze if len(pls) == 1 else [pl.maze for pl, _ in jobs]
        out = polish_plans(pls[0].ctx, mazes, np.stack([pl.start_node.state[:6] for pl, _ in jobs]),
                           np.stack([np.asarray(pl.env.goal, dtype=np.float64)[:2] for pl, _ in jobs]),
                           [run["actions"] for _, run in jobs], **settings)
        for (pl, run), r in zip(jobs, out):
            _apply_polish(run, r, pl.env_dt)
    return results


def _forest_like(cls, e, *args, **kw):
    """A forest engine ``cls(ctx, *args, **kw)`` that runs the round program of the single-tree engine ``e``: its own settings,
    and -- the ant -- its ``goal_radius`` as the value it has there (not re-derived from a factor)."""
    f = cls(e.ctx, *args, **e.round_settings(), **kw)
    if e.HIST:
        f.goal_radius = e.goal_radius
    f.ddpm = e.ddpm
    return f


def _default_tree_capacity(planners):
    """Node slots per run where the caller names none: the largest max_candidates + 1, at most the planners' ``capacity``."""
    return max(pl.capacity if pl.max_candidates is None else min(pl.capacity, int(pl.max_candidates) + 1) for pl in planners)


# ---------------------------------------------------------------------- a scenario set at once
def _plan_scene_runs(planners, seeds, concurrent, tree_capacity, check_planners, forest_cls, scene_goal):
    """The body of ``plan_scenario_runs`` and ``plan_ant_scenario_runs``: ``check_planners`` is the scope check with the
    settings list, ``forest_cls`` the scene forest, ``scene_goal(planner)`` the fourth entry of a scene after the planner's
    ``reset()``."""
    from ._runs import Job, run_jobs
    planners = list(planners)
    if not planners:
        return []
    if len(seeds) != len(planners):
        raise ValueError(f"seeds: one list per planner ({len(planners)}), got {len(seeds)}")
    check_planners(planners)
    seeds = [[int(s) for s in ss] for ss in seeds]
    results = [[None] * len(ss) for ss in seeds]
    jobs = [Job(planners[i], s, (results[i], k), (i,)) for i, ss in enumerate(seeds) for k, s in enumerate(ss)]
    if not jobs:
        return results
    p0 = planners[0]
    T = len(jobs) if concurrent is None else max(1, min(int(concurrent), len(jobs)))
    if tree_capacity is None:
        tree_capacity = _default_tree_capacity(planners)
    for pl in planners:
        pl.reset()                                           # env.reset(options) as before every sequential plan()
    scenes = [(pl.maze, pl.start_node.state, pl.goal_state, scene_goal(pl)) for pl in planners]
    eng = _forest_like(forest_cls, p0._engine, scenes, T, int(tree_capacity), batch=T * p0.batch)
    if hasattr(p0.sampler, "ensure_bound"):
        p0.sampler.ensure_bound(T * p0.batch)
    run_jobs(eng, jobs, p0.batch, p0.ctx.device)
    return results


def _scene_settings(pl):
    """What every planner of one scene forest must share (the forest runs one round program for all its trees)."""
    e = pl._engine
    return [("ctx", pl.ctx), ("sampler", pl.sampler), ("action_horizon", e.A), ("pred_horizon", e.P), ("local map size", e.lm_n),
            ("local map scale", float(e.lm_scale)), ("s_global", float(e.s_global)), ("k_steps", e.k_steps),
            ("norm", e.norm.tobytes()), ("emulate_sticky_done", e.sticky), ("early_exit", e.early_exit),
            ("prop_duration", tuple(e.schedule)), ("batch", pl.batch), ("solution", getattr(pl, "solution", "first")),
            ("bound_speed", getattr(pl, "bound_speed", None)), ("near_radius", getattr(pl, "near_radius", None)),
            ("near_speed", getattr(pl, "near_speed", None)), ("sparse_cell", getattr(pl, "sparse_cell", None)),
            ("sparse_headings", getattr(pl, "sparse_headings", None))]


def _check_scene_planners(planners):
    from ._runs import check_forest_scope
    for pl in planners:
        if pl.is_ant:
            raise NotImplementedError("plan_scenario_runs: the car (carmaze) only (antmaze planners: plan_ant_scenario_runs)")
        check_forest_scope(pl, "plan_scenario_runs")
    _check_shared_settings(planners, _scene_settings, "plan_scenario_runs")


def _check_shared_settings(planners, settings, who):
    """ValueError naming the first entry of ``settings(planner)`` in which a planner differs from planner 0."""
    ref = settings(planners[0])
    for i, pl in enumerate(planners[1:], 1):
        for (name, a), (_, b) in zip(ref, settings(pl)):
            same = a is b if name in ("ctx", "sampler") else a == b
            if not same:
                raise ValueError(f"{who}: planner {i} differs from planner 0 in {name}"
                                 + ("" if name in ("ctx", "sampler") else f" ({b!r} != {a!r})")
                                 + ("; all planners must share one object" if name in ("ctx", "sampler") else ""))


def plan_scenario_runs(planners, seeds, concurrent=None, tree_capacity=None):
    """Seeded runs of several scenarios (one ``RRT_Planner`` each: its own maze, start and goal) expanded together as one
    scene forest (forest.SceneForestEngine) on one GPU -- the whole benchmark loop of run_scenarios.py:203-250,336-343 as
    one stream of rounds.

    ``seeds``: one list per planner.  Returns one list per planner of ``plan_runs``-shaped dicts: run (i, s) is what
    ``random.seed(s); np.random.seed(s); torch.manual_seed(s); planners[i].reset(); planners[i].plan()`` leaves.  Each run
    draws through its own planner's ``draw_round`` (sampling bounds and goal bias are per maze), with its own random streams,
    its planner's ``time_budget`` and ``max_candidates``, and is rolled out against its planner's ``env.goal``.  Runs queue
    planner by planner; at most ``concurrent`` are in flight (default: all), and a finished tree takes the next queued run,
    whatever its scenario.  ``tree_capacity``: node slots per run (default: the largest max_candidates + 1, at most the
    planners' ``capacity``).  The caller's ``random`` / ``np.random`` / torch generator states are left as they were; the
    summed collision-check count is added to ``common.map_utils.cc_calls`` once.  All planners must share one ctx and one
    sampler object and agree on the round settings (ValueError names the first difference); the scope is ``plan_runs``'."""
    from ..forest import SceneForestEngine
    return _plan_scene_runs(planners, seeds, concurrent, tree_capacity, _check_scene_planners, SceneForestEngine,
                            lambda pl: np.asarray(pl.env.goal, dtype=np.float64))


# ---------------------------------------------------------------------- an antmaze scenario set at once
def _ant_scene_settings(pl):
    """What every planner of one ant scene forest must share (one round program, one goal_radius / ball_radius / s_global)."""
    e = pl._engine
    return [("ctx", pl.ctx), ("sampler", pl.sampler), ("edge_length", e.H), ("action_horizon", e.A), ("pred_horizon", e.P),
            ("local map size", e.lm_n), ("local map scale", float(e.lm_scale)), ("s_global", float(e.s_global)),
            ("k_steps", e.k_steps), ("norm", e.norm.tobytes()), ("early_exit", e.early_exit), ("batch", pl.batch),
            ("ant_dynamics", pl.ant_dynamics), ("ant_model", bytes(e.model)), ("ball_radius", float(e.ball_radius)),
            ("goal_radius", float(e.goal_radius))]


def _check_ant_scene_planners(planners):
    from ._runs import check_forest_scope
    for pl in planners:
        if not pl.is_ant:
            raise NotImplementedError("plan_ant_scenario_runs: antmaze planners only (the car: plan_scenario_runs)")
        check_forest_scope(pl, "plan_ant_scenario_runs")
    _check_shared_settings(planners, _ant_scene_settings, "plan_ant_scenario_runs")


def plan_ant_scenario_runs(planners, seeds, concurrent=None, tree_capacity=None):
    """``plan_scenario_runs`` for ``env_id='antmaze'`` planners: the seeded runs of several ant scenarios (one ``RRT_Planner``
    each: its own maze, start, goal and ``desired_goal``) expanded together as one ant scene forest
    (forest.AntSceneForestEngine) on one GPU -- the ant benchmark loop of run_scenarios.py:202-233,336-343 as one stream of
    rounds.

    ``seeds``: one list per planner.  Returns one list per planner of ``plan_runs``-shaped dicts: run (i, s) is what
    ``random.seed(s); np.random.seed(s); torch.manual_seed(s); planners[i].reset(); planners[i].plan()`` leaves.  Queueing,
    ``concurrent``, ``tree_capacity``, the per-run streams and budgets and the caller's generator states are
    ``plan_scenario_runs``'; ant runs report ``cc_calls`` 0 (``is_colliding_ant`` does not count its calls).  Each planner's
    ``reset()`` is called ONCE and scene i's ``desired_goal`` is what that reset left, for all of its runs: as in ``plan_runs``,
    equality with the sequential runs holds for an env whose ``reset`` returns the same ``desired_goal`` every time -- a gym env
    that adds position noise per reset gives one draw per scenario here, a fresh one per run in the loop.  Scope: run_type 0,
    one rank, ``ant_dynamics`` "model" or "tape", a network sampler or one with ``sample_round``.  All planners must share one
    ctx and one sampler object and agree on the round settings, the dynamics and its model, ``ball_radius`` and
    ``goal_radius`` (ValueError names the first difference)."""
    from ..forest import AntSceneForestEngine
    return _plan_scene_runs(planners, seeds, concurrent, tree_capacity, _check_ant_scene_planners, AntSceneForestEngine,
                            lambda pl: pl._engine.env_goal.copy())
