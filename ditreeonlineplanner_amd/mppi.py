"""`MPPI.mppi.MPPI` -- the controller `run_scenarios_with_lidar_MPPI.py:10,339-449` constructs as
`MPPI(maze_data, T, K, nx, nu)` and drives through `.reset / .step / .is_done / .set_ref_path / .reference_path /
.update_maze / .env` (`:392-394,402,410,414,417,422,442,447-449`).

The reference repository does NOT contain this module ("no oracle exists at all"), so there are no
semantics to be faithful to: the controller below is the build's own -- information-theoretic MPPI (Williams et al. 2017)
on the reference's car dynamics, two-ball collision test and goal radius, every controller step on the GPU
(`ditree_mppi_step`: K x T rollouts with on-device noise, soft-min weights by wavefront reductions, weighted control update,
one executed env step).  The cost function is stated in include/ditree.h and DESIGN.md; **parity with the reference is
unpinned**, the kernels are held to the build's numpy restatement (oracle/mppi.py) and to invariants
(tests/test_gpu_mppi.py).  There is no CPU path.

`step(state) -> (next_state, action, done)` keeps the driver's contract: `done is None` when the executed step collides
with the KNOWN maze (the state does not advance, the nominal controls restart from rest and the next call draws fresh
noise: the driver retries up to ALLOWED_TRIALS times), `True` inside the goal radius, else `False`.

`follow(...)` runs the driver's whole control loop (`:417-452`: steps, collision retries, the scan and known-maze update every
scan_time) as one launch of the mission kernel (`ditree_mppi_missions`), `follow_fleet(...)` the missions of M controllers at
once; both leave every controller bit for bit where the same `step()` / `update_maze()` calls leave it (car, K <= 256).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .car_env import CarEnv
from .ops import default_context


class MPPI:
    def __new__(cls, maze_data=None, T=16, K=1024, nx=6, nu=2, *a, **kw):
        # MPPI(maze_data, T, K, nx=29, nu=8): BASELINE config 5's antmaze variant -- the same controller on the higher-DoF slot
        if cls is MPPI and (nx, nu) == (29, 8):
            return super().__new__(AntMPPI)
        return super().__new__(cls)

    NX, NU = 6, 2                                    # state / action widths
    N_RESULT, ACTION_AT, STATE_AT = 16, 0, 8         # the result block (include/ditree.h): its length, where action and state stand
    ENTRY = "ditree_mppi_step"

    def __init__(self, maze_data=None, T=16, K=1024, nx=6, nu=2, lam=1.0, sigma=(3.0, 0.6), w_track=20.0, w_progress=0.5,
                 w_collision=1.0e3, w_goal=50.0, window_back=8, window_fwd=56, seed=0, lanes=0, ctx=None, env=None,
                 rank=None, world_size=None, process_group=None, **kw):
        if maze_data is None:
            raise ValueError("MPPI needs the known maze (maze_data)")
        if nx != 6 or nu != 2:
            raise NotImplementedError("the controller drives the car model: nx = 6 (x, y, psi, v, D, delta), nu = 2 (dD, ddelta)")
        self._set_up(maze_data, T, K, ctx, rank, world_size, process_group)
        self.env = env if env is not None else CarEnv(maze_map=np.asarray(maze_data), collision_checking=False, ctx=self.ctx)
        self.params = _lib.MppiParams(self.T, self.K_local, float(lam), (C.c_double * 2)(float(sigma[0]), float(sigma[1])),
                                      float(w_track), float(w_progress), float(w_collision), float(w_goal), int(seed),
                                      int(window_back), int(window_fwd), int(lanes), int(self.k_lo))
        self.ctx.upload_maze(self.maze, owner=self)

    def _set_up(self, maze_data, T, K, ctx, rank, world_size, process_group):
        """What every model's controller holds: sizes, its shard of the rollouts, the context, the device buffers."""
        if not (1 <= int(T) <= 64) or int(K) < 1:
            raise ValueError("1 <= T <= 64, K >= 1")
        self.T, self.K, self.nx, self.nu = int(T), int(K), self.NX, self.NU
        # K is the GLOBAL number of rollouts; with world_size > 1 (one process per GPU) every rank runs a contiguous block
        from .engine import default_shard
        d_rank, d_world, d_pg = default_shard()
        self.world = int(d_world if world_size is None else world_size)
        self.rank = int((d_rank if self.world == d_world else 0) if rank is None else rank)
        self.pg = d_pg if process_group is None else process_group
        per = (self.K + self.world - 1) // self.world
        self.k_lo = min(self.rank * per, self.K)
        self.K_local = max(min(self.k_lo + per, self.K) - self.k_lo, 0)
        if self.K_local < 1:
            raise ValueError("fewer rollouts than ranks")
        self.ctx = ctx or default_context()
        self.maze = np.float32(maze_data)
        dev = self.ctx.device
        f64 = torch.float64
        self._state = torch.zeros(self.NX, dtype=f64, device=dev)
        self._U = torch.zeros(self.T, self.NU, dtype=f64, device=dev)
        self._costs = torch.zeros(self.K_local, dtype=f64, device=dev)
        self._flags = torch.zeros(self.K_local, dtype=torch.int32, device=dev)
        self._result = torch.zeros(self.N_RESULT, dtype=f64, device=dev)
        self._state_host = None            # the state the device holds (skip the upload when the driver hands it back)
        self._sums = torch.zeros(3 + self.NU * self.T, dtype=f64, device=dev)
        self._path = None
        self.reference_path = None
        self.goal_state = None
        self.counter = 0                   # one noise stream per step() call (also the retried ones)
        self.last = {}

    # ------------------------------------------------------------------ the surface the driver uses
    def reset(self, start_state=None, goal_state=None):
        if start_state is not None:
            start_state = np.asarray(start_state, dtype=np.float64)
            self.goal_state = np.asarray(goal_state, dtype=np.float64)
            opts = {"reset_cell": self.env.cell_xy_to_rowcol(start_state[:2]), "reset_deg": np.rad2deg(start_state[2]),
                    "goal_cell": self.env.cell_xy_to_rowcol(self.goal_state[:2])}
            self.env.reset(options=opts)
            self.env.set_state(start_state.copy())
        self._U.zero_()
        self.counter = 0

    def update_maze(self, new_maze):
        self.maze = np.float32(new_maze)
        self.env.maze_map = new_maze
        self.ctx.upload_maze(self.maze, owner=self)

    def set_ref_path(self, path):
        """The plan to track: (P, >= 2) states; more than 4096 points are thinned uniformly (the kernel stages the path in LDS)."""
        path = np.asarray(path, dtype=np.float64)
        if path.ndim != 2 or path.shape[1] < 2 or len(path) < 1:
            raise ValueError("reference path must be (P, >= 2)")
        self.reference_path = path
        xy = np.ascontiguousarray(path[:, :2])
        if len(xy) > 4096:
            xy = np.ascontiguousarray(xy[np.round(np.linspace(0, len(xy) - 1, 4096)).astype(int)])
        self._path = torch.as_tensor(xy, device=self.ctx.device)

    def is_done(self, state):
        return self.env.is_done(state)

    def step(self, state, noise=None):
        """One controller step from `state` (NX,): -> (next_state (NX,) f64, action (NU,) f64, done in {False, True, None})."""
        if self._path is None:
            raise _lib.DitreeError("MPPI.step: set_ref_path(path) first")
        if self.ctx.maze_owner is not self:
            self.ctx.upload_maze(self.maze, owner=self)
        state = np.asarray(state, dtype=np.float64)
        if self._state_host is None or not np.array_equal(state, self._state_host):
            self._state.copy_(torch.as_tensor(state))
        self.controller_step(noise=noise)
        res = self._result.cpu().numpy()            # the one D2H (and sync) of a step: action, status, statistics, new state
        self.counter += 1
        status = int(res[2])
        self.last = {"beta": float(res[3]), "eta": float(res[4]), "nearest_path_index": int(res[5]),
                     "collided_rollouts": int(res[6]), "effective_samples": float(res[7])}
        nxt = res[self.STATE_AT:self.STATE_AT + self.NX].copy()
        self._state_host = nxt.copy()
        action = res[self.ACTION_AT:self.ACTION_AT + self.NU].copy()
        if status == 2:
            return nxt, action, None
        self.env.set_state(nxt.copy())
        if status == 1:
            self.env.done = True
        return nxt, action, status == 1

    def controller_step(self, noise=None, weights=None):
        """One controller step on the device state / controls.  One rank: a single C-ABI call.  Sharded: rollouts + local
        minimum, all-reduce(MIN) of beta, weighted sums, all-reduce(SUM) of 3 + NU T doubles, then the (replicated) update and
        executed step -- every rank ends with the same state and controls."""
        if self.world <= 1:
            return self.launch(_lib.MPPI_ALL, noise=noise, weights=weights)
        import torch.distributed as dist
        gloo = dist.get_backend(self.pg) == "gloo"

        def allreduce(t, op):
            if gloo:
                h = t.cpu()
                dist.all_reduce(h, op=op, group=self.pg)
                t.copy_(h)
            else:
                dist.all_reduce(t, op=op, group=self.pg)
        self.launch(_lib.MPPI_ROLLOUTS | _lib.MPPI_MIN, noise=noise)
        allreduce(self._result[3:4], dist.ReduceOp.MIN)
        self.launch(_lib.MPPI_SUMS, noise=noise, weights=weights)
        allreduce(self._sums, dist.ReduceOp.SUM)
        self.launch(_lib.MPPI_APPLY | _lib.MPPI_EXECUTE, noise=noise, weights=weights)

    # ------------------------------------------------------------------ a whole mission in one launch
    def follow(self, state, maze_data, maze_data_with_obstacle, scanned_maze, max_steps, allowed_trials=1,
               action_time_count=0.0, trials=0, noise=None):
        """The driver's control loop `run_scenarios_with_lidar_MPPI.py:417-452` from `state`, on the device (ditree_mppi_missions):
        up to `max_steps` controller calls, each `step()` + the driver's bookkeeping, with a lidar scan of
        `maze_data_with_obstacle` and the known-maze update whenever the accumulated step time exceeds the lidar's scan_time.
        Stops at the goal radius (MEV_GOAL), after `allowed_trials` collided executed steps in a row (MEV_TRIALS) or when the
        calls run out (MEV_STEPS_DONE).  `maze_data` (which must be the controller's known maze) and `scanned_maze` are
        updated in place; the controller, its env and its device state end exactly as after the same `step()` /
        `update_maze()` calls.  -> (state, executed_states (n, 6), executed_actions (n, 2), event, info); `info` carries
        `action_time_count` and `trials`, to be passed back in to resume."""
        if noise is not None:
            raise ValueError("MPPI.follow: a noise tape has no mission form (the mission kernel regenerates the counter noise)")
        return follow_fleet([self], [state], [maze_data], [maze_data_with_obstacle], [scanned_maze], max_steps,
                            allowed_trials=allowed_trials, action_time_counts=action_time_count, trials=trials)[0]

    # ------------------------------------------------------------------ one C-ABI call (stages: _lib.MPPI_*)
    def launch(self, stages, noise=None, weights=None):
        goal = (C.c_double * 2)(float(self.env.goal[0]), float(self.env.goal[1]))
        _lib.check(self.ctx._h, getattr(_lib.lib(), self.ENTRY)(
            self.ctx._h, C.byref(self.params), self._state.data_ptr(), self._U.data_ptr(), self._path.data_ptr(),
            int(self._path.shape[0]), goal, None if noise is None else noise.data_ptr(), self.counter, int(stages),
            self._costs.data_ptr(), None if weights is None else weights.data_ptr(), self._flags.data_ptr(),
            self._sums.data_ptr(), self._result.data_ptr(), self.ctx.stream), self.ENTRY[len("ditree_"):])


MEV_STEPS_DONE, MEV_GOAL, MEV_TRIALS = 0, 1, 2     # include/ditree.h DITREE_MEV_*
MISSION_MAX_K = 256                                # one rollout per thread of a mission's work-group
MISSION_MAX_STEPS = 2048                           # include/ditree.h DITREE_MPPI_MISSION_MAX_STEPS: controller calls per launch


def fleet_settings(c):
    """What the controllers of one fleet share (ditree_mppi_missions takes ONE parameter block and ONE maze shape)."""
    p = c.params
    return (("T", int(c.T)), ("K", int(c.K)), ("lam", float(p.lam)), ("sigma", (float(p.sigma[0]), float(p.sigma[1]))),
            ("w_track", float(p.w_track)), ("w_progress", float(p.w_progress)), ("w_collision", float(p.w_collision)),
            ("w_goal", float(p.w_goal)), ("window_back", int(p.window_back)), ("window_fwd", int(p.window_fwd)),
            ("maze shape", tuple(np.shape(c.maze))))


def check_fleet(controllers):
    """ValueError naming the first setting in which a controller differs from the first one."""
    if len(controllers) < 1:
        raise ValueError("follow_fleet: no controllers")
    first = fleet_settings(controllers[0])
    for i, c in enumerate(controllers[1:], start=1):
        for (name, v0), (_, v) in zip(first, fleet_settings(c)):
            if v != v0:
                raise ValueError(f"follow_fleet: controller {i} differs from controller 0 in {name}: {v} != {v0}")


def _check_mission_form(c):
    if isinstance(c, AntMPPI):
        raise NotImplementedError("AntMPPI has no mission form: the reference has no ant mission driver and the ant slot has no "
                                  "lidar; drive it with step()")
    if c.world > 1:
        raise ValueError("a sharded controller (world_size > 1) has no mission form; drive it with step()")
    if c.K > MISSION_MAX_K:
        raise ValueError(f"K = {c.K} > {MISSION_MAX_K}: the mission kernel runs one rollout per thread of one work-group; "
                         "larger controllers keep step()")
    if c._path is None:
        raise _lib.DitreeError("MPPI.follow: set_ref_path(path) first")


def _per_mission(v, M, dtype, name):
    a = np.asarray(v, dtype=dtype)
    if a.ndim == 0:
        return np.full(M, a, dtype=dtype)
    if a.shape != (M,):
        raise ValueError(f"follow_fleet: {name} must be a scalar or one value per controller")
    return a.copy()


def follow_fleet(controllers, states, mazes, mazes_with_obstacle, scanned_mazes, max_steps, allowed_trials=1,
                 action_time_counts=0.0, trials=0):
    """`MPPI.follow` for M controllers as ONE launch per `MISSION_MAX_STEPS` controller calls (ditree_mppi_missions: one
    work-group per mission, no mission waits for another).  The controllers share T, K, the cost weights, sigma, the windows,
    the maze shape and the context (ValueError naming the first difference); each keeps its own seed, counter, nominal controls,
    reference path, goal and mazes and ends in the state its own `follow` would leave.  `states`, the three maze lists: one entry
    per controller (the known and scanned mazes are updated in place); `max_steps`, `allowed_trials`, `action_time_counts`,
    `trials`: a scalar or one value per controller.  -> [(state, executed_states, executed_actions, event, info)] per controller."""
    controllers = list(controllers)
    for c in controllers:
        _check_mission_form(c)
    check_fleet(controllers)
    M = len(controllers)
    ctx = controllers[0].ctx
    for i, c in enumerate(controllers):
        if c.ctx is not ctx:
            raise ValueError(f"follow_fleet: controller {i} differs from controller 0 in ctx")
    if not (len(states) == len(mazes) == len(mazes_with_obstacle) == len(scanned_mazes) == M):
        raise ValueError("follow_fleet: one state and one known / true / scanned maze per controller")
    shape = tuple(np.shape(controllers[0].maze))
    for i, c in enumerate(controllers):
        for nm, mz in (("maze_data", mazes[i]), ("maze_data_with_obstacle", mazes_with_obstacle[i]), ("scanned_maze", scanned_mazes[i])):
            if tuple(np.shape(mz)) != shape:
                raise ValueError(f"follow_fleet: {nm} of controller {i} has shape {np.shape(mz)}, the controller's maze {shape}")
        if not np.array_equal(np.float32(mazes[i]), c.maze):
            raise ValueError(f"follow_fleet: maze_data of controller {i} is not the controller's known maze (update_maze first)")
    remaining = _per_mission(max_steps, M, np.int64, "max_steps")
    allowed = _per_mission(allowed_trials, M, np.int32, "allowed_trials")
    t_acc_h = _per_mission(action_time_counts, M, np.float64, "action_time_counts")
    trials_h = _per_mission(trials, M, np.int32, "trials")
    if (remaining < 0).any():
        raise ValueError("follow_fleet: max_steps < 0")

    dev = ctx.device
    T = controllers[0].T
    rows, cols = shape
    i32, f64 = torch.int32, torch.float64

    def up(a):
        return torch.as_tensor(np.ascontiguousarray(a), device=dev)

    # the state every controller's device copy holds (uploaded only when the driver hands in another one, as step())
    for c, st in zip(controllers, states):
        st = np.asarray(st, dtype=np.float64)
        if c._state_host is None or not np.array_equal(st, c._state_host):
            c._state.copy_(torch.as_tensor(st))
    single = M == 1
    state_t = controllers[0]._state.view(1, 6) if single else torch.stack([c._state for c in controllers])
    U_t = controllers[0]._U.view(1, T, 2) if single else torch.stack([c._U for c in controllers])
    path_t = controllers[0]._path if single else torch.cat([c._path for c in controllers])
    plen = np.array([int(c._path.shape[0]) for c in controllers], dtype=np.int32)
    poff = (np.cumsum(plen) - plen).astype(np.int32)
    seed_t = up(np.array([int(c.params.seed) for c in controllers], dtype=np.uint64).view(np.int64))
    goal_t = up(np.array([[float(c.env.goal[0]), float(c.env.goal[1])] for c in controllers], dtype=np.float64))
    dt_t = up(np.array([float(c.env.dt) for c in controllers], dtype=np.float64))
    scan_t = up(np.array([float(c.env.lidar2dsim.scan_time) for c in controllers], dtype=np.float64))
    known_t = up(np.stack([np.asarray(m, dtype=np.float32) for m in mazes]))
    truth_t = up(np.stack([np.asarray(m, dtype=np.float32) for m in mazes_with_obstacle]))
    scanned_t = up(np.stack([np.asarray(m, dtype=np.float32) for m in scanned_mazes]))
    poff_t, plen_t, allowed_t = up(poff), up(plen), up(allowed)
    t_acc_t, trials_t = up(t_acc_h), up(trials_h)
    result_t = torch.zeros(M, 16, dtype=f64, device=dev)
    last_owner = controllers[-1]                    # the ctx's own maze copy follows the last mission's known maze
    if tuple(ctx.maze_shape or ()) != shape:
        ctx.upload_maze(last_owner.maze, owner=last_owner)

    active = np.ones(M, dtype=bool)
    events = np.full(M, MEV_STEPS_DONE, dtype=np.int64)
    calls, scans = np.zeros(M, dtype=np.int64), np.zeros(M, dtype=np.int64)
    ex_s = [[] for _ in range(M)]
    ex_a = [[] for _ in range(M)]
    last = [None] * M
    first = True
    while first or (active & (remaining > 0)).any():
        first = False
        chunk = np.where(active, np.minimum(remaining, MISSION_MAX_STEPS), 0).astype(np.int32)
        trace = int(chunk.max())
        chunk_t = up(chunk)
        counter_t = up(np.array([int(c.counter) + int(n) for c, n in zip(controllers, calls)], dtype=np.uint64).view(np.int64))
        es = torch.empty(M, max(trace, 1), 6, dtype=f64, device=dev)
        ea = torch.empty(M, max(trace, 1), 2, dtype=f64, device=dev)
        _lib.check(ctx._h, _lib.lib().ditree_mppi_missions(
            ctx._h, C.byref(controllers[0].params), M, seed_t.data_ptr(), counter_t.data_ptr(), state_t.data_ptr(), U_t.data_ptr(),
            path_t.data_ptr(), poff_t.data_ptr(), plen_t.data_ptr(), int(plen.max()), goal_t.data_ptr(), known_t.data_ptr(),
            truth_t.data_ptr(), scanned_t.data_ptr(), rows, cols, chunk_t.data_ptr(), trace, allowed_t.data_ptr(), dt_t.data_ptr(),
            scan_t.data_ptr(), t_acc_t.data_ptr(), trials_t.data_ptr(), es.data_ptr(), ea.data_ptr(), result_t.data_ptr(), M - 1,
            ctx.stream), "mppi_missions")
        ctx.maze_owner = last_owner
        res = result_t.cpu().numpy()
        if (res[:, 0] < 0).any():
            raise _lib.DitreeError(f"mppi_missions: mission {int(np.argmax(res[:, 0] < 0))} was refused (path length or step bound)")
        n_exec = res[:, 2].astype(np.int64)
        nmax = int(n_exec[active].max()) if active.any() else 0
        es_h = es[:, :nmax].cpu().numpy() if nmax else None
        ea_h = ea[:, :nmax].cpu().numpy() if nmax else None
        for m in np.flatnonzero(active):
            events[m] = int(res[m, 0])
            calls[m] += int(res[m, 1])
            scans[m] += int(res[m, 3])
            remaining[m] -= int(chunk[m])
            if n_exec[m]:
                ex_s[m].append(es_h[m, :n_exec[m]].copy())
                ex_a[m].append(ea_h[m, :n_exec[m]].copy())
            if res[m, 1] > 0:
                last[m] = {"beta": float(res[m, 4]), "eta": float(res[m, 5]), "nearest_path_index": int(res[m, 6]),
                           "collided_rollouts": int(res[m, 7]), "effective_samples": float(res[m, 8])}
            if events[m] != MEV_STEPS_DONE:
                active[m] = False

    state_h = state_t.cpu().numpy()
    t_acc_h, trials_h = t_acc_t.cpu().numpy(), trials_t.cpu().numpy()
    known_h = scanned_h = None
    if scans.any():
        known_h, scanned_h = known_t.cpu().numpy(), scanned_t.cpu().numpy()
    out = []
    for m, c in enumerate(controllers):
        if not single:
            c._state.copy_(state_t[m])
            c._U.copy_(U_t[m])
        final = state_h[m].copy()
        c._state_host = final.copy()
        c.counter += int(calls[m])
        if last[m] is not None:
            c.last = last[m]
        states_m = np.concatenate(ex_s[m]) if ex_s[m] else np.zeros((0, 6))
        actions_m = np.concatenate(ex_a[m]) if ex_a[m] else np.zeros((0, 2))
        if len(states_m):
            c.env.set_state(final.copy())
            if events[m] == MEV_GOAL:
                c.env.done = True
        if scans[m]:                                # what update_maze(maze_data) leaves after the last scan
            mazes[m][...] = known_h[m]
            scanned_mazes[m][...] = scanned_h[m]
            c.maze = np.float32(mazes[m])
            c.env.maze_map = mazes[m]
        info = {"action_time_count": float(t_acc_h[m]), "trials": int(trials_h[m]), "controller_calls": int(calls[m]),
                "scans": int(scans[m])}
        out.append((final, states_m, actions_m, int(events[m]), info))
    return out


class _AntGoalEnv:
    """What the driver reads from ``mppi.env`` for the ant: the goal and the state (no physics here: the rollouts and the
    executed step run the build's stand-in model on the device)."""

    def __init__(self, maze, s_global):
        self.maze_map, self.s_global = np.asarray(maze), float(s_global)
        self.goal = np.zeros(2)
        self.state = np.zeros(29)
        self.done = False

    def set_state(self, state):
        self.state = np.asarray(state, dtype=np.float64)

    def is_done(self, state):
        d = np.asarray(state, dtype=np.float64)[:2] - self.goal
        return bool(np.linalg.norm(d) < 0.45 * self.s_global)            # planners/base_planner.py:296-297


class AntMPPI(MPPI):
    """`MPPI(maze_data, T, K, nx=29, nu=8)`: BASELINE config 5 as written ("MPPI antmaze, 65 536 rollouts") -- the build's MPPI
    controller (above) on the higher-DoF rollout slot: every rollout step is one env step of the build's STAND-IN crawler model
    (include/ditree.h ditree_ant_model; NOT MuJoCo), followed by the reference's ant collision test (common/map_utils.py:
    126-219) and goal radius (planners/base_planner.py:296-297).  The reference has neither an MPPI module nor the ant's
    physics in its repository: PARITY UNPINNED BY CONSTRUCTION; held to oracle/mppi.py (tests/test_gpu_mppi.py)."""

    NX, NU = 29, 8
    N_RESULT, ACTION_AT, STATE_AT = 64, 16, 24
    ENTRY = "ditree_mppi_step_ant"

    def __init__(self, maze_data=None, T=16, K=1024, nx=29, nu=8, lam=1.0, sigma=0.5, w_track=2.0, w_progress=0.5, w_collision=1.0e3,
                 w_goal=50.0, window_back=8, window_fwd=56, seed=0, ctx=None, s_global=4.0, ball_radius=1.2, model=None,
                 rank=None, world_size=None, process_group=None, **kw):
        if maze_data is None:
            raise ValueError("MPPI needs the known maze (maze_data)")
        if (nx, nu) != (29, 8):
            raise NotImplementedError("AntMPPI: nx = 29, nu = 8")
        self._set_up(maze_data, T, K, ctx, rank, world_size, process_group)
        self.s_global = float(s_global)
        self.env = _AntGoalEnv(maze_data, s_global)
        sg = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (8,))
        self.params = _lib.MppiAntParams(self.T, self.K_local, float(lam), (C.c_double * 8)(*[float(v) for v in sg]), float(w_track),
                                         float(w_progress), float(w_collision), float(w_goal), int(seed), int(window_back),
                                         int(window_fwd), int(self.k_lo), 0.45 * float(s_global), float(ball_radius), float(s_global),
                                         _lib.AntModel.default() if model is None else model)
        self.ctx.upload_maze(self.maze, owner=self)

    def reset(self, start_state=None, goal_state=None, desired_goal=None):
        if start_state is not None:
            self.goal_state = np.asarray(goal_state, dtype=np.float64)
            self.env.goal = np.asarray(self.goal_state[:2] if desired_goal is None else desired_goal, dtype=np.float64)[:2].copy()
            self.env.set_state(np.asarray(start_state, dtype=np.float64).copy())
            self.env.done = False
        self._U.zero_()
        self.counter = 0

    def update_maze(self, new_maze):
        self.maze = np.float32(new_maze)
        self.env.maze_map = np.asarray(new_maze)
        self.ctx.upload_maze(self.maze, owner=self)

    def follow(self, *a, **kw):
        raise NotImplementedError("AntMPPI has no mission form: the reference has no ant mission driver and the ant slot has no "
                                  "lidar; drive it with step()")
