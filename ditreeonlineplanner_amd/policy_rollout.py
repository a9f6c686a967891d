"""Closed-loop policy roll-outs on the device: the validation episodes of rollout_manager.py:545-838 as one batch.

N = S scenes x E episodes of the car, each driven by the sampler alone -- local map -> conditioning vector -> sampler ->
``action_horizon`` env steps with the success and collision tests -- until it succeeds, collides or runs out of steps
(include/ditree.h "policy roll-outs": ``ditree_policy_begin`` / ``ditree_policy_chunk``).  ``PolicyRolloutEngine`` owns the
device arrays of a batch and loops over chunks; ``reference_trajectory`` rebuilds the reference's ``traj`` array from the
per-episode results on the host.  ``rollout_manager.rollout`` is the reference-shaped function on top.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import PolicyBatch, PolicyParams, check, lib
from .ops import Context, _dbl, _flt, local_axis


def reference_trajectory(rows, n_steps, terminated, final_state, max_episode_steps):
    """The reference's ``traj`` (rollout_manager.py:702,767-768,813-815) from per-episode results: ``rows`` (N, >= max n_steps, 8)
    with row t = [state, action] of step t, ``n_steps`` (N,), ``terminated`` (N,) bool (the episode ended on success or
    collision), ``final_state`` (N, 6) -> (N, max_episode_steps + 1, 8) float64.  With T = max n_steps, the loop's final
    ``curr_step``: a terminated episode repeats its last written row up to and including row T, an episode that ran out of
    steps gets [final state, 0, 0] at row T, later rows stay zero."""
    rows = np.asarray(rows, dtype=np.float64)
    n_steps = np.asarray(n_steps, dtype=np.int64)
    terminated = np.asarray(terminated, dtype=bool)
    final_state = np.asarray(final_state, dtype=np.float64)
    N, M = n_steps.shape[0], int(max_episode_steps)
    if rows.shape[0] != N or final_state.shape != (N, 6) or terminated.shape != (N,) or rows.shape[2:] != (8,):
        raise ValueError("rows (N, steps, 8), n_steps (N,), terminated (N,), final_state (N, 6)")
    if (n_steps < 0).any() or (n_steps > M).any() or (n_steps > rows.shape[1]).any():
        raise ValueError("n_steps must lie in [0, max_episode_steps] and within the rows given")
    if (terminated & (n_steps == 0)).any():
        raise ValueError("an episode cannot have ended before its first step")
    traj = np.zeros((N, M + 1, 8))
    T = int(n_steps.max()) if N else 0
    if (~terminated & (n_steps != T)).any():
        raise ValueError("episodes that did not end all stop at the loop's last step")
    for i in range(N):
        n = int(n_steps[i])
        traj[i, :n] = rows[i, :n]
        if terminated[i]:
            traj[i, n:T + 1] = rows[i, n - 1]
        else:
            traj[i, T, :6] = final_state[i]
    return traj


class PolicyRolloutEngine:
    """A batch of N car episodes on the device.

    ``scenes``: a list of ``(maze, goal_xy)`` -- ``goal_xy`` is the env's goal, the centre of the goal cell (car_env.py:225-226);
    ``starts`` (N, 6) float64 start states; ``scene_of`` (N,) the scene of every episode.  Exactly one of ``sampler`` (the
    ``DiffusionSampler`` facade, or any object with ``norm`` (16,), ``num_diffusion_iters`` and optionally ``ensure_bound(n)`` /
    ``ddpm_tables()`` whose network is bound to ``ctx``) and ``tape_fn(chunk, N, P) -> (N, P, 2)`` float64 actions.

    ``run(max_episode_steps)`` loops over chunks.  With a sampler the chunk's start noise is ``torch.randn((N, P, 2))`` on the
    device from torch's current generator -- for the WHOLE batch, as fm_policy.py:158 draws it, and only when a chunk actually
    runs, so the generator ends where the reference loop leaves it; the DDPM branch then draws the chunk's step noise
    ``(N, K, P, 2)`` the way ``RRT_Planner.plan`` does.  ``noise_fn(chunk) -> (noise[, step_noise])`` replaces the draw (tests).
    """

    def __init__(self, ctx: Context, scenes, starts, scene_of, sampler=None, tape_fn=None, action_horizon=8, pred_horizon=64,
                 local_map_size=20, local_map_scale=0.2, s_global=1.0):
        if (sampler is None) == (tape_fn is None):
            raise ValueError("PolicyRolloutEngine: exactly one of sampler / tape_fn")
        scenes = list(scenes)
        if not 1 <= len(scenes) <= _lib.MAX_SCENES:
            raise ValueError(f"a policy roll-out holds 1..{_lib.MAX_SCENES} scenes, got {len(scenes)}")
        self.ctx, self.sampler, self.tape_fn = ctx, sampler, tape_fn
        # the DDPM branch runs on the device from the scheduler's tables; any other scheduler object has no roll-out form
        self._tables = sampler.ddpm_tables() if hasattr(sampler, "ddpm_tables") else None
        if getattr(sampler, "policy", "flow_matching") == "diffusion" and self._tables is None:
            raise NotImplementedError("policy roll-out: policy='diffusion' needs a DDPM scheduler of the configuration the device "
                                      "loop implements (ddpm.ddpm_tables)")
        self.mazes = [np.asarray(m, dtype=np.float32) for m, _ in scenes]
        self.goals = np.stack([np.asarray(g, dtype=np.float64)[:2] for _, g in scenes])
        cells = sum(m.size for m in self.mazes)
        if cells > _lib.MAX_ATLAS_CELLS:
            raise ValueError(f"the scenes' mazes hold {cells} cells, more than the atlas's {_lib.MAX_ATLAS_CELLS}")
        starts = np.ascontiguousarray(starts, dtype=np.float64)
        scene_of = np.ascontiguousarray(scene_of, dtype=np.int32)
        if starts.ndim != 2 or starts.shape[1] != 6 or scene_of.shape != (starts.shape[0],) or starts.shape[0] < 1:
            raise ValueError("starts must be (N, 6) and scene_of (N,), N >= 1")
        if scene_of.min() < 0 or scene_of.max() >= len(scenes):
            raise ValueError(f"scene_of: every id must lie in [0, {len(scenes)})")
        self.N, self.A, self.P = starts.shape[0], int(action_horizon), int(pred_horizon)
        if not 1 <= self.A <= 64 or self.A > self.P:
            raise ValueError("need 1 <= action_horizon <= 64 and action_horizon <= pred_horizon")
        self.starts, self.scene_of = starts, scene_of
        self.lm_n, self.lm_scale, self.s_global = int(local_map_size), float(local_map_scale), float(s_global)
        self.axis = local_axis(self.lm_n, self.lm_scale)
        self._scene_host = (C.c_int32 * self.N)(*[int(v) for v in scene_of])
        self._scene_dev = torch.as_tensor(scene_of, device=ctx.device)
        self._max_steps = 0
        self.chunks_run = 0
        self.upload_scenes()

    # ------------------------------------------------------------------ device state
    def upload_scenes(self):
        self.ctx.upload_scenes(self.mazes, self.goals, owner=self)

    def _alloc(self, max_steps):
        dev, N = self.ctx.device, self.N
        f64, i32 = torch.float64, torch.int32
        self._max_steps = int(max_steps)
        self.state = torch.zeros(N, 6, dtype=f64, device=dev)
        self.rows = torch.zeros(N, self._max_steps, 8, dtype=f64, device=dev)
        self.n_steps = torch.zeros(N, dtype=i32, device=dev)
        self.success_step = torch.zeros(N, dtype=i32, device=dev)
        self.collided = torch.zeros(N, dtype=i32, device=dev)
        self.status = torch.zeros(N, dtype=i32, device=dev)
        self.best_dist = torch.zeros(N, dtype=f64, device=dev)
        self.last_action = torch.zeros(N, 2, dtype=f64, device=dev)
        self.has_prev = torch.zeros(N, dtype=torch.uint8, device=dev)
        self.goal_xy = torch.zeros(N, 2, dtype=f64, device=dev)
        self.idx = torch.zeros(N, dtype=i32, device=dev)
        self.desc = PolicyBatch(N, self.A, self._max_steps, self._scene_dev.data_ptr(), self._scene_host, *[
            t.data_ptr() for t in (self.state, self.rows, self.n_steps, self.success_step, self.collided, self.status,
                                   self.best_dist, self.last_action, self.has_prev, self.goal_xy, self.idx)])

    def begin(self, max_episode_steps):
        """Every episode back to its start state with fresh bookkeeping (rollout_manager.py:687-703)."""
        M = int(max_episode_steps)
        if M < 1:
            raise ValueError("max_episode_steps must be >= 1")
        if self.ctx.scenes_owner is not self:
            self.upload_scenes()
        if M != self._max_steps:
            self._alloc(M)
        if hasattr(self.sampler, "ensure_bound"):
            self.sampler.ensure_bound(self.N)
        self.state.copy_(torch.as_tensor(self.starts, device=self.ctx.device))
        self.rows.zero_()
        check(self.ctx._h, lib().ditree_policy_begin(self.ctx._h, C.byref(self.desc), self.ctx.stream), "policy_begin")
        self.step_limit, self.n_active, self.chunks_run = M, self.N, 0

    # ------------------------------------------------------------------ one chunk
    def _sampler_params(self, pp, keep, noise, step_noise):
        sm = self.sampler
        K = int(getattr(sm, "num_diffusion_iters", 1))
        tables = self._tables
        want = (self.N, self.P, 2)
        if tuple(noise.shape) != want or noise.dtype != torch.float32 or not noise.is_contiguous():
            raise ValueError(f"noise must be a contiguous float32 {want} tensor")
        pp.noise = noise.data_ptr()
        if tables is None:
            if hasattr(sm, "t0"):
                t0, dt = sm.t0, sm.dt
            else:
                from .common.fm_utils import get_timesteps
                t0, dt = (t.numpy().copy() for t in get_timesteps("exp", K, 4.0))
            a, pp.t0 = _flt(t0)
            b, pp.dt = _flt(dt)
            pp.K = len(a)
            keep += [a, b]
        else:
            a, pp.t0 = _flt(tables[0])
            b, pp.ddpm_coef = _flt(tables[1])
            pp.K = len(a)
            keep += [a, b]
            want = (self.N, pp.K, self.P, 2)
            if step_noise is None or tuple(step_noise.shape) != want or step_noise.dtype != torch.float32 or not step_noise.is_contiguous():
                raise ValueError(f"the DDPM branch needs step_noise, a contiguous float32 {want} tensor")
            pp.step_noise = step_noise.data_ptr()
        for name, arr in (("norm", sm.norm), ("axis", self.axis)):
            a, ptr = _dbl(arr)
            keep.append(a)
            setattr(pp, name, ptr)
        # fm_policy.py:125-143: the goal offset is divided by the sampler's local_map_size
        pp.lm_n, pp.lm_size, pp.s_global = self.lm_n, float(self.lm_n), self.s_global

    def chunk(self, noise=None, step_noise=None, tape=None):
        """One chunk for the running episodes -> how many are still running.  ``noise`` (N, P, 2) f32 [, ``step_noise``
        (N, K, P, 2) f32] with a sampler, ``tape`` (N, P, 2) f64 otherwise [device tensors]."""
        if self.ctx.scenes_owner is not self:             # another engine uploaded its scene table since begin()
            self.upload_scenes()
        pp = PolicyParams()
        pp.step_limit, pp.P = self.step_limit, self.P
        keep = [noise, step_noise, tape]
        if self.sampler is not None:
            self._sampler_params(pp, keep, noise, step_noise)
        else:
            if tape is None or tuple(tape.shape) != (self.N, self.P, 2) or tape.dtype != torch.float64 or not tape.is_contiguous():
                raise ValueError(f"tape must be a contiguous float64 ({self.N}, {self.P}, 2) tensor")
            pp.tape = tape.data_ptr()
        n = C.c_int32(0)
        check(self.ctx._h, lib().ditree_policy_chunk(self.ctx._h, C.byref(self.desc), C.byref(pp), C.byref(n), self.ctx.stream),
              "policy_chunk")
        del keep
        self.n_active = int(n.value)
        self.chunks_run += 1
        return self.n_active

    def run(self, max_episode_steps, noise_fn=None):
        """rollout_manager.py:706-807: chunks until every episode has ended or ``max_episode_steps`` steps have run.
        -> ``results()``."""
        self.begin(max_episode_steps)
        dev = self.ctx.device
        steps = 0
        while steps < self.step_limit and self.n_active > 0:
            c = self.chunks_run
            if self.sampler is None:
                tape = torch.as_tensor(np.ascontiguousarray(self.tape_fn(c, self.N, self.P), dtype=np.float64), device=dev)
                self.chunk(tape=tape.contiguous())
            else:
                if noise_fn is not None:
                    got = noise_fn(c)
                    noise, z = got if isinstance(got, tuple) else (got, None)
                else:
                    noise = torch.randn((self.N, self.P, 2), device=dev)                       # fm_policy.py:158
                    z = None if self._tables is None else torch.randn((self.N, len(self._tables[0]), self.P, 2), device=dev)
                self.chunk(noise=noise, step_noise=z)
            steps += self.A
        if self.sampler is not None:
            self.ctx.check_range()
        return self.results()

    # ------------------------------------------------------------------ results
    def results(self):
        """Per-episode results on the host: ``n_steps``, ``success_step`` (-1 = never), ``collided`` (bool), ``status``
        (_lib.EP_* | ST_FLAG_GOAL_AT_COLLISION), ``best_dist``, ``rows`` (N, max_episode_steps, 8), ``final_state`` (N, 6)."""
        st = self.status.cpu().numpy()
        return dict(n_steps=self.n_steps.cpu().numpy(), success_step=self.success_step.cpu().numpy(),
                    collided=self.collided.cpu().numpy().astype(bool), status=st, best_dist=self.best_dist.cpu().numpy(),
                    rows=self.rows.cpu().numpy(), final_state=self.state.cpu().numpy())

    def trajectory(self, res=None):
        """The reference-shaped ``traj`` (N, max_episode_steps + 1, 8) of the last run."""
        r = self.results() if res is None else res
        code = r["status"] & 0xFF
        return reference_trajectory(r["rows"], r["n_steps"], (code == _lib.EP_SUCCESS) | (code == _lib.EP_COLLIDED),
                                    r["final_state"], self._max_steps)
