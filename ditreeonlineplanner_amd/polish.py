"""Plan polishing: shorten a found plan's action tape by sampled roll-outs on the device (include/ditree.h "plan polishing",
``ditree_polish_plans``).

A plan is a start state, a goal, a maze and an action tape.  The tape is replayed; then, ``iterations`` times, ``rollouts``
perturbed copies of the incumbent tape are rolled out and the one that reaches the goal radius earliest -- if it does so strictly
earlier than the incumbent -- becomes the incumbent.  The result is a rolled, collision-free, arriving tape with no more rows
and no later arrival than the plan that went in.  The rule is this build's own (the reference has no such step).

The defaults below are settings picked from the sweep of profiles/polish_probe.py (profiles/polish_probe.json), not tuned truths.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import Polish, check, lib

DEFAULTS = dict(rollouts=4096, iterations=24, sigma=(2.0, 0.2), hold=8, seed=0)
STATUS_NAMES = {_lib.POLISH_OK: "ok", _lib.POLISH_NO_ARRIVAL: "no_arrival", _lib.POLISH_COLLIDES: "collides",
                _lib.POLISH_START_IN_GOAL: "start_in_goal", _lib.POLISH_NOT_F32: "not_f32"}
TRACE_COLUMNS = ("winner", "tau", "accepted", "rows", "arrival", "arriving")


def check_settings(rollouts, iterations, sigma, hold):
    """The setting rules of ditree_polish_plans, by name and without a device -> (K, N, (s0, s1), hold)."""
    K, N, hold = int(rollouts), int(iterations), int(hold)
    if K < 64 or K % 64 != 0:
        raise ValueError(f"polish: rollouts = {rollouts} is not a positive multiple of 64")
    if N < 0:
        raise ValueError(f"polish: iterations = {iterations} < 0")
    if hold < 1:
        raise ValueError(f"polish: hold = {hold} < 1")
    s = tuple(float(v) for v in np.asarray(sigma, dtype=np.float64).reshape(-1))
    if len(s) != 2 or not all(math.isfinite(v) and v >= 0.0 for v in s):
        raise ValueError(f"polish: sigma = {sigma!r} must be two finite values >= 0")
    return K, N, s, hold


def polish_plans(ctx, mazes, starts, goals, tapes, *, rollouts=DEFAULTS["rollouts"], iterations=DEFAULTS["iterations"],
                 sigma=DEFAULTS["sigma"], hold=DEFAULTS["hold"], seed=DEFAULTS["seed"], noise=None, first_row=None):
    """Polish P plans in one call.

    ``mazes``: one 2-D map for all plans, or a list of P maps (then they travel as a scene table: ditree_upload_scenes);
    ``starts`` (P, 6) float64 start states; ``goals`` (P, 2) the env's goals; ``tapes`` a list of P (T_i, 2) action arrays
    (float32, as ``plan()`` returns them; anything else is rounded to float32 first).  ``noise`` (N, K, NB, 2) float64 with
    NB * hold >= max T_i and ``first_row`` (N, K) int32 replace the on-device generator and hash for every plan alike (tests).

    -> one dict per plan: ``path`` float32 (rows_out + 1, 6) = the start state plus one state per action, ``actions`` float32
    (rows_out, 2), ``rows_in`` (of the tape given), ``rows_out``, ``arrival_in`` / ``arrival_out`` (arrival times in rows,
    continuous; None for a refused plan), ``status`` ("ok", or why the plan was refused: "no_arrival", "collides",
    "start_in_goal" -- then ``path`` is None, ``actions`` the input tape and ``rows_out`` = ``rows_in``), ``trace`` (a dict of
    (N,) arrays: TRACE_COLUMNS); and for tests ``path64`` (the path in the device's float64) and ``raw`` (the plan's device
    buffers as the call left them: ``rows``, ``tape``, ``states``, ``arrival``, ``trace``).
    """
    K, N, s, hold = check_settings(rollouts, iterations, sigma, hold)
    tapes = [np.ascontiguousarray(np.asarray(t, dtype=np.float32).reshape(-1, 2)) for t in tapes]
    P = len(tapes)
    if P < 1:
        return []
    starts = np.ascontiguousarray(np.asarray(starts, dtype=np.float64).reshape(-1, 6))
    goals = np.ascontiguousarray(np.asarray(goals, dtype=np.float64).reshape(len(starts), -1)[:, :2])
    if len(starts) != P or len(goals) != P:
        raise ValueError(f"polish_plans: {P} tapes need {P} starts and goals")
    if any(len(t) < 1 for t in tapes):
        raise ValueError("polish_plans: an empty tape")
    one_maze = isinstance(mazes, np.ndarray) and mazes.ndim == 2
    maze_list = [np.asarray(mazes, dtype=np.float32)] if one_maze else [np.asarray(m, dtype=np.float32) for m in mazes]
    if not one_maze and len(maze_list) != P:
        raise ValueError(f"polish_plans: {P} plans need one maze or {P} mazes")
    for m in maze_list:
        if m.ndim != 2 or m.size > _lib.POLISH_MAX_CELLS:
            raise ValueError(f"polish_plans: a maze must be 2-D with at most {_lib.POLISH_MAX_CELLS} cells (it is staged in LDS)")
    cap = max(len(t) for t in tapes)
    dev = ctx.device
    keep = []
    d = Polish()
    d.n_plans, d.state_dim, d.action_dim, d.capacity = P, 6, 2, cap
    d.K, d.N, d.hold, d.seed = K, N, hold, int(seed) & 0xFFFFFFFFFFFFFFFF
    d.sigma[0], d.sigma[1] = s
    if noise is not None:
        nz = torch.as_tensor(np.ascontiguousarray(noise, dtype=np.float64), device=dev)
        if nz.ndim != 4 or tuple(nz.shape[:2]) != (N, K) or nz.shape[3] != 2 or nz.shape[2] * hold < cap:
            raise ValueError(f"polish_plans: noise must be ({N}, {K}, NB, 2) with NB * hold >= {cap}")
        d.noise, d.noise_blocks = nz.data_ptr(), int(nz.shape[2])
        keep.append(nz)
    if first_row is not None:
        fr = torch.as_tensor(np.ascontiguousarray(first_row, dtype=np.int32), device=dev)
        if tuple(fr.shape) != (N, K):
            raise ValueError(f"polish_plans: first_row must be ({N}, {K})")
        d.first_row = fr.data_ptr()
        keep.append(fr)
    if one_maze:
        ctx.upload_maze(maze_list[0], owner=None)
    else:
        # identical maps share their atlas bytes; more plans than the table holds scenes go in several calls
        if P > _lib.MAX_SCENES or sum(m.size for m in maze_list) > _lib.MAX_ATLAS_CELLS:
            half = P // 2
            kw = dict(rollouts=K, iterations=N, sigma=s, hold=hold, seed=seed, noise=noise, first_row=first_row)
            return (polish_plans(ctx, maze_list[:half], starts[:half], goals[:half], tapes[:half], **kw)
                    + polish_plans(ctx, maze_list[half:], starts[half:], goals[half:], tapes[half:], **kw))
        ctx.upload_scenes(maze_list, goals, owner=None)
        scene = torch.arange(P, dtype=torch.int32, device=dev)
        scene_host = (C.c_int32 * P)(*range(P))
        d.scene, d.scene_host = scene.data_ptr(), scene_host
        keep += [scene, scene_host]
    tape_h = np.zeros((P, cap, 2))
    for i, t in enumerate(tapes):
        tape_h[i, :len(t)] = t
    rows_h = np.array([len(t) for t in tapes], dtype=np.int32)
    tape = torch.as_tensor(tape_h, device=dev)
    rows = torch.as_tensor(rows_h, device=dev)
    rows_host = (C.c_int32 * P)(*[int(v) for v in rows_h])
    x0 = torch.as_tensor(starts, device=dev)
    gl = torch.as_tensor(goals, device=dev)
    states = torch.zeros(P, cap + 1, 6, dtype=torch.float64, device=dev)
    arrival = torch.zeros(P, 2, dtype=torch.float64, device=dev)
    status = torch.full((P,), -1, dtype=torch.int32, device=dev)
    trace = torch.zeros(P, max(N, 1), _lib.POLISH_TRACE, dtype=torch.float64, device=dev)
    d.x0, d.goal_xy, d.tape, d.rows, d.rows_host = x0.data_ptr(), gl.data_ptr(), tape.data_ptr(), rows.data_ptr(), rows_host
    d.states, d.arrival, d.status, d.trace = states.data_ptr(), arrival.data_ptr(), status.data_ptr(), trace.data_ptr()
    check(ctx._h, lib().ditree_polish_plans(ctx._h, C.byref(d), ctx.stream), "polish_plans")
    status_h = status.cpu().numpy()                    # (synchronises: everything above has run)
    del keep
    rows_o, tape_o, states_o, arr, tr = (t.cpu().numpy() for t in (rows, tape, states, arrival, trace))
    out = []
    for i in range(P):
        ok = int(status_h[i]) == _lib.POLISH_OK
        n = int(rows_o[i])
        t = tr[i, :N]
        out.append(dict(
            path=states_o[i, :n + 1].astype(np.float32) if ok else None,
            actions=tape_o[i, :n].astype(np.float32) if ok else tapes[i],
            rows_in=int(rows_h[i]), rows_out=n if ok else int(rows_h[i]),
            arrival_in=float(arr[i, 0]) if ok else None, arrival_out=float(arr[i, 1]) if ok else None,
            status=STATUS_NAMES.get(int(status_h[i]), str(int(status_h[i]))),
            trace=dict(winner=t[:, 0].astype(np.int64), tau=t[:, 1].copy(), accepted=t[:, 2] != 0, rows=t[:, 3].astype(np.int64),
                       arrival=t[:, 4].copy(), arriving=t[:, 5].astype(np.int64)) if ok else
            {c: np.zeros(0) for c in TRACE_COLUMNS},
            path64=states_o[i, :n + 1].copy() if ok else None,
            raw=dict(rows=int(rows_o[i]), tape=tape_o[i], states=states_o[i], arrival=arr[i], trace=tr[i, :N])))
    return out
