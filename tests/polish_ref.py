"""numpy restatement of plan polishing (include/ditree.h "plan polishing") -- TEST INFRASTRUCTURE ONLY.

Written on the pinned pieces of the oracle -- ``oracle.geometry`` (``car_step``, ``is_colliding_car``, ``norm2``) and
``oracle.mppi`` (``device_noise``, ``_splitmix64``) -- and independently of the HIP kernels: every candidate's WHOLE tape is
rolled from the start state, all candidates of an iteration at once, where the device integrates a candidate from the
incumbent's state at its first perturbed row.  The rule is the build's own (no counterpart in the reference: parity unpinned).
"""
from __future__ import annotations

import numpy as np

from oracle import geometry as G
from oracle import mppi as OM

OK, NO_ARRIVAL, COLLIDES, START_IN_GOAL, NOT_F32 = 0, 1, 2, 3, 4
STATUS_NAMES = {OK: "ok", NO_ARRIVAL: "no_arrival", COLLIDES: "collides", START_IN_GOAL: "start_in_goal", NOT_F32: "not_f32"}
CRITICAL = 1e-9          # a candidate this close to the radius or to a wall may flip on the device (the pinned state bound)


def first_rows(seed, n, K, T):
    """a[k] = H(seed, n, k) mod T, the hash as include/ditree.h states it."""
    with np.errstate(over="ignore"):
        h = OM._splitmix64(np.uint64(seed) ^ OM._splitmix64(np.uint64(n)))
        k = np.arange(K, dtype=np.uint64)
        h = OM._splitmix64(h ^ (k * np.uint64(0xD1B54A32D192ED03)))
        H = OM._splitmix64(h ^ np.uint64(0xA24BAED4963EE407))
    return (H % np.uint64(T)).astype(np.int64)


def given_first_rows(r, T):
    """The caller-supplied first_row values: r mod T for r >= 0, max(T + r, 0) for r < 0."""
    r = np.asarray(r, dtype=np.int64)
    return np.where(r >= 0, r % T, np.maximum(T + r, 0))


def _near_wall(x, maze):
    """Rows of x whose collision flag changes when the pose moves by CRITICAL."""
    base = G.is_colliding_car(x, maze)
    out = np.zeros(len(x), dtype=bool)
    for dx, dy, dp in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (1, 1, 0), (1, -1, 0), (-1, 1, 0), (-1, -1, 0), (0, 0, 1),
                       (0, 0, -1)):
        y = x.copy()
        y[:, 0] += dx * CRITICAL
        y[:, 1] += dy * CRITICAL
        y[:, 2] += dp * CRITICAL
        out |= G.is_colliding_car(y, maze) != base
    return out


def roll(maze, x0, goal, tapes, critical=False):
    """Roll K whole tapes (K, T, 2) from x0.  -> dict: ``arrived`` (K,) bool, ``collided`` (K,) bool, ``rows`` (K,) (the arrival
    row count s, 0 when not arrived), ``tau`` (K,) (inf when not arrived), ``states`` (K, T + 1, 6) (rows after the end stay
    zero), ``ran`` (K,) rows executed, ``d0`` and, with ``critical``, which tapes came within CRITICAL of the radius or of a wall on a row they ran."""
    tapes = np.asarray(tapes, dtype=np.float64)
    K, T = tapes.shape[:2]
    goal = np.asarray(goal, dtype=np.float64)
    x = np.tile(np.asarray(x0, dtype=np.float64), (K, 1))
    states = np.zeros((K, T + 1, 6))
    states[:, 0] = x
    d_prev = G.norm2(x[:, 0] - goal[0], x[:, 1] - goal[1])
    d0 = float(d_prev[0]) if K else np.inf
    alive = np.ones(K, dtype=bool)
    arrived = np.zeros(K, dtype=bool)
    collided = np.zeros(K, dtype=bool)
    rows = np.zeros(K, dtype=np.int64)
    tau = np.full(K, np.inf)
    crit = np.zeros(K, dtype=bool)
    ran = np.zeros(K, dtype=np.int64)
    for t in range(T):
        idx = np.nonzero(alive)[0]
        if idx.size == 0:
            break
        a = np.clip(tapes[idx, t], G.ACT_LOW, G.ACT_HIGH)             # clipped as the env clips it
        xn = G.car_step(x[idx], a)
        x[idx] = xn
        states[idx, t + 1] = xn
        ran[idx] = t + 1
        coll = G.is_colliding_car(xn, maze)
        d = G.norm2(xn[:, 0] - goal[0], xn[:, 1] - goal[1])
        if critical:
            crit[idx] |= (np.abs(d - G.GOAL_RADIUS) < CRITICAL) | _near_wall(xn, maze)
        hit = ~coll & (d < G.GOAL_RADIUS)
        collided[idx[coll]] = True
        arrived[idx[hit]] = True
        rows[idx[hit]] = t + 1
        dp = d_prev[idx]
        tau[idx[hit]] = float(t) + (dp[hit] - 0.5) / (dp[hit] - d[hit])
        d_prev[idx] = d
        alive[idx[coll | hit]] = False
    return dict(arrived=arrived, collided=collided, rows=rows, tau=tau, states=states, d0=d0, critical=crit, ran=ran)


def replay(maze, x0, goal, tape):
    """Step 1 of the rule for one tape (T, 2) -> dict(status, rows, tau, states (rows + 1, 6))."""
    tape = np.asarray(tape, dtype=np.float64)
    goal = np.asarray(goal, dtype=np.float64)
    x0 = np.asarray(x0, dtype=np.float64)
    if float(G.norm2(x0[0] - goal[0], x0[1] - goal[1])) < G.GOAL_RADIUS:
        return dict(status=START_IN_GOAL, rows=len(tape), tau=np.inf, states=None)
    r = roll(maze, x0, goal, tape[None])
    ran = int(r["ran"][0])                                # the rows are met in order: one that is not f32-exact counts when reached
    if not np.array_equal(tape[:ran].astype(np.float32).astype(np.float64), tape[:ran]):
        return dict(status=NOT_F32, rows=len(tape), tau=np.inf, states=None)
    if r["collided"][0]:
        return dict(status=COLLIDES, rows=len(tape), tau=np.inf, states=None)
    if not r["arrived"][0]:
        return dict(status=NO_ARRIVAL, rows=len(tape), tau=np.inf, states=None)
    s = int(r["rows"][0])
    return dict(status=OK, rows=s, tau=float(r["tau"][0]), states=r["states"][0, :s + 1].copy())


def candidate_tapes(U, a, eps, hold):
    """u_k[t] = (double)(float) clip(U[t] + (t >= a[k] ? eps[k, t div hold] : 0)): U (T, 2), a (K,), eps (K, NB, 2) -> (K, T, 2)."""
    U = np.asarray(U, dtype=np.float64)
    T = len(U)
    t = np.arange(T)
    e = np.asarray(eps, dtype=np.float64)[:, t // hold]                   # (K, T, 2)
    e = np.where((t[None, :] >= np.asarray(a)[:, None])[..., None], e, 0.0)
    return np.clip(U[None] + e, G.ACT_LOW, G.ACT_HIGH).astype(np.float32).astype(np.float64)


def iterate(maze, x0, goal, U, tau_star, a, eps, hold, critical=False):
    """One iteration on the incumbent (U, tau_star).  -> dict: per candidate ``tau``, ``rows``, ``arrived``, ``critical``; the
    ``winner`` (-1: nothing arrived), ``accepted``, and the incumbent after it: ``tape``, ``tau_star``, ``states``."""
    tapes = candidate_tapes(U, a, eps, hold)
    r = roll(maze, x0, goal, tapes, critical=critical)
    tau = r["tau"]
    winner = int(np.argmin(tau)) if r["arrived"].any() else -1            # first occurrence of the minimum: ties to the lowest k
    accepted = winner >= 0 and bool(tau[winner] < tau_star)
    out = dict(tau=tau, rows=r["rows"], arrived=r["arrived"], critical=r["critical"], winner=winner, accepted=accepted,
               tapes=tapes, tape=np.asarray(U, dtype=np.float64), tau_star=tau_star, states=None)
    if accepted:
        s = int(r["rows"][winner])
        out.update(tape=tapes[winner, :s].copy(), tau_star=float(tau[winner]), states=r["states"][winner, :s + 1].copy())
    return out


def polish(maze, x0, goal, tape, K, N, sigma, hold, seed, noise=None, first_row=None, critical=False):
    """The whole rule for one plan.  noise (N, K, NB, 2) / first_row (N, K) replace the generator and the hash.  -> dict(status,
    tape, rows, states, arrival_in, arrival_out, trace: one dict per iteration with winner, tau, accepted, rows, tau_star,
    arriving, critical)."""
    rp = replay(maze, x0, goal, tape)
    if rp["status"] != OK:
        return dict(status=rp["status"], tape=np.asarray(tape, dtype=np.float64), rows=len(tape), states=None, arrival_in=None,
                    arrival_out=None, trace=[])
    U = np.asarray(tape, dtype=np.float64)[:rp["rows"]].copy()
    tau_star, states = rp["tau"], rp["states"]
    trace = []
    for n in range(N):
        T = len(U)
        a = first_rows(seed, n, K, T) if first_row is None else given_first_rows(first_row[n], T)
        nb = (T + hold - 1) // hold
        eps = OM.device_noise(seed, n, K, nb, sigma) if noise is None else np.asarray(noise[n], dtype=np.float64)
        it = iterate(maze, x0, goal, U, tau_star, a, eps, hold, critical=critical)
        if it["accepted"]:
            U, tau_star, states = it["tape"], it["tau_star"], it["states"]
        w = it["winner"]
        trace.append(dict(winner=w, tau=float(it["tau"][w]) if w >= 0 else np.inf, accepted=it["accepted"], rows=len(U),
                          tau_star=tau_star, arriving=int(it["arrived"].sum()), critical=int(it["critical"].sum())))
    return dict(status=OK, tape=U, rows=len(U), states=states, arrival_in=rp["tau"], arrival_out=tau_star, trace=trace)
