"""MPPI missions: the stepwise driver loop (`MPPI.step` + `online.scan_and_update_maze` every scan_time: the only way to run
a mission before `ditree_mppi_missions`) against the fused forms, in the same process, alternating, after warm-up, best of
``--reps``; the host clock of either form ends in a device synchronise.

  (a) missions along the free L-shaped path through boxes.csv, one after another until ``--steps`` controller calls are made
      (one mission ends by GOAL or TRIALS after a few hundred), at (K, T) = (20, 8), (20, 16) and (256, 16): stepwise loop
      against `MPPI.follow`, ms per controller call each.  Both forms must leave the same state, controls, mazes and counts
      (they are bit-exact: tests/test_gpu_mppi_mission.py).
  (b) fleets of M = 1, 16, 64, 256, 512 of that mission (own seeds) at (20, 16) through `mppi.follow_fleet`: seconds per
      call (one launch), missions per second.

Prints one JSON line (and writes it to --out).

    timeout -k 10 600 python profiles/mppi_mission_probe.py --out profiles/r09_mppi_mission_probe.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ALLOWED_TRIALS = 5


def boxes():
    return np.loadtxt(os.path.join(REPO, "ditreeonlineplanner_amd", "data", "boxes.csv"), delimiter=",")


def controller(ctx, maze, K, T, seed):
    """East along the bottom corridor of boxes.csv (row 18), then north along column 18, points every 0.02; start at rest."""
    from ditreeonlineplanner_amd.mppi import MPPI
    m = MPPI(maze_data=maze, T=T, K=K, nx=6, nu=2, ctx=ctx, seed=seed)
    a, b, c = (m.env.cell_rowcol_to_xy(rc) for rc in ([18, 1], [18, 18], [1, 18]))
    seg1 = a + (b - a) * np.linspace(0, 1, int(np.linalg.norm(b - a) / 0.02))[:, None]
    seg2 = b + (c - b) * np.linspace(0, 1, int(np.linalg.norm(c - b) / 0.02))[1:, None]
    path = np.concatenate([seg1, seg2])
    start = np.array([path[0, 0], path[0, 1], 0.0, 0.0, 0.0, 0.0])
    goal = np.array([c[0], c[1], 0, 0, 0, 0.0])
    m.reset(start_state=start, goal_state=goal)
    m.set_ref_path(path)
    return m, start, goal


def stepwise(m, state, known, truth, scanned, max_steps):
    """run_scenarios_with_lidar_MPPI.py:417-452 with at most `max_steps` controller calls."""
    from ditreeonlineplanner_amd import online
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    calls = trials = n = 0
    t_acc = 0.0
    while calls < max_steps and not m.is_done(state) and trials < ALLOWED_TRIALS:
        nxt, action, done = m.step(state)
        calls += 1
        if done is None:
            trials += 1
            continue
        trials = 0
        state = nxt
        m.env.set_state(state)
        n += 1
        t_acc += m.env.dt
        if t_acc > m.env.lidar2dsim.scan_time:
            online.scan_and_update_maze(m, known, truth, scanned)
            t_acc = 0.0
    torch.cuda.synchronize()
    return time.perf_counter() - t0, calls, n, state


def fused(m, state, known, truth, scanned, max_steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = m.follow(state, known, truth, scanned, max_steps, allowed_trials=ALLOWED_TRIALS)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out[4]["controller_calls"], len(out[1]), out[0]


def one_mission(ctx, maze, K, T, steps, reps):
    """A mission on this path ends by GOAL or TRIALS after a few hundred controller calls, so the timed window of either form
    is a series of missions (seeds 7, 8, ...) run one after another until `steps` controller calls are made: the same series
    for both forms, the controllers built outside the clock."""
    def run(form, seed, n):
        m, start, _ = controller(ctx, maze, K, T, seed=seed)
        known, scanned = maze.copy(), maze.copy()
        t, calls, n_exec, state = form(m, start, known, maze, scanned, n)
        return t, calls, n_exec, state, m._U.cpu().numpy(), known, scanned
    run(fused, 7, 40)
    seeds, total = [], 0
    while total < steps and len(seeds) < 64:             # also the stepwise form's warm-up
        seeds.append(7 + len(seeds))
        total += run(stepwise, seeds[-1], steps)[1]
    t_s, t_f, same = [], [], True
    for _ in range(reps):
        s = [run(stepwise, seed, steps) for seed in seeds]
        f = [run(fused, seed, steps) for seed in seeds]
        t_s.append(sum(r[0] for r in s))
        t_f.append(sum(r[0] for r in f))
        for a, b in zip(s, f):
            same = same and a[1:3] == b[1:3] and all(np.array_equal(x, y) for x, y in zip(a[3:], b[3:]))
    calls = sum(r[1] for r in s)
    return {"K": K, "T": T, "missions": len(seeds), "controller_calls": calls, "steps_executed": sum(r[2] for r in s),
            "stepwise_s": t_s, "follow_s": t_f, "stepwise_ms_per_call": 1e3 * min(t_s) / calls,
            "follow_ms_per_call": 1e3 * min(t_f) / calls, "ratio": min(t_s) / min(t_f), "same_result": bool(same)}


def fleets(ctx, maze, K, T, steps, sizes, reps):
    from ditreeonlineplanner_amd import mppi
    made = [controller(ctx, maze, K, T, seed=100 + i) for i in range(max(sizes))]
    out = []
    for M in sizes:
        ts = []
        for rep in range(reps + 1):                       # the first run of every size is its warm-up
            cs = [c for c, _, _ in made[:M]]
            for c, start, goal in made[:M]:
                c.reset(start_state=start, goal_state=goal)
                c.update_maze(maze.copy())
            known = [maze.copy() for _ in range(M)]
            scanned = [maze.copy() for _ in range(M)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = mppi.follow_fleet(cs, [s for _, s, _ in made[:M]], known, [maze] * M, scanned, steps, allowed_trials=ALLOWED_TRIALS)
            torch.cuda.synchronize()
            if rep:
                ts.append(time.perf_counter() - t0)
        out.append({"M": M, "seconds": ts, "missions_per_s": M / min(ts),
                    "controller_calls": int(sum(r[4]["controller_calls"] for r in res))})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--fleets", type=int, nargs="*", default=[1, 16, 64, 256, 512])
    a = ap.parse_args()
    from ditreeonlineplanner_amd.ops import Context
    ctx = Context(0)
    maze = boxes()
    single = [one_mission(ctx, maze, K, T, a.steps, a.reps) for K, T in ((20, 8), (20, 16), (256, 16))]
    fl = fleets(ctx, maze, 20, 16, a.steps, a.fleets, a.reps) if a.fleets else []
    t1 = next((min(f["seconds"]) for f in fl if f["M"] == 1), None)
    t64 = next((min(f["seconds"]) for f in fl if f["M"] == 64), None)
    out = {"probe": "mppi_mission_probe", "device": torch.cuda.get_device_name(0), "steps": a.steps, "dt": 0.02, "scan_time": 0.2,
           "allowed_trials": ALLOWED_TRIALS, "one_mission": single, "fleets_K20_T16": fl,
           "follow_not_slower_at_every_size": all(s["ratio"] >= 1.0 for s in single),
           "fleet_64_under_64x_one": (t64 < 64 * t1) if t1 is not None and t64 is not None else None,
           "same_result": all(s["same_result"] for s in single)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not out["same_result"]:
        sys.exit("the fused mission and the stepwise loop left different results")


if __name__ == "__main__":
    main()
