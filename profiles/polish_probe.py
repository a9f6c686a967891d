"""What ``RRT_Planner.polish`` does to found plans.  A report, not a gate.  One JSON line (and --out).

The car scenarios x --seeds seeds at one fixed ``max_candidates``, ``solution`` "first" and "anytime", with the sampler, budgets
and scenarios of the `solution`-modes table (profiles/near_parent_plan_probe.py).  Per goal-reaching run: rows and arrival time
before and after ``polish()`` at the defaults, the share of candidates that still arrive per iteration, the wall time of the
polish next to the wall time of the plan.  Then a small sweep of ``rollouts``, ``sigma`` and ``hold`` over the same "first"
plans, all plans of a setting in one ``polish_plans`` call.  polish.DEFAULTS were picked from this sweep: settings, not tuned
truths.

    timeout -k 10 900 python profiles/polish_probe.py --out profiles/polish_probe.json
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

MODES = ("first", "anytime")
SWEEP = [dict(rollouts=k, iterations=24, sigma=s, hold=h)
         for k, s, h in ((256, (1.0, 0.1), 8), (1024, (1.0, 0.1), 8), (4096, (1.0, 0.1), 8), (1024, (0.5, 0.05), 8),
                         (1024, (2.0, 0.2), 8), (1024, (1.0, 0.1), 1), (1024, (1.0, 0.1), 4), (1024, (1.0, 0.1), 16),
                         (1024, (1.0, 0.1), 64), (4096, (1.0, 0.1), 1), (4096, (2.0, 0.2), 8), (4096, (2.0, 0.2), 1))]


def planner(sc, mode, batch, max_candidates):
    from ditreeonlineplanner_amd.car_env import CarEnv
    from ditreeonlineplanner_amd.planners.RRT import RRT_Planner
    from ditreeonlineplanner_amd.policies.uniform_policy import UniformSampler
    env = CarEnv(maze_map=sc["maze"], collision_checking=False)
    return RRT_Planner(sc["start"], sc["goal"], env_id="carmaze", environment=env, sampler=UniformSampler(env.action_space, seed=3),
                       action_horizon=8, local_map_size=20, local_map_scale=0.2, global_map_scale=1.0, goal_conditioning_bias=0.85,
                       prop_duration=[64], time_budget=600, batch=batch, max_candidates=max_candidates,
                       capacity=max_candidates + 1, emulate_sticky_done=False, solution=mode)


def mean(v):
    v = [x for x in v if x is not None]
    return float(np.mean(v)) if v else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--max-candidates", type=int, default=4096)
    ap.add_argument("--seeds", type=int, default=4)
    a = ap.parse_args()
    from ditreeonlineplanner_amd.polish import DEFAULTS, polish_plans
    from ditreeonlineplanner_amd.scenarios import car_scenarios
    scenarios = car_scenarios()
    runs, kept = {}, []
    for mode in MODES:
        rs = runs[mode] = []
        for i, sc in enumerate(scenarios):
            pl = planner(sc, mode, a.batch, a.max_candidates)
            for s in range(a.seeds):
                random.seed(s)
                np.random.seed(s)
                torch.manual_seed(s)
                pl.reset()
                t0 = time.perf_counter()
                pl.plan()
                torch.cuda.synchronize()
                t_plan = time.perf_counter() - t0
                goal = pl._engine.goal_node is not None
                row = dict(scenario=i, seed=s, goal=goal, plan_wall_s=t_plan, path_time_in=pl.results.get("path_time"))
                if goal:
                    if mode == "first":
                        kept.append((pl.maze.copy(), pl.start_node.state.copy(), np.asarray(pl.env.goal, dtype=np.float64).copy(),
                                     pl.results["actions"].copy()))
                    t0 = time.perf_counter()
                    pl.polish()
                    t_pol = time.perf_counter() - t0
                    p = pl.results["polish"]
                    row.update(status=p["status"], rows_in=p["rows_in"], rows_out=p["rows_out"], arrival_in=p["arrival_in"],
                               arrival_out=p["arrival_out"], polish_wall_s=t_pol, path_time_out=pl.results["path_time"],
                               arriving_share=None if p["trace"] is None or not len(p["trace"]["arriving"]) else
                               [float(v) / DEFAULTS["rollouts"] for v in p["trace"]["arriving"]])
                rs.append(row)
            del pl
    summary = {}
    for mode, rs in runs.items():
        ok = [r for r in rs if r.get("status") == "ok"]
        summary[mode] = dict(runs=len(rs), goal_reached=sum(r["goal"] for r in rs), polished=len(ok),
                             refused={k: sum(r.get("status") == k for r in rs) for k in ("no_arrival", "collides", "start_in_goal")},
                             mean_rows_in=mean([r["rows_in"] for r in ok]), mean_rows_out=mean([r["rows_out"] for r in ok]),
                             mean_arrival_in=mean([r["arrival_in"] for r in ok]), mean_arrival_out=mean([r["arrival_out"] for r in ok]),
                             mean_path_time_in=mean([r["path_time_in"] for r in ok]), mean_path_time_out=mean([r["path_time_out"] for r in ok]),
                             mean_arriving_share=mean([np.mean(r["arriving_share"]) for r in ok if r["arriving_share"]]),
                             mean_plan_wall_s=mean([r["plan_wall_s"] for r in ok]), mean_polish_wall_s=mean([r["polish_wall_s"] for r in ok]))
    sweep = []
    if kept:
        ctx_pl = planner(scenarios[0], "first", a.batch, a.max_candidates)
        for st in SWEEP:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = polish_plans(ctx_pl.ctx, [k[0] for k in kept], np.stack([k[1] for k in kept]), np.stack([k[2] for k in kept]),
                               [k[3] for k in kept], seed=0, **st)
            wall = time.perf_counter() - t0
            ok = [r for r in out if r["status"] == "ok"]
            sweep.append(dict(rollouts=st["rollouts"], iterations=st["iterations"], sigma=list(st["sigma"]), hold=st["hold"], plans=len(out),
                              polished=len(ok), mean_rows_in=mean([r["rows_in"] for r in ok]), mean_rows_out=mean([r["rows_out"] for r in ok]),
                              mean_arrival_in=mean([r["arrival_in"] for r in ok]), mean_arrival_out=mean([r["arrival_out"] for r in ok]),
                              mean_arriving_share=mean([float(np.mean(r["trace"]["arriving"])) / st["rollouts"] for r in ok]),
                              wall_s_all_plans=wall))
    out = {"probe": "polish_probe", "device": torch.cuda.get_device_name(0), "sampler": "UniformSampler(seed=3)", "batch": a.batch,
           "max_candidates": a.max_candidates, "prop_duration": [64], "seeds": list(range(a.seeds)), "scenarios": len(scenarios),
           "defaults": {k: (list(v) if isinstance(v, tuple) else v) for k, v in DEFAULTS.items()}, "summary": summary, "sweep": sweep,
           "runs": runs}
    print(json.dumps({"summary": summary, "sweep": sweep}))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
