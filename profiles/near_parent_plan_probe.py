"""What ``near_radius`` does to plans.  A report, not a gate.  One JSON line (and --out).

The car scenarios x --seeds seeds at one fixed ``max_candidates``, ``solution`` "anytime" and "anytime_pruned", each with
``near_radius`` None, 0.5, 1 and 2 maze cells (1 cell = 1 m) at the default ``near_speed``; the sampler, budgets and scenarios
of profiles/solution_modes_probe.py.  Per run: the final incumbent's cost (path rows), the round of the first goal path, the
node count.  Summed up per setting, and run by run against the same run without the kwarg.

    timeout -k 10 600 python profiles/near_parent_plan_probe.py --out profiles/near_parent_plan_probe.json
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
sys.path.insert(0, os.path.join(REPO, "profiles"))

MODES = ("anytime", "anytime_pruned")
RADII = (None, 0.5, 1.0, 2.0)


def planner(sc, mode, batch, max_candidates, radius, speed):
    from ditreeonlineplanner_amd.car_env import CarEnv
    from ditreeonlineplanner_amd.planners.RRT import RRT_Planner
    from ditreeonlineplanner_amd.policies.uniform_policy import UniformSampler
    env = CarEnv(maze_map=sc["maze"], collision_checking=False)
    kw = {} if radius is None else dict(near_radius=radius, **({} if speed is None else dict(near_speed=speed)))
    return RRT_Planner(sc["start"], sc["goal"], env_id="carmaze", environment=env, sampler=UniformSampler(env.action_space, seed=3),
                       action_horizon=8, local_map_size=20, local_map_scale=0.2, global_map_scale=1.0, goal_conditioning_bias=0.85,
                       prop_duration=[64], time_budget=600, batch=batch, max_candidates=max_candidates,
                       capacity=max_candidates + 1, emulate_sticky_done=False, solution=mode, **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--max-candidates", type=int, default=4096)
    ap.add_argument("--seeds", type=int, default=4)
    ap.add_argument("--near-speed", type=float, default=None, help="default: the planner's (max_v)")
    a = ap.parse_args()
    from ditreeonlineplanner_amd.scenarios import car_scenarios
    scenarios = car_scenarios()
    runs = {}
    for mode in MODES:
        for radius in RADII:
            rs = runs[f"{mode}/{radius}"] = []
            for i, sc in enumerate(scenarios):
                pl = planner(sc, mode, a.batch, a.max_candidates, radius, a.near_speed)
                for s in range(a.seeds):
                    random.seed(s)
                    np.random.seed(s)
                    torch.manual_seed(s)
                    pl.reset()
                    t0 = time.perf_counter()
                    pl.plan()
                    r, eng = pl.results, pl._engine
                    g = eng.goal_node
                    first = r["first_solution_candidates"]
                    rs.append(dict(scenario=i, seed=s, cost=None if g is None else int(eng.tree.cost[g].item()),
                                   first_goal_round=None if first is None else -(-first // a.batch), nodes=r["number_of_nodes"],
                                   candidates=int(eng.tree.counters[4].item()), wall_s=time.perf_counter() - t0))
                del pl
    summary = {}
    for k, rs in runs.items():
        mode = k.split("/")[0]
        base = runs[f"{mode}/None"]
        goal = [x for x in rs if x["cost"] is not None]
        both = [(b["cost"], x["cost"]) for b, x in zip(base, rs) if b["cost"] is not None and x["cost"] is not None]
        summary[k] = {"runs": len(rs), "goal_reached": len(goal),
                      "mean_cost": float(np.mean([x["cost"] for x in goal])) if goal else None,
                      "mean_first_goal_round": float(np.mean([x["first_goal_round"] for x in goal])) if goal else None,
                      "mean_nodes": float(np.mean([x["nodes"] for x in rs])), "mean_candidates": float(np.mean([x["candidates"] for x in rs])),
                      "mean_wall_s": float(np.mean([x["wall_s"] for x in rs])),
                      "against_no_near": {"both_reached": len(both), "cheaper": sum(x < b for b, x in both), "equal": sum(x == b for b, x in both),
                                          "dearer": sum(x > b for b, x in both),
                                          "goal_lost": sum(b["cost"] is not None and x["cost"] is None for b, x in zip(base, rs)),
                                          "goal_won": sum(b["cost"] is None and x["cost"] is not None for b, x in zip(base, rs)),
                                          "mean_cost_both": [float(np.mean([b for b, _ in both])), float(np.mean([x for _, x in both]))]
                                          if both else None}}
    out = {"probe": "near_parent_plan_probe", "device": torch.cuda.get_device_name(0), "sampler": "UniformSampler(seed=3)",
           "batch": a.batch, "max_candidates": a.max_candidates, "prop_duration": [64], "seeds": list(range(a.seeds)),
           "scenarios": len(scenarios), "near_speed": a.near_speed, "cell_m": 1.0, "summary": summary, "runs": runs}
    print(json.dumps(out["summary"]))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
