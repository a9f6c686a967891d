"""Path quality of the planner's three ``solution`` modes on the 15 car scenarios (data/test_scenarios_car.csv): the same seeded
runs with ``UniformSampler`` and the same ``max_candidates`` in every mode, mean ``path_time`` over the runs that reached the
goal, the share of runs that did, and the success rate (a path came back: run_scenarios.py:350-353) per mode.  A report, not
a gate.  Prints one JSON line (and writes it to --out).

    timeout -k 10 600 python profiles/solution_modes_probe.py --out profiles/r11_solution_modes_probe.json
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

MODES = ("first", "best_of_round", "anytime")


def planner(sc, mode, batch, max_candidates):
    from ditreeonlineplanner_amd.car_env import CarEnv
    from ditreeonlineplanner_amd.planners.RRT import RRT_Planner
    from ditreeonlineplanner_amd.policies.uniform_policy import UniformSampler
    env = CarEnv(maze_map=sc["maze"], collision_checking=False)
    return RRT_Planner(sc["start"], sc["goal"], env_id="carmaze", environment=env, sampler=UniformSampler(env.action_space, seed=3),
                       action_horizon=8, local_map_size=20, local_map_scale=0.2, global_map_scale=1.0, goal_conditioning_bias=0.85,
                       prop_duration=[64], time_budget=600, batch=batch, max_candidates=max_candidates,
                       capacity=max_candidates + 1, emulate_sticky_done=False, solution=mode)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--max-candidates", type=int, default=4096)
    ap.add_argument("--seeds", type=int, default=3)
    a = ap.parse_args()
    from ditreeonlineplanner_amd.scenarios import car_scenarios
    scenarios = car_scenarios()
    out = {"probe": "solution_modes_probe", "device": torch.cuda.get_device_name(0), "sampler": "UniformSampler(seed=3)",
           "batch": a.batch, "max_candidates": a.max_candidates, "prop_duration": [64], "seeds": list(range(a.seeds)),
           "scenarios": len(scenarios), "modes": {}, "per_scenario": {}}
    runs = {m: [] for m in MODES}
    for sc in scenarios:
        row = {}
        for mode in MODES:
            pl = planner(sc, mode, a.batch, a.max_candidates)
            res = []
            for s in range(a.seeds):
                random.seed(s)
                np.random.seed(s)
                torch.manual_seed(s)
                pl.reset()
                t0 = time.perf_counter()
                pl.plan()
                r = pl.results
                res.append(dict(goal=pl._engine.goal_node is not None, path=r["path"] is not None,
                                path_time=r.get("path_time") if r["path"] is not None else None,
                                solutions=r["solutions"], first_solution_candidates=r["first_solution_candidates"],
                                nodes=r["number_of_nodes"], wall_s=time.perf_counter() - t0))
            runs[mode] += res
            reached = [x["path_time"] for x in res if x["goal"]]
            row[mode] = {"goal_reached": len(reached), "mean_path_time": float(np.mean(reached)) if reached else None,
                         "mean_solutions": float(np.mean([x["solutions"] for x in res]))}
            del pl
        out["per_scenario"][sc["name"]] = row
    # the modes differ only behind the first goal-reaching round, so they reach the goal in the same runs: the means compare
    for mode in MODES:
        reached = [x["path_time"] for x in runs[mode] if x["goal"]]
        out["modes"][mode] = {"runs": len(runs[mode]), "success": float(np.mean([x["path"] for x in runs[mode]])),
                              "goal_reached": len(reached) / len(runs[mode]),
                              "mean_path_time": float(np.mean(reached)) if reached else None,
                              "mean_solutions": float(np.mean([x["solutions"] for x in runs[mode]])),
                              "mean_wall_s": float(np.mean([x["wall_s"] for x in runs[mode]]))}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
