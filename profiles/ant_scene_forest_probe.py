"""Runs/s of the seeded runs of the whole ANT scenario set (tests/golden/test_scenarios_ant.csv: 15 scenarios on 7 mazes) done
as 15 ``RRT_Planner.plan_runs`` calls one after another (one AntForestEngine per scenario: what there was before ant scene
forests) and as one ``plan_ant_scenario_runs`` (one forest.AntSceneForestEngine for all of them), in the same process,
alternating, after warm-up, best of ``--reps``.  The ant network in f16x3, the stand-in model dynamics on the device, H = 48,
early exit, a fixed ``max_candidates`` per run.  The host clock of either form ends in a device synchronise; the node counts
of every run must be equal in both forms.  Prints one JSON line (and writes it to --out).

    timeout -k 10 900 python profiles/ant_scene_forest_probe.py --out out/r08_ant_scene_forest_probe.json
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

from profiles.ant_forest_probe import S_GLOBAL, StaticAntEnv  # noqa: E402

SCENARIOS = os.path.join(REPO, "tests", "golden", "test_scenarios_ant.csv")


def planners(batch, max_candidates):
    from ditreeonlineplanner_amd.planners.RRT import RRT_Planner
    from ditreeonlineplanner_amd.policies.fm_policy import DiffusionSampler
    from ditreeonlineplanner_amd.scenarios import ant_scenarios
    from ditreeonlineplanner_amd.train_diffusion_policy import init_noise_pred_net
    torch.manual_seed(0)
    net = init_noise_pred_net(input_dim=8, action_dim=8, obs_dim=29, obs_history=3, action_history=1, goal_conditioned=True,
                              goal_dim=2, local_map_conditioned=True, local_map_encoder="resnet", local_map_embedding_dim=400,
                              local_map_size=16, down_dims=[512, 1024, 2048])
    smp = DiffusionSampler(net, None, "antmaze", policy="flow_matching", pred_horizon=16, action_dim=8, prediction_type="actions",
                           obs_history=3, action_history=1, goal_conditioned=True, num_diffusion_iters=1, local_map_size=16)
    out = []
    for sc in ant_scenarios(SCENARIOS, s_global=S_GLOBAL):
        env = StaticAntEnv(sc["maze"], sc["goal"][:2] + np.array([0.3, -0.2]))
        out.append(RRT_Planner(sc["start"], sc["goal"], env_id="antmaze", environment=env, sampler=smp, prediction_type="actions",
                               action_horizon=2, local_map_size=16, local_map_scale=0.8, global_map_scale=S_GLOBAL,
                               goal_conditioning_bias=0.85, prop_duration=[48], time_budget=600, verbose=False, batch=batch,
                               max_candidates=max_candidates, capacity=1024, ant_dynamics="model", early_exit=True))
    return out


def one_by_one(pls, seeds):
    """The scenario set as one plan_runs call per scenario."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    nodes = [[r["number_of_nodes"] for r in pl.plan_runs(seeds)] for pl in pls]
    torch.cuda.synchronize()
    return time.perf_counter() - t0, nodes


def scene_forest(pls, seeds):
    from ditreeonlineplanner_amd.planners.RRT import plan_ant_scenario_runs
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    runs = plan_ant_scenario_runs(pls, [seeds] * len(pls))
    torch.cuda.synchronize()
    return time.perf_counter() - t0, [[r["number_of_nodes"] for r in rs] for rs in runs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--seeds", type=int, default=4)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--max-candidates", type=int, default=96)
    a = ap.parse_args()
    pls = planners(a.batch, a.max_candidates)
    seeds = list(range(1000, 1000 + a.seeds))
    scene_forest(pls, seeds)                                    # warm-up: bind, reserve, the forests' slots, first launches
    one_by_one(pls, seeds)
    t_one, t_for, same = [], [], True
    for _ in range(a.reps):
        t, n_one = one_by_one(pls, seeds)
        t_one.append(t)
        t, n_for = scene_forest(pls, seeds)
        t_for.append(t)
        same = same and n_one == n_for
    runs = len(pls) * len(seeds)
    out = {"probe": "ant_scene_forest_probe", "device": torch.cuda.get_device_name(0), "precision": "f16x3", "dynamics": "model",
           "prop_duration": [48], "early_exit": True, "scenarios": len(pls), "seeds_per_scenario": len(seeds), "runs": runs,
           "batch_per_run": a.batch, "max_candidates": a.max_candidates, "plan_runs_per_scenario_s": t_one,
           "scene_forest_s": t_for, "plan_runs_per_scenario_runs_per_s": runs / min(t_one),
           "scene_forest_runs_per_s": runs / min(t_for), "ratio": min(t_one) / min(t_for), "same_node_counts": same,
           "number_of_nodes": n_for}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not same:
        sys.exit("node counts differ between the per-scenario and the scene forest form")


if __name__ == "__main__":
    main()
