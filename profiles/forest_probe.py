"""Runs/s of the same seeded runs done one after another (``reset(); plan()`` per seed) and as one forest
(``RRT_Planner.plan_runs``), in the same process, alternating, after warm-up.  `boxes`, the config-2 network in f16x3,
a fixed ``max_candidates`` per run.  Prints one JSON line (and writes it to --out).

    timeout -k 10 900 python profiles/forest_probe.py --out out/r05_forest_probe.json
    rocprofv3 --kernel-trace --stats -d out/forest_rocprof -o forest -- python profiles/forest_probe.py --forest-only
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

# (per-run batch, runs, max_candidates per run)
CASES = {"64x16": (64, 16, 192), "1x256": (1, 256, 2)}


def planner(batch, max_candidates):
    from ditreeonlineplanner_amd.car_env import CarEnv
    from ditreeonlineplanner_amd.planners.RRT import RRT_Planner
    from ditreeonlineplanner_amd.policies.fm_policy import DiffusionSampler
    from ditreeonlineplanner_amd.train_diffusion_policy import init_noise_pred_net
    from oracle import denoiser as OD
    torch.manual_seed(0)
    onet = OD.init_noise_pred_net().eval()
    net = init_noise_pred_net(input_dim=2, action_dim=2, obs_dim=3, obs_history=1, action_history=1, goal_conditioned=True,
                              goal_dim=2, local_map_conditioned=True, local_map_encoder="resnet", local_map_embedding_dim=400,
                              local_map_size=20, down_dims=[512, 1024, 2048])
    net.load_state_dict(onet.state_dict())
    smp = DiffusionSampler(net, None, "carmaze", policy="flow_matching", pred_horizon=64, action_dim=2, prediction_type="actions",
                           obs_history=1, action_history=1, goal_conditioned=True, num_diffusion_iters=1, local_map_size=20).eval()
    maze = np.loadtxt(os.path.join(REPO, "ditreeonlineplanner_amd", "data", "boxes.csv"), delimiter=",")
    env = CarEnv(maze_map=maze, collision_checking=False)
    start = np.array([*env.cell_rowcol_to_xy(np.array([17, 2])), np.deg2rad(45.0), 0.0, 0.0, 0.0])
    goal = np.array([*env.cell_rowcol_to_xy(np.array([2, 17])), 0, 0, 0, 0.0])
    return RRT_Planner(start, goal, env_id="carmaze", environment=env, sampler=smp, action_horizon=8, local_map_size=20,
                       local_map_scale=0.2, global_map_scale=1.0, goal_conditioning_bias=0.85, prop_duration=[64], time_budget=600,
                       batch=batch, max_candidates=max_candidates)


def sequential(pl, seeds):
    nodes = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in seeds:
        random.seed(s)
        np.random.seed(s)
        torch.manual_seed(s)
        pl.reset()
        pl.plan()
        nodes.append(pl.results["number_of_nodes"])
    torch.cuda.synchronize()
    return time.perf_counter() - t0, nodes


def forest(pl, seeds):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    runs = pl.plan_runs(seeds)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, [r["number_of_nodes"] for r in runs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--forest-only", action="store_true", help="only the forest form of the 64 x 16 case (profiler runs)")
    a = ap.parse_args()
    out = {"probe": "forest_probe", "device": torch.cuda.get_device_name(0), "precision": "f16x3", "maze": "boxes",
           "prop_duration": [64], "cases": {}}
    for name, (batch, runs, mc) in CASES.items():
        if a.forest_only and name != "64x16":
            continue
        pl = planner(batch, mc)
        seeds = list(range(1000, 1000 + runs))
        forest(pl, seeds)                                       # warm-up: bind, reserve, the forest's slots, first launches
        if not a.forest_only:
            sequential(pl, seeds[:2])
        ts, tf = [], []
        same = True
        for _ in range(a.reps):
            if not a.forest_only:
                t, n_seq = sequential(pl, seeds)
                ts.append(t)
            t, n_for = forest(pl, seeds)
            tf.append(t)
            if not a.forest_only:
                same = same and n_seq == n_for
        c = {"batch_per_run": batch, "runs": runs, "max_candidates": mc, "forest_s": tf, "forest_runs_per_s": runs / min(tf)}
        if not a.forest_only:
            c.update(sequential_s=ts, sequential_runs_per_s=runs / min(ts), ratio=min(ts) / min(tf), same_node_counts=same)
        out["cases"][name] = c
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
