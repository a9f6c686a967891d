"""Runs/s of the same seeded ANT runs (BASELINE config 3) done one after another (``reset(); plan()`` per seed) and as one
forest (``RRT_Planner.plan_runs`` -> forest.AntForestEngine), in the same process, alternating, after warm-up.  `boxes`, the
ant network in f16x3, the stand-in model dynamics on the device, H = 48, a fixed ``max_candidates`` per run.  The host clock
of either form ends in a device synchronise; the node counts of every run must be equal in both forms.  Prints one JSON line
(and writes it to --out).

    timeout -k 10 900 python profiles/ant_forest_probe.py --out out/r06_ant_forest_probe.json
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

# (per-run batch, runs, max_candidates per run); 128 x 16 is one full tile-wave of the ant network (2 048 candidates)
CASES = {"64x16": (64, 16, 192), "1x256": (1, 256, 2), "128x16": (128, 16, 384)}
S_GLOBAL = 4.0


class MazeData:
    def __init__(self, maze, s):
        self.maze_map, self.maze_size_scaling = np.asarray(maze), s
        self.map_length, self.map_width = self.maze_map.shape
        self.x_map_center, self.y_map_center = self.map_width / 2 * s, self.map_length / 2 * s

    def cell_xy_to_rowcol(self, xy):
        return np.array([np.floor((self.y_map_center - xy[1]) / self.maze_size_scaling),
                         np.floor((xy[0] + self.x_map_center) / self.maze_size_scaling)])


class StaticAntEnv:
    """The gym surface the planner touches with on-device dynamics: ``reset`` returns the same desired goal every time (the
    condition under which plan_runs equals the sequential runs); the env is never stepped."""

    def __init__(self, maze, desired):
        self.maze_data = MazeData(maze, S_GLOBAL)
        self.ant_env = self
        self.desired = np.asarray(desired, dtype=np.float64)

    def reset(self, options=None, **kw):
        return {"achieved_goal": np.zeros(2), "desired_goal": self.desired.copy(), "observation": np.zeros(27)}, {}


def planner(batch, max_candidates):
    from ditreeonlineplanner_amd.planners.RRT import RRT_Planner
    from ditreeonlineplanner_amd.policies.fm_policy import DiffusionSampler
    from ditreeonlineplanner_amd.train_diffusion_policy import init_noise_pred_net
    torch.manual_seed(0)
    net = init_noise_pred_net(input_dim=8, action_dim=8, obs_dim=29, obs_history=3, action_history=1, goal_conditioned=True,
                              goal_dim=2, local_map_conditioned=True, local_map_encoder="resnet", local_map_embedding_dim=400,
                              local_map_size=16, down_dims=[512, 1024, 2048])
    smp = DiffusionSampler(net, None, "antmaze", policy="flow_matching", pred_horizon=16, action_dim=8, prediction_type="actions",
                           obs_history=3, action_history=1, goal_conditioned=True, num_diffusion_iters=1, local_map_size=16)
    maze = np.loadtxt(os.path.join(REPO, "ditreeonlineplanner_amd", "data", "boxes.csv"), delimiter=",")
    start = np.zeros(29)
    start[:2] = [-30.0, -30.0]
    start[2], start[3] = 0.75, 1.0
    start[7:15] = np.tile([0.0, 0.87], 4)                        # the stand-in model's rest pose (ank_rest)
    goal = np.zeros(29)
    goal[:2] = [30.0, 30.0]
    env = StaticAntEnv(maze, goal[:2] + np.array([0.3, -0.2]))
    return RRT_Planner(start, goal, env_id="antmaze", environment=env, sampler=smp, prediction_type="actions", action_horizon=2,
                       local_map_size=16, local_map_scale=0.8, global_map_scale=S_GLOBAL, goal_conditioning_bias=0.85,
                       prop_duration=[48], time_budget=600, verbose=False, batch=batch, max_candidates=max_candidates,
                       capacity=1024, ant_dynamics="model")


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
    ap.add_argument("--cases", default=",".join(CASES))
    a = ap.parse_args()
    out = {"probe": "ant_forest_probe", "device": torch.cuda.get_device_name(0), "precision": "f16x3", "maze": "boxes",
           "prop_duration": [48], "dynamics": "model", "cases": {}}
    for name in a.cases.split(","):
        batch, runs, mc = CASES[name]
        pl = planner(batch, mc)
        seeds = list(range(1000, 1000 + runs))
        forest(pl, seeds)                                       # warm-up: bind, reserve, the forest's slots, first launches
        sequential(pl, seeds[:2])
        ts, tf = [], []
        same = True
        for _ in range(a.reps):
            t, n_seq = sequential(pl, seeds)
            ts.append(t)
            t, n_for = forest(pl, seeds)
            tf.append(t)
            same = same and n_seq == n_for
        out["cases"][name] = {"batch_per_run": batch, "runs": runs, "max_candidates": mc, "sequential_s": ts, "forest_s": tf,
                              "sequential_runs_per_s": runs / min(ts), "forest_runs_per_s": runs / min(tf),
                              "ratio": min(ts) / min(tf), "same_node_counts": same}
        print(name, json.dumps(out["cases"][name]), flush=True)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not all(c["same_node_counts"] for c in out["cases"].values()):
        sys.exit("node counts differ between the sequential and the forest form")


if __name__ == "__main__":
    main()
