"""Measure what `reuse_tree` costs and buys on one MI355X -> profiles/tree_reuse_probe.json.

  rebase   `ExpansionEngine.rebase` on trees of 1 024 / 16 384 / 65 536 nodes at edge length 64 (a binary heap of whole edges in
           free cells; node 1 stands in a wall, so its half of the tree goes), device events around the call, median of 25.
  round    one expansion round of the planner's default batch of 512 (f16x3 denoiser, edge length 64) on the same engine.
  mission  one scripted mission on an action tape (the room of tests/test_gpu_tree_reuse.py, a wall inserted after the first
           drive): per re-plan the candidates drawn until its first goal node, with and without `reuse_tree`, the nodes
           reused and dropped, and the largest |car - matched plan row| over x, y, heading, speed.

    python profiles/tree_reuse_probe.py [--out profiles/tree_reuse_probe.json]
"""
import argparse
import json
import os
import random
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def timed(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def heap_tree(eng, n, maze):
    """n nodes, parent (m - 1) // 2, whole edges, every row in a free cell but the state of node 1 (a border cell)."""
    t, dev = eng.tree, eng.ctx.device
    g = torch.Generator(device="cpu").manual_seed(n)
    H, W = maze.shape
    free = torch.as_tensor(np.argwhere(maze == 0), dtype=torch.float64)

    def rows(k):
        rc = free[torch.randint(len(free), (k,), generator=g)]
        s = torch.zeros(k, 6, dtype=torch.float64)
        s[:, 0] = rc[:, 1] + 0.5 - W / 2 + (torch.rand(k, generator=g, dtype=torch.float64) - 0.5) * 0.4
        s[:, 1] = H / 2 - (rc[:, 0] + 0.5) + (torch.rand(k, generator=g, dtype=torch.float64) - 0.5) * 0.4
        s[:, 2] = (torch.rand(k, generator=g, dtype=torch.float64) - 0.5) * 6.28
        return s

    es_cap, ea_cap = t.edge_states.shape[1], t.edge_actions.shape[1]
    t.state[:n] = rows(n).to(dev)
    t.state[1, 0], t.state[1, 1] = 0.5 - W / 2, H / 2 - 0.5                  # cell (0, 0): the border
    t.xy[:n] = t.state[:n, :2]
    t.parent[:n] = ((torch.arange(n) - 1) // 2).to(torch.int32).to(dev)
    t.parent[0] = -1
    for lo in range(0, n, 4096):
        hi = min(n, lo + 4096)
        t.edge_states[lo:hi] = rows((hi - lo) * es_cap).reshape(hi - lo, es_cap, 6).to(dev)
    t.edge_actions[:n] = 0.5
    t.edge_nstates[:n], t.edge_nactions[:n] = es_cap, ea_cap
    t.edge_nstates[0] = t.edge_nactions[0] = 0
    t.has_prev[:n] = 1
    t.counters[0], t.counters[1] = n, -1
    t.n_nodes_host = n


def probe_rebase_and_round(out):
    from ditreeonlineplanner_amd import _lib
    from ditreeonlineplanner_amd.engine import ExpansionEngine
    from ditreeonlineplanner_amd.model import NoisePredNet
    from ditreeonlineplanner_amd.ops import Context
    from oracle import geometry as G
    maze = np.loadtxt(os.path.join(REPO, "ditreeonlineplanner_amd", "data", "boxes.csv"), delimiter=",")
    start = np.array([*G.cell_rowcol_to_xy([17, 2], maze), np.deg2rad(45.0), 0, 0, 0])
    goal = np.array([*G.cell_rowcol_to_xy([2, 17], maze), 0, 0, 0, 0])
    ctx = Context(0)
    B = 512
    torch.manual_seed(0)
    net = NoisePredNet()
    net.bind(ctx, precision=_lib.PREC_F16X3, max_batch=B)
    eng = ExpansionEngine(ctx, maze, start, goal, edge_length=64, action_horizon=8, batch=B, capacity=65536,
                          emulate_sticky_done=False)
    dev = ctx.device
    out["rebase_ms"] = {}
    for n in (1024, 16384, 65536):
        heap_tree(eng, n, maze)
        kept = []

        def once():
            kept.append(eng.rebase(0))
            eng.tree, eng._spare_tree = eng._spare_tree, eng.tree            # back to the full tree for the next run
            eng.tree.n_nodes_host = n

        once()
        ms = timed(once, 25)
        out["rebase_ms"][str(n)] = dict(median=statistics.median(ms), min=min(ms), max=max(ms), kept=kept[-1][0],
                                        dropped=kept[-1][1], runs=len(ms))
    # one round of 512 candidates on the 16 384-node tree (the accept appends: the size barely moves over the timed rounds)
    heap_tree(eng, 16384, maze)
    g = torch.Generator().manual_seed(1)
    s = torch.zeros(B, 6, dtype=torch.float64)
    s[:, 0], s[:, 1] = (torch.rand(B, generator=g) - 0.5) * 18, (torch.rand(B, generator=g) - 0.5) * 18
    s, c = s.to(dev), s[:, :2].contiguous().to(dev)
    noise = torch.randn(B, eng.n_chunks, eng.P, 2, generator=g).to(dev)
    for _ in range(3):
        eng.expand_round(s, c, noise=noise)
    ms = timed(lambda: eng.expand_round(s, c, noise=noise), 20)
    out["round_ms"] = dict(batch=B, edge_length=64, median=statistics.median(ms), min=min(ms), max=max(ms), runs=len(ms),
                           note="this build; the round path is the parent commit's, unchanged")
    ctx.close()


def probe_mission(out):
    from tests.test_gpu_tree_reuse import SEED, drive, planner, walled
    out["mission"] = {}
    for reuse in (False, True):
        pl = planner(reuse_tree=reuse, max_candidates=16 * 16)
        random.seed(SEED), np.random.seed(SEED), torch.manual_seed(SEED)
        plans, worst = [], 0.0
        path, actions = pl.plan()
        plans.append(dict(first_solution_candidates=pl.results["first_solution_candidates"], nodes=pl.results["number_of_nodes"]))
        start = pl.test_start
        for step in range(3):
            if path is None or len(actions) < 4:
                break
            pl.test_start = start
            car = drive(pl, actions, 3)
            worst = max(worst, float(np.abs(path[:, :4].astype(np.float64) - car[:4]).max(axis=1).min()))   # the nearest row
            if step == 0:
                pl.update_maze(walled())
            pl.reset(start_state=car, goal_state=pl.test_goal)
            rec = dict(reused_nodes=pl.results.get("reused_nodes", 0), dropped_nodes=pl.results.get("dropped_nodes", 0))
            path, actions = pl.plan()
            rec.update(first_solution_candidates=pl.results["first_solution_candidates"], nodes=pl.results["number_of_nodes"],
                       iterations=pl.results["iterations"], goal=pl._engine.goal_node is not None)
            plans.append(rec)
            start = car
        out["mission"]["reuse_tree" if reuse else "reset"] = dict(plans=plans, max_abs_dev_car_vs_f32_plan_row=worst,
                                                                  reuse_tol=pl.reuse_tol)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tree_reuse_probe.json"))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0)}
    probe_rebase_and_round(res)
    probe_mission(res)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
