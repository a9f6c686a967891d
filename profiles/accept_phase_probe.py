"""Device time of the accept phase of one round of 1024 candidates on the benchmark's tree (bench.py: boxes, a 1024-node
snapshot, edge length 32): ``ditree_accept`` (scan + commit) and, where the library has it, ``ditree_accept_best`` (scan +
commit + pick) on the SAME expanded round, alternating, events around the entry point alone (no counter read-back).  The
round is expanded once on seeded uniform actions (the accept does not care where the actions came from); before every
timed call the counters and visit counts go back to the snapshot's.  Prints one JSON line (and writes it to --out).

    timeout -k 10 300 python profiles/accept_phase_probe.py --out profiles/r11_accept_phase_probe.json
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import bench
    from ditreeonlineplanner_amd import _lib
    from ditreeonlineplanner_amd.engine import CNT_GOAL, CNT_NODES, ExpansionEngine
    from ditreeonlineplanner_amd.ops import Context
    B, N0 = 1024, bench.N0
    maze = bench.load_maze("boxes")
    nodes, goal, samples, cond, _ = bench.synth_inputs(maze, B)
    ctx = Context(0)
    dev = ctx.device
    best = "ditree_accept_best" in _lib.SIGNATURES
    kw = dict(edge_length=bench.H, action_horizon=bench.A, pred_horizon=bench.P, batch=B, capacity=N0 + B, emulate_sticky_done=False)
    eng = ExpansionEngine(ctx, maze, nodes[0], goal, **(dict(kw, solution="anytime") if best else kw))
    t = eng.tree
    nd = torch.as_tensor(nodes, device=dev)
    t.state[:N0] = nd
    t.xy[:N0] = nd[:, :2]
    t.parent[:N0] = torch.arange(-1, N0 - 1, device=dev, dtype=torch.int32).clamp(min=0)
    t.parent[0] = -1
    t.has_prev[1:N0] = 1
    if best:
        t.cost[:N0] = torch.arange(1, N0 + 1, device=dev, dtype=torch.int32)       # the chain's costs grow with the index

    def reset_tree():
        t.counters[CNT_NODES] = N0
        t.counters[CNT_GOAL] = -1
        t.num_visit.zero_()
    reset_tree()
    t.n_nodes_host = N0
    g = torch.Generator().manual_seed(1)
    acts = torch.stack([torch.rand(B, bench.H // bench.A, bench.P, generator=g, dtype=torch.float64) * 15.0 - 5.0,
                        torch.rand(B, bench.H // bench.A, bench.P, generator=g, dtype=torch.float64) * 0.8 - 0.4], dim=3)
    eng.expand_round(torch.as_tensor(samples, device=dev), torch.as_tensor(cond, device=dev), inject_actions=acts.to(dev),
                     accept=False)
    status = eng.rb.status[:B].cpu().numpy() & 0xFF
    rd = eng.rb.desc(0, B)
    h, L, td = ctx._h, _lib.lib(), C.byref(t.desc)
    calls = {"accept": lambda: L.ditree_accept(h, td, C.byref(rd), 0, ctx.stream)}
    if best:
        calls["accept_best"] = lambda: L.ditree_accept_best(h, td, C.byref(rd), t.cost.data_ptr(), ctx.stream)
    ms = {k: [] for k in calls}
    nodes_after = {}
    for i in range(a.warmup + a.rounds):
        for name, call in calls.items():                                           # alternating
            reset_tree()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(h, call(), name)
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                ms[name].append(e0.elapsed_time(e1))
            nodes_after[name] = int(t.counters[CNT_NODES].item()) - N0
    out = {"probe": "accept_phase_probe", "device": torch.cuda.get_device_name(0), "candidates": B, "tree_nodes": N0,
           "edge_length": bench.H, "rounds": a.rounds, "timing": "hip events around the entry point, one call per pair",
           "round": {"ok": int((status == 0).sum()), "goal": int((status == 1).sum()), "collided": int((status == 2).sum())},
           "nodes_appended": nodes_after,
           "median_us": {k: float(np.median(v) * 1e3) for k, v in ms.items()},
           "min_us": {k: float(np.min(v) * 1e3) for k, v in ms.items()},
           "p90_us": {k: float(np.percentile(v, 90) * 1e3) for k, v in ms.items()}}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
