"""What ``solution="anytime_pruned"`` costs and buys.  A report, not a gate.  Four parts, one JSON line (and --out):

  scan     the masked nearest-node search (ditree_nn_argmin_bounded) against the unmasked kernel of the same build
           (ditree_nn_argmin), 1 024 queries on 1 024 / 16 384 / 65 536 nodes with no, half and nine tenths of the nodes
           closed; hip events around the entry point, medians, the two alternating;
  accept   ditree_accept_bounded -- without an incumbent, and with one that prunes about half of the round -- against
           ditree_accept_best on the round of profiles/accept_phase_probe.py, alternating;
  read     the per-round counter read-back with and without the stats row behind it (host clock, medians);
  quality  the path-quality table of profiles/solution_modes_probe.py with the fourth mode: the same scenarios, seeds, sampler
           and budgets, plus nodes appended, candidates pruned and runs exhausted.

    timeout -k 10 600 python profiles/anytime_pruned_probe.py --out profiles/anytime_pruned_probe.json
"""
import argparse
import ctypes as C
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

MODES = ("first", "best_of_round", "anytime", "anytime_pruned")


def timed(calls, rounds, warmup, before=None):
    """``calls``: name -> callable returning the entry point's code; alternating; -> name -> list of ms."""
    from ditreeonlineplanner_amd import _lib
    ms = {k: [] for k in calls}
    for i in range(warmup + rounds):
        for name, call in calls.items():
            if before is not None:
                before(name)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = call()
            e1.record()
            torch.cuda.synchronize()
            if rc != 0:
                raise _lib.DitreeError(f"{name} failed ({rc})")
            if i >= warmup:
                ms[name].append(e0.elapsed_time(e1))
    return ms


def us(ms):
    return {k: {"median_us": float(np.median(v) * 1e3), "min_us": float(np.min(v) * 1e3)} for k, v in ms.items()}


def scan_part(ctx, rounds, warmup):
    from ditreeonlineplanner_amd import _lib
    from ditreeonlineplanner_amd.engine import DeviceTree
    L, h, B = _lib.lib(), ctx._h, 1024
    g = torch.Generator().manual_seed(2)
    out = []
    for N in (1024, 16384, 65536):
        t = DeviceTree(ctx, N + 1, 1, 1, cost=True, key=True)
        t.xy.copy_((torch.rand(N + 1, 2, generator=g, dtype=torch.float64) * 20 - 10).to(ctx.device))
        q = (torch.rand(B, 6, generator=g, dtype=torch.float64) * 20 - 10).to(ctx.device)
        idx = torch.zeros(B, dtype=torch.int32, device=ctx.device)
        t.cost[N] = 100                                                          # the incumbent: the slot behind the scanned nodes
        t.counters[0], t.counters[1] = N, N
        bd = _lib.Bound(t.cost.data_ptr(), t.key.data_ptr(), None, 0.5, 0.1, None)
        for share in (0.0, 0.5, 0.9):
            closed = torch.rand(N + 1, generator=g) < share
            t.key.copy_(torch.where(closed, 100, 99).to(torch.int32).to(ctx.device))
            calls = {"unmasked": lambda: L.ditree_nn_argmin(h, q.data_ptr(), 6, B, t.xy.data_ptr(), N, idx.data_ptr(), None, None, None,
                                                            None, None, None, ctx.stream),
                     "masked": lambda: L.ditree_nn_argmin_bounded(h, C.byref(t.desc), C.byref(bd), q.data_ptr(), 6, B, N,
                                                                  idx.data_ptr(), None, None, None, ctx.stream)}
            out.append(dict(nodes=N, queries=B, closed_share=share, **us(timed(calls, rounds, warmup))))
    return out


def accept_part(ctx, rounds, warmup):
    import bench
    from ditreeonlineplanner_amd import _lib
    from ditreeonlineplanner_amd.engine import CNT_GOAL, CNT_NODES, STATS_ROOT, ExpansionEngine
    B, N0 = 1024, bench.N0
    maze = bench.load_maze("boxes")
    nodes, goal, samples, cond, _ = bench.synth_inputs(maze, B)
    dev = ctx.device
    eng = ExpansionEngine(ctx, maze, nodes[0], goal, edge_length=bench.H, action_horizon=bench.A, pred_horizon=bench.P, batch=B,
                          capacity=N0 + B + 1, emulate_sticky_done=False, solution="anytime_pruned")
    t = eng.tree
    nd = torch.as_tensor(nodes, device=dev)
    t.state[:N0] = nd
    t.xy[:N0] = nd[:, :2]
    t.parent[:N0] = torch.arange(-1, N0 - 1, device=dev, dtype=torch.int32).clamp(min=0)
    t.parent[0] = -1
    t.has_prev[1:N0] = 1
    t.cost[:N0] = torch.arange(1, N0 + 1, device=dev, dtype=torch.int32)
    inc = N0 + B                                                                  # an incumbent slot no round writes
    t.cost[inc] = N0 // 2
    t.counters[CNT_NODES] = N0
    t.n_nodes_host = N0
    eng._bound_sync()
    L, h, td = _lib.lib(), ctx._h, C.byref(t.desc)
    _lib.check(h, L.ditree_bound_keys(h, td, C.byref(eng.bound), 0, N0, 0, ctx.stream), "bound_keys")
    g = torch.Generator().manual_seed(1)
    acts = torch.stack([torch.rand(B, bench.H // bench.A, bench.P, generator=g, dtype=torch.float64) * 15.0 - 5.0,
                        torch.rand(B, bench.H // bench.A, bench.P, generator=g, dtype=torch.float64) * 0.8 - 0.4], dim=3)
    eng.expand_round(torch.as_tensor(samples, device=dev), torch.as_tensor(cond, device=dev), inject_actions=acts.to(dev), accept=False)
    status = eng.rb.status[:B].cpu().numpy() & 0xFF
    rd = eng.rb.desc(0, B)
    root = torch.as_tensor(STATS_ROOT, device=dev)
    after = {}

    def before(name):
        t.counters[CNT_NODES] = N0
        t.counters[CNT_GOAL] = inc if name == "accept_bounded_incumbent" else -1
        t.num_visit.zero_()
        t.stats.copy_(root)
    calls = {"accept_best": lambda: L.ditree_accept_best(h, td, C.byref(rd), t.cost.data_ptr(), ctx.stream),
             "accept_bounded_no_incumbent": lambda: L.ditree_accept_bounded(h, td, C.byref(rd), C.byref(eng.bound), ctx.stream),
             "accept_bounded_incumbent": lambda: L.ditree_accept_bounded(h, td, C.byref(rd), C.byref(eng.bound), ctx.stream)}
    ms = timed(calls, rounds, warmup, before)
    for name, call in calls.items():
        before(name)
        call()
        torch.cuda.synchronize()
        after[name] = {"nodes_appended": int(t.counters[CNT_NODES].item()) - N0,
                       "pruned": int(t.stats[3].item()) if name != "accept_best" else 0}
    # the per-round read-back: 8 counters, or the 12 ints of counters + stats row, one copy either way
    plain = ExpansionEngine(ctx, maze, nodes[0], goal, edge_length=bench.H, action_horizon=bench.A, pred_horizon=bench.P, batch=8,
                            capacity=16, emulate_sticky_done=False, solution="anytime")
    read = {}
    for name, tr in (("counters_8_ints", plain.tree), ("counters_and_stats_12_ints", t)):
        ts = []
        for _ in range(300):
            t0 = time.perf_counter()
            tr.read_counters()
            ts.append(time.perf_counter() - t0)
        read[name] = {"median_us": float(np.median(ts[50:]) * 1e6)}
    return dict(candidates=B, tree_nodes=N0, edge_length=bench.H,
                round={"ok": int((status == 0).sum()), "goal": int((status == 1).sum()), "collided": int((status == 2).sum())},
                result=after, **us(ms)), read


def quality_part(batch, max_candidates, seeds):
    import solution_modes_probe as SMP
    from ditreeonlineplanner_amd.scenarios import car_scenarios
    scenarios = car_scenarios()
    runs = {m: [] for m in MODES}
    for sc in scenarios:
        for mode in MODES:
            pl = SMP.planner(sc, mode, batch, max_candidates)
            for s in range(seeds):
                random.seed(s)
                np.random.seed(s)
                torch.manual_seed(s)
                pl.reset()
                t0 = time.perf_counter()
                pl.plan()
                r = pl.results
                runs[mode].append(dict(goal=pl._engine.goal_node is not None, path=r["path"] is not None,
                                       path_time=r.get("path_time") if r["path"] is not None else None, solutions=r["solutions"],
                                       nodes=r["number_of_nodes"], candidates=int(pl._engine.tree.counters[4].item()),
                                       pruned=r.get("pruned_candidates", 0), closed=r.get("closed_nodes", 0),
                                       exhausted=bool(r.get("bound_exhausted", False)), wall_s=time.perf_counter() - t0))
            del pl
    out = {}
    for mode in MODES:
        rs = runs[mode]
        reached = [x["path_time"] for x in rs if x["goal"]]
        out[mode] = {"runs": len(rs), "success": float(np.mean([x["path"] for x in rs])), "goal_reached": len(reached) / len(rs),
                     "mean_path_time": float(np.mean(reached)) if reached else None,
                     "mean_solutions": float(np.mean([x["solutions"] for x in rs])),
                     "mean_nodes": float(np.mean([x["nodes"] for x in rs])),
                     "mean_nodes_goal_runs": float(np.mean([x["nodes"] for x in rs if x["goal"]])) if reached else None,
                     "mean_candidates": float(np.mean([x["candidates"] for x in rs])),
                     "mean_pruned_goal_runs": float(np.mean([x["pruned"] for x in rs if x["goal"]])) if reached else None,
                     "mean_closed_goal_runs": float(np.mean([x["closed"] for x in rs if x["goal"]])) if reached else None,
                     "runs_exhausted": int(sum(x["exhausted"] for x in rs)), "mean_wall_s": float(np.mean([x["wall_s"] for x in rs]))}
    # run by run: where the pruned mode's path differs from plain anytime's
    pairs = [(a["path_time"], b["path_time"]) for a, b in zip(runs["anytime"], runs["anytime_pruned"]) if a["goal"] and b["goal"]]
    out["pruned_vs_anytime"] = {"shorter": sum(b < a for a, b in pairs), "equal": sum(b == a for a, b in pairs),
                                "longer": sum(b > a for a, b in pairs)}
    return len(scenarios), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--max-candidates", type=int, default=4096)
    ap.add_argument("--seeds", type=int, default=3)
    a = ap.parse_args()
    from ditreeonlineplanner_amd.ops import Context
    ctx = Context(0)
    out = {"probe": "anytime_pruned_probe", "device": torch.cuda.get_device_name(0),
           "timing": "hip events around the entry point, alternating, medians of --rounds calls"}
    out["scan"] = scan_part(ctx, a.rounds, a.warmup)
    out["accept"], out["read"] = accept_part(ctx, a.rounds, a.warmup)
    n, q = quality_part(a.batch, a.max_candidates, a.seeds)
    out["quality"] = dict(scenarios=n, sampler="UniformSampler(seed=3)", batch=a.batch, max_candidates=a.max_candidates,
                          prop_duration=[64], seeds=list(range(a.seeds)), bound_speed=5.0, modes=q)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
