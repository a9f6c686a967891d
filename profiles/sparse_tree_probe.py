"""What ``sparse_cell`` does to plans, to a tree that fills up, and to the accept's time.  A report, not a gate.  One JSON line
(and --out).

1. The set-up of profiles/near_parent_plan_probe.py -- the car scenarios x --seeds seeds, batch 512, 4 096 candidates, uniform
   actions -- with ``sparse_cell`` None / 0.25 / 0.5 / 1.0 (8 headings) in "anytime" and "anytime_pruned", each with ``near_radius``
   None and 1.  Per setting: runs with a goal path, runs lost or won against None, the mean incumbent cost, nodes and active nodes
   per run, dominated candidates.
2. One long "anytime" run of --long-candidates candidates at ``capacity = 65536``, with and without the kwarg: whether the
   overflow flag (counters[6]) rose, and at which candidate.
3. The sparse accept against ditree_accept_best of the same build on the same synthetic round: B = 512, a tree of 16 384 nodes,
   device events, median of 30 after 5 warm-up, calls alternating.

    timeout -k 10 900 python profiles/sparse_tree_probe.py --out profiles/sparse_tree_probe.json
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

MODES = ("anytime", "anytime_pruned")
CELLS = (None, 0.25, 0.5, 1.0)
RADII = (None, 1.0)


def planner(sc, mode, batch, max_candidates, cell, radius, capacity=None):
    from ditreeonlineplanner_amd.car_env import CarEnv
    from ditreeonlineplanner_amd.planners.RRT import RRT_Planner
    from ditreeonlineplanner_amd.policies.uniform_policy import UniformSampler
    env = CarEnv(maze_map=sc["maze"], collision_checking=False)
    kw = {} if radius is None else dict(near_radius=radius)
    if cell is not None:
        kw["sparse_cell"] = cell
    return RRT_Planner(sc["start"], sc["goal"], env_id="carmaze", environment=env, sampler=UniformSampler(env.action_space, seed=3),
                       action_horizon=8, local_map_size=20, local_map_scale=0.2, global_map_scale=1.0, goal_conditioning_bias=0.85,
                       prop_duration=[64], time_budget=600, batch=batch, max_candidates=max_candidates,
                       capacity=max_candidates + 1 if capacity is None else capacity, emulate_sticky_done=False, solution=mode, **kw)


def seeded(pl, s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)
    pl.reset()
    return pl.plan()


def plans(a, scenarios):
    runs = {}
    for mode in MODES:
        for radius in RADII:
            for cell in CELLS:
                rs = runs[f"{mode}/near={radius}/cell={cell}"] = []
                for i, sc in enumerate(scenarios):
                    pl = planner(sc, mode, a.batch, a.max_candidates, cell, radius)
                    for s in range(a.seeds):
                        t0 = time.perf_counter()
                        seeded(pl, s)
                        r, eng = pl.results, pl._engine
                        g = eng.goal_node
                        rs.append(dict(scenario=i, seed=s, cost=None if g is None else int(eng.tree.cost[g].item()),
                                       nodes=r["number_of_nodes"], active=r.get("active_nodes"), dominated=r.get("dominated_candidates"),
                                       retired=r.get("retired_nodes"), wall_s=time.perf_counter() - t0))
                    del pl
    summary = {}
    for k, rs in runs.items():
        base = runs[k.rsplit("/", 1)[0] + "/cell=None"]
        goal = [x for x in rs if x["cost"] is not None]
        both = [(b["cost"], x["cost"]) for b, x in zip(base, rs) if b["cost"] is not None and x["cost"] is not None]

        def mean(key):
            v = [x[key] for x in rs if x[key] is not None]
            return float(np.mean(v)) if v else None
        summary[k] = {"runs": len(rs), "goal_reached": len(goal),
                      "goal_lost": sum(b["cost"] is not None and x["cost"] is None for b, x in zip(base, rs)),
                      "goal_won": sum(b["cost"] is None and x["cost"] is not None for b, x in zip(base, rs)),
                      "mean_cost": float(np.mean([x["cost"] for x in goal])) if goal else None,
                      "mean_cost_both": [float(np.mean([b for b, _ in both])), float(np.mean([x for _, x in both]))] if both else None,
                      "mean_nodes": mean("nodes"), "mean_active": mean("active"), "mean_dominated": mean("dominated"),
                      "mean_retired": mean("retired"), "mean_wall_s": mean("wall_s")}
    return summary, runs


def long_run(a, sc):
    """-> per setting: nodes, whether counters[6] rose and the candidates drawn when it did (whole rounds)."""
    from ditreeonlineplanner_amd.engine import CNT_OVERFLOW
    out = {}
    for cell in (None, 0.5):
        pl = planner(sc, "anytime", a.batch, a.long_candidates, cell, None, capacity=65536)
        eng = pl._engine
        accept, seen = eng.accept, dict(at=None)

        def watched(B=None, accept=accept, eng=eng, seen=seen):
            cnt = accept(B)
            if seen["at"] is None and int(cnt[CNT_OVERFLOW]):
                seen["at"] = int(cnt[4])
            return cnt
        eng.accept = watched
        t0 = time.perf_counter()
        seeded(pl, 0)
        r = pl.results
        out[f"cell={cell}"] = dict(candidates=int(eng.tree.counters[4].item()), nodes=r["number_of_nodes"], overflow_at=seen["at"],
                                   active=r.get("active_nodes"), dominated=r.get("dominated_candidates"),
                                   cost=None if eng.goal_node is None else int(eng.tree.cost[eng.goal_node].item()),
                                   wall_s=time.perf_counter() - t0)
        del pl, eng
    return out


def accept_timing(ctx, B=512, N=16384, reps=30, warm=5):
    """ditree_accept_sparse against ditree_accept_best on one synthetic round: the same tree, the same candidates, each call on a
    fresh copy of the counters (the tree's slots past N are scratch)."""
    from ditreeonlineplanner_amd import _lib
    from ditreeonlineplanner_amd.engine import ExpansionEngine
    maze = np.zeros((20, 20), dtype=np.float32)
    eng = ExpansionEngine(ctx, maze, np.zeros(6), np.zeros(6), edge_length=64, action_horizon=8, batch=B, capacity=N + 2 * B,
                          emulate_sticky_done=False, solution="anytime", sparse_cell=0.5)
    g = torch.Generator(device="cuda").manual_seed(1)
    t, rb = eng.tree, eng.rb
    t.state[:N].uniform_(-10, 10, generator=g)
    t.xy[:N].copy_(t.state[:N, :2])
    t.cost[:N].copy_(torch.randint(2, 400, (N,), device="cuda", generator=g, dtype=torch.int32))
    t.cost[0] = 1
    rb.parent.copy_(torch.randint(0, N, (B,), device="cuda", generator=g, dtype=torch.int32))
    rb.status.copy_((torch.rand(B, device="cuda", generator=g) < 0.25).int() * 2)
    rb.chunks_run.fill_(eng.n_chunks)
    rb.end_state.uniform_(-10, 10, generator=g)
    rb.states.uniform_(1, 2, generator=g)
    rb.actions.uniform_(1, 2, generator=g)
    start = torch.tensor([N, -1, 0, 0, 0, 0, 0, -1], dtype=torch.int32, device="cuda")
    eng._sparse_roots = [0]
    t.counters.copy_(start)
    eng._sparse_sync()
    table0, stats0 = eng._sparse_table.clone(), t.sparse_stats.clone()
    rd = rb.desc(0, B)
    L, h = _lib.lib(), ctx._h

    def best():
        return L.ditree_accept_best(h, C.byref(t.desc), C.byref(rd), t.cost.data_ptr(), ctx.stream)

    def sparse():
        return L.ditree_accept_sparse(h, C.byref(t.desc), C.byref(rd), t.cost.data_ptr(), None, C.byref(eng._sparse_desc()), ctx.stream)
    times = {"best": [], "sparse": []}
    for k in range(warm + reps):
        for name, call in (("best", best), ("sparse", sparse)):
            t.counters.copy_(start)
            eng._sparse_table.copy_(table0)
            t.sparse_stats.copy_(stats0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = call()
            e1.record()
            torch.cuda.synchronize()
            assert rc == 0, L.ditree_last_error(h)
            if k >= warm:
                times[name].append(e0.elapsed_time(e1))
    return {"B": B, "nodes": N, "reps": reps, "best_ms_median": float(np.median(times["best"])),
            "sparse_ms_median": float(np.median(times["sparse"])), "new_nodes_sparse": int(t.counters[0].item()) - N}


def compact(out):
    """The result with one line per top-level entry and per setting of the summary."""
    def entry(k, v):
        if k == "summary":
            return '"summary": {\n' + ",\n".join(f"  {json.dumps(s)}: {json.dumps(x)}" for s, x in v.items()) + "\n }"
        return f"{json.dumps(k)}: {json.dumps(v)}"
    return "{\n " + ",\n ".join(entry(k, v) for k, v in out.items()) + "\n}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--max-candidates", type=int, default=4096)
    ap.add_argument("--long-candidates", type=int, default=131072)
    ap.add_argument("--seeds", type=int, default=4)
    ap.add_argument("--skip", default="", help="comma list of: plans, long, timing")
    ap.add_argument("--runs", action="store_true", help="--out keeps the per-run records too (thousands of lines)")
    a = ap.parse_args()
    skip = set(a.skip.split(","))
    from ditreeonlineplanner_amd.ops import Context
    from ditreeonlineplanner_amd.scenarios import car_scenarios
    scenarios = car_scenarios()
    out = {"probe": "sparse_tree_probe", "device": torch.cuda.get_device_name(0), "sampler": "UniformSampler(seed=3)",
           "batch": a.batch, "max_candidates": a.max_candidates, "prop_duration": [64], "seeds": list(range(a.seeds)),
           "scenarios": len(scenarios), "sparse_headings": 8}
    if "timing" not in skip:
        ctx = Context(0)
        out["accept_timing"] = accept_timing(ctx)
        ctx.close()
    if "long" not in skip:
        out["long_run"] = long_run(a, scenarios[0])
    if "plans" not in skip:
        out["summary"], runs = plans(a, scenarios)
        if a.runs:
            out["runs"] = runs
    print(json.dumps({k: out[k] for k in ("accept_timing", "long_run", "summary") if k in out}))
    if a.out:
        with open(a.out, "w") as f:
            f.write(compact(out) + "\n")


if __name__ == "__main__":
    main()
