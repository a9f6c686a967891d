"""Wall time of one early-exit round, host code included (the pool scheduler reads one count back per call, so host overhead of
the round code shows here and not in kernel times):

  ant       the round of tests/test_gpu_ant_round.py::test_ant_round_full_size_through_accept -- 4096 candidates, 24 chunks of 2,
            f16x3 ant denoiser, stand-in model dynamics, a 512-node snapshot;
  car       the round of tests/test_gpu_fullsize.py::test_early_exit_round_is_bit_identical -- 512 candidates, 4 chunks of 8, the
            car denoiser, a 256-node snapshot;
  car_tape  the shape of test_round_of_8192_candidates_vs_oracle on its action tape, with early exit: no denoiser, so almost all
            of it is launches and read-backs.

Every round runs without accept, so each repetition starts from the same tree.  time.perf_counter around expand_round plus a
device synchronize.  Prints one JSON line (and writes it to --out).

    timeout -k 10 300 python profiles/round_host_probe.py --out profiles/round_host_probe.json
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


def timed(fn, reps, warmup):
    ms = []
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "p90_ms": float(np.percentile(ms, 90)), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from ditreeonlineplanner_amd.engine import AntExpansionEngine, ExpansionEngine
    from ditreeonlineplanner_amd.model import NoisePredNet
    from ditreeonlineplanner_amd.ops import Context
    from oracle import ant as OA
    from oracle import geometry as G
    from oracle import rrt as ORRT
    from oracle.tapes import ActionTape
    from tests import test_gpu_ant_round as TA
    from tests.test_gpu_fullsize import _free_states
    from tests.util import load_maze
    ctx = Context(0)
    dev = TA.dev
    maze = load_maze("boxes")
    out = {"probe": "round_host_probe", "device": torch.cuda.get_device_name(0), "timing": "perf_counter around expand_round + synchronize"}

    def stats():
        r = ctx.round_stats()
        return [r["denoiser_calls"], r["tile_waves"]]

    # ---- ant
    B, nC, N0 = 4096, 24, 512
    rng = np.random.default_rng(11)
    start = np.zeros(29)
    start[:2], start[2], start[3] = [-30.0, -30.0], 0.75, 1.0
    start[7:15] = np.tile([0.0, OA.AntModel.ank_rest], 4)
    goal = np.zeros(29)
    goal[:2] = [30.0, 30.0]
    TA._bind(ctx, TA.make_ant_net(), 2, B)
    eng = AntExpansionEngine(ctx, maze, start, goal, norm=TA.ant_norm(), batch=B, capacity=B + 600, dynamics="model", early_exit=True)
    _, nodes, _ = TA._model_inputs(N0, 1, seed=12)
    t = eng.tree
    nd = dev(nodes)
    t.state[:N0] = nd
    t.xy[:N0] = nd[:, :2]
    t.parent[:N0] = torch.arange(-1, N0 - 1, device="cuda", dtype=torch.int32).clamp(min=0)
    t.parent[0] = -1
    t.has_prev[1:N0] = 1
    t.last_action[1:N0] = dev(rng.uniform(-1, 1, (N0 - 1, 8)))
    t.hist[:N0] = dev(np.repeat(nodes[:, None, :], 3, axis=1))
    t.hist_n[:N0] = 3
    t.counters[0] = N0
    t.n_nodes_host = N0
    s = np.zeros((B, 29))
    s[:, 0], s[:, 1] = rng.uniform(-40, 40, B), rng.uniform(-40, 40, B)
    c = np.where((rng.random(B) > 0.85)[:, None], s[:, :2], goal[None, :2])
    noise = torch.randn(B, nC, 16, 8, generator=torch.Generator().manual_seed(4)).cuda()
    sd, cd = dev(s), dev(c)
    out["ant"] = timed(lambda: eng.expand_round(sd, cd, noise=noise, accept=False), a.reps, a.warmup)
    st = eng.rb.status[:B].cpu().numpy() & 0xFF
    out["ant"].update(candidates=B, chunks=nC, collided=int((st == 2).sum()), pool_calls_waves=stats())

    # ---- car, with the denoiser
    def car_engine(B, N0, seed, **kw):
        rng = np.random.default_rng(seed)
        nodes = _free_states(rng, maze, N0)
        goal = np.array([*G.cell_rowcol_to_xy([2, 17], maze), 0, 0, 0, 0])
        e = ExpansionEngine(ctx, maze, nodes[0], goal, edge_length=32, action_horizon=8, batch=B, capacity=N0 + B,
                            emulate_sticky_done=False, early_exit=True, **kw)
        nd = dev(nodes)
        e.tree.state[:N0] = nd
        e.tree.xy[:N0] = nd[:, :2]
        e.tree.parent[:N0] = 0
        e.tree.parent[0] = -1
        e.tree.has_prev[:N0] = 1
        e.tree.counters[0] = N0
        e.tree.n_nodes_host = N0
        return e, goal
    B = 512
    NoisePredNet(seed=5).bind(ctx, precision=0, max_batch=B)
    ec, goal = car_engine(B, 256, 8)
    s, c = ORRT.RandomTape(2).draw_round(B, 20, 20, goal)
    noise_c = torch.randn(B, 4, 64, 2, generator=torch.Generator().manual_seed(4)).cuda()
    sc_, cc_ = dev(s), dev(c)
    out["car"] = timed(lambda: ec.expand_round(sc_, cc_, noise=noise_c, accept=False), a.reps, a.warmup)
    st = ec.rb.status[:B].cpu().numpy() & 0xFF
    out["car"].update(candidates=B, chunks=4, collided=int((st == 2).sum()), pool_calls_waves=stats())

    # ---- car, action tape
    B = 8192
    et, goal = car_engine(B, 1024, 7)
    s, c = ORRT.RandomTape(1).draw_round(B, 20, 20, goal)
    acts = dev(np.stack([ActionTape(3).actions(np.arange(B), j) for j in range(4)], axis=1))
    st_, ct_ = dev(s), dev(c)
    out["car_tape"] = timed(lambda: et.expand_round(st_, ct_, inject_actions=acts, accept=False), 10 * a.reps, a.warmup)     # half a millisecond each
    st = et.rb.status[:B].cpu().numpy() & 0xFF
    out["car_tape"].update(candidates=B, chunks=4, collided=int((st == 2).sum()), pool_calls_waves=stats())
    ctx.close()
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
