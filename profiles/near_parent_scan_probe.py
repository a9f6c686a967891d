"""What the near-parent search costs.  A report, not a gate.  One JSON line (and --out).

The near scan (ditree_nn_argmin_near: two passes over the nodes, the second with the cost column and, for the near nodes only,
an FP64 sqrt and a divide) against the plain nearest-node kernel of the same build (ditree_nn_argmin, which this search leaves
untouched), both on the same nodes and queries: 1 024 queries on 10^3, 10^5 and 10^6 nodes spread over a 20 m x 20 m map, radius
0.5 / 1 / 2 m (the share of the tree that is near a query grows with the square of the radius), reach 0.1 m per row.  hip events
around the entry point, the calls alternating, medians of --rounds launches after --warmup.

    timeout -k 10 300 python profiles/near_parent_scan_probe.py --out profiles/near_parent_scan_probe.json
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
sys.path.insert(0, os.path.join(REPO, "profiles"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    from anytime_pruned_probe import timed, us
    from ditreeonlineplanner_amd import _lib
    from ditreeonlineplanner_amd.engine import DeviceTree
    from ditreeonlineplanner_amd.ops import Context
    ctx = Context(0)
    L, h, B = _lib.lib(), ctx._h, 1024
    g = torch.Generator().manual_seed(2)
    rows = []
    for N in (1000, 100000, 1000000):
        t = DeviceTree(ctx, N, 1, 1, cost=True)
        t.xy.copy_((torch.rand(N, 2, generator=g, dtype=torch.float64) * 20 - 10).to(ctx.device))
        t.cost.copy_(torch.randint(1, 2000, (N,), generator=g, dtype=torch.int32).to(ctx.device))
        t.counters[0] = N
        q = (torch.rand(B, 6, generator=g, dtype=torch.float64) * 20 - 10).to(ctx.device)
        idx = torch.zeros(B, dtype=torch.int32, device=ctx.device)
        near = {r: _lib.Near(t.cost.data_ptr(), r, 0.1) for r in (0.5, 1.0, 2.0)}
        calls = {"nearest": lambda: L.ditree_nn_argmin(h, q.data_ptr(), 6, B, t.xy.data_ptr(), N, idx.data_ptr(), None, None, None,
                                                       None, None, None, ctx.stream)}
        for r, nr in near.items():
            calls[f"near_{r}"] = lambda nr=nr: L.ditree_nn_argmin_near(h, C.byref(t.desc), C.byref(nr), None, q.data_ptr(), 6, B, N,
                                                                       idx.data_ptr(), None, None, None, ctx.stream)
        res = us(timed(calls, a.rounds, a.warmup))
        plain = idx.clone()
        L.ditree_nn_argmin(h, q.data_ptr(), 6, B, t.xy.data_ptr(), N, plain.data_ptr(), None, None, None, None, None, None, ctx.stream)
        moved = {}
        for r, nr in near.items():
            L.ditree_nn_argmin_near(h, C.byref(t.desc), C.byref(nr), None, q.data_ptr(), 6, B, N, idx.data_ptr(), None, None, None,
                                    ctx.stream)
            torch.cuda.synchronize()
            moved[f"near_{r}"] = float((idx != plain).float().mean().item())
        base = res["nearest"]["median_us"]
        rows.append(dict(nodes=N, queries=B, near_share_of_map={f"near_{r}": float(np.pi * r * r / 400.0) for r in near},
                         parents_not_nearest=moved, ratio_to_nearest={k: v["median_us"] / base for k, v in res.items()}, **res))
        del t
    out = {"probe": "near_parent_scan_probe", "device": torch.cuda.get_device_name(0), "reach": 0.1,
           "timing": f"hip events around the entry point, alternating, medians of {a.rounds} calls after {a.warmup}", "scan": rows}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
