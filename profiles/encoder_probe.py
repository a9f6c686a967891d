"""Per-call device time of the local-map encoders at B = 1024 (car, 20 x 20 maps, f16x3 U-Net of down_dims 256 / 512 / 1024:
the encoder's cost does not depend on the U-Net's width).

    rocprofv3 --kernel-trace --stats --output-format csv -d out/enc -o enc -- python profiles/encoder_probe.py --calls 20
    python profiles/encoder_probe.py --summarize out/enc --calls 20 --warmup 2 --out out/encoder_probe.json

The run mode makes `warmup + calls` denoiser calls of 1024 candidates per encoder, all six in one process.  The summary adds up
the rocprofv3 per-kernel totals by the kernels only an encoder launches: enc_* for the five small ones; for 'resnet' the stem,
the implicit Conv2d tiles, the GroupNorm / pooling kernels (its fc layer runs on gemm16_kernel, which the U-Net shares and which
is therefore NOT counted: the ResNet figure is a lower bound).
"""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

B = 1024
ENCODERS = (("resnet", 400), ("identity", 400), ("mlp", 400), ("max", 9), ("grid", 144), ("cnn", 576))
OWN = {"identity": ("enc_identity_kernel",), "mlp": ("enc_mlp_kernel",), "max": ("enc_max_kernel",),
       "grid": ("enc_conv_kernel<0>",), "cnn": ("enc_conv_kernel<1>",),
       "resnet": ("encoder_stem_kernel", "conv2d_small_kernel", "gn2d_kernel", "avgpool2d_kernel")}


def run(calls, warmup):
    from ditreeonlineplanner_amd import _lib
    from ditreeonlineplanner_amd.ops import Context
    from ditreeonlineplanner_amd.train_diffusion_policy import init_noise_pred_net
    ctx = Context(0)
    g = torch.Generator().manual_seed(0)
    noise = torch.randn(B, 64, 2, generator=g).cuda()
    cond = (torch.randn(B, 7, generator=g) * 0.7).cuda()
    lm = ((torch.rand(B, 20, 20, generator=g) < 0.3).float() * 2 - 1).cuda()
    for enc, emb in ENCODERS:
        net = init_noise_pred_net(input_dim=2, action_dim=2, obs_dim=3, obs_history=1, action_history=1, goal_conditioned=True,
                                  goal_dim=2, local_map_conditioned=True, local_map_encoder=enc, local_map_embedding_dim=emb,
                                  local_map_size=20, down_dims=[256, 512, 1024])
        net.bind(ctx, precision=_lib.PREC_F16X3, max_batch=B)
        for _ in range(warmup + calls):
            ctx.denoise(noise, lm, cond, want_actions=False, check_range=False)
        torch.cuda.synchronize()
        print(enc, "done", flush=True)
    ctx.close()


def summarize(path, calls, warmup, out):
    f = glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True)[0]
    per = {e: dict(total_ns=0, launches=0, kernels={}) for e, _ in ENCODERS}
    with open(f) as fh:
        for row in csv.DictReader(fh):
            for enc, names in OWN.items():
                if any(n in row["Name"] for n in names):
                    short = row["Name"].split("(")[0].replace("void ", "")
                    per[enc]["total_ns"] += int(row["TotalDurationNs"])
                    per[enc]["launches"] += int(row["Calls"])
                    per[enc]["kernels"][short] = dict(calls=int(row["Calls"]), avg_ns=float(row["AverageNs"]))
    n = calls + warmup
    res = {"batch": B, "calls_per_encoder": n}
    for enc, d in per.items():
        res[enc] = dict(us_per_call=d["total_ns"] / n / 1e3, launches_per_call=d["launches"] / n, kernels=d["kernels"])
    text = json.dumps(res, indent=1)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--summarize", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize, a.calls, a.warmup, a.out)
    else:
        run(a.calls, a.warmup)
