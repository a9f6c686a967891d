"""GPU: every launch of the denoiser's plan against a storage-rounded float64 restatement of that launch alone.

tests/test_gpu_denoiser.py and tests/test_gpu_denoiser_shapes.py bound each tapped layer end to end: the error at a layer is all
that accumulated above it, so plain bf16 is allowed 1.6e-2 in L2 and 8.5 % of rms per element -- room enough for one wrong
channel-tap in a conv, a truncating store, a FiLM column off by one or a variance over n - 1 (tests/
test_denoiser_launch_ref_host.py shows four such defects passing those bounds).  Here every launch is checked on its own: the
plan's activation buffers all persist after a call and ditree_denoise_debug_read names every one, so the DEVICE'S OWN stored
input(s) of a launch go through tests/denoiser_launch_ref.py (float64, weights rounded as DenoiserState::pack rounds them,
written from oracle/denoiser.py and the storage points of DESIGN 3a, never from a kernel) and the result, rounded to the
output's storage format, is compared with what the device stored.  What remains is fp32 summation order and the odd rounding
flip, whatever the depth of the layer.

ELEMENT BOUND  |got - rnd_storage(ref64)| <= ulp_storage(ref64) + 8 A  for every element.
  A            max |ref32 - ref64| over the launch's output before the storage rounding, ref32 the same restatement in float32
               (with the instantiation's documented Mish formula): what fp32 arithmetic alone does.  8 is the margin for the
               device's other summation order (MFMA trees, the K loop).  Computed from the restatement, never from the device.
  ulp_storage  the distance between neighbouring values of the output's storage format at ref64, i.e. ONE rounding flip:
               2^(floor(log2 |ref|) + 1 - p) with p = 8 (bf16), 11 (f16), 16 (bf16x3), 21 (f16x3), 24 (f32: film, map_emb, x1 in
               every precision).  That is between 2^-p |ref| and 2^(1-p) |ref|; 2^-p |ref| itself is half a step at the bottom
               of a binade and would refuse every flip, the reference's own included.  An f16 plane has nothing finer than its
               subnormal step 2^-24.
  slack        three things debug_read cannot see widen an element's bound, each by what the float64 pass works out for that
               element (storage points), never by a device figure:
               * an unfused GroupNorm launch stores conv + bias and reads it back in place.  The device's stored value is
                 within one storage step + 8 A_conv of rnd_storage(conv64) (A_conv: ref32 against ref64 of the conv alone); that
                 times |d out / d (conv + bias)| is admitted, and A is then float32's effect on the GroupNorm pass alone;
               * the FiLM GEMM's stored input Mish(time embedding | map_emb | cond) has no debug name.  It is known to within
                 8 x what float32 does to the time MLP and to Mish; an element that close to a rounding tie may be stored on
                 either side, and |W| times that spread is admitted for the sample's row;
               * a split value whose lo plane is exactly half a step of hi has two splits with the same sum, and the dropped
                 lo * lo term differs between them by 2 |lo| |w_lo|.  Admitted at the first layer (2 to 8 live columns);
                 with thousands of terms it is far below A.
  f32 format   the float32 pass sums a sample of rows as one running f32 sum over pairs of K, as the f32-input MFMA does
               (v_mfma_f32_32x32x2_f32: K / 2 roundings in a row); a CPU GEMM's short partial sums hide that effect and 8 x its
               error did not hold for the f32 instantiation (a handful of elements of 0.5 M at 9 to 10 x, K = 6144).
FLIP CAP       the share of elements further than 8 A from rnd_storage(ref64) is at most max(8 x the reference's own share, 1e-3);
               the reference's own share is that of rnd_storage(ref32) != rnd_storage(ref64).

Per launch A, both shares, the worst element in ulps and the cap go to denoiser_launches_<config>_prec<p>.json in the GPU tests'
output folder (OUT of tests/test_gpu_denoiser.py; a full run: profiles/denoiser_launches.json).  A failure names the launch, its state-dict layer, (sample, row, channel) of the
worst element and the violations per row position and per channel mod 32: a halo, tile-edge or K-chunk defect each leave their
own pattern there.

CONFIGURATIONS -- B is the smallest batch that crosses a 256-row tile at every level and leaves the last tile ragged.
`xlarge` stays with the end-to-end bounds of test_gpu_denoiser_shapes.py: its float64 weights alone are several GB."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import geometry as G
from oracle import sampler as OS
from tests import denoiser_launch_ref as R
from tests.range_guard_ref import runs_fused
from tests.test_gpu_denoiser import OUT
from tests.test_gpu_denoiser_shapes import _denoise, _device_net, _oracle_net
from tests.util import load_maze

pytestmark = pytest.mark.gpu

# name -> (family, size, P, B, precisions, DITREE_DENOISE_SPLITK)
CONFIGS = {
    "car_large_p64": ("car", "large", 64, 17, (0, 4, 2, 3, 1), None),        # the benchmark's network; 4 / 8 / 16 samples per tile
    "car_large_p16": ("car", "large", 16, 65, (0, 4, 2, 3), None),           # L = 16 / 8 / 4: SHORT epilogue, six-piece L = 4 halo, gemm16 short
    "ant_large_p16": ("ant", "large", 16, 65, (0, 4, 2, 3, 1), None),        # D = 8, 16 x 16 maps, MODE_BIAS at L = 4
    "car_large_p256": ("car", "large", 256, 3, (0, 2), None),                # one sample per tile; GroupNorm cells summed across waves
    "car_medium_p64": ("car", "medium", 64, 17, (0, 4, 2, 3, 1), None),      # unfused gn1d at C = 256 beside fused levels
    "car_small_p64": ("car", "small", 64, 17, (0, 4, 1), None),              # conv_gemm_kernel with N = 64 / 128, everything unfused
    "car_large_p64_splitk": ("car", "large", 64, 1, (2, 3), "1"),            # the split-K instantiations
}
CASES = [(c, p) for c, v in CONFIGS.items() for p in v[4]]

_IN = {}


def _inputs(family, P, B):
    """(noise, scaled local map, cond) of B seeded rows, drawn as the other denoiser tests draw theirs: once per configuration."""
    key = (family, P, B)
    if key not in _IN:
        if family == "ant":
            g = torch.Generator().manual_seed(21)
            noise = torch.randn(B, P, 8, generator=g)
            cond = torch.randn(B, 97, generator=g) * 0.6
            lm = (torch.rand(B, 16, 16, generator=g) < 0.3).float() * 2 - 1
        else:
            g = torch.Generator().manual_seed(5)
            maze = load_maze("boxes").astype(np.float32)
            rng = np.random.default_rng(2)
            poses = np.stack([rng.uniform(-9, 9, B), rng.uniform(-9, 9, B), rng.uniform(-3.1, 3.1, B)], axis=1)
            lm = torch.tensor(OS.scale_local_map(G.create_local_map(maze, poses[:, 0], poses[:, 1], poses[:, 2], 20, 0.2, 1.0, (10.0, 10.0))))
            noise = torch.randn(B, P, 2, generator=g)
            cond = torch.randn(B, 7, generator=g) * 0.7
        _IN[key] = (noise, lm, cond)
    return _IN[key]


@pytest.fixture(scope="module")
def ctx():
    from ditreeonlineplanner_amd.ops import Context
    c = Context(0)
    yield c
    c.close()
    _IN.clear()


def _output_of(launch, bufs):
    if "#" in launch.out:
        base, par = launch.out.split("#")
        return bufs[base][:, (0 if par == "even" else 1)::2]
    return bufs[launch.out]


@pytest.mark.parametrize("config,prec", CASES)
def test_every_launch_against_its_restatement(ctx, config, prec, monkeypatch):
    family, size, P, B, _, splitk = CONFIGS[config]
    fmt = R.PREC_FORMAT[prec]
    onet = _oracle_net(family, size)
    noise, lm, cond = _inputs(family, P, B)
    net = _device_net(family, size, P)
    net.load_state_dict(onet.state_dict())
    net.bind(ctx, precision=prec, max_batch=B)
    if splitk is not None:
        plain = _denoise(ctx, family, noise, lm, cond).cpu()
        monkeypatch.setenv("DITREE_DENOISE_SPLITK", splitk)
    x1 = _denoise(ctx, family, noise, lm, cond).cpu()
    if splitk is not None:
        assert not torch.equal(x1, plain)                                            # (the mode really ran: another summation order)
    plan = R.Plan({k: v.detach() for k, v in onet.state_dict().items()}, P, fmt,
                  fused=lambda cout, L: runs_fused(cout, L, sixteen_bit=fmt != "f32"))
    bufs = {"sample": noise, "local_map": lm, "cond": cond, "timestep": 0.0, "dt": 1.0, "x1": x1}
    for l in plan.launches:
        for name in l.ins + [l.out.split("#")[0]]:
            if name not in bufs:
                bufs[name] = ctx.debug_read(name, B).cpu()
    report, bad = {}, []
    for l in plan.launches:
        exp = R.expected(l, plan, bufs)
        got = _output_of(l, bufs)
        assert got.shape == exp["ref"].shape, (l.name, got.shape, exp["ref"].shape)
        res = R.check_launch(got, exp, l.out_fmt)
        report[l.name] = dict(layer=l.layer, kind=l.kind, buffer=l.out, storage=l.out_fmt, A=res["A"], rms=res["rms"], share_beyond_8A=res["share"],
                              reference_share=res["own"], share_cap=res["cap"], worst_ulps=res["worst_ulps"], max_abs_diff=res["max_abs"],
                              outside_element_bound=res["n_bad"], bound=f"ulp_storage + {R.MARGIN:g} * A" + (" + inner-store slack" if exp["slack"] is not None else ""))
        print(f"LAUNCH {config} prec {prec} {l.name}: A {res['A']:.3g} rms {res['rms']:.3g} share {res['share']:.3g} own {res['own']:.3g} "
              f"cap {res['cap']:.3g} worst {res['worst_ulps']:.3g} ulp max|d| {res['max_abs']:.3g} bad {res['n_bad']}", flush=True)
        if not res["ok"]:
            bad.append(R.describe_failure(l, res, got, exp))
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, f"denoiser_launches_{config}_prec{prec}.json"), "w") as f:
        json.dump(dict(config=config, precision=prec, format=fmt, batch=B, splitk=splitk, margin=R.MARGIN, flip_floor=R.FLIP_FLOOR,
                       launches=report), f, indent=1)
    assert not bad, "\n".join(bad)
