"""GPU parity of the denoiser at every supported horizon and size, layer by layer (tests/test_gpu_denoiser.py holds `large` at
pred_horizon 64, tests/test_gpu_ant.py the ant's `large` at 16; this module the rest of what the library accepts).

MATRIX -- every tapped layer, `map_emb` and the flow-step output against the fp32 torch oracle of the same configuration,
under the three bounds of tests/test_gpu_denoiser.py (relative L2, max|err| / rms, element-wise with no violation):
  horizons   car `large` at P = 32 / 128 / 256: the tile kernels at L = 128 and 256 (two / one sample per 256-row tile), the
             car network on the SHORT L = 8 epilogue, final_proj_flow_kernel / prep_sample_kernel at those lengths;
  sizes      car small / medium / xlarge at P = 64: the unfused gn1d_kernel / gn1d_short_kernel in every format and
             conv_gemm_kernel with N = 64 / 128 inside a 256-wide tile; `small` refuses the split precisions;
  ant x size ant small / medium / xlarge: L = 8 and 4 with unfused GroupNorm in the 16-bit formats, MODE_BIAS at L = 4.

BOUNDS -- TOL of tests/test_gpu_denoiser.py was measured on `large` at P = 64 and stays the base.  No other configuration has
a measurement, and none may be read off the kernels under test: a configuration's bound is TOL[prec] x scale with
scale = max(1, e(config) / e(base)), e a CPU-only error of the ORACLE, worst over the tapped layers (one scale for the L2
bound, one for the three max-type bounds), base = `large` of the same family (car P = 64, ant P = 16) on inputs drawn the
same way:
  precisions 1, 2, 3 (f32-class): the fp32 oracle against the same oracle in float64 (how much fp32 summation itself moves);
  precisions 0 and 4: the fp32 oracle against a storage-rounded oracle (U-Net weights of >= 2 dimensions, the output of
  every tapped block and of every Mish rounded to bf16 / f16).  It rounds at fewer points than the device and gives about
  half the device's error at `large`: it is a ratio, never a bound.
scale <= 3 is asserted, so a broken emulation cannot quietly widen a bound.  Each scale is printed as a SHAPE_SCALE line.

SELF-CHECK -- at bf16 (the loosest bounds) in every configuration, one layer of each level gets one element overwritten by a
value at least rms away; check_close must report it under the bounds that configuration really uses.

BIT IDENTITY -- see test_new_horizons_are_bit_identical_across_batches."""
import contextlib
import copy
import gc
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle import denoiser as OD
from oracle import geometry as G
from oracle import sampler as OS
from tests.test_gpu_ant import _ant_inputs
from tests.test_gpu_denoiser import LAYERS, OUT, TOL, _make_oracle_net, check_close, err_stats, tap_to_blc
from tests.util import load_maze

pytestmark = pytest.mark.gpu
TAPS = [name for name, _ in LAYERS if name != "enc.pool"]
SCALE_CAP = 3.0
N_IN = 48                                   # input rows drawn per horizon: row b is the same whatever batch it is sliced into

SIZES = {"small": (64, 128, 256), "medium": (256, 512, 1024), "large": (512, 1024, 2048), "xlarge": (1024, 2048, 4096)}
# name -> (family, size, P, B, precisions that run, precisions that are refused)
CONFIGS = {
    "car_large_p32": ("car", "large", 32, 24, (1, 2, 3, 4, 0), ()),
    "car_large_p128": ("car", "large", 128, 5, (1, 2, 3, 4, 0), ()),
    "car_large_p256": ("car", "large", 256, 3, (1, 2, 3, 4, 0), ()),
    "car_small_p64": ("car", "small", 64, 8, (1, 4, 0), (2, 3)),
    "car_medium_p64": ("car", "medium", 64, 8, (1, 2, 3, 4, 0), ()),
    "car_xlarge_p64": ("car", "xlarge", 64, 4, (1, 2, 3, 4, 0), ()),
    "ant_small_p16": ("ant", "small", 16, 24, (1, 4, 0), (2, 3)),
    "ant_medium_p16": ("ant", "medium", 16, 24, (1, 2, 3, 4, 0), ()),
    "ant_xlarge_p16": ("ant", "xlarge", 16, 8, (1, 2, 0), ()),
}
BASE = {"car": ("car", "large", 64, 24), "ant": ("ant", "large", 16, 24)}
MATRIX = [(c, p) for c, v in CONFIGS.items() for p in v[4]]
REFUSED = [(c, p) for c, v in CONFIGS.items() for p in v[5]]
ERR_CLASS = {1: "f64", 2: "f64", 3: "f64", 0: "bf16", 4: "f16"}     # which oracle-side error scales a precision's bounds


# ------------------------------------------------------------------------------------------------ inputs and networks
_INPUTS = {}


def _inputs(family, P):
    """(noise, scaled local map, cond): N_IN seeded rows, drawn as _make_inputs / _ant_inputs draw theirs."""
    key = (family, P)
    if key not in _INPUTS:
        if family == "ant":
            B, noise, lm, cond = _ant_inputs()
            _INPUTS[key] = (noise, lm, cond)
        else:
            g = torch.Generator().manual_seed(5)
            maze = load_maze("boxes").astype(np.float32)
            rng = np.random.default_rng(2)
            poses = np.stack([rng.uniform(-9, 9, N_IN), rng.uniform(-9, 9, N_IN), rng.uniform(-3.1, 3.1, N_IN)], axis=1)
            lm = OS.scale_local_map(G.create_local_map(maze, poses[:, 0], poses[:, 1], poses[:, 2], 20, 0.2, 1.0, (10.0, 10.0)))
            noise = torch.randn(N_IN, P, 2, generator=g)
            cond = torch.randn(N_IN, 7, generator=g) * 0.7
            _INPUTS[key] = (noise, torch.tensor(lm), cond)
    return _INPUTS[key]


def _rows(t3, rows):
    return tuple(t[rows].contiguous() for t in t3)


_NET = {}                                   # one network besides the two `large` ones at a time (xlarge: 690 M parameters)
_LARGE = {}


def _oracle_net(family, size):
    if size == "large":
        if family not in _LARGE:
            _LARGE[family] = _make_oracle_net() if family == "car" else _build_net(family, size, 0)
        return _LARGE[family]
    if (family, size) not in _NET:
        _NET.clear()
        _MEMO.clear()
        gc.collect()
        _NET[(family, size)] = _build_net(family, size, 3)
    return _NET[(family, size)]


def _build_net(family, size, seed):
    torch.manual_seed(seed)
    kw = dict(input_dim=8, action_dim=8, obs_dim=29, obs_history=3, action_history=1) if family == "ant" else {}
    net = OD.init_noise_pred_net(down_dims=SIZES[size], **kw).eval()
    g = torch.Generator().manual_seed(1)      # live FiLM / GroupNorm terms, as _make_oracle_net
    with torch.no_grad():
        for n, p in net.named_parameters():
            if p.dim() == 1:
                p.add_(0.2 * torch.randn(p.shape, generator=g))
    return net


def _device_net(family, size, P):
    from ditreeonlineplanner_amd.model import NoisePredNet
    if family == "ant":
        return NoisePredNet(input_dim=8, additional_global_cond_dim=97, pred_horizon=P, local_map_size=16,
                            down_dims=SIZES[size], init=False)
    return NoisePredNet(down_dims=SIZES[size], pred_horizon=P, init=False)


def _denoise(ctx, family, noise, lm, cond):
    kw = dict(act_norm=np.concatenate([np.zeros(8), np.ones(8)])) if family == "ant" else {}
    return ctx.denoise(noise.cuda().contiguous(), lm.cuda().contiguous(), cond.cuda().contiguous(), want_actions=False, **kw)


# ------------------------------------------------------------------------------------------------ the oracle side
def _time_embedding64(unet):
    """OracleUnet1D.time_embedding casts the timestep to float32: the float64 copy embeds in float64."""
    def emb(timestep, batch):
        t = torch.as_tensor(timestep, dtype=torch.float64).reshape(-1).expand(batch)
        half = unet.dsed // 2
        f = torch.exp(torch.arange(half, dtype=torch.float64) * -(math.log(10000) / (half - 1)))
        e = t[:, None] * f[None, :]
        enc = unet.diffusion_step_encoder._modules
        return enc["3"](torch.nn.functional.mish(enc["1"](torch.cat((e.sin(), e.cos()), dim=-1))))
    return emb


@contextlib.contextmanager
def _rounded_mish(dt):
    """The oracle calls the functional Mish: while this is open its output goes through the storage type."""
    F = torch.nn.functional
    plain = F.mish
    F.mish = lambda x, inplace=False: plain(x).to(dt).to(x.dtype)
    try:
        yield
    finally:
        F.mish = plain


@torch.no_grad()
def _run_with_taps(net, noise, lm, cond, dtype=torch.float32, round_to=None):
    """One flow step (t = 0, dt = 1: oracle/sampler.py flow_sample with k_steps = 1) in `dtype`, with the tapped tensors.
    round_to: every tapped output (and, through _rounded_mish, every Mish) is rounded through that storage type."""
    taps, hooks = {}, []
    mods = dict(net.named_modules())

    def hook(name):
        def h(mod, i, o):
            if round_to is not None:
                o = o.to(round_to).to(o.dtype)
            taps[name] = o.detach()
            return o
        return h
    for name, path in LAYERS:
        if name == "enc.pool":
            continue
        m = mods[path]
        if path.endswith(".2"):
            m = m.conv
        hooks.append(m.register_forward_hook(hook(name)))
    x = noise.to(dtype)
    ts = torch.zeros(x.shape[0], dtype=dtype)
    with _rounded_mish(round_to) if round_to is not None else contextlib.nullcontext():
        v = net(sample=x, local_map=lm.to(dtype), timestep=ts * 20, global_cond=cond.to(dtype))
    for h in hooks:
        h.remove()
    return (x + v).numpy(), {k: t.numpy() for k, t in taps.items()}


_MEMO = {}


def _memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


def _oracle(family, size, P, B):
    """(x1, taps) of the fp32 oracle on the first B input rows: once per configuration, never written to."""
    return _memo(("fp32", family, size, P, B),
                 lambda: _run_with_taps(_oracle_net(family, size), *_rows(_inputs(family, P), slice(0, B))))


def _worst(got, ref):
    """Worst relative L2 and worst max|err| / rms over the tapped layers."""
    st = [err_stats(got[n], ref[n]) for n in TAPS]
    return max(s["rel_l2"] for s in st), max(s["max_norm"] for s in st)


_E = {}


def oracle_error(family, size, P, B, cls):
    """e(config) for an error class: "f64" (fp32 oracle against its float64 copy), "bf16" / "f16" (storage-rounded oracle
    against the fp32 oracle).  CPU only.  xlarge is derived at B = 2, its copy freed at once."""
    if size == "xlarge":
        B = 2
    key = (family, size, P, B, cls)
    if key in _E:
        return _E[key]
    net = _oracle_net(family, size)
    rows = _rows(_inputs(family, P), slice(0, B))
    _, t32 = _oracle(family, size, P, B)
    if cls == "f64":
        n64 = copy.deepcopy(net).double()
        n64.unet.time_embedding = _time_embedding64(n64.unet)
        _, t64 = _run_with_taps(n64, *rows, dtype=torch.float64)
        del n64
        e = _worst(t32, t64)
    else:
        dt = torch.bfloat16 if cls == "bf16" else torch.float16
        nr = copy.deepcopy(net)
        with torch.no_grad():
            for p in nr.unet.parameters():
                if p.dim() >= 2:
                    p.copy_(p.to(dt).float())
        _, tr = _run_with_taps(nr, *rows, round_to=dt)
        del nr
        e = _worst(tr, t32)
    gc.collect()
    _E[key] = e
    return e


def scales(config, prec):
    """(scale of the L2 bound, scale of the max-type bounds) of a configuration: e(config) / e(base), at least 1."""
    family, size, P, B = CONFIGS[config][:4]
    cls = ERR_CLASS[prec]
    ec = oracle_error(family, size, P, B, cls)
    eb = oracle_error(*BASE[family], cls)
    s = (max(1.0, ec[0] / eb[0]), max(1.0, ec[1] / eb[1]))
    print(f"SHAPE_SCALE {config} prec {prec} ({cls}): l2 {s[0]:.3f} max {s[1]:.3f}   e(config) {ec[0]:.3g} {ec[1]:.3g}   "
          f"e(base) {eb[0]:.3g} {eb[1]:.3g}", flush=True)
    return s, ec, eb


def scaled_tol(prec, s):
    t = TOL[prec]
    return dict(l2=t["l2"] * s[0], maxn=t["maxn"] * s[1], atol=t["atol"] * s[1], rtol=t["rtol"] * s[1])


# ------------------------------------------------------------------------------------------------ the tests
@pytest.fixture(scope="module")
def ctx():
    from ditreeonlineplanner_amd.ops import Context
    c = Context(0)
    yield c
    c.close()
    for cache in (_NET, _LARGE, _MEMO, _INPUTS):          # the networks (xlarge: 2.7 GB) do not outlive the module
        cache.clear()
    gc.collect()


def _level_layers():
    return ("d0b1.out", "skip1", "mid2.out")            # one tapped layer of each level: L, L / 2, L / 4


@pytest.mark.parametrize("config,prec", MATRIX)
def test_shape_matrix_layers_and_output(ctx, config, prec):
    family, size, P, B = CONFIGS[config][:4]
    onet = _oracle_net(family, size)
    x_ref, taps = _oracle(family, size, P, B)
    s, ec, eb = scales(config, prec)
    assert max(s) <= SCALE_CAP, (config, prec, s)
    tol = scaled_tol(prec, s)
    net = _device_net(family, size, P)
    net.load_state_dict(onet.state_dict())
    net.bind(ctx, precision=prec, max_batch=B)
    assert ctx.denoise_dims() == ((P, 8, 16, 97, 400) if family == "ant" else (P, 2, 20, 7, 400))
    x = _denoise(ctx, family, *_rows(_inputs(family, P), slice(0, B))).cpu().numpy()
    report, bad, got_all = {}, [], {}
    for name in TAPS:
        got = ctx.debug_read(name, B).cpu().numpy()
        ref = tap_to_blc(taps[name], B)
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        got_all[name] = got
        report[name] = err_stats(got, ref)
        bad += check_close(got, ref, tol, name)
    assert x.shape == x_ref.shape
    report["x1"] = err_stats(x, x_ref)
    bad += check_close(x, x_ref, tol, "x1")
    for name, st in report.items():
        print(f"SHAPE_LAYER {config} prec {prec} {name}: l2 {st['rel_l2']:.3g} maxn {st['max_norm']:.3g} elem {st['rel_elem']:.3g}")
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, f"denoiser_shapes_{config}_prec{prec}.json"), "w") as f:
        json.dump(dict(config=config, precision=prec, batch=B, scale=dict(l2=s[0], max=s[1]), e_config=ec, e_base=eb, tol=tol,
                       layers=report), f, indent=1)
    assert not bad, bad
    if prec == 0:                                        # self-check, under the loosest bounds of the configuration
        rng = np.random.default_rng(7)
        for name in _level_layers():
            got, ref = got_all[name], tap_to_blc(taps[name], B)
            rms = float(np.sqrt(np.mean(ref ** 2)))
            flat = got.reshape(-1).copy()
            for _ in range(1000):
                i, j = rng.integers(0, flat.size, 2)
                if abs(flat[i] - flat[j]) >= rms:
                    break
            assert abs(flat[i] - flat[j]) >= rms
            flat[i] = flat[j]
            assert check_close(flat.reshape(got.shape), ref, tol, name), (config, name, "corruption not detected")


@pytest.mark.parametrize("config,prec", REFUSED)
def test_small_networks_refuse_the_split_precisions(ctx, config, prec):
    """down_dims (64, 128, 256) fit no 256-channel tile, and the hi / lo split exists on those tiles only: a clean error
    that says so, for the car and for the ant, not a fall-back."""
    from ditreeonlineplanner_amd._lib import DitreeError
    family, size, P, B = CONFIGS[config][:4]
    net = _device_net(family, size, P)
    net.load_state_dict(_oracle_net(family, size).state_dict())
    with pytest.raises(DitreeError, match="multiples of 256"):
        net.bind(ctx, precision=prec, max_batch=B)


# (P, matrix batch, rows in front of it in the larger batch).  In front of the batch go other input rows, so that the
# samples land in another tile row and, the count being odd, in another position of their tile at every level.
IDENTITY = [(32, 24, 13), (128, 5, 33), (256, 3, 17)]


@pytest.mark.parametrize("prec", [2, 0])
@pytest.mark.parametrize("P,B,front", IDENTITY)
def test_new_horizons_are_bit_identical_across_batches(ctx, P, B, front, prec):
    """The planner relies on a sample's result not depending on the batch it is part of (early-exit compaction; a forest run
    equal to its sequential run).  At P = 32 / 128 / 256: the same call three times, the first and the last row alone in a
    batch of 1, and the whole batch behind `front` other rows of a larger one (P = 128: rows 33 .. 37 of 38) give equal bits.

    What the code did: the fused GroupNorm epilogues (gemm_epilogue16, and gemm_epilogue of conv_gemm_kernel) added every
    16-row block's partial into the sample's LDS cell with atomicAdd.  Up to pred_horizon 64 of `large` a cell gets the adds
    of one wave in program order, or one add from each of two waves: no order to depend on.  At L >= 128 a sample's rows span
    two or four waves with four adds each, and with a 256-channel group at L = 32 / 64 (`large` at P = 128 / 256, `xlarge` at
    P = 64) both column waves add two or four times: the float sum then depends on the order the adds land in.
    What it does now: at exactly those levels (a uniform branch; every other level keeps its instruction stream) a wave adds
    its blocks in registers, writes a cell of its own, and the cells of a sample are added in index order after the barrier.
    These tests cannot force an interleaving: they guard the fixed order, they do not prove it.  (Measured on MI355X: with
    the atomicAdd form P = 128 and P = 256 failed in both precisions, already at the repeated call; P = 32 has no such
    level and passed.  profiles/r07_denoiser_shapes.json.)"""
    onet = _oracle_net("car", "large")
    net = _device_net("car", "large", P)
    net.load_state_dict(onet.state_dict())
    net.bind(ctx, precision=prec, max_batch=64)           # one reservation for every call below
    inp = _inputs("car", P)
    full = _denoise(ctx, "car", *_rows(inp, slice(0, B))).cpu().numpy()
    assert np.isfinite(full).all()

    def same(a, b):                                       # (the number of differing values, not two tensors, in a failure report)
        return int((a.view(np.uint32) != b.view(np.uint32)).sum()) == 0
    for rep in range(2):
        again = _denoise(ctx, "car", *_rows(inp, slice(0, B))).cpu().numpy()
        assert same(again, full), ("repeated call", rep, int((again != full).sum()))
    for b in (0, B - 1):
        alone = _denoise(ctx, "car", *_rows(inp, slice(b, b + 1))).cpu().numpy()
        assert same(alone[0], full[b]), ("alone", b, int((alone[0] != full[b]).sum()))
    order = list(range(B, B + front)) + list(range(B))
    big = _denoise(ctx, "car", *_rows(inp, order)).cpu().numpy()
    assert same(big[front:], full), ("behind other rows", front, int((big[front:] != full).sum()))
