"""GPU parity: MFMA denoiser (encoder + FiLM U-Net + flow step) against the torch-CPU fp32 oracle.

Every instantiation (include/ditree.h DITREE_PREC_*) is held to three bounds per tapped layer and on the output, set at
about twice what profiles/r02_denoiser_precision_report.json records on MI355X (TOL below):
  * relative L2 over the tensor;
  * max |err| / rms(ref)  -- one wrong element in a layer (an O(1) error) breaks this by orders of magnitude;
  * element-wise  |got - ref| <= atol * rms(ref) + rtol * |ref|  with NO violation allowed.
The oracle's U-Net half is bit-identical to the reference class (tests/golden/network.npz);
its ResNet-18-GN half is restated from the torchvision topology: parity unpinned there."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import denoiser as OD
from oracle import sampler as OS
from tests.util import REPO, load_maze

pytestmark = pytest.mark.gpu
OUT = os.path.join(REPO, "gpurun_out")


def rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


# precision -> (rel L2, max|err| / rms(ref), element-wise atol (x rms), rtol)
TOL = {   # measured (worst tapped layer): see profiles/r02_denoiser_precision_report.json
    1: dict(l2=4e-6, maxn=5e-5, atol=2.5e-5, rtol=2.5e-5),    # f32 MFMA: 1.7e-6 / 2.3e-5 / 1.1e-5 (summation order only)
    2: dict(l2=3e-6, maxn=3e-5, atol=2e-5, rtol=2e-5),        # f16 x3: 1.2e-6 / 1.3e-5 / 7.5e-6 (f32-class)
    3: dict(l2=3e-5, maxn=2e-4, atol=1.8e-4, rtol=1.8e-4),    # bf16 x3: 1.4e-5 / 9.7e-5 / 9.2e-5 (16 significand bits, encoder split too)
    4: dict(l2=2e-3, maxn=1.4e-2, atol=1e-2, rtol=1e-2),      # plain f16: 9.4e-4 / 6.9e-3 / 5.0e-3 (11 bits)
    0: dict(l2=1.6e-2, maxn=1.1e-1, atol=8.5e-2, rtol=8.5e-2),  # plain bf16: 7.8e-3 / 5.3e-2 / 4.1e-2 (8 bits)
}
PRECS = sorted(TOL)


def err_stats(got, ref):
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    d = np.abs(got - ref)
    rms = float(np.sqrt(np.mean(ref ** 2)) + 1e-30)
    return dict(rel_l2=float(np.linalg.norm(got - ref) / (np.linalg.norm(ref) + 1e-30)), max_norm=float(d.max() / rms),
                rms=rms, rel_elem=float((d / (np.abs(ref) + rms)).max()))


def check_close(got, ref, tol, what):
    """-> list of violated bounds (empty = pass)."""
    st = err_stats(got, ref)
    bad = []
    if not st["rel_l2"] < tol["l2"]:
        bad.append(f"{what}: rel L2 {st['rel_l2']:.3g} >= {tol['l2']}")
    if not st["max_norm"] < tol["maxn"]:
        bad.append(f"{what}: max|err|/rms {st['max_norm']:.3g} >= {tol['maxn']}")
    d = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64))
    viol = int((d > tol["atol"] * st["rms"] + tol["rtol"] * np.abs(ref)).sum())
    if viol or not np.isfinite(d).all():
        bad.append(f"{what}: {viol} element(s) outside atol*rms + rtol*|ref|")
    return bad


def tap_to_blc(ref, B):
    if ref.ndim == 2:
        return ref.reshape(B, 1, -1)
    if ref.ndim == 4:                                                                        # (B,C,H,W) -> (B,HW,C)
        return np.transpose(ref.reshape(B, ref.shape[1], -1), (0, 2, 1))
    return np.transpose(ref, (0, 2, 1))                                                      # (B,C,L) -> (B,L,C)


def _make_oracle_net():
    torch.manual_seed(0)
    net = OD.init_noise_pred_net().eval()
    # default init leaves the FiLM / GN parameters trivial; perturb so every epilogue term is exercised
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for n, p in net.named_parameters():
            if p.dim() == 1:
                p.add_(0.2 * torch.randn(p.shape, generator=g))
    return net


@pytest.fixture(scope="module")
def oracle_net():
    return _make_oracle_net()


@pytest.fixture(scope="module")
def inputs():
    return _make_inputs()


def _make_inputs():
    g = torch.Generator().manual_seed(5)
    B = 24
    from oracle import geometry as G
    maze = load_maze("boxes").astype(np.float32)
    rng = np.random.default_rng(2)
    poses = np.stack([rng.uniform(-9, 9, B), rng.uniform(-9, 9, B), rng.uniform(-3.1, 3.1, B)], axis=1)
    lm = OS.scale_local_map(G.create_local_map(maze, poses[:, 0], poses[:, 1], poses[:, 2], 20, 0.2, 1.0, (10.0, 10.0)))
    noise = torch.randn(B, 64, 2, generator=g)
    cond = torch.randn(B, 7, generator=g) * 0.7
    return noise, torch.tensor(lm), cond


@pytest.fixture(scope="module")
def ctx():
    from ditreeonlineplanner_amd.ops import Context
    c = Context(0)
    yield c
    c.close()


def _bind(ctx, oracle_net, prec, B):
    from ditreeonlineplanner_amd.model import NoisePredNet
    net = NoisePredNet(init=False)
    net.load_state_dict(oracle_net.state_dict())
    net.bind(ctx, precision=prec, max_batch=B)
    return net


LAYERS = [  # (engine buffer, oracle module path)
    ("enc.pool", "encoder.resnet18.bn1"),            # placeholder path: replaced below by a functional tap
    ("enc.l1.0.out", "encoder.resnet18.layer1.0"), ("enc.l1.1.out", "encoder.resnet18.layer1.1"),
    ("enc.l2.0.out", "encoder.resnet18.layer2.0"), ("enc.l2.1.out", "encoder.resnet18.layer2.1"),
    ("enc.l3.0.out", "encoder.resnet18.layer3.0"), ("enc.l3.1.out", "encoder.resnet18.layer3.1"),
    ("enc.l4.0.out", "encoder.resnet18.layer4.0"), ("enc.l4.1.out", "encoder.resnet18.layer4.1"),
    ("map_emb", "encoder"), ("d0b1.out", "unet.down_modules.0.0"), ("skip0", "unet.down_modules.0.1"),
    ("d1.in", "unet.down_modules.0.2"), ("d1b1.out", "unet.down_modules.1.0"), ("skip1", "unet.down_modules.1.1"),
    ("d2.in", "unet.down_modules.1.2"), ("d2b1.out", "unet.down_modules.2.0"), ("skip2", "unet.down_modules.2.1"),
    ("mid1.out", "unet.mid_modules.0"), ("mid2.out", "unet.mid_modules.1"), ("u0b1.out", "unet.up_modules.0.0"),
    ("u0b2.out", "unet.up_modules.0.1"), ("up0.out", "unet.up_modules.0.2"), ("u1b1.out", "unet.up_modules.1.0"),
    ("u1b2.out", "unet.up_modules.1.1"), ("final.in", "unet.up_modules.1.2"),
]


_ORACLE_MEMO = {}


def memo(key, fn):
    """The oracle side of a test does not depend on the instantiation under test: computed once per module run."""
    if key not in _ORACLE_MEMO:
        _ORACLE_MEMO[key] = fn()
    return _ORACLE_MEMO[key]


def _oracle_with_taps(net, noise, lm, cond):
    return memo(("taps", id(net), tuple(noise.shape)), lambda: _oracle_with_taps_compute(net, noise, lm, cond))


def _oracle_with_taps_compute(net, noise, lm, cond):
    taps = {}
    hooks = []
    mods = dict(net.named_modules())
    for name, path in LAYERS:
        if name == "enc.pool":
            continue
        m = mods[path]
        if path.endswith(".2"):          # _Down/_Up hold a conv child that is what gets called
            m = m.conv
        hooks.append(m.register_forward_hook(lambda mod, i, o, name=name: taps.__setitem__(name, o.detach())))
    x1 = OS.flow_sample(net, noise, lm, cond, k_steps=1)
    for h in hooks:
        h.remove()
    return x1, taps


@pytest.mark.parametrize("prec", PRECS)
def test_denoiser_layers_and_output(ctx, oracle_net, inputs, prec):
    noise, lm, cond = inputs
    B = noise.shape[0]
    _bind(ctx, oracle_net, prec, B)
    x1_ref, taps = _oracle_with_taps(oracle_net, noise, lm, cond)
    x1 = ctx.denoise(noise.cuda(), lm.cuda(), cond.cuda(), want_actions=False)
    report, bad = {}, []
    for name, _ in LAYERS:
        if name == "enc.pool":
            continue
        got = ctx.debug_read(name, B).cpu().numpy()
        ref = tap_to_blc(taps[name].numpy(), B)
        report[name] = err_stats(got, ref)
        bad += check_close(got, ref, TOL[prec], name)
    report["x1"] = err_stats(x1.cpu().numpy(), x1_ref)
    bad += check_close(x1.cpu().numpy(), x1_ref, TOL[prec], "x1")
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, f"denoiser_layers_prec{prec}.json"), "w") as f:
        json.dump(report, f, indent=1)
    assert not bad, bad


@pytest.mark.parametrize("prec", [2, 3])
def test_latency_mode_split_k_keeps_the_layer_bounds(ctx, oracle_net, inputs, prec, monkeypatch):
    """DITREE_DENOISE_SPLITK=1 (opt-in latency mode for small batches: several work-groups per tile of the 3-tap convs, partial
    accumulators added in split order by the last one): every tapped layer and the output stay inside the same bounds against
    the fp32 oracle, repeated calls give the same bits, and switching the mode off restores the one-pass result exactly."""
    noise, lm, cond = inputs
    B = noise.shape[0]
    _bind(ctx, oracle_net, prec, B)
    x1_ref, taps = _oracle_with_taps(oracle_net, noise, lm, cond)
    plain = ctx.denoise(noise.cuda(), lm.cuda(), cond.cuda(), want_actions=False).cpu().numpy()
    monkeypatch.setenv("DITREE_DENOISE_SPLITK", "1")
    x1 = ctx.denoise(noise.cuda(), lm.cuda(), cond.cuda(), want_actions=False).cpu().numpy()
    bad = []
    for name, _ in LAYERS:
        if name == "enc.pool":
            continue
        bad += check_close(ctx.debug_read(name, B).cpu().numpy(), tap_to_blc(taps[name].numpy(), B), TOL[prec], name)
    bad += check_close(x1, x1_ref, TOL[prec], "x1")
    assert not bad, bad
    again = ctx.denoise(noise.cuda(), lm.cuda(), cond.cuda(), want_actions=False).cpu().numpy()
    assert np.array_equal(again, x1)                                   # deterministic: fixed summation order
    _bind(ctx, oracle_net, prec, B + 200)                               # a larger reservation rebuilds the workspace (and the partial-tile slabs)
    assert np.array_equal(ctx.denoise(noise.cuda(), lm.cuda(), cond.cuda(), want_actions=False).cpu().numpy(), x1)
    assert not np.array_equal(x1, plain)                               # (the mode really ran: another summation order)
    assert np.abs(x1 - plain).max() < 2e-5 * max(1.0, float(np.abs(plain).max()))
    monkeypatch.setenv("DITREE_DENOISE_SPLITK", "0")
    assert np.array_equal(ctx.denoise(noise.cuda(), lm.cuda(), cond.cuda(), want_actions=False).cpu().numpy(), plain)


@pytest.mark.parametrize("prec", PRECS)
def test_one_corrupted_element_is_caught(ctx, oracle_net, inputs, prec):
    """The bounds must see a single wrong element per layer (round 1 recorded a kernel variant with exactly that defect
    that a whole-tensor L2 at 4e-2 could not see): overwrite one element of every tapped tensor with a neighbour's value."""
    noise, lm, cond = inputs
    B = noise.shape[0]
    _bind(ctx, oracle_net, prec, B)
    _, taps = _oracle_with_taps(oracle_net, noise, lm, cond)
    ctx.denoise(noise.cuda(), lm.cuda(), cond.cuda(), want_actions=False)
    rng = np.random.default_rng(7)
    for name in ("d0b1.out", "skip1", "mid2.out", "u1b2.out", "final.in"):
        got = ctx.debug_read(name, B).cpu().numpy()
        ref = tap_to_blc(taps[name].numpy(), B)
        assert not check_close(got, ref, TOL[prec], name)
        rms = float(np.sqrt(np.mean(ref ** 2)))
        # a wrong value of typical magnitude in one place: pick an element that differs from its replacement by >= rms
        flat = got.reshape(-1).copy()
        for _ in range(1000):
            i, j = rng.integers(0, flat.size, 2)
            if abs(flat[i] - flat[j]) >= rms:
                break
        flat[i] = flat[j]
        assert check_close(flat.reshape(got.shape), ref, TOL[prec], name), (name, "corruption not detected")


def test_bench_size_batch_rows_against_oracle(ctx, oracle_net):
    """16 random rows of a B = 1024 call (the bench configuration, bf16) against the oracle run on those rows alone."""
    g = torch.Generator().manual_seed(11)
    B = 1024
    from oracle import geometry as G
    maze = load_maze("boxes").astype(np.float32)
    rng = np.random.default_rng(12)
    poses = np.stack([rng.uniform(-9, 9, B), rng.uniform(-9, 9, B), rng.uniform(-3.1, 3.1, B)], axis=1)
    lm = torch.tensor(OS.scale_local_map(G.create_local_map(maze, poses[:, 0], poses[:, 1], poses[:, 2], 20, 0.2, 1.0, (10.0, 10.0))))
    noise = torch.randn(B, 64, 2, generator=g)
    cond = torch.randn(B, 7, generator=g) * 0.7
    rows = np.sort(rng.choice(B, 16, replace=False))
    x_ref = OS.flow_sample(oracle_net, noise[rows], lm[rows], cond[rows], k_steps=1)
    for prec in (0, 2):
        _bind(ctx, oracle_net, prec, B)
        x = ctx.denoise(noise.cuda(), lm.cuda(), cond.cuda(), want_actions=False).cpu().numpy()
        bad = check_close(x[rows], x_ref, TOL[prec], f"x1 rows of B=1024, prec {prec}")
        assert not bad, bad


@pytest.mark.parametrize("prec", PRECS)
def test_actions_and_multi_step(ctx, oracle_net, inputs, prec):
    """K = 4 flow steps (exp schedule, fm_utils.py) and the un-normalised f64 actions."""
    noise, lm, cond = inputs
    B = noise.shape[0]
    _bind(ctx, oracle_net, prec, B)
    t0, dt = OS.get_timesteps("exp", 4, 4.0)
    xk_ref = memo(("k4", id(oracle_net)), lambda: OS.flow_sample(oracle_net, noise, lm, cond, k_steps=4))
    a_ref = OS.unnormalize_actions(xk_ref)
    a = ctx.denoise(noise.cuda(), lm.cuda(), cond.cuda(), t0=t0.numpy(), dt=dt.numpy(), want_actions=True)
    assert a.dtype == torch.float64
    # four network evaluations feed each other: allow twice the single-step bound
    assert rel(a.cpu().numpy(), a_ref) < 2 * TOL[prec]["l2"]


@pytest.mark.parametrize("prec", [0, 1, 2])
def test_batch_sizes_agree(ctx, oracle_net, inputs, prec):
    """Rows are independent: a sub-batch gives the same rows and the same map embedding, bit for bit (ragged B, padding rows
    inert).  The full call fills the whole reservation: the encoder's one scratch region end to end."""
    noise, lm, cond = inputs
    _bind(ctx, oracle_net, prec, 24)
    full = ctx.denoise(noise.cuda(), lm.cuda(), cond.cuda(), want_actions=False).cpu().numpy()
    full_emb = ctx.debug_read("map_emb", 24).cpu().numpy()
    for b in (1, 5, 17):
        part = ctx.denoise(noise[:b].cuda().contiguous(), lm[:b].cuda().contiguous(), cond[:b].cuda().contiguous(),
                           want_actions=False).cpu().numpy()
        assert np.array_equal(part, full[:b]), b
        assert np.array_equal(ctx.debug_read("map_emb", b).cpu().numpy(), full_emb[:b]), b


class _ToyScheduler:
    """Minimal scheduler with the diffusers call surface the sampler uses (set_timesteps / timesteps / step):
    a deterministic DDIM-like update, enough to drive the policy='diffusion' loop (fm_policy.py:164-182).
    diffusers itself is absent here, so the real DDPMScheduler arithmetic is not part of this test."""

    class _Out:
        def __init__(self, prev):
            self.prev_sample = prev

    def set_timesteps(self, n):
        self.timesteps = torch.arange(n - 1, -1, -1) * 7

    def step(self, model_output, timestep, sample):
        a = 1.0 / (1.0 + 0.01 * float(timestep))
        return self._Out(a * sample - 0.1 * model_output)


@pytest.mark.parametrize("prec", [1, 2, 0])
def test_raw_network_evaluation_and_diffusion_loop(ctx, oracle_net, inputs, prec):
    """ditree_denoise_eval = net(sample, map, timestep, cond) at arbitrary (unscaled) timesteps, with and without
    re-using the map embedding; then the sampler facade's policy='diffusion' branch against the same loop on the oracle."""
    noise, lm, cond = inputs
    B = noise.shape[0]
    tol = 2 * TOL[prec]["l2"]
    _bind(ctx, oracle_net, prec, B)
    with torch.no_grad():
        for i, t in enumerate((0.0, 7.0, 63.0)):
            ref = memo(("raw", id(oracle_net), t), lambda: oracle_net(sample=noise, local_map=lm, timestep=torch.full((B,), t),
                                                                        global_cond=cond).numpy())
            got = ctx.denoise_eval(noise.cuda(), lm.cuda(), cond.cuda(), t, reuse_encoder=i > 0).cpu().numpy()
            assert rel(got, ref) < tol, (t, rel(got, ref))
        # the facade loop
        def toy_loop():
            sch = _ToyScheduler()
            sch.set_timesteps(3)
            x = noise.clone()
            for k in sch.timesteps:
                eps = oracle_net(sample=x, local_map=lm, timestep=torch.full((B,), float(k)), global_cond=cond)
                x = sch.step(eps, k, x).prev_sample
            return x
        x = memo(("toy", id(oracle_net)), toy_loop)
    from ditreeonlineplanner_amd.policies.fm_policy import DiffusionSampler
    from ditreeonlineplanner_amd.model import NoisePredNet
    net = NoisePredNet(init=False)
    net.load_state_dict(oracle_net.state_dict())
    smp = DiffusionSampler(net, _ToyScheduler(), "carmaze", policy="diffusion", pred_horizon=64, action_dim=2,
                           prediction_type="actions", obs_history=1, action_history=1, goal_conditioned=True,
                           num_diffusion_iters=3, local_map_size=20, ctx=ctx, precision=prec)
    # the same loop on the device, on the same inputs
    state = np.zeros((B, 1, 6))
    xs = noise.cuda()
    sch2 = _ToyScheduler()
    sch2.set_timesteps(3)
    for i, k in enumerate(sch2.timesteps):
        eps = ctx.denoise_eval(xs.contiguous(), lm.cuda(), cond.cuda(), float(k), reuse_encoder=i > 0)
        xs = sch2.step(eps, k, xs).prev_sample.to(torch.float32)
    assert rel(xs.cpu().numpy(), x.numpy()) < tol
    # and the facade end to end: shapes, dtype, finite, un-normalised with the action statistics
    a = smp(state, prev_actions=None, goal=np.array([3.0, 4.0]), local_map=(lm[:, :, :] + 1) / 2)
    assert a.shape == (B, 64, 2) and a.dtype == np.float64 and np.isfinite(a).all()
    with pytest.raises(ValueError):
        DiffusionSampler(net, None, "carmaze", policy="diffusion", pred_horizon=64, action_dim=2)


@pytest.mark.parametrize("prec", [1, 2])
def test_ddpm_reverse_process_on_the_device(ctx, oracle_net, inputs, prec):
    """ditree_denoise_ddpm (policies/fm_policy.py:164-182 with the reference's DDPMScheduler configuration, run_scenarios.py:
    157-158): K = 5 reverse steps inside the library against the numpy restatement of the published algorithm (oracle/ddpm.py)
    around the torch-CPU oracle network, on the same start and step noise.  diffusers itself is absent: PARITY UNPINNED."""
    from oracle import ddpm as ODD
    from ditreeonlineplanner_amd.ddpm import DDPMScheduler, ddpm_tables
    noise, lm, cond = inputs
    B, K = 6, 5
    noise, lm, cond = noise[:B].contiguous(), lm[:B].contiguous(), cond[:B].contiguous()
    z = torch.randn(B, K, 64, 2, generator=torch.Generator().manual_seed(9))
    sch = DDPMScheduler(num_train_timesteps=K, beta_schedule="squaredcos_cap_v2", clip_sample=True, prediction_type="epsilon")
    ts, coef = ddpm_tables(sch, K)
    assert list(ts) == [4.0, 3.0, 2.0, 1.0, 0.0] and coef[-1, 4] == 0.0 and (coef[:-1, 4] > 0).all()

    def eps_fn(x, t):
        with torch.no_grad():
            return oracle_net(sample=torch.as_tensor(x), local_map=lm, timestep=torch.full((B,), t), global_cond=cond).numpy()
    ref = ODD.reverse_process(eps_fn, noise.numpy(), K, z.permute(1, 0, 2, 3).numpy())
    _bind(ctx, oracle_net, prec, B)
    got = ctx.denoise_ddpm(noise.cuda(), z.cuda(), lm.cuda(), cond.cuda(), ts, coef, want_actions=False).cpu().numpy()
    assert np.abs(got).max() <= 1.0 + 1e-6                    # the last step returns the clipped x0
    assert rel(got, ref) < 20 * TOL[prec]["l2"], rel(got, ref)
    # un-normalised actions of the same call, and a sub-batch larger than nothing: rows independent
    unit = np.array([0.5, -0.25, 2.0, 3.0])
    a = ctx.denoise_ddpm(noise.cuda(), z.cuda(), lm.cuda(), cond.cuda(), ts, coef, act_norm=unit).cpu().numpy()
    assert np.abs(a - (got.astype(np.float64) * unit[2:] + unit[:2])).max() < 1e-12
    part = ctx.denoise_ddpm(noise[:2].cuda().contiguous(), z[:2].cuda().contiguous(), lm[:2].cuda().contiguous(),
                            cond[:2].cuda().contiguous(), ts, coef, want_actions=False).cpu().numpy()
    assert np.array_equal(part, got[:2])
    with pytest.raises(ValueError):
        ctx.denoise_ddpm(noise.cuda(), z[:, :3].cuda().contiguous(), lm.cuda(), cond.cuda(), ts, coef)


_SIZE_CACHE = {}


@pytest.mark.parametrize("prec", [1, 2, 0])
@pytest.mark.parametrize("size,dims", [("small", (64, 128, 256)), ("medium", (256, 512, 1024)), ("xlarge", (1024, 2048, 4096))])
def test_other_denoiser_sizes(ctx, inputs, size, dims, prec):
    """The reference's `denoiser_size` small / medium / xlarge (run_scenarios.py:92-97): channel counts whose GroupNorm groups do
    not fit the fused 256-channel epilogue run conv + bias in the GEMM and GroupNorm / Mish / FiLM / residual in
    gn1d_kernel; one flow step and the actions against the oracle network of the same size."""
    from ditreeonlineplanner_amd.model import NoisePredNet
    noise, lm, cond = inputs
    B = 8
    tol = 2 * TOL[prec]["l2"]
    if size not in _SIZE_CACHE:                       # the oracle network of a size (xlarge: 690 M parameters) once for all precisions
        torch.manual_seed(3)
        onet = OD.init_noise_pred_net(down_dims=dims).eval()
        g = torch.Generator().manual_seed(1)
        with torch.no_grad():
            for n, p in onet.named_parameters():
                if p.dim() == 1:
                    p.add_(0.2 * torch.randn(p.shape, generator=g))
        _SIZE_CACHE.clear()                           # keep one size at a time (memory)
        _SIZE_CACHE[size] = (onet, OS.flow_sample(onet, noise[:B], lm[:B], cond[:B], k_steps=1))
    onet, x_ref = _SIZE_CACHE[size]
    net = NoisePredNet(down_dims=dims, init=False)
    net.load_state_dict(onet.state_dict())
    if prec == 2 and size == "small":
        # the split instantiations only exist on the 256-channel tiles: a clean error, not a fallback
        from ditreeonlineplanner_amd._lib import DitreeError
        with pytest.raises(DitreeError, match="multiples of 256"):
            net.bind(ctx, precision=prec, max_batch=B)
        return
    net.bind(ctx, precision=prec, max_batch=B)
    x = ctx.denoise(noise[:B].cuda().contiguous(), lm[:B].cuda().contiguous(), cond[:B].cuda().contiguous(), want_actions=False)
    assert rel(x.cpu().numpy(), x_ref) < tol, (size, prec, rel(x.cpu().numpy(), x_ref))


def test_f16_range_guard_reports_a_clamped_layer(ctx, oracle_net, inputs):
    """f16x3 stores activations as f16 hi + lo and saturates at +-65504.  The reference's FiLM layer `scale * out + bias`
    (model/diffusion/conditional_unet1d.py:110-117) has no bound, so a checkpoint may leave that range: the library must SAY
    so (ditree_denoise_status names the layer, Context.denoise raises) instead of returning wrong actions with rc 0, and
    the range-safe split (bf16x3) must stay within its bound on the same weights."""
    import copy
    from ditreeonlineplanner_amd import _lib
    noise, lm, cond = inputs
    B = noise.shape[0]
    dev = ctx.device
    args = (noise.to(dev), lm.to(dev), cond.to(dev))
    # healthy network: the guard stays silent (the other f16 instantiation is covered by every other test of this module:
    # Context.denoise raises when it fires)
    _bind(ctx, oracle_net, 2, B)
    ctx.denoise(*args, want_actions=False)
    assert ctx.denoise_status() == []
    big = copy.deepcopy(oracle_net)
    key = "unet.mid_modules.0.cond_encoder.1"
    with torch.no_grad():
        sd = big.state_dict()
        sd[key + ".weight"].mul_(3e5)              # FiLM scale / bias of mid block 1: O(1) -> O(1e5)
        sd[key + ".bias"].mul_(3e5)
    x_ref = OS.flow_sample(big, noise.numpy(), lm.numpy(), cond.numpy(), k_steps=1)
    assert np.isfinite(x_ref).all()
    for prec in (2, 4):
        _bind(ctx, big, prec, B)
        x = ctx.denoise(*args, want_actions=False, check_range=False)      # rc 0: the launch itself is fine
        layers = ctx.denoise_status(clear=False)
        assert "unet.mid_modules.0.blocks.0.block.0" in layers, layers     # the layer whose epilogue applies the FiLM row
        assert ctx.denoise_status(clear=True) == layers                     # sticky until cleared
        assert ctx.denoise_status() == []
        with pytest.raises(_lib.DitreeError, match="f16 range guard.*unet.mid_modules.0.blocks.0.block.0"):
            ctx.denoise(*args, want_actions=False)
        assert rel(x.cpu().numpy(), x_ref) > 1e-3                           # and the clamped result IS wrong (measured 7e-3)
    # the range-safe split on the same weights: within its usual bound, guard silent
    _bind(ctx, big, 3, B)
    x = ctx.denoise(*args, want_actions=False)
    assert ctx.denoise_status() == []
    assert rel(x.cpu().numpy(), x_ref) < TOL[3]["l2"] * 4, rel(x.cpu().numpy(), x_ref)
