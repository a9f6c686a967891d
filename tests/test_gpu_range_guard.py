"""The f16 range guard of every kernel that stores f16 activations, against a clamping oracle.

PREC_F16X3 (the default) and PREC_F16 store activations as f16, which ends at +-65504; a checkpoint that leaves that range
must be REPORTED: the storing kernel ORs a sticky per-layer flag, ditree_denoise_status names the layers, Context.denoise
and the engines raise.  tests/range_guard_ref.py predicts the names on the CPU (the fp32 torch oracle with a record-and-clamp
hook at every stored point); here one driver at a time (a power of two on the parameters that scale one stored point) is
bound, and the device's status list must be the predicted set.

  ISOLATION   car `medium` (precisions 2, 4) and `small` (4) at P = 16, B = 3: every slot's post driver and every GroupNorm
              layer's pre driver, one bind each -- names, slot wiring, the fused / unfused split of the GroupNorm layers.
  SWEEP       `large` at the sizes that select the other kernels (car P = 64 / 16 / 256, ant P = 16, car P = 64 in split-K
              latency mode): every post driver in one bind, every pre driver in one bind; one driven ROW at three positions of
              a batch that spans two tiles of the shortest level, the other rows bit-identical to an undriven call.
  THRESHOLD   65504 itself is stored silently and exactly, the next float32 is clamped to 65504 and reported.
  STALE ROWS  a healthy small call after a saturating larger one.
  ENGINES     ExpansionEngine, ForestEngine and PolicyRolloutEngine raise, and run cleanly again on healthy weights.

DECIDED NAMES.  A stored point whose oracle maximum lies within a factor 2 of 65504 is UNDECIDED: the f16 instantiations'
own error (1e-3 relative) may move it across the line.  Healthy points are O(10) and driven points O(1e5), so every healthy
network and every driven target must be decided, and the CPU test asserts that.  Downstream of a clamp, however, undecided
points cannot be avoided by any choice of driver: a clamped value IS +-65504, the identity residual of the next block stores
65504 + O(1), and a 1 x 1 or resampling conv stores 65504 x O(1).  Those names (listed per network by the CPU test's
output) are left out of the comparison on both sides; every other name -- the target, everything upstream, every decided
point downstream -- must match the oracle exactly.  The band itself stays at the factor 2."""
import copy

import numpy as np
import pytest
import torch

from tests import range_guard_ref as R
from tests import test_gpu_denoiser_shapes as S
from tests.test_gpu_denoiser import check_close, tap_to_blc
from tests.util import load_maze

gpu = pytest.mark.gpu

# configuration -> (family, size, P)
ISO = {"car_medium_p16": ("car", "medium", 16), "car_small_p16": ("car", "small", 16)}
ISO_PRECS = {"car_medium_p16": (2, 4), "car_small_p16": (4,)}
SWEEP = {"car_large_p64": ("car", "large", 64), "car_large_p16": ("car", "large", 16), "car_large_p256": ("car", "large", 256),
         "ant_large_p16": ("ant", "large", 16), "car_large_p64_splitk": ("car", "large", 64)}
SWEEP_PRECS = {c: ((2,) if c.endswith("splitk") else (2, 4)) for c in SWEEP}
ENGINE = ("car", "medium", 64)
# Which GroupNorm layers run UNFUSED (conv + bias stored, then gn1d_kernel), as (level of C_out, level of L) pairs: DESIGN's
# rule -- fused iff C_out % 256 == 0 and C_out / 8 in {64, 128, 256} and (16 | L or (L in {8, 4} and a 16-bit format)) --
# worked out by hand per configuration.  Levels: (0, 0) down 0 and final_conv, (1, 1) down 1, (2, 2) down 2 and mid,
# (1, 2) up 0, (0, 1) up 1.
ALL_LEVELS = {(0, 0), (1, 1), (2, 2), (1, 2), (0, 1)}
UNFUSED = {
    "car_medium_p16": {(0, 0), (0, 1)},        # 256 channels: groups of 32;  512 at L = 8 / 4 and 1024 at L = 4 fuse (16-bit)
    "car_small_p16": ALL_LEVELS,               # 64 / 128 channels fit no 256-channel tile, 256 has groups of 32
    "car_medium_p64": {(0, 0), (0, 1)},
    "car_large_p64": set(), "car_large_p16": set(), "car_large_p256": set(), "ant_large_p16": set(), "car_large_p64_splitk": set(),
}


def unfused_layers(config):
    return {n for n, lv in R.gn_layers().items() if lv in UNFUSED[config]}


def config_of(family, size, P):
    return f"{family}_{size}_p{P}"


# ------------------------------------------------------------------------------------------------ inputs, oracle predictions
_IN = {}


def inputs(family, P, n):
    """n seeded input rows: the rows of tests/test_gpu_denoiser_shapes.py, or (batches larger than it draws) drawn likewise."""
    base = S._inputs(family, P)
    if n <= base[0].shape[0]:
        return S._rows(base, slice(0, n))
    key = (family, P, n)
    if key not in _IN:
        g = torch.Generator().manual_seed(31)
        if family == "ant":
            _IN[key] = (torch.randn(n, P, 8, generator=g), (torch.rand(n, 16, 16, generator=g) < 0.3).float() * 2 - 1,
                        torch.randn(n, 97, generator=g) * 0.6)
        else:
            from oracle import geometry as G
            from oracle import sampler as OS
            rng = np.random.default_rng(32)
            poses = np.stack([rng.uniform(-9, 9, n), rng.uniform(-9, 9, n), rng.uniform(-3.1, 3.1, n)], axis=1)
            lm = OS.scale_local_map(G.create_local_map(load_maze("boxes").astype(np.float32), poses[:, 0], poses[:, 1],
                                                       poses[:, 2], 20, 0.2, 1.0, (10.0, 10.0)))
            _IN[key] = (torch.randn(n, P, 2, generator=g), torch.tensor(lm), torch.randn(n, 7, generator=g) * 0.7)
    return _IN[key]


_PRED = {}


def predicted(config, family, size, P, drivers, rows3):
    """(names, ratios, undecided) of the clamping oracle for `drivers` on the input rows `rows3` (every row driven)."""
    drivers = tuple(drivers)
    key = (config, drivers, tuple(rows3[0].shape), float(rows3[0].abs().sum()))
    if key not in _PRED:
        net = S._oracle_net(family, size)
        noise, lm, cond = rows3
        with R.driven(net, drivers):
            n2, c2 = R.drive_inputs(drivers, noise, cond)
            seen = R.clamped_run(net, n2, lm, c2, unfused_layers(config))
        names, ratios = R.predict(seen)
        _PRED[key] = (names, ratios, set(R.in_band(ratios)))
    return _PRED[key]


def check_network(config, family, size, P, drivers, rows3, expect=None):
    """The CPU condition on one test network: every driven target decided and named (a pre driver on a fused layer: nothing
    stored beyond half the range at all); `expect`: the exact predicted set."""
    names, ratios, und = predicted(config, family, size, P, drivers, rows3)
    unf = unfused_layers(config)
    fused_pre = all(k == "pre" and n not in unf for k, n in drivers)
    for k, n in drivers:
        if k == "pre" and n not in unf:
            continue
        assert ratios[n] > 2.0 and n in names, (config, (k, n), ratios[n])
    if fused_pre:
        assert not names and not und, (config, drivers[:3], names, und)
    if expect is not None:
        assert names == set(expect) and not und, (config, names ^ set(expect), und)
    if und:
        print(f"UNDECIDED {config} {drivers[0] if len(drivers) == 1 else len(drivers)}: "
              + ", ".join(f"{n} {ratios[n]:.6f}" for n in sorted(und)))
    return names, und


# ------------------------------------------------------------------------------------------------ the driver blocks
def iso_blocks(net):
    """block id -> the drivers bound one at a time in that test id.  Together: every slot's post driver, every GN layer's pre."""
    mods = dict(net.named_modules())
    blocks = {"inputs": [("post", R.SAMPLE), ("post", R.COND)]}
    for crb in R.CRBS:
        d = [("post", crb + ".blocks.0.block.0"), ("post", crb + ".blocks.1.block.0")]
        if isinstance(mods[crb + ".residual_conv"], torch.nn.Conv1d):
            d.append(("post", crb + ".residual_conv"))
        d += [("pre", crb + ".blocks.0.block.0"), ("pre", crb + ".blocks.1.block.0")]
        blocks[crb[len("unet."):]] = d
    blocks["final_conv"] = [("post", R.FINAL), ("pre", R.FINAL)]
    blocks["resample"] = [("post", n) for n in R.RESAMPLE]
    enc = R.encoder_slots(net)
    blocks["encoder.stem_layer1"] = [("post", n) for n in enc if n == R.STEM or ".layer1." in n]
    for li in (2, 3, 4):
        blocks[f"encoder.layer{li}"] = [("post", n) for n in enc if f".layer{li}." in n]
    return blocks


# the block ids, without building a network at collection time (iso_blocks is checked against this list on the CPU)
BLOCK_IDS = ["inputs"] + [c[len("unet."):] for c in R.CRBS] + ["final_conv", "resample", "encoder.stem_layer1", "encoder.layer2",
                                                             "encoder.layer3", "encoder.layer4"]
ISO_MATRIX = [(c, p, b) for c in ISO for p in ISO_PRECS[c] for b in BLOCK_IDS]
B_ISO = 3


# ------------------------------------------------------------------------------------------------ CPU: the oracle's condition
@pytest.mark.parametrize("config", list(ISO))
def test_oracle_condition_isolation_networks(config):
    """Every isolation network: the healthy one predicts the empty set with every point below half the range, every driver's
    target is decided and named, a pre driver on a fused layer stores nothing large; every slot and every GroupNorm layer has
    its driver; the declared fused / unfused table is DESIGN's rule."""
    family, size, P = ISO[config]
    net = S._oracle_net(family, size)
    rows3 = inputs(family, P, B_ISO)
    assert unfused_layers(config) == R.unfused_by_rule(S.SIZES[size], P)
    check_network(config, family, size, P, (), rows3, expect=())
    blocks = iso_blocks(net)
    assert list(blocks) == BLOCK_IDS
    flat = [d for b in blocks.values() for d in b]
    assert sorted(n for k, n in flat if k == "post") == sorted(R.all_slots(net))
    assert sorted(n for k, n in flat if k == "pre") == sorted(R.gn_layers())
    assert len(R.unet_slots(net)) == 36 and len(R.encoder_slots(net)) == 20
    for d in flat:
        names, _ = check_network(config, family, size, P, (d,), rows3)
        if d[0] == "pre":
            assert names == ({d[1]} if d[1] in unfused_layers(config) else set()), (d, names)


def position_batch(P):
    return 1024 // P + 1                         # one sample more than a 256-row tile of the shortest level (L = P / 4) holds


def sweep_batch(config):
    return 1 if config.endswith("splitk") else 3


def all_post(net):
    return tuple(R.post_drivers(net))


@pytest.mark.parametrize("config", list(SWEEP))
def test_oracle_condition_sweep_networks(config):
    """Every sweep network: all-post names EVERY slot, all-pre names exactly the table's unfused layers (`large`: none), the
    row driven through both inputs names the two input slots; the healthy network predicts the empty set."""
    family, size, P = SWEEP[config]
    net = S._oracle_net(family, size)
    B = sweep_batch(config)
    assert unfused_layers(config) == R.unfused_by_rule(S.SIZES[size], P)
    check_network(config, family, size, P, (), inputs(family, P, B), expect=())
    names, und = check_network(config, family, size, P, all_post(net), inputs(family, P, B))
    assert names - und == set(R.all_slots(net)) - und and names >= set(R.all_slots(net)), set(R.all_slots(net)) - names
    check_network(config, family, size, P, tuple(R.pre_drivers()), inputs(family, P, B), expect=unfused_layers(config))
    if not config.endswith("splitk"):
        Bp = position_batch(P)
        for r in sorted({0, Bp - 1, 1024 // P}):
            row = tuple(t[r:r + 1] for t in inputs(family, P, Bp))
            names, _ = check_network(config, family, size, P, (("post", R.SAMPLE), ("post", R.COND)), row)
            assert {R.SAMPLE, R.COND} <= names


def test_oracle_condition_engine_network():
    family, size, P = ENGINE
    names, _ = check_network(config_of(*ENGINE), family, size, P, (ENGINE_DRIVER,), inputs(family, P, B_ISO))
    assert ENGINE_DRIVER[1] in names


# ------------------------------------------------------------------------------------------------ the device side
@pytest.fixture(scope="module")
def ctx():
    from ditreeonlineplanner_amd.ops import Context
    c = Context(0)
    yield c
    c.close()
    for cache in (S._NET, S._LARGE, S._MEMO, S._INPUTS, _PRED, _IN):
        cache.clear()


def bind(ctx, family, size, P, prec, B, drivers=(), state=None):
    """A device network of the configuration with `drivers` applied to the oracle's weights (or with `state`), bound."""
    dnet = S._device_net(family, size, P)
    if state is not None:
        dnet.load_state_dict(state)
    else:
        onet = S._oracle_net(family, size)
        with R.driven(onet, drivers):
            dnet.load_state_dict(onet.state_dict())
    dnet.bind(ctx, precision=prec, max_batch=B)
    return dnet


def denoise(ctx, family, rows3, **kw):
    noise, lm, cond = rows3
    if family == "ant":
        kw["act_norm"] = np.concatenate([np.zeros(8), np.ones(8)])
    return ctx.denoise(noise.cuda().contiguous(), lm.cuda().contiguous(), cond.cuda().contiguous(), want_actions=False, **kw)


def status_protocol(ctx, family, rows3, target):
    """What the guard promises beyond the names: the list is sticky until cleared, clearing empties it, and a call that checks
    raises with the target's name.  -> the status list of the (already made) unchecked call."""
    from ditreeonlineplanner_amd._lib import DitreeError
    got = ctx.denoise_status(clear=False)
    assert len(set(got)) == len(got), got
    assert ctx.denoise_status(clear=True) == got
    assert ctx.denoise_status() == []
    if target is not None:
        with pytest.raises(DitreeError, match="f16 range guard") as e:
            denoise(ctx, family, rows3)
        assert target in str(e.value), (target, str(e.value))
        assert ctx.denoise_status() == []                       # (the raising call cleared it)
    return got


def healthy_tol(family, size, P, B, prec):
    """The bounds tests/test_gpu_denoiser_shapes.py derives for a configuration and precision (its `scales`, for a
    configuration that is not in its table)."""
    cls = S.ERR_CLASS[prec]
    ec = S.oracle_error(family, size, P, B, cls)
    eb = S.oracle_error(*S.BASE[family], cls)
    s = (max(1.0, ec[0] / eb[0]), max(1.0, ec[1] / eb[1]))
    assert max(s) <= S.SCALE_CAP, (family, size, P, prec, s)
    return S.scaled_tol(prec, s)


@gpu
@pytest.mark.parametrize("config,prec,block", ISO_MATRIX)
def test_isolation_one_driver_names_its_layer(ctx, config, prec, block):
    family, size, P = ISO[config]
    onet = S._oracle_net(family, size)
    rows3 = inputs(family, P, B_ISO)
    unf = unfused_layers(config)
    if block == "inputs":                                       # the healthy network first: silent
        bind(ctx, family, size, P, prec, B_ISO)
        denoise(ctx, family, rows3)
        assert ctx.denoise_status() == []
    for d in iso_blocks(onet)[block]:
        names, und = check_network(config, family, size, P, (d,), rows3)
        bind(ctx, family, size, P, prec, B_ISO, (d,))
        driven3 = (*R.drive_inputs((d,), rows3[0], rows3[2]),)
        driven3 = (driven3[0], rows3[1], driven3[1])
        x = denoise(ctx, family, driven3, check_range=False)
        if d[0] == "pre" and d[1] not in unf:
            # fused: conv + bias stays in the f32 accumulator, nothing large is stored -- and the 2^20 is exact on both sides
            assert ctx.denoise_status() == [], d
            with R.driven(onet, (d,)):
                x_ref, taps = S._run_with_taps(onet, *rows3)
            tol = healthy_tol(family, size, P, B_ISO, prec)
            bad = check_close(x.cpu().numpy(), x_ref, tol, "x1")
            for name in S.TAPS:
                bad += check_close(ctx.debug_read(name, B_ISO).cpu().numpy(), tap_to_blc(taps[name], B_ISO), tol, name)
            assert not bad, (d, bad)
            continue
        got = status_protocol(ctx, family, driven3, d[1])
        print(f"RANGE_GUARD {config} prec {prec} {d}: device {len(got)} names, oracle {len(names)}, undecided {len(und)}")
        assert d[1] in got, (d, got)
        assert set(got) - und == names - und, (d, sorted(set(got) ^ names - und))


SWEEP_MATRIX = [(c, p) for c in SWEEP for p in SWEEP_PRECS[c]]


def _splitk(config, monkeypatch):
    if config.endswith("splitk"):
        monkeypatch.setenv("DITREE_DENOISE_SPLITK", "1")


@gpu
@pytest.mark.parametrize("config,prec", SWEEP_MATRIX)
def test_sweep_all_post_drivers_name_every_slot(ctx, config, prec, monkeypatch):
    family, size, P = SWEEP[config]
    _splitk(config, monkeypatch)
    B = sweep_batch(config)
    rows3 = inputs(family, P, B)
    drivers = all_post(S._oracle_net(family, size))
    names, und = check_network(config, family, size, P, drivers, rows3)
    bind(ctx, family, size, P, prec, B, drivers)
    noise, cond = R.drive_inputs(drivers, rows3[0], rows3[2])
    driven3 = (noise, rows3[1], cond)
    denoise(ctx, family, driven3, check_range=False)
    got = status_protocol(ctx, family, driven3, R.STEM)         # (the message names the first six in execution order)
    assert set(got) - und == names - und, sorted(set(got) ^ names - und)
    assert set(got) >= set(R.all_slots(S._oracle_net(family, size))) - und


@gpu
@pytest.mark.parametrize("config,prec", SWEEP_MATRIX)
def test_sweep_all_pre_drivers_name_the_unfused_layers_only(ctx, config, prec, monkeypatch):
    family, size, P = SWEEP[config]
    _splitk(config, monkeypatch)
    B = sweep_batch(config)
    rows3 = inputs(family, P, B)
    drivers = tuple(R.pre_drivers())
    check_network(config, family, size, P, drivers, rows3, expect=unfused_layers(config))
    bind(ctx, family, size, P, prec, B, drivers)
    denoise(ctx, family, rows3, check_range=False)
    assert set(ctx.denoise_status()) == unfused_layers(config)


POSITIONS = ["first", "last", "second_tile"]


@gpu
@pytest.mark.parametrize("pos", POSITIONS)
@pytest.mark.parametrize("config,prec", [(c, p) for c, p in SWEEP_MATRIX if not c.endswith("splitk")])
def test_sweep_one_driven_row_is_named_wherever_it_sits(ctx, config, prec, pos):
    """One row of a healthy bind carries noise x 2^18 and cond x 2^18: the two input slots are named from that single row,
    first, last, or at the first row of the second 256-row tile of the shortest level; every other row of x1 and of each
    tapped layer equals, bit for bit, the same row of the call in which no row is driven (DESIGN: batch invariance)."""
    family, size, P = SWEEP[config]
    B = position_batch(P)
    r = {"first": 0, "last": B - 1, "second_tile": 1024 // P}[pos]
    rows3 = inputs(family, P, B)
    drivers = (("post", R.SAMPLE), ("post", R.COND))
    names, und = check_network(config, family, size, P, drivers, tuple(t[r:r + 1] for t in rows3))
    bind(ctx, family, size, P, prec, B)
    x0 = denoise(ctx, family, rows3).cpu().numpy()
    assert ctx.denoise_status() == []
    taps0 = {n: ctx.debug_read(n, B).cpu().numpy() for n in S.TAPS}
    noise, cond = R.drive_inputs(drivers, rows3[0], rows3[2], rows=slice(r, r + 1))
    driven3 = (noise, rows3[1], cond)
    x = denoise(ctx, family, driven3, check_range=False).cpu().numpy()
    keep = np.arange(B) != r
    diff = {n: int((ctx.debug_read(n, B).cpu().numpy()[keep].view(np.uint32) != taps0[n][keep].view(np.uint32)).sum()) for n in S.TAPS}
    diff["x1"] = int((x[keep].view(np.uint32) != x0[keep].view(np.uint32)).sum())
    got = status_protocol(ctx, family, driven3, R.COND)
    assert {R.SAMPLE, R.COND} <= set(got), got
    assert set(got) - und == names - und, sorted(set(got) ^ names - und)
    assert not any(diff.values()), {k: v for k, v in diff.items() if v}


# ------------------------------------------------------------------------------------------------ threshold
THRESHOLD = [("unet.down_modules.1.0.residual_conv", "d1b1.res"), ("unet.down_modules.0.2.conv", "d1.in"),
             ("unet.up_modules.0.2.conv", "up0.out")]


@gpu
@pytest.mark.parametrize("prec", [2, 4])
@pytest.mark.parametrize("layer,tap", THRESHOLD)
def test_threshold_65504_passes_silently_and_the_next_float_is_reported(ctx, layer, tap, prec):
    """A plain-store layer with zero weight and constant bias b stores b everywhere.  b = +-65504: silent, stored exactly.
    b = +- the next float32: named, stored as +-65504; never an inf or a NaN.  (`>` against `>=`, and the clamp itself.)
    Every other U-Net parameter is zero as well, so that what the layer stores travels on through identity residuals only,
    as exact copies: nothing downstream can exceed what the layer stored, and the expected status is the layer alone."""
    family, size, P = "car", "medium", 16
    rows3 = inputs(family, P, B_ISO)
    state = copy.deepcopy(S._oracle_net(family, size).state_dict())
    for k, t in state.items():
        if k.startswith("unet."):
            t.zero_()
    top = np.float32(R.F16_MAX)
    above = np.nextafter(top, np.float32(np.inf))
    assert above > top and float(above) - float(top) < 0.01
    for b, named in ((top, False), (-top, False), (above, True), (-above, True)):
        state[layer + ".bias"].fill_(float(b))
        assert state[layer + ".bias"].dtype == torch.float32 and float(state[layer + ".bias"][0]) == float(b)
        bind(ctx, family, size, P, prec, B_ISO, state=state)
        denoise(ctx, family, rows3, check_range=False)
        got = ctx.debug_read(tap, B_ISO).cpu().numpy()
        assert np.isfinite(got).all(), (layer, b)
        assert (got == np.float32(np.sign(b)) * top).all(), (layer, b, np.unique(got)[:4])
        assert ctx.denoise_status() == ([layer] if named else []), (layer, float(b))


# ------------------------------------------------------------------------------------------------ stale padding rows
@gpu
@pytest.mark.parametrize("which", ["sample", "cond"])
def test_stale_padding_rows_raise_no_false_alarm(ctx, which):
    """A call of B samples runs on B rounded up to the batch granule.  The padding rows used to hold whatever an earlier,
    larger call left in them (its x1 in the sample buffer, its FiLM input), and the guard saw them: a healthy call after a
    saturating one reported layers that it had not saturated.  They are zero now.  Either way the healthy rows' bits are
    the fresh bind's (rows are independent)."""
    family, size, P, prec = "car", "medium", 16, 2
    gran = max(16, 1024 // P)
    rowsA = inputs(family, P, gran)
    one = tuple(t[:1] for t in rowsA)
    bind(ctx, family, size, P, prec, gran)
    fresh = denoise(ctx, family, one).cpu().numpy()
    bind(ctx, family, size, P, prec, gran)
    driver = (("post", R.SAMPLE if which == "sample" else R.COND),)
    noise, cond = R.drive_inputs(driver, rowsA[0], rowsA[2])
    denoise(ctx, family, (noise, rowsA[1], cond), check_range=False)
    assert driver[0][1] in ctx.denoise_status(clear=True)
    x = denoise(ctx, family, one, check_range=False).cpu().numpy()
    assert ctx.denoise_status() == []
    assert np.array_equal(x.view(np.uint32), fresh.view(np.uint32))


# ------------------------------------------------------------------------------------------------ the engines raise
ENGINE_DRIVER = ("post", "unet.mid_modules.0.blocks.0.block.0")
ENGINE_MATCH = "f16 range guard.*unet.mid_modules.0.blocks.0.block.0"


def _round_inputs(B, n_chunks, P, seed):
    from oracle import geometry as G
    from oracle import rrt as ORRT
    maze = load_maze("boxes")
    start = np.array([*G.cell_rowcol_to_xy([17, 2], maze), np.deg2rad(45.0), 0, 0, 0])
    goal = np.array([*G.cell_rowcol_to_xy([2, 17], maze), 0, 0, 0, 0])
    samples, cond = ORRT.RandomTape(seed).draw_round(B, maze.shape[1], maze.shape[0], goal)
    noise = torch.randn(B, n_chunks, P, 2, generator=torch.Generator().manual_seed(seed))
    return maze, start, goal, torch.as_tensor(samples).cuda(), torch.as_tensor(cond).cuda(), noise.cuda()


@gpu
@pytest.mark.parametrize("engine", ["expansion", "forest", "policy_rollout"])
def test_engines_raise_and_recover(ctx, engine):
    """ExpansionEngine._range_guard, ForestTrees.accept and PolicyRolloutEngine.run end in check_range: on a network with one
    post driver each raises DitreeError naming the layer; the same engine object then runs cleanly on healthy weights (the
    status was cleared by the raise, it does not stick)."""
    from ditreeonlineplanner_amd._lib import DitreeError
    family, size, P = ENGINE
    prec, B = 2, 16

    def run_both(step):
        bind(ctx, family, size, P, prec, 64, (ENGINE_DRIVER,))
        with pytest.raises(DitreeError, match=ENGINE_MATCH):
            step()
        assert ctx.denoise_status() == []
        bind(ctx, family, size, P, prec, 64)
        step()
        assert ctx.denoise_status() == []

    if engine == "policy_rollout":
        from tests.test_gpu_policy_rollout import net_cases, net_engine
        goals, starts, scene_of = net_cases()
        noise = torch.randn(2, len(starts), P, 2, generator=torch.Generator().manual_seed(4)).cuda()
        bind(ctx, family, size, P, prec, 64)
        eng = net_engine(ctx, goals, starts, scene_of)
        run_both(lambda: eng.run(16, noise_fn=lambda c: noise[c].contiguous()))
        return
    from ditreeonlineplanner_amd.engine import ExpansionEngine
    from ditreeonlineplanner_amd.forest import ForestEngine
    T = 2 if engine == "forest" else 1
    maze, start, goal, samples, cond, noise = _round_inputs(T * B, 4, P, 6)
    bind(ctx, family, size, P, prec, 64)
    if engine == "forest":
        eng = ForestEngine(ctx, maze, start, goal, T, 128, edge_length=32, batch=T * B)
        assert eng.n_chunks == 4 and eng.P == P
        run_both(lambda: eng.expand_round(samples, cond, noise=noise, counts_per_tree=[B] * T))
    else:
        eng = ExpansionEngine(ctx, maze, start, goal, edge_length=32, batch=B, capacity=128)
        run_both(lambda: eng.expand_round(samples, cond, noise=noise))
