"""CPU side of tests/test_gpu_range_guard.py: a CLAMPING oracle of the f16 range guard.  No device code involved.

The fp32 torch oracle (oracle/denoiser.py) gets a hook at every point where the f16 instantiations store an activation
(ditreeonlineplanner_amd/csrc/denoise_plan.hip build_unet / build_encoder_resnet).  A hook records max |v| of what the device
is handed there, under the name the device reports the store under (the state-dict prefix `sat_slot` is called with, or the
fixed string of one of the two input slots), and then clamps v to +-65504 as the store does.  So the oracle predicts, for
any weights and inputs, WHICH names the guard must report: the driven layer, and whatever the clamped values saturate
further down.

Stored points (name <- what is recorded):
  SAMPLE                                    the sample rows (the U-Net's input)
  COND                                      Mish(time | map_emb | cond), the input of every cond_encoder Linear
  <crb>.blocks.0.block.0                    FiLM(Mish(GN(conv)))       (the input of the block's second conv)
  <crb>.blocks.1.block.0                    Mish(GN(conv)) + residual  (the block's output)
  unet.final_conv.0.block.0                 Mish(GN(conv))             (the input of the last projection)
  ... and, for a layer in `unfused`, conv + bias before the GroupNorm as well, under the same name
  <crb>.residual_conv, unet.*_modules.i.2.conv   conv + bias (an up conv's even and odd halves share the name)
  encoder.resnet18.conv1                    the stem: max-pool(ReLU(GN(conv)))
  encoder.resnet18.layerX.Y.bn1 / .bn2 / .downsample.1    ReLU(GN) / ReLU(GN + identity) / GN

Drivers multiply parameters or input rows by a power of two, so the fp32 oracle is scaled exactly:
  ("post", name)  2^18 on what scales the value stored under `name`
  ("pre", conv)   2^20 on the weight and bias of a GroupNorm layer's conv: stored (so clamped) on the unfused path only."""
import contextlib

import torch

F16_MAX = 65504.0
POST, PRE = 2.0 ** 18, 2.0 ** 20
SAMPLE = "sample (the noisy action sequence)"
COND = "cond_encoder input: Mish(time | map embedding | observation)"
CRBS = ["unet.down_modules.0.0", "unet.down_modules.0.1", "unet.down_modules.1.0", "unet.down_modules.1.1",
        "unet.down_modules.2.0", "unet.down_modules.2.1", "unet.mid_modules.0", "unet.mid_modules.1",
        "unet.up_modules.0.0", "unet.up_modules.0.1", "unet.up_modules.1.0", "unet.up_modules.1.1"]
FINAL = "unet.final_conv.0.block.0"
RESAMPLE = ["unet.down_modules.0.2.conv", "unet.down_modules.1.2.conv", "unet.up_modules.0.2.conv", "unet.up_modules.1.2.conv"]
STEM = "encoder.resnet18.conv1"


def gn_layers():
    """Every GroupNorm conv layer of the U-Net: name -> (level of its C_out, level of its L)."""
    out = {}
    for crb in CRBS:
        part = crb.split(".")
        if part[1] == "down_modules":
            lv = (int(part[2]), int(part[2]))
        elif part[1] == "mid_modules":
            lv = (2, 2)
        else:                                         # up_modules.0: C1 at L2; up_modules.1: C0 at L1 (the upsample comes after)
            lv = (1 - int(part[2]), 2 - int(part[2]))
        out[crb + ".blocks.0.block.0"] = lv
        out[crb + ".blocks.1.block.0"] = lv
    out[FINAL] = (0, 0)
    return out


def runs_fused(cout, L, sixteen_bit=True):
    """DESIGN's rule (emit_block): the GroupNorm epilogue is fused into the GEMM iff ..."""
    return cout % 256 == 0 and cout // 8 in (64, 128, 256) and (L % 16 == 0 or (L in (8, 4) and sixteen_bit))


def unfused_by_rule(dims, P):
    return {n for n, (ci, li) in gn_layers().items() if not runs_fused(dims[ci], P >> li)}


def encoder_slots(net):
    names = [STEM]
    for li in range(1, 5):
        for bi in range(2):
            pre = f"encoder.resnet18.layer{li}.{bi}"
            names.append(pre + ".bn1")
            if dict(net.named_modules())[pre].downsample is not None:
                names.append(pre + ".downsample.1")
            names.append(pre + ".bn2")
    return names


def unet_slots(net):
    mods = dict(net.named_modules())
    names = [COND, SAMPLE]
    for crb in CRBS:
        names.append(crb + ".blocks.0.block.0")
        if isinstance(mods[crb + ".residual_conv"], torch.nn.Conv1d):
            names.append(crb + ".residual_conv")
        names.append(crb + ".blocks.1.block.0")
    return names + RESAMPLE + [FINAL]


def all_slots(net):
    return unet_slots(net) + encoder_slots(net)


# ------------------------------------------------------------------------------------------------ the clamping oracle
@torch.no_grad()
def clamped_run(net, noise, lm, cond, unfused):
    """One network evaluation at t = 0 with the stored points recorded and clamped -> {name: max |v| handed to the store}."""
    seen, hooks = {}, []
    mods = dict(net.named_modules())

    def see(name, v):
        seen[name] = max(seen.get(name, 0.0), float(v.abs().max()))
        return v.clamp(-F16_MAX, F16_MAX)

    def on_output(path, name, what=lambda v: v):
        hooks.append(mods[path].register_forward_hook(lambda m, i, o: see(name, what(o))))

    def on_input(path, name, arg=0):
        def h(m, args):
            return args[:arg] + (see(name, args[arg]),) + args[arg + 1:]
        hooks.append(mods[path].register_forward_pre_hook(h))

    on_input("unet", SAMPLE)
    for crb in CRBS:
        on_input(crb + ".cond_encoder.1", COND)
        on_input(crb + ".blocks.1.block.0", crb + ".blocks.0.block.0")          # what the FiLM epilogue stored
        on_output(crb, crb + ".blocks.1.block.0")                                # Mish(GN) + residual
        if isinstance(mods[crb + ".residual_conv"], torch.nn.Conv1d):
            on_output(crb + ".residual_conv", crb + ".residual_conv")
    on_input("unet.final_conv.1", FINAL)
    for name in RESAMPLE:
        on_output(name, name)
    for name in sorted(unfused):                                                 # conv + bias, stored before gn1d normalises it
        on_output(name, name)
    # the stem stores max-pool(ReLU(GN)); the pool windows cover the map, so its largest value is the largest ReLU(GN)
    hooks.append(mods["encoder.resnet18.bn1"].register_forward_hook(
        lambda m, i, o: (see(STEM, o.clamp(min=0)), o.clamp(-F16_MAX, F16_MAX))[1]))
    for li in range(1, 5):
        for bi in range(2):
            pre = f"encoder.resnet18.layer{li}.{bi}"
            on_input(pre + ".conv2", pre + ".bn1")                               # ReLU(GN)
            on_output(pre, pre + ".bn2")                                         # ReLU(GN + identity)
            if mods[pre].downsample is not None:
                on_output(pre + ".downsample.1", pre + ".downsample.1")
    try:
        B = noise.shape[0]
        net(sample=noise, local_map=lm, timestep=torch.zeros(B), global_cond=cond)
    finally:
        for h in hooks:
            h.remove()
    return seen


def predict(seen):
    """-> (the names the guard must report, {name: max / 65504})."""
    return {n for n, m in seen.items() if m > F16_MAX}, {n: m / F16_MAX for n, m in seen.items()}


def in_band(ratios):
    """Stored points whose maximum lies within a factor 2 of 65504 (or is not finite): the f16 instantiations' own error could
    move such a name across the line, so a network that has one is no test network."""
    return {n: r for n, r in ratios.items() if not (r < 0.5 or 2.0 < r < float("inf"))}


# ------------------------------------------------------------------------------------------------ drivers
def driver_params(driver):
    """The state-dict prefixes a weight driver scales (weight and bias of each); [] for the two input slots."""
    kind, name = driver
    if kind == "pre":
        assert name in gn_layers(), name
        return [name]
    if name in (SAMPLE, COND):
        return []
    if name == STEM:
        return ["encoder.resnet18.bn1"]
    if name.startswith("encoder."):
        return [name]                                                            # the named GroupNorm's gamma and beta
    if name.endswith(".blocks.0.block.0") and name != FINAL:
        return [name[:-len(".blocks.0.block.0")] + ".cond_encoder.1"]            # FiLM scale and bias
    if name.endswith(".block.0"):
        return [name[:-1] + "1"]                                                 # GroupNorm gamma and beta
    return [name]                                                                # a plain-store conv


@contextlib.contextmanager
def driven(net, drivers):
    """`net` with the weight drivers applied, restored bit for bit afterwards."""
    sd = net.state_dict()
    saved = {}
    with torch.no_grad():
        for d in drivers:
            for prefix in driver_params(d):
                for leaf in (".weight", ".bias"):
                    t = sd[prefix + leaf]
                    saved.setdefault(prefix + leaf, t.clone())
                    t.mul_(PRE if d[0] == "pre" else POST)
    try:
        yield net
    finally:
        with torch.no_grad():
            for k, t in saved.items():
                sd[k].copy_(t)


def drive_inputs(drivers, noise, cond, rows=slice(None)):
    """The input drivers of `drivers` on the given rows -> (noise, cond), copies."""
    noise, cond = noise.clone(), cond.clone()
    if ("post", SAMPLE) in drivers:
        noise[rows] *= POST
    if ("post", COND) in drivers:
        cond[rows] *= POST
    return noise, cond


def post_drivers(net):
    return [("post", n) for n in all_slots(net)]


def pre_drivers():
    return [("pre", n) for n in gn_layers()]
