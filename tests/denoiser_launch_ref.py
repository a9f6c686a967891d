"""CPU side of tests/test_gpu_denoiser_launches.py: every launch of the denoiser's plan restated in float64.  No device code.

The plan (ditreeonlineplanner_amd/csrc/denoise_plan.hip: build_film, build_unet, build_encoder_resnet) is a fixed sequence of
launches, each reading activation buffers that an earlier launch stored and storing one buffer of its own.  A launch is
restated here from the reference network's definition (oracle/denoiser.py) and the documented storage points: take
the launch's stored input(s), apply the layer with the weights rounded as DenoiserState::pack rounds them, and return the value
the launch is about to store.  Nothing here follows the kernels' arithmetic: no tile, no summation order, no instruction.

Every function runs in float64 (the reference) or in float32 (what fp32 summation alone does to the same operands: the
yardstick `A` of the device test, and the healthy candidate of the host test's mutants).  The float32 pass evaluates Mish by the
documented formula of the instantiation: x - 2x / (n (n + 2) + 2), n = e^x, for plain 16-bit storage, torch's otherwise.

Layout: activations are channels-last, (B, L, C) for the U-Net and (B, H * W, C) for the encoder, as debug_read returns them.

Formats (include/ditree.h DITREE_PREC_*): 0 bf16, 4 f16, 3 bf16x3, 2 f16x3, 1 f32.
  weights      bf16 / f16 round to nearest even; a split format keeps hi = rnd16(w) and lo = rnd16(w - hi); f16 first multiplies
               the whole packed matrix by the power of two that puts max |w| in [2^13, 2^14) and the accumulator by its inverse;
               f32 is left as is.
  products     a split format forms hi*hi + hi*lo + lo*hi and drops lo*lo, with the activation split the same way (hi and lo
               follow from the stored sum: hi = rnd16(sum), lo = sum - hi).
  activations  rounded at the points the plan stores (the list in tests/range_guard_ref.py, the table in DESIGN 3a): a fused
               epilogue normalises, applies Mish and FiLM or adds the residual on the f32 accumulator and stores once; the
               unfused path stores conv + bias, and the GroupNorm pass reads that stored value."""
import math

import torch

F = torch.nn.functional

# name -> (16-bit element type, split, significand bits p: neighbouring storage values at v are 2^(floor(log2 |v|) + 1 - p) apart)
FORMATS = {"bf16": (torch.bfloat16, False, 8), "f16": (torch.float16, False, 11), "bf16x3": (torch.bfloat16, True, 16),
           "f16x3": (torch.float16, True, 21), "f32": (None, False, 24)}
PREC_FORMAT = {0: "bf16", 1: "f32", 2: "f16x3", 3: "bf16x3", 4: "f16"}
F16_MAX = 65504.0
MARGIN = 8.0                 # on A, for the device's other summation order
FLIP_FLOOR = 1e-3            # floor of the flip cap
CRBS = [("d0b1", "unet.down_modules.0.0"), ("d0b2", "unet.down_modules.0.1"), ("d1b1", "unet.down_modules.1.0"),
        ("d1b2", "unet.down_modules.1.1"), ("d2b1", "unet.down_modules.2.0"), ("d2b2", "unet.down_modules.2.1"),
        ("mid1", "unet.mid_modules.0"), ("mid2", "unet.mid_modules.1"), ("u0b1", "unet.up_modules.0.0"),
        ("u0b2", "unet.up_modules.0.1"), ("u1b1", "unet.up_modules.1.0"), ("u1b2", "unet.up_modules.1.1")]   # FiLM column order


# ------------------------------------------------------------------------------------------------ rounding
def rnd16(x, dt, mode="nearest"):
    """x through the 16-bit type `dt` (f16 saturates at +-65504 as the device's stores do); `truncate` chops instead."""
    x32 = x.to(torch.float32)
    if dt is torch.float16:
        x32 = x32.clamp(-F16_MAX, F16_MAX)
    if mode == "truncate":
        assert dt is torch.bfloat16
        return (x32.view(torch.int32) & -65536).view(torch.float32).to(x.dtype)
    return x32.to(dt).to(x.dtype)


def store(x, fmt, mode="nearest"):
    """The value an activation store of format `fmt` leaves behind (None: nothing is rounded)."""
    if fmt is None:
        return x
    dt, split, _ = FORMATS[fmt]
    if dt is None:
        return x.to(torch.float32).to(x.dtype)
    hi = rnd16(x, dt, mode)
    return hi + rnd16(x - hi, dt, mode) if split else hi


def lo_part(x, fmt):
    """The lo plane of a stored split activation, from the sum debug_read returns."""
    return x - rnd16(x, FORMATS[fmt][0])


def ulp_storage(ref, fmt):
    """Distance between neighbouring storage values at `ref`: 2^(floor(log2 |ref|) + 1 - p), which lies between 2^-p |ref| and
    2^(1-p) |ref|.  f16 elements have subnormals below 2^-14: nothing in an f16 plane is finer than 2^-24."""
    dt, _, p = FORMATS[fmt]
    _, e = torch.frexp(ref.abs().double())                      # |ref| = m * 2^e, m in [0.5, 1)
    u = torch.ldexp(torch.ones_like(ref, dtype=torch.float64), e - p)
    u = torch.where(ref == 0, torch.zeros_like(u), u)
    return u.clamp(min=2.0 ** -24) if dt is torch.float16 else u


_LAST_PACK = [None, None, None]


def pack(w, fmt):
    """DenoiserState::pack restated: the GEMM matrix `w` (float32, any shape, zero where the device pads) -> (hi, lo) in float64
    with the f16 scale already divided out; lo is None unless the format is split."""
    if _LAST_PACK[0] is w and _LAST_PACK[1] == fmt:             # the float32 pass of a launch follows its float64 pass
        return _LAST_PACK[2]
    src, w = w, w.double()
    if fmt is None or FORMATS[fmt][0] is None:
        return w, None
    dt, split, _ = FORMATS[fmt]
    mul = 1.0
    if dt is torch.float16:
        m = float(w.abs().max())
        if m > 0 and math.isfinite(m):
            mul = 2.0 ** (14 - math.frexp(m)[1])                # m * mul in [2^13, 2^14)
    ws = w * mul
    hi = rnd16(ws, dt)
    _LAST_PACK[:] = [src, fmt, (hi / mul, (rnd16(ws - hi, dt) / mul if split else None))]   # one layer's weights at a time
    return _LAST_PACK[2]


SEQ_ROWS = 64


def mm(x, wp, fmt, dtype):
    """x (..., K) @ w (N, K)^T with the packed pair `wp`; split formats: hi*hi + hi*lo + lo*hi = x w - x_lo w_lo.

    The float32 pass of format f32 models the one f32 effect a library GEMM hides: the f32-input MFMA (v_mfma_f32_32x32x2_f32,
    DESIGN 3a) adds two products per instruction to ONE running f32 accumulator, K / 2 roundings in a row, where a CPU GEMM
    keeps many short partial sums.  SEQ_ROWS evenly spaced rows are therefore summed as a running float32 sum over pairs of
    K; they carry that error into the launch's A (the maximum over a launch, so a sample of rows is enough)."""
    hi, lo = wp
    x = x.to(dtype)
    if lo is None:
        w = hi.to(dtype)
        y = x @ w.T
        if fmt == "f32" and dtype == torch.float32:
            K, N = w.shape[1], w.shape[0]
            x2, y2 = x.reshape(-1, K), y.reshape(-1, N).clone()
            rows = torch.unique(torch.linspace(0, x2.shape[0] - 1, min(x2.shape[0], SEQ_ROWS)).long())
            xs, wt, acc = x2[rows].contiguous(), w.T.contiguous(), torch.zeros(len(rows), N, dtype=dtype)
            for i in range(0, K, 2):
                acc.addmm_(xs[:, i:i + 2], wt[i:i + 2])
            y2[rows] = acc
            y = y2.reshape(y.shape)
        return y
    return x @ (hi + lo).to(dtype).T - lo_part(x, fmt) @ lo.to(dtype).T


def tie_slack(x, wp, fmt):
    """A stored split value whose lo plane is exactly half a step of its hi plane has two splits, (hi, +h) and (hi + 2 h, -h),
    with the same sum: debug_read cannot tell which one the device holds, and the dropped lo * lo term differs between them
    by 2 h |w_lo|.  Thousands of terms bury that far below A; the 2 to 8 live columns of the first layer do not."""
    hi, lo = wp
    if lo is None:
        return None
    x = x.double()
    xl = lo_part(x, fmt)
    other = x + xl                                                              # hi + 2 lo: a 16-bit value only at a tie
    tie = (rnd16(other, FORMATS[fmt][0]) == other) & (xl != 0)
    return (2 * xl.abs() * tie) @ lo.abs().T


# ------------------------------------------------------------------------------------------------ pieces of a layer
def mish(x, fmt):
    if x.dtype == torch.float32 and fmt in ("bf16", "f16"):
        n = torch.exp(x)
        return x - 2.0 * x / (n * (n + 2.0) + 2.0)
    return F.mish(x)


def mish_slope(z):
    sp = F.softplus(z)
    t = torch.tanh(sp)
    return t + z * (1 - t * t) * torch.sigmoid(z)


def group_norm(y, groups, gamma, beta, eps=1e-5, ddof=0):
    """GroupNorm on channels-last (B, L, C): statistics over a group's channels and all positions of a sample."""
    B, L, C = y.shape
    v = y.reshape(B, L, groups, C // groups)
    mean = v.mean(dim=(1, 3), keepdim=True)
    var = ((v - mean) ** 2).sum(dim=(1, 3), keepdim=True) / (L * (C // groups) - ddof)
    rstd = 1.0 / torch.sqrt(var + eps)
    z = ((v - mean) * rstd).reshape(B, L, C) * gamma.to(y.dtype) + beta.to(y.dtype)
    return z, rstd.expand(B, L, groups, C // groups).reshape(B, L, C)


def shifted(x, s):
    """rows l + s of every sample, zero outside (the padding rows of a padded activation)."""
    if s == 0:
        return x
    z = torch.zeros_like(x)
    if s > 0:
        z[:, :-s] = x[:, s:]
    else:
        z[:, -s:] = x[:, :s]
    return z


def conv1d(x, w, bias, fmt, dtype, stride=1, ties=False):
    """Conv1d(k, padding k // 2, stride) on (B, L, C_in) with w (C_out, C_in, k) + bias -> (B, L / stride, C_out) as one GEMM over
    K = k C_in (tap-major); with `ties` also the tie_slack of that GEMM."""
    k = w.shape[2]
    hi, lo = pack(w, fmt)
    flat = lambda m: None if m is None else m.permute(0, 2, 1).reshape(m.shape[0], -1)
    xc = torch.cat([shifted(x, t - k // 2)[:, ::stride] for t in range(k)], dim=2) if k > 1 else x
    wp = (flat(hi), flat(lo))
    y = mm(xc, wp, fmt, dtype) + bias.to(dtype)
    return (y, tie_slack(xc, wp, fmt)) if ties else y


def epilogue(y, gamma, beta, fmt, film=None, res=None, ddof=0):
    """GroupNorm(8) + Mish (+ FiLM (scale, bias), each (B, C) | + residual (B, L, C)) -> (value, d value / d y per element)."""
    z, rstd = group_norm(y, 8, gamma, beta, ddof=ddof)
    out = mish(z, fmt)
    slope = (rstd * gamma.to(y.dtype) * mish_slope(z)).abs()
    if film is not None:
        out = out * film[0].to(y.dtype)[:, None, :] + film[1].to(y.dtype)[:, None, :]
        slope = slope * film[0].to(y.dtype)[:, None, :].abs()
    if res is not None:
        out = out + res.to(y.dtype)
    return out, slope


def film_columns(sd):
    """-> {crb prefix: (first column, C_out)} of the batched FiLM output: 2 C_out columns per block, scale then bias."""
    cols, at = {}, 0
    for _, pre in CRBS:
        n = sd[pre + ".cond_encoder.1.weight"].shape[0]
        cols[pre] = (at, n // 2)
        at += n
    return cols


# ------------------------------------------------------------------------------------------------ the launches
class Launch:
    """name; layer = the state-dict name the device reports it under; ins / out = buffer names; fn(bufs, dtype) ->
    (value about to be stored, slack), slack None or a per-element allowance for what debug_read cannot see of the launch (a
    storage point inside it, an input no buffer names, a split at a tie).  An unfused GroupNorm launch appends its stored
    conv + bias, the same before the store and d out / d (conv + bias): see `expected`."""

    def __init__(self, name, layer, kind, ins, out, out_fmt, fn):
        self.name, self.layer, self.kind, self.ins, self.out, self.out_fmt, self.fn = name, layer, kind, ins, out, out_fmt, fn


class Plan:
    """The launches of one network (state dict `sd`, float32 tensors) at pred_horizon P in format `fmt` (None: the reference
    network itself, nothing rounded).  `fused(C_out, L)` says whether a GroupNorm layer runs the fused epilogue."""

    def __init__(self, sd, P, fmt, fused=lambda cout, L: True, store_mode="nearest", ddof=None):
        self.sd, self.P, self.fmt, self.fused = sd, P, fmt, fused
        self.D = sd["unet.down_modules.0.0.blocks.0.block.0.weight"].shape[1]
        self.film_cols = film_columns(sd)
        self.store_mode = store_mode                 # host-test mutants: {launch name: "truncate"}
        self.ddof = ddof or {}                       # host-test mutants: {launch name: 1}
        self.launches = []
        self._encoder()
        self._film()
        self._unet()
        self.by_name = {l.name: l for l in self.launches}

    def _add(self, name, layer, kind, ins, out, fn, out_fmt="act"):
        self.launches.append(Launch(name, layer, kind, ins, out, self.fmt if out_fmt == "act" else (None if self.fmt is None else "f32"), fn))

    def st(self, x, name=None):
        mode = self.store_mode.get(name, "nearest") if isinstance(self.store_mode, dict) else self.store_mode
        return store(x, self.fmt, mode)

    # -------------------------------------------------------------------------------------------- encoder
    def _encoder(self):
        sd, fmt, R = self.sd, self.fmt, "encoder.resnet18."

        def to_map(x):                               # (B, HW, C) -> (B, C, H, H)
            B, HW, C = x.shape
            H = int(round(math.sqrt(HW)))
            return x.transpose(1, 2).reshape(B, C, H, H)

        def to_rows(x):
            return x.reshape(x.shape[0], x.shape[1], -1).transpose(1, 2)

        def stem(b, dt):
            lm = b["local_map"].to(dt)
            x = lm.unsqueeze(1).repeat(1, 3, 1, 1)
            y = F.conv2d(x, sd[R + "conv1.weight"].to(dt), None, 2, 3)
            y = F.relu(F.group_norm(y, 4, sd[R + "bn1.weight"].to(dt), sd[R + "bn1.bias"].to(dt), 1e-5))
            return to_rows(F.max_pool2d(y, 3, 2, 1)), None
        self._add("enc.stem", R + "conv1", "encoder stem", ["local_map"], "enc.pool", stem)

        def conv_gn(conv, gn, src, stride, res, relu):
            w = sd[conv + ".weight"]
            k = w.shape[2]

            def fn(b, dt):
                x = to_map(b[src])
                H = x.shape[2]
                OH = (H + 2 * (k // 2) - k) // stride + 1
                live = [any(0 <= o * stride + t - k // 2 < H for o in range(OH)) for t in range(k)]
                mask = torch.tensor([[float(live[i] and live[j]) for j in range(k)] for i in range(k)])
                hi, lo = pack(w * mask, fmt)            # taps that only ever meet the zero padding are not packed
                xd = x.to(dt)
                if lo is None:
                    y = F.conv2d(xd, hi.to(dt), None, stride, k // 2)
                else:
                    y = F.conv2d(xd, (hi + lo).to(dt), None, stride, k // 2) - F.conv2d(lo_part(xd, fmt), lo.to(dt), None, stride, k // 2)
                y = F.group_norm(y, y.shape[1] // 16, sd[gn + ".weight"].to(dt), sd[gn + ".bias"].to(dt), 1e-5)
                if res is not None:
                    y = y + to_map(b[res]).to(dt)
                return to_rows(F.relu(y) if relu else y), None
            return fn

        cur = "enc.pool"
        for li in range(1, 5):
            for bi in range(2):
                pre, tag = f"{R}layer{li}.{bi}", f"enc.l{li}.{bi}"
                stride = 2 if (bi == 0 and li > 1) else 1
                self._add(tag + ".conv1", pre + ".bn1", "encoder conv + GN + ReLU", [cur], tag + ".t",
                          conv_gn(pre + ".conv1", pre + ".bn1", cur, stride, None, True))
                idt = cur
                if pre + ".downsample.0.weight" in sd:
                    self._add(tag + ".downsample", pre + ".downsample.1", "encoder 1x1 conv + GN", [cur], tag + ".ds",
                              conv_gn(pre + ".downsample.0", pre + ".downsample.1", cur, stride, None, False))
                    idt = tag + ".ds"
                self._add(tag + ".conv2", pre + ".bn2", "encoder conv + GN + identity + ReLU", [tag + ".t", idt], tag + ".out",
                          conv_gn(pre + ".conv2", pre + ".bn2", tag + ".t", 1, idt, True))
                cur = tag + ".out"
        self._add("enc.avgpool", R + "avgpool", "average pool", [cur], "enc.avg", lambda b, dt, cur=cur: (b[cur].to(dt).mean(dim=1, keepdim=True), None))

        def fc(b, dt):
            return mm(b["enc.avg"], pack(sd[R + "fc.weight"], fmt), fmt, dt) + sd[R + "fc.bias"].to(dt), None
        self._add("enc.fc", R + "fc", "encoder fc", ["enc.avg"], "map_emb", fc, out_fmt="f32")

    # -------------------------------------------------------------------------------------------- FiLM
    def time_embedding(self, t, dt):
        sd = self.sd
        half = 128
        f = torch.exp(torch.arange(half, dtype=dt) * -(math.log(10000) / (half - 1)))
        e = torch.as_tensor([t], dtype=dt)[:, None] * f[None, :]
        e = torch.cat((e.sin(), e.cos()), dim=-1)
        pre = "unet.diffusion_step_encoder."
        h = F.mish(F.linear(e, sd[pre + "1.weight"].to(dt), sd[pre + "1.bias"].to(dt)))
        return F.linear(h, sd[pre + "3.weight"].to(dt), sd[pre + "3.bias"].to(dt))

    def _film(self):
        sd, fmt = self.sd, self.fmt

        def feat(b, dt):
            emb = b["map_emb"].to(dt).reshape(b["map_emb"].shape[0], -1)
            f = torch.cat([self.time_embedding(b["timestep"], dt).expand(emb.shape[0], -1), emb, b["cond"].to(dt)], dim=-1)
            return mish(f, fmt)

        def fn(b, dt):
            v = feat(b, dt)
            x = self.st(v)                                                         # the stored input of every cond_encoder Linear
            w = torch.cat([sd[pre + ".cond_encoder.1.weight"] for _, pre in CRBS])  # one matrix, one f16 scale
            bias = torch.cat([sd[pre + ".cond_encoder.1.bias"] for _, pre in CRBS])
            wp = pack(w, fmt)
            slack = None
            if dt == torch.float64 and fmt is not None:
                # debug_read names no buffer for that stored input: it is known to within what float32 does to the time MLP
                # and to Mish, so an element that close to a rounding tie may sit on either side of it
                a_in = MARGIN * float((feat(b, torch.float32).double() - v).abs().max())
                slack = (self.st(v + a_in) - self.st(v - a_in)).abs() @ (wp[0] if wp[1] is None else wp[0] + wp[1]).abs().T
                slack = slack[:, None, :]
            return (mm(x, wp, fmt, dt) + bias.to(dt))[:, None, :], slack
        self._add("film", "unet.*.cond_encoder.1", "batched FiLM GEMM", ["map_emb", "cond", "timestep"], "film", fn, out_fmt="f32")

    def film_of(self, b, pre, dt):
        at, C = self.film_cols[pre]
        f = b["film"].reshape(b["film"].shape[0], -1).to(dt)
        return f[:, at:at + C], f[:, at + C:at + 2 * C]

    # -------------------------------------------------------------------------------------------- U-Net
    def _gn_conv(self, name, conv, gn, src, out, film_pre=None, res=None, first=False):
        """k = 3 conv + GroupNorm + Mish (+ FiLM | + residual).  `first`: the 1-tap im2col layer, `src` holds [x[l-1], x[l], x[l+1]]."""
        sd, fmt, D = self.sd, self.fmt, self.D
        w = sd[conv + ".weight"]

        def fn(b, dt, mid=None):
            """mid: the stored conv + bias of an unfused launch, to run the GroupNorm pass alone on it."""
            x = b[src][:, :, D:2 * D] if first else b[src]
            want = fmt is not None and dt == torch.float64
            fused = self.fused(w.shape[0], x.shape[1])
            inner = None
            raw = None
            if mid is not None:
                y = mid.to(dt)
            else:
                y, inner = conv1d(x, w, sd[conv + ".bias"], fmt, dt, ties=True) if first and want else (conv1d(x, w, sd[conv + ".bias"], fmt, dt), None)
                raw = y
                if not fused:
                    if want:                                                      # a flip of the inner store
                        inner = ulp_storage(y, fmt) + (0 if inner is None else inner)
                    y = self.st(y)                                                # conv + bias is stored, the GroupNorm pass reads it
            out, slope = epilogue(y, sd[gn + ".weight"], sd[gn + ".bias"], fmt, film=self.film_of(b, film_pre, dt) if film_pre else None,
                                  res=b[res] if res else None, ddof=self.ddof.get(name, 0))
            slack = None if inner is None else inner * slope                       # ... carried to the output
            return (out, slack) if fused or fmt is None else (out, slack, y, raw, slope)
        kind = "k3 conv + GN + Mish" + (" + FiLM" if film_pre else " + residual" if res else "")
        ins = [src] + (["film"] if film_pre else []) + ([res] if res else [])
        self._add(name, conv, ("1-tap im2col " if first else "") + kind, ins, out, fn)

    def _crb(self, tag, pre, src, out, first=False):
        sd, fmt, D = self.sd, self.fmt, self.D
        self._gn_conv(tag + ".conv1", pre + ".blocks.0.block.0", pre + ".blocks.0.block.1", src, tag + ".h", film_pre=pre, first=first)
        res = src
        if pre + ".residual_conv.weight" in sd:
            res = tag + ".res"

            def fn(b, dt):
                x = b[src][:, :, D:2 * D] if first else b[src]
                if first and fmt is not None and dt == torch.float64:
                    return conv1d(x, sd[pre + ".residual_conv.weight"], sd[pre + ".residual_conv.bias"], fmt, dt, ties=True)
                return conv1d(x, sd[pre + ".residual_conv.weight"], sd[pre + ".residual_conv.bias"], fmt, dt), None
            self._add(tag + ".res", pre + ".residual_conv", ("1-tap im2col " if first else "") + "1x1 residual conv", [src], res, fn)
        self._gn_conv(tag + ".conv2", pre + ".blocks.1.block.0", pre + ".blocks.1.block.1", tag + ".h", out, res=res)

    def _down(self, name, pre, src, out):
        sd, fmt = self.sd, self.fmt
        self._add(name, pre, "stride-2 down conv", [src], out,
                  lambda b, dt: (conv1d(b[src], sd[pre + ".weight"], sd[pre + ".bias"], fmt, dt, stride=2), None))

    def _up(self, name, pre, src, out):
        """ConvTranspose1d(C, C, 4, 2, 1): out[j] = sum over (m, k) with j = 2 m - 1 + k of x[m] W[:, :, k].  The plan runs the even
        and the odd outputs as two 2-tap GEMMs, each with a packed matrix (and an f16 scale) of its own."""
        sd, fmt = self.sd, self.fmt
        w = sd[pre + ".weight"]                                                    # (C_in, C_out, 4)

        def half(par):
            def fn(b, dt):
                x = b[src]
                taps = [k for k in range(4) if (k - 1) % 2 == par]                 # j = 2 m - 1 + k has parity `par`
                hi, lo = pack(torch.stack([w[:, :, k].T for k in taps], dim=2), fmt)   # (C_out, C_in, 2)
                y = None
                for i, k in enumerate(taps):
                    m_shift = (par + 1 - k) // 2                                    # j = 2 q + par  ->  m = q + (par + 1 - k) / 2
                    term = mm(shifted(x, m_shift), (hi[:, :, i], None if lo is None else lo[:, :, i]), fmt, dt)
                    y = term if y is None else y + term
                return y + sd[pre + ".bias"].to(dt), None
            return fn
        for par, nm in ((0, ".even"), (1, ".odd")):
            self._add(name + nm, pre, "2-tap half of the transposed up conv", [src], out + ("#even" if par == 0 else "#odd"), half(par))

    def _unet(self):
        sd, D = self.sd, self.D
        self._add("prep_sample", "sample", "im2col of the sample", ["sample"], "a0", self._prep_sample)
        self._crb("d0b1", CRBS[0][1], "a0", "d0b1.out", first=True)
        self._crb("d0b2", CRBS[1][1], "d0b1.out", "skip0")
        self._down("down0", "unet.down_modules.0.2.conv", "skip0", "d1.in")
        self._crb("d1b1", CRBS[2][1], "d1.in", "d1b1.out")
        self._crb("d1b2", CRBS[3][1], "d1b1.out", "skip1")
        self._down("down1", "unet.down_modules.1.2.conv", "skip1", "d2.in")
        self._crb("d2b1", CRBS[4][1], "d2.in", "d2b1.out")
        self._crb("d2b2", CRBS[5][1], "d2b1.out", "skip2")
        self._crb("mid1", CRBS[6][1], "skip2", "mid1.out")
        self._crb("mid2", CRBS[7][1], "mid1.out", "mid2.out")
        self._crb("u0b1", CRBS[8][1], "cat0", "u0b1.out")
        self._crb("u0b2", CRBS[9][1], "u0b1.out", "u0b2.out")
        self._up("up0", "unet.up_modules.0.2.conv", "u0b2.out", "up0.out")
        self._crb("u1b1", CRBS[10][1], "cat1", "u1b1.out")
        self._crb("u1b2", CRBS[11][1], "u1b1.out", "u1b2.out")
        self._up("up1", "unet.up_modules.1.2.conv", "u1b2.out", "final.in")
        self._gn_conv("final.conv", "unet.final_conv.0.block.0", "unet.final_conv.0.block.1", "final.in", "final.h")

        def proj(b, dt):                                                           # f32 weights in every format; x1 = x + v * dt
            v = b["final.h"].to(dt) @ sd["unet.final_conv.1.weight"][:, :, 0].to(dt).T + sd["unet.final_conv.1.bias"].to(dt)
            return b["sample"].to(dt) + v * b["dt"], None
        self._add("final.proj", "unet.final_conv.1", "final projection + flow step", ["final.h", "sample"], "x1", proj, out_fmt="f32")

    def _prep_sample(self, b, dt):
        x = b["sample"].to(dt)                                                     # (B, P, D)
        cols = torch.cat([shifted(x, -1), x, shifted(x, 1)], dim=2)
        return torch.cat([cols, torch.zeros(x.shape[0], x.shape[1], 64 - 3 * self.D, dtype=dt)], dim=2), None

    # -------------------------------------------------------------------------------------------- running
    def stored(self, launch, value):
        """What the launch leaves in its buffer."""
        return store(value, launch.out_fmt, self.store_mode.get(launch.name, "nearest") if isinstance(self.store_mode, dict) else self.store_mode)

    def put(self, bufs, launch, value):
        """File a stored output under its buffer name (the halves of an up conv interleave into one buffer)."""
        if "#" in launch.out:
            base, par = launch.out.split("#")
            if par == "even":
                bufs[base] = torch.zeros(value.shape[0], value.shape[1] * 2, value.shape[2], dtype=value.dtype)
            bufs[base][:, (0 if par == "even" else 1)::2] = value
        else:
            bufs[launch.out] = value

    CATS = {"cat0": ("mid2.out", "skip2"), "cat1": ("up0.out", "skip1")}         # [x | skip]: two views of one buffer in the plan

    def chain(self, inputs, dtype, upto=None, start=None, bufs=None):
        """Run the launches one after the other, each on what the ones before it stored -> the buffers."""
        bufs = dict(inputs) if bufs is None else bufs
        go = start is None
        for l in self.launches:
            if not go:
                go = l.name == start
                if not go:
                    continue
            for name in l.ins:
                if name in self.CATS and name not in bufs:
                    bufs[name] = torch.cat([bufs[self.CATS[name][0]], bufs[self.CATS[name][1]]], dim=2)
            self.put(bufs, l, self.stored(l, l.fn(bufs, dtype)[0]))
            if l.name == upto:
                break
        return bufs


def expected(launch, plan, bufs):
    """One launch on the given stored inputs -> dict(ref = rnd_storage(ref64), raw64, A = max |ref32 - ref64| before the storage
    rounding, own = share of elements where rnd_storage(ref32) != rnd_storage(ref64), slack)."""
    r64 = launch.fn(bufs, torch.float64)
    v64, slack = r64[:2]
    r32 = launch.fn(bufs, torch.float32)
    v32 = r32[0].double()
    ref = store(v64, launch.out_fmt)
    own = float((store(v32, launch.out_fmt) != ref).double().mean())
    if len(r64) > 2:
        # an unfused GroupNorm launch, two passes around a store that debug_read cannot see.  The device's stored conv + bias is
        # rnd(conv64 + e) with |e| <= 8 A_conv, at most 8 A_conv + one storage step from rnd(conv64): that much, carried to
        # the output by the float64 slope, is slack (for bf16 / f16 the step dominates, for f32 storage A_conv does); A itself
        # is float32's effect on the pass that reads the stored value.
        a_conv = float((r32[3].double() - r64[3]).abs().max())
        slack = slack + MARGIN * a_conv * r64[4]
        v32 = launch.fn(bufs, torch.float32, mid=r64[2])[0].double()
    return dict(ref=ref, raw64=v64, raw32=v32, A=float((v32 - v64).abs().max()), own=own, slack=slack)


def check_launch(got, exp, fmt):
    """The two bounds of a launch: every element within ulp_storage(ref64) (+ slack) + 8 A of rnd_storage(ref64), and the share
    of elements further than 8 A away at most max(8 x the reference's own share, 1e-3).
    -> dict(ok, A, bound_share, share, own, worst_ulps, n_bad, bad = mask of elements outside the element bound)."""
    got = got.double()
    ref = exp["ref"]
    d = (got - ref).abs()
    ulp = ulp_storage(exp["raw64"], fmt)
    allow = ulp + MARGIN * exp["A"]
    if exp["slack"] is not None:
        allow = allow + exp["slack"]
    bad = ~(d <= allow)                                                              # (a NaN is bad)
    share = float((d > MARGIN * exp["A"]).double().mean())
    cap = max(8.0 * exp["own"], FLIP_FLOOR)
    worst = float((d / ulp.clamp(min=1e-300)).max()) if d.numel() else 0.0
    return dict(ok=not bool(bad.any()) and share <= cap, A=exp["A"], share=share, own=exp["own"], cap=cap, worst_ulps=worst,
                n_bad=int(bad.sum()), bad=bad, max_abs=float(d.max()), rms=float(ref.pow(2).mean().sqrt()))


def describe_failure(launch, res, got, exp):
    """Names the launch, its layer, the worst element and how the violations spread over row positions and channels mod 32."""
    d = (got.double() - exp["ref"]).abs()
    B, L, C = d.shape
    b, l, c = [int(i) for i in torch.unravel_index(torch.argmax(torch.nan_to_num(d, nan=float("inf"))), d.shape)]
    bad = res["bad"]
    rows = {int(i): int(n) for i, n in enumerate(bad.sum(dim=(0, 2))) if n}
    ch = bad.sum(dim=(0, 1))
    ch32 = {i: int(ch[i::32].sum()) for i in range(min(32, C)) if int(ch[i::32].sum())}
    return (f"launch {launch.name} ({launch.kind}; layer {launch.layer}; buffer {launch.out}): {res['n_bad']} element(s) outside "
            f"ulp + {MARGIN:g} A (A {res['A']:.3g}), share beyond {MARGIN:g} A {res['share']:.3g} (cap {res['cap']:.3g}); worst "
            f"(sample {b}, row {l}, channel {c}): got {float(got[b, l, c]):.9g} ref {float(exp['ref'][b, l, c]):.9g} = "
            f"{res['worst_ulps']:.3g} ulp; violations per row position {rows}; per channel mod 32 {ch32}")
