"""CPU checks of tests/denoiser_launch_ref.py, the float64 restatement that tests/test_gpu_denoiser_launches.py holds every launch to.

COMPOSITION -- with nothing rounded, the launch functions chained from the network's inputs ARE the reference network: every tap
of tests/test_gpu_denoiser.py::LAYERS and x1 equal the float64 copy of the oracle to 1e-10 of the tap's rms (car `large` at
P = 64, ant `large` at P = 16, B = 2).  So the restatement is the reference's network, not the device's.
PACK -- the weight rounding against hand-worked values.
MUTANTS -- the gap the per-launch test closes, shown without a device: the float32 pass of the restatement in bf16 storage is a
healthy candidate; five defects of the kinds the tile kernels have had are applied inside it, one at a time.  The per-launch
check must reject every one; the end-to-end bounds of tests/test_gpu_denoiser.py (check_close under TOL[0], at the tap that
follows the launch, against the fp32 oracle run from the inputs) let at least three of them pass."""
import copy

import numpy as np
import pytest
import torch

from tests import denoiser_launch_ref as R
from tests.test_gpu_denoiser import LAYERS, TOL, check_close, tap_to_blc
from tests.test_gpu_denoiser_shapes import _inputs, _oracle_net, _rows, _run_with_taps, _time_embedding64

TAPS = [name for name, _ in LAYERS if name != "enc.pool"]


def _plan_inputs(noise, lm, cond):
    return {"sample": noise, "local_map": lm, "cond": cond, "timestep": 0.0, "dt": 1.0}


def _sd(net):
    return {k: v.detach() for k, v in net.state_dict().items()}


@pytest.mark.parametrize("family,P", [("car", 64), ("ant", 16)])
def test_chained_launches_are_the_reference_network(family, P):
    net = _oracle_net(family, "large")
    rows = _rows(_inputs(family, P), slice(0, 2))
    n64 = copy.deepcopy(net).double()
    n64.unet.time_embedding = _time_embedding64(n64.unet)
    x_ref, taps = _run_with_taps(n64, *rows, dtype=torch.float64)
    del n64
    plan = R.Plan(_sd(net), P, None)
    bufs = plan.chain(_plan_inputs(*rows), torch.float64)
    worst = {}
    for name in TAPS + ["x1"]:
        ref = x_ref if name == "x1" else tap_to_blc(taps[name], 2)
        got = bufs[name].numpy()
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        worst[name] = float(np.abs(got - ref).max() / np.sqrt(np.mean(ref ** 2)))
    assert max(worst.values()) < 1e-10, worst
    # and every named buffer of the plan is produced: the device test reads them all
    for l in plan.launches:
        assert l.out.split("#")[0] in bufs, l.name


def test_pack_rounding_hand_worked():
    t = lambda *v: torch.tensor(v, dtype=torch.float32)
    # bf16, 8 significand bits: 1 + 2^-8 is a tie -> even (1); 1 + 3 * 2^-8 is a tie -> even (1 + 2^-6); 1 + 2^-8 + 2^-20 goes up
    hi, lo = R.pack(t(1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, -0.3), "bf16")
    assert lo is None and hi.dtype == torch.float64
    assert hi.tolist() == [1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7, -0.30078125]
    # the split keeps the remainder: hi + lo = w where 16 bits hold it, lo = rnd16(w - hi) where they do not
    hi, lo = R.pack(t(1 + 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, 1 + 2.0 ** -18), "bf16x3")
    assert hi.tolist() == [1.0, 1 + 2.0 ** -7, 1.0]
    assert lo.tolist() == [2.0 ** -8, -(2.0 ** -8), 2.0 ** -18]                       # (-2^-8 + 2^-20 has 13 bits: 8 keep -2^-8)
    # f16 without the scale would lose 2^-26 (below the smallest subnormal 2^-24); max |w| = 2^-3 is scaled by 2^16 to 2^13 exactly
    hi, _ = R.pack(t(2.0 ** -3, 2.0 ** -26, 2.0 ** -3 * (1 + 2.0 ** -11), 2.0 ** -3 * (1 - 2.0 ** -12)), "f16")
    assert hi.tolist() == [2.0 ** -3, 2.0 ** -26, 2.0 ** -3, 2.0 ** -3]             # (tie to even; the nearest below 2^13 is 2^13 itself)
    # a maximum exactly at a power of two sits at the LOW end of [2^13, 2^14): one bit more and the scale halves
    hi, _ = R.pack(t(1.0, 2.0 ** -38), "f16")                                        # scale 2^13: 2^-38 -> 2^-25, a tie to 0
    assert hi.tolist() == [1.0, 0.0]
    hi, _ = R.pack(t(1.0 - 2.0 ** -24, 2.0 ** -38), "f16")                           # max just below 1: scale 2^14, 2^-38 -> 2^-24 survives
    assert hi.tolist() == [1.0, 2.0 ** -38]
    hi, lo = R.pack(t(0.1, -0.7), "f16x3")                                           # 22 bits: within 2^-22 relative of w
    w = t(0.1, -0.7).double()
    assert float(((hi + lo - w).abs() / w.abs()).max()) < 2.0 ** -22 and float((hi - w).abs().max()) > 0
    hi, lo = R.pack(t(0.1, -0.7), "f32")
    assert lo is None and torch.equal(hi, w)
    # activations: the lo plane follows from the stored sum, and truncation is not nearest
    x = torch.tensor([0.3, -1.7, 100.25], dtype=torch.float64)
    s = R.store(x, "bf16x3")
    assert torch.equal(R.store(s, "bf16x3"), s) and torch.equal(R.rnd16(s, torch.bfloat16) + R.lo_part(s, "bf16x3"), s)
    assert R.store(torch.tensor([1 + 3 * 2.0 ** -8]), "bf16", "truncate").item() == 1 + 2.0 ** -7
    assert R.store(torch.tensor([7e4]), "f16").item() == 65504.0
    assert R.ulp_storage(torch.tensor([1.0, 1.99, -2.0, 1e-6]), "bf16").tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -27]
    assert R.ulp_storage(torch.tensor([1.0, 1e-6]), "f16").tolist() == [2.0 ** -10, 2.0 ** -24]


# ------------------------------------------------------------------------------------------------ mutants
class _Bench:
    """Car `large`, P = 64, bf16, B = 2: the healthy candidate (float32 pass chained with bf16 stores) and the old oracle taps."""

    def __init__(self):
        net = _oracle_net("car", "large")
        self.sd = _sd(net)
        self.rows = _rows(_inputs("car", 64), slice(0, 2))
        x_ref, taps = _run_with_taps(net, *self.rows)                                   # the fp32 oracle of the end-to-end tests
        self.old = {n: tap_to_blc(taps[n], 2) for n in TAPS}
        self.plan = R.Plan(self.sd, 64, "bf16")
        self.cand = self.plan.chain(_plan_inputs(*self.rows), torch.float32)

    def new_check(self, name, got):
        l = self.plan.by_name[name]
        return R.check_launch(got, R.expected(l, self.plan, self.cand), l.out_fmt)

    def old_check(self, name, got, tap):
        """The candidate's buffers with `got` in place of launch `name`'s output, run on to `tap` -> check_close's complaints."""
        l = self.plan.by_name[name]
        bufs = dict(self.cand)
        self.plan.put(bufs, l, got)
        writer = [k.name for k in self.plan.launches if k.out == tap][0]
        if writer != name:
            nxt = self.plan.launches[self.plan.launches.index(l) + 1].name
            self.plan.chain(None, torch.float32, upto=writer, start=nxt, bufs=bufs)
        return check_close(bufs[tap].numpy(), self.old[tap], TOL[0], tap)


@pytest.fixture(scope="module")
def bench():
    return _Bench()


def test_healthy_candidate_passes_both_checks(bench):
    for name in TAPS:
        assert not check_close(bench.cand[name].numpy(), bench.old[name], TOL[0], name)
    for l in bench.plan.launches:
        if l.name in ("film", "prep_sample") or l.name.startswith("enc."):
            continue                                                                   # (the U-Net launches carry the mutants)
        got = bench.cand[l.out.split("#")[0]]
        if "#" in l.out:
            got = got[:, (0 if l.out.endswith("even") else 1)::2]
        res = bench.new_check(l.name, got)
        assert res["ok"], R.describe_failure(l, res, got, R.expected(l, bench.plan, bench.cand))


def _mutants(bench):
    """-> [(label, launch, its mutated stored output, the tap that follows)]"""
    plan, cand, sd = bench.plan, bench.cand, bench.sd
    out = []

    def run(p, name, bufs=cand):
        l = p.by_name[name]
        return p.stored(l, l.fn(bufs, torch.float32)[0])
    # (a) one channel-tap's weight zeroed in one k = 3 conv: 1 of 3 x 2048
    key = "unet.mid_modules.0.blocks.1.block.0.weight"
    w = sd[key].clone()
    w[:, 777, 2] = 0.0
    out.append(("a: one channel-tap zeroed", "mid1.conv2", run(R.Plan({**sd, key: w}, 64, "bf16"), "mid1.conv2"), "mid1.out"))
    # (b) one store truncates
    out.append(("b: truncating store", "d1b2.conv2", run(R.Plan(sd, 64, "bf16", store_mode={"d1b2.conv2": "truncate"}), "d1b2.conv2"), "skip1"))
    # (c) row 0 of every sample after the first reads the previous sample's last row, at a 1 x 1 residual conv only
    x = cand["d1.in"].clone()
    x[1:, 0] = cand["d1.in"][:-1, -1]
    out.append(("c: halo row from the previous sample (.res)", "d1b1.res", run(plan, "d1b1.res", {**cand, "d1.in": x}), "d1b1.out"))
    # (d) FiLM bias column off by one channel, for one channel of one block
    at, C = plan.film_cols["unet.down_modules.2.0"]
    film = cand["film"].clone()
    film[:, 0, at + C + 100] = cand["film"][:, 0, at + C + 101]
    out.append(("d: FiLM bias column off by one", "d2b1.conv1", run(plan, "d2b1.conv1", {**cand, "film": film}), "d2b1.out"))
    # (e) GroupNorm variance over n - 1
    out.append(("e: variance / (n - 1)", "u1b2.conv2", run(R.Plan(sd, 64, "bf16", ddof={"u1b2.conv2": 1}), "u1b2.conv2"), "u1b2.out"))
    return out


def test_mutants_are_rejected_per_launch_and_mostly_pass_end_to_end(bench):
    passed_old, report = [], []
    for label, name, got, tap in _mutants(bench):
        healthy = bench.cand[bench.plan.by_name[name].out]
        assert not torch.equal(got, healthy), label                                    # the defect changed something
        res = bench.new_check(name, got)
        old = bench.old_check(name, got, tap)
        report.append(f"{label}: per-launch n_bad {res['n_bad']} share {res['share']:.3g} (cap {res['cap']:.3g}) worst {res['worst_ulps']:.3g} ulp; "
                      f"end-to-end at {tap}: {'PASSES' if not old else old}")
        assert not res["ok"], (label, "not rejected by the per-launch check", report[-1])
        if not old:
            passed_old.append(label)
    print("\n".join(report))
    assert len(passed_old) >= 3, report


@pytest.mark.parametrize("fmt", ["bf16", "f32"])
def test_unfused_groupnorm_launches_on_the_small_network(fmt):
    """Car `small` runs every GroupNorm layer unfused: conv + bias is stored inside the launch, where debug_read cannot look.
    The healthy float32 candidate passes every launch, and a variance over n - 1 in one of them is still rejected."""
    from tests.range_guard_ref import runs_fused
    sd = _sd(_oracle_net("car", "small"))
    rows = _rows(_inputs("car", 64), slice(0, 3))
    fused = lambda cout, L: runs_fused(cout, L, sixteen_bit=fmt != "f32")
    plan = R.Plan(sd, 64, fmt, fused=fused)
    assert not any(fused(c, L) for c, L in ((64, 64), (128, 32), (256, 16)))
    cand = plan.chain(_plan_inputs(*rows), torch.float32)
    for l in plan.launches:
        got = cand[l.out.split("#")[0]]
        if "#" in l.out:
            got = got[:, (0 if l.out.endswith("even") else 1)::2]
        exp = R.expected(l, plan, cand)
        res = R.check_launch(got, exp, l.out_fmt)
        assert res["ok"], R.describe_failure(l, res, got, exp)
    name = "d1b2.conv2"
    bad = R.Plan(sd, 64, fmt, fused=fused, ddof={name: 1})
    l = bad.by_name[name]
    got = bad.stored(l, l.fn(cand, torch.float32)[0])
    assert not R.check_launch(got, R.expected(plan.by_name[name], plan, cand), l.out_fmt)["ok"]
