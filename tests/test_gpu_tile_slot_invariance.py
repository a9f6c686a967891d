"""A sample's result does not depend on the slot of the 256-row tile it occupies.

The MFMA tile kernels put 256 / L samples into one tile; the sample in slot sb starts at LDS row sb * (L + 2), so the XOR
swizzle keys of its rows, and with them the addresses its activation fragments are read from, differ from slot to slot.  A
wrong address for one (row block, tap) pair of one slot reads another row: the parity suites, whose oracle is the fp32 network,
would see it too, but only if the slot is one their small batches fill.  Here every slot is filled and compared with slot
arithmetic alone: rolling the batch by k moves sample i from slot (i mod S) to ((i + k) mod S) at every level, and

    tap(roll(X, k))[i] == tap(X)[i - k]        bit for bit, every tapped layer and the flow-step output, k = 1, 3, 7

must hold (GroupNorm cells are per sample and order-independent, the MFMA order of a row does not depend on its slot).
Together with the parity suites (slot 0 is right) this says every slot is right.

car `large`, B = 64 distinct seeded samples (one to four tiles per level, the smallest batch that fills a tile at L = 4):
  P = 64: levels L = 64 / 32 / 16, 4 / 8 / 16 slots per tile: the whole-tile halo forms with fixed fragment addresses;
  P = 16: levels L = 16 / 8 / 4: the SHORT and the six-piece forms, gemm16 at L = 8 / 4 in the unsplit formats.
"""
import numpy as np
import pytest
import torch

from oracle import geometry as G
from oracle import sampler as OS
from tests.test_gpu_denoiser import LAYERS, _make_oracle_net
from tests.util import load_maze

pytestmark = pytest.mark.gpu
TAPS = [name for name, _ in LAYERS if name != "enc.pool"]
B = 64
SHIFTS = (1, 3, 7)
PRECS = {"f16x3": 2, "bf16x3": 3, "bf16": 0, "f16": 4}


@pytest.fixture(scope="module")
def ctx():
    from ditreeonlineplanner_amd.ops import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def weights():
    """The car `large` network of tests/test_gpu_denoiser.py (live FiLM / GroupNorm terms), made once for the module."""
    return _make_oracle_net().state_dict()


_INPUTS = {}


def _inputs(P):
    if P not in _INPUTS:
        g = torch.Generator().manual_seed(11)
        maze = load_maze("boxes").astype(np.float32)
        rng = np.random.default_rng(4)
        poses = np.stack([rng.uniform(-9, 9, B), rng.uniform(-9, 9, B), rng.uniform(-3.1, 3.1, B)], axis=1)
        lm = OS.scale_local_map(G.create_local_map(maze, poses[:, 0], poses[:, 1], poses[:, 2], 20, 0.2, 1.0, (10.0, 10.0)))
        noise = torch.randn(B, P, 2, generator=g)
        cond = torch.randn(B, 7, generator=g) * 0.7
        _INPUTS[P] = (noise.cuda(), torch.tensor(lm).cuda(), cond.cuda())
    return _INPUTS[P]


def _run(ctx, inp, k):
    """One flow step on the batch rolled by k along the batch axis -> {tap: uint32 bits}, "x1" the output."""
    noise, lm, cond = (t.roll(k, 0).contiguous() for t in inp)
    out = {"x1": ctx.denoise(noise, lm, cond, want_actions=False)}
    for name in TAPS:
        out[name] = ctx.debug_read(name, B, capacity=1 << 23)
    return {n: t.cpu().numpy().view(np.uint32) for n, t in out.items()}


@pytest.mark.parametrize("P", [64, 16])
@pytest.mark.parametrize("prec", list(PRECS))
def test_result_does_not_depend_on_the_tile_slot(ctx, weights, prec, P):
    from ditreeonlineplanner_amd.model import NoisePredNet
    net = NoisePredNet(pred_horizon=P, init=False)
    net.load_state_dict(weights)
    net.bind(ctx, precision=PRECS[prec], max_batch=B)
    inp = _inputs(P)
    base = _run(ctx, inp, 0)
    assert np.isfinite(base["x1"].view(np.float32)).all()
    assert len({base["x1"][i].tobytes() for i in range(B)}) == B            # distinct samples: a roll is visible
    bad = []
    for k in SHIFTS:
        got = _run(ctx, inp, k)
        for name in ["x1"] + TAPS:
            want = np.roll(base[name], k, axis=0)                             # want[i] = base[i - k]
            diff = int((got[name] != want).sum())
            if diff:
                rows = np.nonzero((got[name] != want).reshape(B, -1).any(axis=1))[0]
                bad.append(f"{name} roll {k}: {diff} value(s) differ, samples {rows[:8].tolist()}")
    assert not bad, bad
