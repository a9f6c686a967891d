"""The split formats' weight layout changes no bit: chunk-interleaved (the default: the 32 channels of a K-step are one 128-byte
unit [32 hi | 32 lo]) against planar (`DITREE_SPLIT_PLANAR=1`, read when a workspace is built), two binds in one process.

The layout only says where the tile kernels fetch a staged byte from: the same bytes land in the same LDS slots and no
arithmetic moves, so the expected difference is zero and every comparison here is of bits.  Covered:
  car `large` at P = 16   levels L = 16 / 8 / 4: the SHORT and the six-piece (L = 4) halo instantiations, the gemm16 short epilogue;
  car `large` at P = 64   the benchmark's network;
  ant `large` at P = 16   the ant-sized network (8 action dimensions, 16 x 16 maps);
  batches 1, 17 and 65    65 crosses the 64-sample tile of L = 4 and the padding to the batch granule;
  f16x3 and bf16x3;
every tapped layer through debug_read, the encoder's embedding, the FiLM table and the output x1.  Also the opt-in latency
mode (`DITREE_DENOISE_SPLITK=1`) at batch 1, and one planner round of 64 candidates through ExpansionEngine."""
import numpy as np
import pytest
import torch

from oracle import geometry as G
from tests.test_gpu_denoiser_shapes import TAPS, _denoise, _device_net, _inputs, _oracle_net
from tests.util import load_maze

pytestmark = pytest.mark.gpu
CONFIGS = {"car_p16": ("car", 16), "car_p64": ("car", 64), "ant_p16": ("ant", 16)}
BATCHES = (1, 17, 65)
NAMES = TAPS + ["film"]                     # (TAPS holds map_emb)


@pytest.fixture(scope="module")
def ctx():
    from ditreeonlineplanner_amd.ops import Context
    c = Context(0)
    yield c
    c.close()


def _rows(family, P, B):
    """B input rows: the seeded rows of the family, repeated in order where B exceeds them."""
    t3 = _inputs(family, P)
    idx = [i % t3[0].shape[0] for i in range(B)]
    return tuple(t[idx].contiguous() for t in t3)


def _bind(ctx, family, P, prec, max_batch, planar, monkeypatch):
    monkeypatch.setenv("DITREE_SPLIT_PLANAR", "1" if planar else "0")
    net = _device_net(family, "large", P)
    net.load_state_dict(_oracle_net(family, "large").state_dict())
    net.bind(ctx, precision=prec, max_batch=max_batch)
    return net


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


def _differing(got, ref):
    """Names whose arrays differ in any bit (or in shape), with the count."""
    bad = []
    for k in ref:
        if got[k].shape != ref[k].shape or got[k].dtype != ref[k].dtype:
            bad.append((k, "shape", got[k].shape, ref[k].shape))
        elif not np.array_equal(_bits(got[k]), _bits(ref[k])):
            bad.append((k, int((_bits(got[k]) != _bits(ref[k])).sum())))
    return bad


def _call(ctx, family, P, B):
    out = {"x1": _denoise(ctx, family, *_rows(family, P, B)).cpu().numpy()}
    for name in NAMES:
        out[name] = ctx.debug_read(name, B).cpu().numpy()
    assert np.isfinite(out["x1"]).all()
    return out


@pytest.mark.parametrize("prec", [2, 3])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_layers_and_output_equal_bit_for_bit(ctx, config, prec, monkeypatch):
    family, P = CONFIGS[config]
    res = {}
    for planar in (True, False):
        _bind(ctx, family, P, prec, max(BATCHES), planar, monkeypatch)
        res[planar] = {B: _call(ctx, family, P, B) for B in BATCHES}
    for B in BATCHES:
        bad = _differing(res[False][B], res[True][B])
        assert not bad, (config, prec, B, bad)
    # (the two binds really ran the network: a layer of each level is live)
    for name in ("d0b1.out", "skip1", "mid2.out"):
        assert float(np.abs(res[False][BATCHES[-1]][name]).max()) > 0.0, name


@pytest.mark.parametrize("prec", [2, 3])
def test_latency_mode_equal_bit_for_bit(ctx, prec, monkeypatch):
    """DITREE_DENOISE_SPLITK=1 at batch 1: the SPLITK instantiations of the halo kernel read the same weights."""
    monkeypatch.setenv("DITREE_DENOISE_SPLITK", "1")
    res = {}
    for planar in (True, False):
        _bind(ctx, "car", 64, prec, 1, planar, monkeypatch)
        res[planar] = _call(ctx, "car", 64, 1)
    bad = _differing(res[False], res[True])
    assert not bad, (prec, bad)
    monkeypatch.setenv("DITREE_DENOISE_SPLITK", "0")          # the mode really ran: the one-pass sum has another order
    assert not np.array_equal(_call(ctx, "car", 64, 1)["x1"], res[False]["x1"])


def test_planner_round_equal_round_buffers(ctx, monkeypatch):
    """One round of 64 candidates through ExpansionEngine under either layout: equal round buffers and equal trees."""
    from ditreeonlineplanner_amd._lib import PREC_F16X3
    from ditreeonlineplanner_amd.engine import ExpansionEngine
    maze = load_maze("boxes")
    start = np.array([*G.cell_rowcol_to_xy([17, 2], maze), np.deg2rad(45.0), 0, 0, 0])
    goal = np.array([*G.cell_rowcol_to_xy([2, 17], maze), 0, 0, 0, 0])
    B, Hh, A = 64, 32, 8
    rng = np.random.default_rng(11)
    samples = np.zeros((B, 6))
    samples[:, 0], samples[:, 1], samples[:, 2] = rng.uniform(-9, 9, B), rng.uniform(-9, 9, B), rng.uniform(-3.1, 3.1, B)
    cond = np.tile(goal[:2], (B, 1))
    noise = torch.randn(B, Hh // A, 64, 2, generator=torch.Generator().manual_seed(3))
    res = {}
    for planar in (True, False):
        _bind(ctx, "car", 64, PREC_F16X3, B, planar, monkeypatch)
        eng = ExpansionEngine(ctx, maze, start, goal, edge_length=Hh, action_horizon=A, batch=B, capacity=1024)
        dev = ctx.device
        eng.expand_round(torch.as_tensor(samples, device=dev), torch.as_tensor(cond, device=dev), noise=noise.to(dev))
        rb = eng.rb
        res[planar] = {k: getattr(rb, k)[:B].cpu().numpy()
                       for k in ("status", "parent", "chunks_run", "end_state", "states", "actions", "chunk_steps", "node_id")}
        res[planar]["tree_parents"] = np.asarray(eng.tree_snapshot()["parents"])
    bad = _differing(res[False], res[True])
    assert not bad, bad
    assert (res[False]["chunks_run"] > 0).any()                # candidates really rolled out
