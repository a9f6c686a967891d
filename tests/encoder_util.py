"""Shared by tests/test_encoders_host.py and tests/test_gpu_encoders.py: the fixture of the reference's five small local-map
encoders (tests/golden/encoders*.npz, written by tests/golden/make_encoder_golden.py from the reference's own classes), a
torch restatement of those encoders, and the (engine net, oracle U-Net) pairs the GPU tests run."""
import functools
import json

import numpy as np
import torch
import torch.nn.functional as F

from oracle import denoiser as OD
from tests.util import golden

SMALL = ("identity", "mlp", "max", "grid", "cnn")
SIZES = (20, 16)


def cases():
    """[(case name, encoder, N, embedding width)] -- every case of the fixture."""
    out = []
    for n in SIZES:
        out += [(f"identity_{n}", "identity", n, n * n), (f"mlp_{n}", "mlp", n, n * n), (f"max_{n}_k3", "max", n, 9),
                (f"max_{n}_k{n}", "max", n, n * n), (f"grid_{n}", "grid", n, 144), (f"cnn_{n}", "cnn", n, 4 * (n - 8) ** 2)]
    return out


CASES = cases()
CASE = {c[0]: c for c in CASES}


@functools.lru_cache(maxsize=None)
def fixture():
    z = dict(golden("encoders"))
    z.update(golden("encoders_mlp20"))
    z.update(golden("encoders_mlp16"))
    return z


def key_tables():
    return {k: {n: tuple(s) for n, s in v.items()} for k, v in json.loads(str(fixture()["keys_json"])).items()}


def case_params(case):
    """The seeded encoder parameters of a case as torch tensors, keyed like the encoder's state dict."""
    pre = case + "/p/"
    return {k[len(pre):]: torch.tensor(v) for k, v in fixture().items() if k.startswith(pre)}


def maps(n):
    return fixture()[f"maps_{n}"].astype(np.float32)


def restated_encoder(kind, x, params, emb_dim):
    """local_map_encoder.py:137-218 in functional torch.  x (B, N, N)."""
    p = params
    if kind == "identity":
        return torch.flatten(x, 1)
    if kind == "max":
        k = int(np.floor(np.sqrt(emb_dim)))
        return torch.flatten(F.adaptive_max_pool2d(x.unsqueeze(1), k), 1)
    if kind == "mlp":
        h = F.relu(F.linear(torch.flatten(x, 1), p["fc1.weight"], p["fc1.bias"]))
        h = F.relu(F.linear(h, p["fc2.weight"], p["fc2.bias"]))
        return F.linear(h, p["fc3.weight"], p["fc3.bias"])
    if kind == "grid":
        h = F.relu(F.conv2d(x.unsqueeze(1), p["conv1.weight"], p["conv1.bias"]))
        h = F.relu(F.conv2d(h, p["conv2.weight"], p["conv2.bias"]))
        h = F.conv2d(h, p["conv3.weight"], p["conv3.bias"])
        return torch.flatten(F.adaptive_max_pool2d(h, (6, 6)), 1)
    if kind == "cnn":
        h = x.unsqueeze(1)
        for i in (1, 2, 3, 4):
            h = F.mish(F.conv2d(h, p[f"conv{i}.weight"], p[f"conv{i}.bias"]))
        return torch.flatten(h, 1)
    raise ValueError(kind)


def shape_of(n):
    """(input_dim, obs-cond width, pred_horizon) of the car (N = 20) / ant (N = 16) network."""
    return (2, 7, 64) if n == 20 else (8, 97, 16)


def make_pair(case, dims=(64, 128, 256), seed=11):
    """-> (NoisePredNet of the case's encoder with the fixture's encoder parameters, OracleUnet1D with the same unet.* weights)."""
    from ditreeonlineplanner_amd.model import NoisePredNet
    _, kind, n, E = CASE[case]
    D, G, P = shape_of(n)
    torch.manual_seed(seed)
    ounet = OD.OracleUnet1D(D, E + G, down_dims=dims).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():       # default init leaves the FiLM / GroupNorm parameters trivial: perturb (as tests/test_gpu_denoiser.py)
        for _, p in ounet.named_parameters():
            if p.dim() == 1:
                p.add_(0.2 * torch.randn(p.shape, generator=g))
    net = NoisePredNet(input_dim=D, embedding_dim=E, additional_global_cond_dim=G, down_dims=dims, pred_horizon=P,
                       local_map_size=n, init=False, encoder=kind)
    sd = {f"unet.{k}": v for k, v in ounet.state_dict().items()}
    sd.update({f"encoder.{k}": v for k, v in case_params(case).items()})
    net.load_state_dict(sd)
    return net, ounet


class ComposedNet:
    """The oracle of a small-encoder network: ``embed(local_map)`` + OracleUnet1D on cat(embedding, cond) -- the composition
    make_encoder_golden.py asserts equal to the reference's whole network."""

    def __init__(self, ounet, embed):
        self.ounet, self.embed = ounet, embed

    def __call__(self, sample, local_map, timestep, global_cond):
        with torch.no_grad():
            return self.ounet(sample, timestep, torch.cat([self.embed(local_map), global_cond], dim=1))
