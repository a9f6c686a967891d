"""Generate tests/golden/encoders*.npz from the reference's own small local-map encoder classes.

Runs ONLY in the build container (needs /root/reference), like make_golden.py.  ``local_map_encoder`` is imported
unmodified; ``torchvision`` / ``torchvision.models`` (used by the 'resnet' branch only) and ``termcolor`` are satisfied with
empty in-memory placeholder modules.

    python tests/golden/make_encoder_golden.py

Cases: each of identity, mlp, max, grid, cnn at local_map_size N in {20, 16}; max at k in {3, N}.  Every case runs the 65 maps
of its N (0/1; map 0 all zero, map 1 all one, maps 2..5 a single set cell in one corner each, the rest seeded random at
mixed densities) and stores
    <case>/emb     the reference class's fp32 embeddings (65, E)
    <case>/d_ref   max |fp32 - the same module evaluated in float64|
    <case>/p/<key> the seeded parameters (state-dict keys of the encoder, without the ``encoder.`` prefix)
``keys_json`` holds the key -> shape table of ConditionalUnet1DWithLocalMap(...).state_dict() per encoder and N at
down_dims (64, 128, 256): names and shapes only.

Files: a committed file stays below 1 MiB, and the two mlp parameter sets are 0.75 MB and 0.53 MB of incompressible floats,
so they live in files of their own:
    encoders.npz          maps, embeddings, d_ref, key tables, grid / cnn parameters
    encoders_mlp20.npz    mlp_20/p/*
    encoders_mlp16.npz    mlp_16/p/*

Before anything is written the script asserts, per encoder and N, that the reference's whole network equals
oracle.denoiser.OracleUnet1D applied to cat(embedding, cond) with the same ``unet.*`` weights, bit for bit: the GPU tests
take that composition as their expectation.
"""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, REPO)
sys.path.insert(0, REF)


def _placeholders():
    for name in ("torchvision", "torchvision.models", "termcolor"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["torchvision"].models = sys.modules["torchvision.models"]
    sys.modules["termcolor"].cprint = print


_placeholders()
import local_map_encoder as ref_lme                                  # noqa: E402

from oracle import denoiser as OD                                    # noqa: E402

NMAPS = 65
SIZES = (20, 16)
DOWN = (64, 128, 256)


def make_maps(n, seed):
    rng = np.random.default_rng(seed)
    m = np.zeros((NMAPS, n, n), dtype=np.uint8)
    m[1] = 1
    for i, (r, c) in enumerate(((0, 0), (0, n - 1), (n - 1, 0), (n - 1, n - 1))):
        m[2 + i, r, c] = 1
    dens = rng.uniform(0.05, 0.95, NMAPS)
    for i in range(6, NMAPS):
        m[i] = rng.random((n, n)) < dens[i]
    return m


def encoder_cases(n):
    """(case name, encoder name, embedding_dim, module factory)"""
    return [
        (f"identity_{n}", "identity", n * n, lambda: ref_lme.IdentityEncoder()),
        (f"mlp_{n}", "mlp", n * n, lambda: ref_lme.MLPEncoder(n * n, n * n)),
        (f"max_{n}_k3", "max", 9, lambda: ref_lme.MaxEncoder(9)),
        (f"max_{n}_k{n}", "max", n * n, lambda: ref_lme.MaxEncoder(n * n)),
        (f"grid_{n}", "grid", 144, lambda: ref_lme.GridEncoder()),
        (f"cnn_{n}", "cnn", 4 * (n - 8) ** 2, lambda: ref_lme.CNNEncoder()),
    ]


def whole_network_check(enc_name, n, emb_dim, seed):
    """The reference's network == OracleUnet1D(cat(encoder(map), cond)) with shared unet.* weights; -> its key table."""
    car = n == 20
    input_dim, G, P = (2, 7, 64) if car else (8, 97, 16)
    torch.manual_seed(seed)
    net = ref_lme.ConditionalUnet1DWithLocalMap(input_dim, enc_name, emb_dim, additional_global_cond_dim=G,
                                                local_map_size=n, down_dims=list(DOWN)).eval()
    sd = net.state_dict()
    ounet = OD.OracleUnet1D(input_dim, emb_dim + G, down_dims=DOWN).eval()
    ounet.load_state_dict({k[len("unet."):]: v for k, v in sd.items() if k.startswith("unet.")})
    g = torch.Generator().manual_seed(seed + 1)
    B = 5
    x = torch.randn(B, P, input_dim, generator=g)
    lm = (torch.rand(B, n, n, generator=g) < 0.4).float()
    cond = torch.randn(B, G, generator=g)
    t = torch.ones(B) * 7.0
    with torch.no_grad():
        want = net(x, lm, t, global_cond=cond)
        emb = net.encoder(lm)
        assert emb.shape == (B, emb_dim), (enc_name, n, emb.shape)
        got = ounet(x, t, torch.cat([emb, cond], dim=1))
    assert torch.equal(want, got), (enc_name, n, float((want - got).abs().max()))
    return {k: list(v.shape) for k, v in sd.items()}


def main():
    main_out, mlp_out, keys = {}, {20: {}, 16: {}}, {}
    for n in SIZES:
        maps = make_maps(n, 100 + n)
        main_out[f"maps_{n}"] = maps
        x32 = torch.tensor(maps, dtype=torch.float32)
        for ci, (case, enc_name, emb_dim, factory) in enumerate(encoder_cases(n)):
            torch.manual_seed(1000 * n + ci)
            mod = factory().eval()
            with torch.no_grad():
                e32 = mod(x32)
                params = {k: v.clone() for k, v in mod.state_dict().items()}
                e64 = mod.double()(x32.double())
            assert e32.shape == (NMAPS, emb_dim) and e32.dtype == torch.float32, (case, e32.shape)
            d_ref = float((e32.double() - e64).abs().max())
            if enc_name in ("identity", "max"):
                assert d_ref == 0.0
            main_out[f"{case}/emb"] = e32.numpy()
            main_out[f"{case}/d_ref"] = np.float64(d_ref)
            dst = mlp_out[n] if enc_name == "mlp" else main_out
            for k, v in params.items():
                dst[f"{case}/p/{k}"] = v.numpy()
            print(f"{case:14s} E {emb_dim:4d}  d_ref {d_ref:.3g}  |emb| mean {float(e32.abs().mean()):.3g}")
        for enc_name, emb_dim in (("identity", n * n), ("mlp", n * n), ("max", 9), ("grid", 144), ("cnn", 4 * (n - 8) ** 2)):
            keys[f"{enc_name}_{n}"] = whole_network_check(enc_name, n, emb_dim, 7 * n)
    main_out["keys_json"] = np.array(json.dumps(keys, sort_keys=True))
    np.savez_compressed(os.path.join(HERE, "encoders.npz"), **main_out)
    for n in SIZES:
        np.savez(os.path.join(HERE, f"encoders_mlp{n}.npz"), **mlp_out[n])
    for f in ("encoders.npz", "encoders_mlp20.npz", "encoders_mlp16.npz"):
        size = os.path.getsize(os.path.join(HERE, f))
        assert size < (1 << 20), (f, size)
        print(f, size, "bytes")


if __name__ == "__main__":
    main()
