"""Host side of the six local-map encoders (local_map_encoder.py:78-97): state-dict layout, the embedding-width rule of
``init_noise_pred_net``, the manifest's ``#encoder`` line, and the torch restatement the GPU round test uses, held to the
fixture that tests/golden/make_encoder_golden.py wrote from the reference's own classes."""
import numpy as np
import pytest
import torch

from tests import encoder_util as EU


def _init(encoder, n, emb_dim=9, **kw):
    from ditreeonlineplanner_amd.train_diffusion_policy import init_noise_pred_net
    car = n == 20
    return init_noise_pred_net(input_dim=2 if car else 8, action_dim=2 if car else 8, obs_dim=3 if car else 29,
                               obs_history=1 if car else 3, action_history=1, goal_conditioned=True, goal_dim=2,
                               local_map_conditioned=True, local_map_encoder=encoder, local_map_embedding_dim=emb_dim,
                               local_map_size=n, down_dims=[64, 128, 256], **kw)


WIDTH = {"identity": lambda n: n * n, "mlp": lambda n: n * n, "max": lambda n: 9, "grid": lambda n: 144,
         "cnn": lambda n: 4 * (n - 8) ** 2}


@pytest.mark.parametrize("n", EU.SIZES)
@pytest.mark.parametrize("encoder", EU.SMALL)
def test_state_dict_layout_is_the_references(encoder, n):
    want = EU.key_tables()[f"{encoder}_{n}"]
    # identity and mlp ignore local_map_embedding_dim (train_diffusion_policy.py:46-60): pass the default 9 there
    emb = WIDTH[encoder](n) if encoder not in ("identity", "mlp") else 9
    net = _init(encoder, n, emb)
    got = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert got == want
    assert net.embedding_dim == WIDTH[encoder](n)
    # a reference checkpoint's state dict loads unchanged
    net.load_state_dict({k: torch.zeros(s) for k, s in want.items()})
    if encoder in ("identity", "max"):
        assert not [k for k in got if k.startswith("encoder.")]


def test_small_encoder_parameters_use_torch_default_bounds():
    net = _init("mlp", 20)
    sd = net.state_dict()
    for name, fan_in in (("fc1", 400), ("fc2", 128), ("fc3", 256)):
        b = 1.0 / np.sqrt(fan_in)
        for part in ("weight", "bias"):
            v = sd[f"encoder.{name}.{part}"]
            assert float(v.abs().max()) <= b and float(v.abs().max()) > 0.5 * b, (name, part)
    w = _init("cnn", 20, 576).state_dict()["encoder.conv2.weight"]
    assert float(w.abs().max()) <= 1.0 / np.sqrt(18) and float(w.std()) > 0.3 / np.sqrt(18)


def test_embedding_width_rule_and_errors():
    assert _init("identity", 16, 9).embedding_dim == 256
    assert _init("mlp", 20, 123).embedding_dim == 400
    assert _init("max", 20, 16).embedding_dim == 16
    assert _init("RESNET", 20, 32).embedding_dim == 32             # case-insensitive, as the reference's .lower()
    with pytest.raises(ValueError, match="144"):
        _init("grid", 20, 9)
    with pytest.raises(ValueError, match="576"):
        _init("cnn", 20, 9)
    with pytest.raises(ValueError, match="256"):
        _init("cnn", 16, 576)
    with pytest.raises(ValueError, match="perfect square"):
        _init("max", 20, 10)
    with pytest.raises(ValueError, match="Unknown encoder"):
        _init("vit", 20, 9)
    from ditreeonlineplanner_amd.train_diffusion_policy import init_noise_pred_net
    with pytest.raises(NotImplementedError):
        init_noise_pred_net(2, 2, 3, 1, local_map_conditioned=False, local_map_size=20)


def test_manifest_carries_the_encoder():
    from ditreeonlineplanner_amd.weights import manifest_encoder, pack_state_dict
    net = _init("max", 20, 9)
    blob, manifest = pack_state_dict(net.state_dict(), pred_horizon=64, local_map_size=20, encoder="max", embedding_dim=9)
    assert "#encoder max 9\n" in manifest and "#config pred_horizon 64 local_map_size 20\n" in manifest
    assert manifest_encoder(manifest) == ("max", 9)
    assert blob.size == sum(v.numel() for v in net.state_dict().values())
    # a manifest without the line (every blob stored so far) is a 'resnet' net
    _, old = pack_state_dict(net.state_dict(), pred_horizon=64, local_map_size=20)
    assert "#encoder" not in old and manifest_encoder(old) == ("resnet", None)
    with pytest.raises(ValueError, match="Unknown encoder"):
        pack_state_dict(net.state_dict(), encoder="vit", embedding_dim=9)
    with pytest.raises(ValueError, match="embedding_dim"):
        pack_state_dict(net.state_dict(), encoder="cnn")


def test_fixture_has_the_stated_maps():
    for n in EU.SIZES:
        m = EU.maps(n)
        assert m.shape == (65, n, n) and set(np.unique(m)) == {0.0, 1.0}
        assert m[0].sum() == 0 and m[1].sum() == n * n
        assert [m[2 + i].sum() for i in range(4)] == [1, 1, 1, 1]
        assert m[2, 0, 0] == m[3, 0, n - 1] == m[4, n - 1, 0] == m[5, n - 1, n - 1] == 1


@pytest.mark.parametrize("case", [c[0] for c in EU.CASES])
def test_restated_encoders_match_the_reference(case):
    """identity and max bit for bit; mlp, grid and cnn within d_ref = the reference's own fp32-vs-float64 difference."""
    _, kind, n, E = EU.CASE[case]
    fx = EU.fixture()
    with torch.no_grad():
        got = EU.restated_encoder(kind, torch.tensor(EU.maps(n)), EU.case_params(case), E).numpy()
    want, d_ref = fx[f"{case}/emb"], float(fx[f"{case}/d_ref"])
    assert got.shape == want.shape == (65, E) and got.dtype == np.float32
    d = float(np.abs(got.astype(np.float64) - want).max())
    print(case, "restated vs reference", d, "d_ref", d_ref)
    if kind in ("identity", "max"):
        assert d_ref == 0.0 and np.array_equal(got, want)
    else:
        assert 0.0 < d_ref < 1e-6 and d <= d_ref
