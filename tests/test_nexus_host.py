"""Nexus on the host: the float64 reference of tests/nexus_ref.py against the goldens recorded from the reference model, the
configuration round trip, the constructor's checks, the state_dict layout and AutoModel reloading."""
import os

import pytest
import torch

import golden_cases as G
import nexus_ref as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tiny_config(**kw):
    from multivae_amd.models import NexusConfig

    base = dict(n_modalities=3, latent_dim=5, input_dims=dict(mod1=(2,), mod2=(3,), mod3=(4,)),
                modalities_specific_dim=dict(mod1=3, mod2=4, mod3=2))
    base.update(kw)
    return NexusConfig(**base)


@pytest.mark.parametrize("case", NR.NEXUS_CASES)
def test_float64_reference_matches_golden(case):
    cfg, a = G.load_case(case)
    out, grads = NR.reference_grads(cfg, a)
    assert abs(float(out["loss"]) - float(a["loss"])) <= 1e-6 * abs(float(a["loss"]))
    assert abs(float(out["loss_sum"]) - float(a["loss_sum"])) <= 1e-6 * abs(float(a["loss_sum"]))
    names = {k[len("metric/"):] for k in a if k.startswith("metric/")}
    assert names == set(out["metrics"])
    for k in names:
        ref = float(a["metric/" + k])
        assert abs(float(out["metrics"][k]) - ref) <= 1e-6 * max(1.0, abs(ref)), (k, float(out["metrics"][k]), ref)
    G.check_grads(a, grads, rtol=1e-5, atol_frac=1e-6)


def test_golden_draws_cover_the_dropout_cases():
    """The recorded keep matrices: every row keeps at least one modality; dropout_rate = 1 drops every row, with subset sizes
    1 ... M - 1."""
    for case in NR.NEXUS_CASES:
        cfg, a = G.load_case(case)
        assert (a["keep"].sum(1) >= 1).all()
    cfg, a = G.load_case("nexus_tiny_m4_drop_all")
    assert set(a["keep"].sum(1).astype(int).tolist()) == {1, 2, 3}


def test_config_json_round_trip(tmp_path):
    from multivae_amd.models import AutoConfig, NexusConfig

    cfg = _tiny_config(bottom_betas=dict(mod1=0.5, mod2=1.0, mod3=2.0), gammas=dict(mod1=1.0, mod2=3.0, mod3=1.0),
                       dropout_rate=0.3, msg_dim=7, top_beta=0.5, warmup=5, adapt_top_decoder_variance=["mod2"])
    cfg.save_json(str(tmp_path), "model_config")
    back = NexusConfig.from_json_file(str(tmp_path / "model_config.json"))
    assert back == cfg and back.name == "NexusConfig"
    assert AutoConfig.from_json_file(str(tmp_path / "model_config.json")) == cfg
    d = NexusConfig()
    assert (d.msg_dim, d.aggregator, d.warmup, d.dropout_rate, d.top_beta) == (10, "mean", 20, 0, 1)


def test_constructor_checks():
    from multivae_amd.models import Nexus, NexusConfig
    from multivae_amd.models.base.base_config import BaseAEConfig
    from multivae_amd.models.nn.default_architectures import Decoder_AE_MLP, Encoder_VAE_MLP

    with pytest.raises(AttributeError):
        Nexus(NexusConfig(n_modalities=3, latent_dim=5, input_dims=dict(mod1=(2,), mod2=(3,), mod3=(4,))))
    with pytest.raises(AttributeError):
        Nexus(_tiny_config(bottom_betas=dict(mod1=1.0, mod2=1.0)))
    with pytest.raises(AttributeError):
        Nexus(_tiny_config(gammas=dict(mod1=1.0, mod2=1.0, other=1.0)))
    with pytest.raises(AttributeError):
        Nexus(_tiny_config(adapt_top_decoder_variance=["nope"]))
    dec = {m: Decoder_AE_MLP(BaseAEConfig(input_dim=(s,), latent_dim=5)) for m, s in dict(mod1=3, mod2=4, mod3=2).items()}
    with pytest.raises(AttributeError):
        Nexus(_tiny_config(), top_encoders=dec)
    enc = {m: Encoder_VAE_MLP(BaseAEConfig(input_dim=(s,), latent_dim=10)) for m, s in dict(mod1=3, mod2=4, mod3=2).items()}
    with pytest.raises(AttributeError):
        Nexus(_tiny_config(), top_decoders=enc)
    with pytest.raises(AttributeError):
        Nexus(_tiny_config(), joint_encoder=torch.nn.Linear(10, 5))
    cfg = _tiny_config()
    cfg.aggregator = "sum"
    with pytest.raises(AttributeError):
        Nexus(cfg)
    model = Nexus(_tiny_config(warmup=7), top_encoders=enc, top_decoders=dec,
                  joint_encoder=Encoder_VAE_MLP(BaseAEConfig(input_dim=(10,), latent_dim=5)))
    assert model.start_keep_best_epoch == 8 and model.model_name == "NEXUS"
    assert model.model_config.custom_architectures == ["top_decoders", "top_encoders", "joint_encoder"]
    assert model.graph_key(epoch=3) == 3 and model.graph_key(epoch=30) == 7
    with pytest.raises(NotImplementedError):
        model.compute_joint_nll(None)


@pytest.mark.parametrize("case", NR.NEXUS_CASES)
def test_state_dict_layout_equals_the_reference(case):
    from multivae_amd.models import Nexus, NexusConfig

    cfg, _ = G.load_case(case)
    dims = NR.case_dims(cfg)
    model = Nexus(NexusConfig(n_modalities=len(cfg["names"]), latent_dim=cfg["L"], input_dims=dict(dims),
                              modalities_specific_dim=dict(cfg["S"]), msg_dim=cfg["msg_dim"]))
    got = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    assert got == cfg["sd_shapes"]


def test_automodel_reloads_a_saved_folder(tmp_path):
    from multivae_amd.models import AutoModel, Nexus

    torch.manual_seed(0)
    model = Nexus(_tiny_config(dropout_rate=0.2, adapt_top_decoder_variance=["mod1"]))
    model.save(str(tmp_path / "m"))
    back = AutoModel.load_from_folder(str(tmp_path / "m"))
    assert type(back) is Nexus and back.model_config == model.model_config
    sd = back.state_dict()
    assert all(torch.equal(v, sd[k]) for k, v in model.state_dict().items())
    assert back.adapt_top_decoder_variance == ["mod1"]


def test_forward_path_draws_nothing_on_the_host():
    """FPD and the reparameterisation noise come from the device generator: no host RNG or host synchronisation in the model."""
    src = open(os.path.join(ROOT, "multivae_amd", "models", "nexus", "nexus_model.py")).read()
    for bad in ("torch.randperm", "np.random", ".item()"):
        assert bad not in src, bad
