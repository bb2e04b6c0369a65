"""CVAE on the host: the error constants and the mutation checks of tests/cvae_ref.py (the float64 reference and error model
behind tests/test_gpu_cvae.py) against the same formulas in plain torch fp32, the float64 restatement of the model's loss
against the goldens recorded from the reference model, the configuration round trip, the constructor's checks and the
custom_architectures bookkeeping."""
import pytest
import torch

import cvae_ref as R
import golden_cases as G

_CACHE = {}


def torch32(case):
    """(inputs, the formulas in torch fp32, float64 reference, bases) of a case, computed once and left unchanged."""
    if case.name not in _CACHE:
        inp = R.make_inputs(case)
        ref = R.reference(case, inp)
        _CACHE[case.name] = (inp, R.run_torch32(case, inp), ref, R.bases(case, inp, ref))
    return _CACHE[case.name]


def test_case_table_holds_the_grid():
    assert len(R.CASES) == len(R.CASE_BY_NAME) == 3 * 4 * 2 * 5 * 2
    assert {c.L for c in R.CASES} == {5, 64, 130} and {c.B for c in R.CASES} == {1, 3, 5, 260}
    assert {c.K for c in R.CASES} == {1, 4} and {c.pieces for c in R.CASES} == {(), (3,), (7, 1), (130,), (1024,)}
    for null in ("dzc", "gkl", "kl_rows"):
        assert any(null in c.null and c.prior for c in R.CASES) and any(null in c.null and not c.prior for c in R.CASES)
    assert any((c.L + sum(c.pieces)) % 2 == 1 for c in R.CASES)
    inp = R.make_inputs(next(c for c in R.CASES if c.prior and c.B == 260 and c.L == 130))
    assert float(inp["lv"].min()) < -11 and float(inp["lv"].max()) > 5
    assert float(inp["plv"].min()) < -5 and float(inp["plv"].max()) > 5
    d = inp["lv"] - inp["plv"]
    assert float(d.min()) < -12 and float(d.max()) > 8


def test_error_constants():
    """C_STAGE = 4x the largest |err| / base of the formulas in plain torch fp32 (backward: fp32 autograd) against the float64
    reference, rounded up, over the whole case table; the copied columns are exact.  The measured values and the cases that
    set them are in the docstring of tests/test_gpu_cvae.py."""
    worst = {}
    for case in R.CASES:
        inp, got, ref, base = torch32(case)
        for k, v in R.ratios(case, inp, got, ref=ref, base=base).items():
            if v > worst.get(k, (-1.0, ""))[0]:
                worst[k] = (v, case.name)
    print({k: (round(v, 2), n) for k, (v, n) in sorted(worst.items())})
    assert worst.pop("cond")[0] == 0.0
    assert set(worst) == set(R.C_STAGE)
    for k, (v, name) in worst.items():
        assert 4 * v <= R.C_STAGE[k], f"{k}: torch fp32 shows {v:.3g} on {name}; C = {R.C_STAGE[k]} is less than 4x that"
        assert R.C_STAGE[k] <= 4 * v * 1.25 + 1, f"{k}: C = {R.C_STAGE[k]} is looser than 4 x {v:.3g} rounded up"


@pytest.mark.parametrize("mut,stages,names", R.TEETH, ids=[t[0] for t in R.TEETH])
def test_tolerance_rejects_mutated_reference(mut, stages, names):
    """Every wrong variant of the reference, compared with the unmutated fp32 output, leaves the bound in each stage named for it
    on EVERY case named for it (the GPU test repeats this on the kernel's output)."""
    assert mut in R.MUTATIONS
    for name in names:
        case = R.CASE_BY_NAME[name]
        inp, got, ref, base = torch32(case)
        clean = R.ratios(case, inp, got, ref=ref, base=base)
        assert all(v <= R.C_STAGE.get(k, 0.0) for k, v in clean.items()), clean
        bad = R.ratios(case, inp, got, mut=(mut,), base=base)
        for s in stages:
            f = bad[s] / R.C_STAGE.get(s, 1.0)
            print(mut, name, s, f"{f:.3g}x the bound")
            assert f > 1.0, f"{mut} passes {s} on {name}: {f:.3g}x the bound"


def test_every_mutation_is_covered():
    assert [t[0] for t in R.TEETH] == R.MUTATIONS


@pytest.mark.parametrize("case", R.CVAE_CASES)
def test_float64_reference_matches_golden(case):
    cfg, a = G.load_case(case)
    assert {k: cfg[k] for k in R.CASE_CONFIGS[case]} == R.CASE_CONFIGS[case]
    out, grads = R.reference_grads(cfg, a)
    assert abs(float(out["loss"]) - float(a["loss"])) <= 1e-6 * abs(float(a["loss"]))
    names = {k[len("metric/"):] for k in a if k.startswith("metric/")}
    assert names == set(out["metrics"]) == {"kl", "recon_loss"}
    for k in names:
        ref = float(a["metric/" + k])
        assert abs(float(out["metrics"][k]) - ref) <= 1e-6 * max(1.0, abs(ref)), (k, float(out["metrics"][k]), ref)
    G.check_grads(a, grads, rtol=1e-5, atol_frac=1e-6)
    assert torch.allclose(out["mu"].detach().float(), G.t(a["encode/z"]), rtol=1e-5, atol=1e-6)


def _config(**kw):
    from multivae_amd.models import CVAEConfig

    base = dict(conditioning_modalities=["c1", "c2"], main_modality="x", input_dims=dict(x=(6,), c1=(5,), c2=(3, 2)), latent_dim=4)
    base.update(kw)
    return CVAEConfig(**base)


def _prior(cfg):
    from multivae_amd.models.nn.default_architectures import BaseDictEncoders, MultipleHeadJointEncoder

    dims = {m: cfg.input_dims[m] for m in cfg.conditioning_modalities}
    return MultipleHeadJointEncoder(BaseDictEncoders(dims, cfg.latent_dim), args=cfg)


def test_config_json_round_trip(tmp_path):
    from multivae_amd.models import AutoConfig, CVAEConfig

    cfg = _config(beta=2.5, decoder_dist="laplace", decoder_dist_params={"scale": 0.5})
    cfg.save_json(str(tmp_path), "model_config")
    back = CVAEConfig.from_json_file(str(tmp_path / "model_config.json"))
    assert back == cfg and back.name == "CVAEConfig" and back.input_dims["c2"] == (3, 2)
    assert AutoConfig.from_json_file(str(tmp_path / "model_config.json")) == cfg
    d = CVAEConfig(conditioning_modalities=["c"], main_modality="x")
    assert (d.input_dims, d.latent_dim, d.beta, d.decoder_dist, d.decoder_dist_params, d.custom_architectures) == \
        (None, 10, 1.0, "normal", {}, [])


def test_constructor_checks_and_custom_architectures():
    from multivae_amd.models import CVAE, CVAEConfig
    from multivae_amd.models.base import BaseModel, BaseMultiVAE
    from multivae_amd.models.base.base_config import BaseAEConfig
    from multivae_amd.models.nn.base_architectures import BaseConditionalDecoder
    from multivae_amd.models.nn.default_architectures import ConditionalDecoderMLP, Decoder_AE_MLP, Encoder_VAE_MLP

    no_dims = CVAEConfig(conditioning_modalities=["c"], main_modality="x")
    with pytest.raises(AttributeError):
        CVAE(no_dims)
    cfg = _config()
    with pytest.raises(AttributeError):  # the decoder's default needs input_dims too
        CVAE(CVAEConfig(conditioning_modalities=["c"], main_modality="x"), encoder=_prior(cfg))
    with pytest.raises(ValueError):
        CVAE(_config(), encoder=Encoder_VAE_MLP(BaseAEConfig(input_dim=(6,), latent_dim=4)))
    with pytest.raises(ValueError):
        CVAE(_config(), decoder=Decoder_AE_MLP(BaseAEConfig(input_dim=(6,), latent_dim=4)))
    with pytest.raises(ValueError):
        CVAE(_config(), prior_network=torch.nn.Linear(3, 4))
    with pytest.raises(ValueError):
        CVAE(_config(decoder_dist="normal"))._set_decoder_dist("poisson", {})
    plain = CVAE(_config())
    assert plain.model_name == "CVAE" and plain.prior_network is None and plain.model_config.custom_architectures == []
    assert isinstance(plain, BaseModel) and not isinstance(plain, BaseMultiVAE)
    assert isinstance(plain.decoder, ConditionalDecoderMLP) and isinstance(plain.decoder, BaseConditionalDecoder)
    assert plain.decoder.latent_dim == 4 and plain.decoder.all_dim == 4 + 5 + 6
    keys = list(plain.state_dict())
    assert keys[0].startswith("encoder.encoders.x.") and "decoder.network.layers.0.0.weight" in keys
    assert tuple(plain.state_dict()["decoder.network.layers.0.0.weight"].shape) == (512, 15)
    c = _config()
    dec = ConditionalDecoderMLP(4, dict(c1=(5,), c2=(3, 2)), (6,))
    model = CVAE(c, encoder=plain.encoder, decoder=dec, prior_network=_prior(c))
    assert model.model_config.custom_architectures == ["encoder", "decoder", "prior_network"]
    only_prior = CVAE(_config(), prior_network=_prior(cfg))
    assert only_prior.model_config.custom_architectures == ["prior_network"]
    with pytest.raises(ValueError):
        plain.predict(None, cond_mod=["c1"])


@pytest.mark.parametrize("case", R.CVAE_CASES)
def test_state_dict_layout_equals_the_reference(case):
    from multivae_amd.models import CVAE, CVAEConfig

    cfg, _ = G.load_case(case)
    dims = R.case_dims(cfg)
    ccfg = CVAEConfig(conditioning_modalities=list(cfg["cond"]), main_modality=cfg["main"], input_dims=dict(dims),
                      latent_dim=cfg["L"])
    model = CVAE(ccfg, prior_network=_prior(ccfg) if cfg["prior"] else None)
    assert [[k, list(v.shape)] for k, v in model.state_dict().items()] == cfg["sd_shapes"]


def test_automodel_reloads_a_saved_folder_with_a_pickled_prior_network(tmp_path):
    from multivae_amd.models import CVAE, AutoModel

    torch.manual_seed(0)
    cfg = _config(beta=0.5)
    model = CVAE(cfg, prior_network=_prior(cfg))
    model.save(str(tmp_path / "m"))
    assert (tmp_path / "m" / "prior_network.pkl").exists()
    back = AutoModel.load_from_folder(str(tmp_path / "m"))
    assert type(back) is CVAE and back.model_config == model.model_config
    sd = back.state_dict()
    assert list(sd) == list(model.state_dict()) and all(torch.equal(v, sd[k]) for k, v in model.state_dict().items())
