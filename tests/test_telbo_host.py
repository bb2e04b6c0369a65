"""TELBO on the host: the error constants and the mutation checks of tests/telbo_ref.py (the float64 reference and error model
behind tests/test_gpu_telbo.py) against the same formulas in plain torch fp32, the float64 restatement of both stages' losses
against the goldens recorded from the reference model, the configuration round trip, the constructor's attributes, the
custom_architectures bookkeeping, the stage hooks and encode's refusal of a proper subset."""
import os

import pytest
import torch

import golden_cases as G
import telbo_ref as R

_CACHE = {}


def torch32(case):
    """(inputs, the formulas in torch fp32, float64 reference, bases) of a case, computed once and left unchanged."""
    if case.name not in _CACHE:
        inp = R.make_inputs(case)
        ref = R.reference(case, inp)
        _CACHE[case.name] = (inp, R.run_torch32(case, inp), ref, R.bases(case, inp, ref))
    return _CACHE[case.name]


def test_case_table_holds_the_grid():
    assert len(R.CASES) == len(R.CASE_BY_NAME) == 4 * 3 * 3
    assert {c.L for c in R.CASES} == {1, 5, 64, 130} and {c.B for c in R.CASES} == {1, 3, 260} and {c.M for c in R.CASES} == {1, 2, 5}
    for null in ("dz", "gkld", "djoint_lv"):
        for M in R.MS:
            assert any(null in c.null and c.M == M for c in R.CASES), (null, M)
        for B in R.BS:
            assert any(null in c.null and c.B == B for c in R.CASES), (null, B)
    assert any(c.null == () and c.M == 5 for c in R.CASES)
    inp = R.make_inputs(R.CASE_BY_NAME["l130-b260-m2"])
    assert float(inp["lv"].min()) < -11 and float(inp["lv"].max()) > 5
    assert float(inp["jlv"].min()) < -5 and float(inp["jlv"].max()) > 5


def test_error_constants():
    """C_STAGE = 4x the largest |err| / base of the formulas in plain torch fp32 (backward: fp32 autograd) against the float64
    reference, rounded up, over the whole case table.  The measured values and the cases that set them are in the docstring of
    tests/test_gpu_telbo.py."""
    worst = {}
    for case in R.CASES:
        inp, got, ref, base = torch32(case)
        for k, v in R.ratios(case, inp, got, ref=ref, base=base).items():
            if v > worst.get(k, (-1.0, ""))[0]:
                worst[k] = (v, case.name)
    print({k: (round(v, 2), n) for k, (v, n) in sorted(worst.items())})
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
        assert all(v <= R.C_STAGE[k] for k, v in clean.items()), clean
        bad = R.ratios(case, inp, got, mut=(mut,), base=base)
        for s in stages:
            f = bad[s] / R.C_STAGE[s]
            print(mut, name, s, f"{f:.3g}x the bound")
            assert f > 1.0, f"{mut} passes {s} on {name}: {f:.3g}x the bound"


def test_every_mutation_is_covered():
    assert [t[0] for t in R.TEETH] == R.MUTATIONS


@pytest.mark.parametrize("case", R.TELBO_CASES)
def test_float64_reference_matches_golden(case):
    cfg, a = G.load_case(case)
    assert {k: cfg[k] for k in R.CASE_CONFIGS[case]} == R.CASE_CONFIGS[case]
    out, grads = R.reference_grads(cfg, a)
    stage2 = cfg["epoch"] > cfg["warmup"]
    assert list(out) == (["loss", "loss_sum", "metrics"] if stage2 else ["recon_loss", "KLD", "loss", "metrics"])
    for k in out:
        if k != "metrics":
            assert abs(float(out[k]) - float(a[k])) <= 1e-6 * max(1.0, abs(float(a[k]))), (k, float(out[k]), float(a[k]))
    names = {k[len("metric/"):] for k in a if k.startswith("metric/")}
    assert names == set(out["metrics"]) == (set(R.case_dims(cfg)) if stage2 else {"kld_joint", "recon_joint"})
    for k in names:
        ref = float(a["metric/" + k])
        assert abs(float(out["metrics"][k]) - ref) <= 1e-6 * max(1.0, abs(ref)), (k, float(out["metrics"][k]), ref)
    assert sorted(k for k, g in grads.items() if g is None) == sorted(cfg["nograd"])
    with_grad = {k: g for k, g in grads.items() if g is not None}
    assert {"gsum/" + k for k in with_grad} == {k for k in a if k.startswith("gsum/")}
    G.check_grads(a, with_grad, rtol=1e-5, atol_frac=1e-6)
    if stage2:  # only the unimodal encoders train; everything else is frozen
        assert all(k.startswith("encoders.") for k in with_grad) and cfg["frozen"] == cfg["nograd"]
    else:
        assert cfg["frozen"] == [] and all(k in cfg["nograd"] for k in grads if k.startswith("encoders."))


def _config(**kw):
    from multivae_amd.models import TELBOConfig

    base = dict(n_modalities=3, latent_dim=4, input_dims=dict(m1=(2,), m2=(3,), m3=(2, 2)), warmup=3)
    base.update(kw)
    return TELBOConfig(**base)


def test_config_json_round_trip(tmp_path):
    from multivae_amd.models import AutoConfig, TELBOConfig

    d = TELBOConfig(n_modalities=2, latent_dim=3)
    assert (d.warmup, d.lambda_factors, d.gamma_factors, d.uses_likelihood_rescaling, d.custom_architectures) == (10, None, None, True, [])
    for i, cfg in enumerate((_config(), _config(lambda_factors=dict(m1=0.5, m2=2.0, m3=1.5), gamma_factors=dict(m1=1.0, m2=0.25, m3=3.0),
                                             uses_likelihood_rescaling=False, decoders_dist=dict(m1="normal", m2="laplace", m3="bernoulli"),
                                             decoder_dist_params=dict(m1=dict(scale=0.75))))):
        cfg.save_json(str(tmp_path), f"c{i}")
        back = TELBOConfig.from_json_file(str(tmp_path / f"c{i}.json"))
        assert back == cfg and back.name == "TELBOConfig" and back.input_dims["m3"] == (2, 2)
        assert AutoConfig.from_json_file(str(tmp_path / f"c{i}.json")) == cfg
    ref_path = os.path.join(G.GOLDEN, R.FOLDER, "model_config.json")
    theirs = AutoConfig.from_json_file(ref_path)  # the file the reference wrote
    assert type(theirs) is TELBOConfig and theirs.warmup == R.FOLDER_CONFIG["warmup"] and theirs.lambda_factors == dict(m1=0.5, m2=2.0, m3=1.5)
    assert theirs.gamma_factors is None and theirs.uses_likelihood_rescaling is True


def test_constructor_attributes_and_custom_architectures():
    from multivae_amd.models import TELBO, BaseJointModel
    from multivae_amd.models.base.base_config import BaseAEConfig
    from multivae_amd.models.nn.default_architectures import (BaseDictEncoders, Decoder_AE_MLP, Encoder_VAE_MLP,
                                                              MultipleHeadJointEncoder)

    plain = TELBO(_config())
    assert isinstance(plain, BaseJointModel) and plain.model_name == "TELBO" and plain.model_config.custom_architectures == []
    assert plain.warmup == 3 and plain.reset_optimizer_epochs == [3]  # `warmup`, not `warmup + 1`
    assert plain.lambda_factors == plain.rescale_factors and plain.gamma_factors == plain.rescale_factors
    assert {m: float(v) for m, v in plain.rescale_factors.items()} == dict(m1=2.0, m2=4.0 / 3.0, m3=1.0)
    ones = TELBO(_config(uses_likelihood_rescaling=False))
    assert ones.lambda_factors == dict(m1=1, m2=1, m3=1) == ones.gamma_factors
    lam, gam = dict(m1=0.5, m2=2.0, m3=1.5), dict(m1=1.0, m2=0.25, m3=3.0)
    given = TELBO(_config(lambda_factors=lam, gamma_factors=gam))
    assert given.lambda_factors == lam and given.gamma_factors == gam
    keys = [k.split(".")[0] for k, _ in plain.named_parameters()]
    assert sorted(set(keys), key=keys.index) == ["decoders", "encoders", "joint_encoder"]  # the reference's registration order
    # the stages, as a trainer sees them
    assert plain.graph_key(epoch=3) == 1 and plain.graph_key(epoch=4) == 2 and plain.graph_key() == 1
    names = {id(p): k for k, p in plain.named_parameters()}
    one = [names[id(p)] for p in plain.stage_parameters(3)]
    assert one and not any(k.startswith("encoders.") for k in one) and all(p.requires_grad for p in plain.parameters())
    two = [names[id(p)] for p in plain.stage_parameters(4)]
    assert two == [k for k, _ in plain.named_parameters() if k.startswith("encoders.")]
    assert all(p.requires_grad == k.startswith("encoders.") for k, p in plain.named_parameters())
    # custom architectures
    cfg = _config()
    dims = cfg.input_dims
    enc = {m: Encoder_VAE_MLP(BaseAEConfig(input_dim=d, latent_dim=4)) for m, d in dims.items()}
    dec = {m: Decoder_AE_MLP(BaseAEConfig(input_dim=d, latent_dim=4)) for m, d in dims.items()}
    joint = MultipleHeadJointEncoder(BaseDictEncoders(dims, 4), cfg)
    assert TELBO(cfg, encoders=enc, decoders=dec, joint_encoder=joint).model_config.custom_architectures == \
        ["encoders", "decoders", "joint_encoder"]
    assert TELBO(_config(), joint_encoder=joint).model_config.custom_architectures == ["joint_encoder"]
    with pytest.raises(AttributeError):
        TELBO(_config(), joint_encoder=torch.nn.Linear(2, 2))


def test_encode_refuses_a_proper_subset():
    from multivae_amd.data.datasets.base import DatasetOutput
    from multivae_amd.models import TELBO

    model = TELBO(_config())
    inputs = DatasetOutput(data=dict(m1=torch.rand(2, 2), m2=torch.rand(2, 3), m3=torch.rand(2, 2, 2)))
    with pytest.raises(ValueError, match="Conditioning on subset"):
        model.encode(inputs, cond_mod=["m1", "m3"])


def test_state_dict_layout_equals_the_goldens():
    from multivae_amd.models import TELBO, TELBOConfig

    cfg, _ = G.load_case("telbo_tiny_stage2_factors")
    model = TELBO(TELBOConfig(**R.config_kwargs(cfg)))
    assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == \
        [(k, tuple(v.shape)) for k, v in R.case_state_dict(cfg).items()]
    assert [k for k, _ in model.named_parameters() if not k.startswith("encoders.")] == cfg["frozen"]
