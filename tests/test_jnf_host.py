"""JNF and its flows on the host.  The flow modules (multivae_amd/models/nn/flows.py) against the float64 restatement of
tests/jnf_ref.py and against the definition itself (masks from index arithmetic, strictly triangular Jacobians, the log-determinant
against slogdet of the autograd Jacobian, inverse o forward), their state-dict layout and refusals; the error constants, the
mutation checks and the sampler oracle's own condition of tests/jnf_ref.py (the reference and error model behind
tests/test_gpu_jnf.py) against the same formulas in plain torch fp32; the float64 restatement of both stages' losses against the
goldens recorded from the reference model; the configuration round trip, the constructor's checks and the stage hooks."""
import os

import pytest
import torch

import golden_cases as G
import jnf_ref as R

F64 = torch.float64
_CACHE = {}
SHAPES = [(2, 3, 1, 1), (5, 7, 3, 2), (20, 128, 3, 2)]  # (D, H, hidden layers, blocks)


def torch32(case):
    """(inputs, the formulas in torch fp32, float64 reference, bases) of a case, computed once and left unchanged."""
    if case.name not in _CACHE:
        inp = R.make_inputs(case)
        ref = R.reference(case, inp)
        _CACHE[case.name] = (inp, R.run_torch32(case, inp), ref, R.bases(case, inp, ref))
    return _CACHE[case.name]


def _maf(D, H, nh, nb, seed=0, scale=1.0):
    from multivae_amd.models.nn.flows import MAF, MAFConfig

    torch.manual_seed(seed)
    flow = MAF(MAFConfig(input_dim=(D,), n_made_blocks=nb, n_hidden_in_made=nh, hidden_size=H)).double()
    with torch.no_grad():
        for p in flow.parameters():
            p.mul_(scale)
    return flow


def _params(flow):
    """W[blk][l], b[blk][l] of a MAF module."""
    from multivae_amd.models.nn.flows import MaskedLinear

    W = [[mod.weight for mod in made.net if isinstance(mod, MaskedLinear)] for made in flow.net]
    b = [[mod.bias for mod in made.net if isinstance(mod, MaskedLinear)] for made in flow.net]
    return W, b


# ---- the flow modules -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,H,nh,nb", SHAPES)
def test_flow_modules_match_the_float64_restatement(D, H, nh, nb):
    flow = _maf(D, H, nh, nb, seed=D)
    W, b = _params(flow)
    g = torch.Generator().manual_seed(11 + D)
    x = torch.randn(6, D, generator=g, dtype=F64)
    with torch.no_grad():
        out = flow(x)
        z0, ladj = R.maf_forward(W, b, x)
        assert torch.allclose(out.out, z0, rtol=0, atol=1e-13) and torch.allclose(out.log_abs_det_jac, ladj, rtol=0, atol=1e-13)
        inv = flow.inverse(x)
        xi, li = R.maf_inverse(W, b, x)
        assert torch.allclose(inv.out, xi, rtol=0, atol=1e-12) and torch.allclose(inv.log_abs_det_jac, li, rtol=0, atol=1e-12)
        mu, lv = R.made(W[0], b[0], R.masks(D, H, nh), x)
        first = flow.net[0](x)
        assert torch.equal(first.mu, mu) and torch.equal(first.log_var, lv)


@pytest.mark.parametrize("D,H,nh,nb", SHAPES)
def test_masks_are_the_index_formulas(D, H, nh, nb):
    from multivae_amd.models.nn.flows import MaskedLinear, fused_layout, sequential_masks

    flow = _maf(D, H, nh, nb)
    for made in flow.net:
        lin = [mod for mod in made.net if isinstance(mod, MaskedLinear)]
        assert len(lin) == nh + 1
        for l, mod in enumerate(lin):
            K = D if l == 0 else H
            want = torch.zeros(mod.weight.shape)
            for o in range(mod.weight.shape[0]):
                for k in range(K):
                    if l == nh:
                        want[o, k] = float(k % (D - 1) < (o if o < D else o - D))
                    else:
                        want[o, k] = float(o % (D - 1) >= (k if l == 0 else k % (D - 1)))
            assert torch.equal(mod.mask.float(), want), (l, D, H)
            assert torch.equal(R.masks(D, H, nh)[l].float(), want)
            assert torch.equal(sequential_masks(D, [H] * nh)[l], want)
    assert fused_layout(flow)[:4] == (D, H, nh, nb)
    with torch.no_grad():  # a mask that is not the sequential one: the fused kernels must not stand in
        flow.net[-1].net[0].mask[0, 0] = 1 - flow.net[-1].net[0].mask[0, 0]
    assert fused_layout(flow) is None


@pytest.mark.parametrize("D,H,nh,nb", SHAPES)
def test_jacobian_is_triangular_and_ladj_is_its_log_determinant(D, H, nh, nb):
    flow = _maf(D, H, nh, nb, seed=3)
    x = torch.randn(D, generator=torch.Generator().manual_seed(5), dtype=F64)
    made = flow.net[0]
    for pick in ("mu", "log_var"):
        J = torch.autograd.functional.jacobian(lambda v: made(v.unsqueeze(0))[pick][0], x)
        assert float(J.triu().abs().max()) == 0.0, pick  # output d reads x[:d] only: strictly lower triangular
    J = torch.autograd.functional.jacobian(lambda v: flow(v.unsqueeze(0)).out[0], x)
    sign, logdet = torch.linalg.slogdet(J)
    assert abs(float(flow(x.unsqueeze(0)).log_abs_det_jac[0]) - float(logdet)) <= 1e-12 * max(1.0, abs(float(logdet)))
    xb = torch.randn(5, D, generator=torch.Generator().manual_seed(6), dtype=F64)
    with torch.no_grad():
        fwd = flow(xb)
        back = flow.inverse(fwd.out)
    assert float((back.out - xb).abs().max()) <= 1e-12
    assert float((back.log_abs_det_jac + fwd.log_abs_det_jac).abs().max()) <= 1e-12


def test_state_dict_keys_and_shapes():
    from multivae_amd.models.nn.flows import MADE, MADEConfig, MAF, MAFConfig, BaseNF, MaskedLinear

    flow = MAF(MAFConfig(input_dim=(5,), n_made_blocks=2, n_hidden_in_made=3, hidden_size=7))
    assert isinstance(flow, BaseNF) and flow.input_dim == (5,)
    want = []
    for i in range(2):
        for j, shape in enumerate([(7, 5), (7, 7), (7, 7), (10, 7)]):
            want += [(f"net.{i}.net.{2 * j}.weight", shape), (f"net.{i}.net.{2 * j}.bias", shape[:1]), (f"net.{i}.net.{2 * j}.mask", shape)]
    assert [(k, tuple(v.shape)) for k, v in flow.state_dict().items()] == want
    assert [k for k, _ in flow.named_parameters()] == [k for k, _ in want if not k.endswith("mask")]
    d = MAFConfig(input_dim=(3,))
    assert (d.n_made_blocks, d.n_hidden_in_made, d.hidden_size, d.include_batch_norm) == (2, 3, 128, False)
    m = MADEConfig(input_dim=(3,), output_dim=(3,))
    assert m.hidden_sizes == [128, 128, 128] and m.degrees_ordering == "sequential"
    made = MADE(MADEConfig(input_dim=(2, 2), output_dim=(2, 2), hidden_sizes=[6]))
    out = made(torch.zeros(3, 2, 2))
    assert list(out.keys()) == ["mu", "log_var"] and out.mu.shape == (3, 4) == out.log_var.shape
    lin = MaskedLinear(3, 2, torch.tensor([[1.0, 0.0, 1.0], [0.0, 0.0, 0.0]]))
    x = torch.randn(4, 3)
    assert torch.equal(lin(x), torch.nn.functional.linear(x, lin.mask * lin.weight, lin.bias))
    out = flow(torch.randn(4, 5))
    assert list(out.keys()) == ["out", "log_abs_det_jac"] and out.out.shape == (4, 5) and out.log_abs_det_jac.shape == (4,)
    assert list(flow.inverse(torch.randn(4, 5)).keys()) == ["out", "log_abs_det_jac"]


def test_flow_refusals():
    from multivae_amd.models.nn.flows import MADE, MADEConfig, MAF, MAFConfig, BaseNF

    with pytest.raises(ValueError, match="at least 2"):
        MADE(MADEConfig(input_dim=(1,), output_dim=(1,)))
    with pytest.raises(ValueError, match="at least 2"):
        MAF(MAFConfig(input_dim=(1,)))
    with pytest.raises(NotImplementedError, match="random"):
        MADE(MADEConfig(input_dim=(3,), output_dim=(3,), degrees_ordering="random"))
    with pytest.raises(AttributeError, match="degrees_ordering"):
        MADE(MADEConfig(input_dim=(3,), output_dim=(3,), degrees_ordering="other"))
    with pytest.raises(NotImplementedError, match="include_batch_norm"):
        MAF(MAFConfig(input_dim=(3,), include_batch_norm=True))
    with pytest.raises(AttributeError):
        MAF(MAFConfig())
    with pytest.raises(AttributeError):
        MADE(MADEConfig(input_dim=(3,)))
    with pytest.raises(ValueError, match="output_dim"):
        MADE(MADEConfig(input_dim=(3,), output_dim=(4,)))
    with pytest.raises(NotImplementedError):
        BaseNF()(torch.zeros(1, 2))
    with pytest.raises(NotImplementedError):
        BaseNF().inverse(torch.zeros(1, 2))


def test_fused_range():
    from multivae_amd import kernels

    ok = kernels.maf_fused_ok
    assert ok(2, 1, 1, 1, 1) and ok(512, 512, 4, 4, 8) and ok(20, 128, 3, 2, 2) and ok(20, 128, 3, 2)
    assert not ok(1, 8, 1, 1, 1) and not ok(513, 8, 1, 1, 1) and not ok(8, 0, 1, 1, 1) and not ok(8, 513, 1, 1, 1)
    assert not ok(8, 8, 0, 1, 1) and not ok(8, 8, 5, 1, 1) and not ok(8, 8, 1, 0, 1) and not ok(8, 8, 1, 5, 1)
    assert not ok(8, 8, 1, 1, 0) and not ok(8, 8, 1, 1, 9)


# ---- the reference and its error model -----------------------------------------------------------------------------------------------
def test_case_table_holds_the_grid():
    grid = [c for c in R.CASES if c.backward]
    assert len(grid) == 4 * 3 * 2 * 3 * 3 * 3 and len(R.CASES) == len(R.CASE_BY_NAME) == len(grid) + 1
    assert {(c.D, c.H, c.nh, c.nb, c.B, c.M) for c in grid} == {(D, H, nh, nb, B, M) for D in (2, 3, 20, 65) for H in (3, 64, 130)
                                                                  for nh in (1, 3) for nb in (1, 2, 3) for B in (1, 3, 70)
                                                                  for M in (1, 2, 3)}
    big = R.CASES[-1]
    assert (big.D, big.H, big.B, big.backward) == (512, 128, 3, False)
    for null in ("post", "dz", "wgrad", "ladj_inv"):
        for attr, values in (("D", R.DS), ("H", R.HS), ("nh", R.NHS), ("nb", R.NBS), ("B", R.BS), ("M", R.MS)):
            for v in values:
                assert any(null in c.null and getattr(c, attr) == v for c in grid), (null, attr, v)
    for M in R.MS:
        assert any(c.null == () and c.M == M for c in grid)
    ups = [R.make_inputs(c) for c in grid[:24]]
    assert any(i["dz0"] is None for i in ups) and any(i["dz0"] is not None and i["grows"] is not None for i in ups)
    assert any(i["dladj"] is None for i in ups) and any(i["dladj"] is not None and i["grows"] is not None for i in ups)


def test_fp32_torch_stays_inside_the_first_order_bound():
    """The bases are first-order bounds of the accumulated rounding error: the same formulas in fp32 torch sit strictly inside
    them (and are not exact) in every stage."""
    for name in ("d3-h64-n1-k1-b3-m2", "d20-h64-n3-k2-b3-m2"):
        case = R.CASE_BY_NAME[[n for n in R.CASE_BY_NAME if n.split("-null")[0] == name][0]]
        inp, got, ref, base = torch32(case)
        r = R.ratios(case, inp, got, ref=ref, base=base)
        assert all(0 < v < 1 for v in r.values()), r  # a rigorous first-order bound: fp32 torch stays inside it


def test_error_constants():
    """C_STAGE = 4x the largest |err| / base of the formulas in plain torch fp32 (backward: fp32 autograd) against the float64
    reference, rounded up, over the whole case table; every |lv| of the table stays below LV_MAX (asserted inside `bases`).  The
    measured values and the cases that set them are in the docstring of tests/test_gpu_jnf.py."""
    worst = {}
    for case in R.CASES:
        inp = R.make_inputs(case)  # not cached: 649 cases
        ref = R.reference(case, inp)
        base = R.bases(case, inp, ref)
        for k, v in R.ratios(case, inp, R.run_torch32(case, inp), ref=ref, base=base).items():
            if v > worst.get(k, (-1.0, ""))[0]:
                worst[k] = (v, case.name)
    print({k: (round(v, 3), n) for k, (v, n) in sorted(worst.items())})
    assert set(worst) == set(R.C_STAGE)
    for k, (v, name) in worst.items():
        assert 4 * v <= R.C_STAGE[k], f"{k}: torch fp32 shows {v:.3g} on {name}; C = {R.C_STAGE[k]} is less than 4x that"
        assert R.C_STAGE[k] <= 4 * v * 1.25 + 1, f"{k}: C = {R.C_STAGE[k]} is looser than 4 x {v:.3g} rounded up"


def _named(name):
    return R.CASE_BY_NAME[[n for n in R.CASE_BY_NAME if n.split("-null")[0] == name][0]]


@pytest.mark.parametrize("mut,stages,names", R.TEETH, ids=[t[0] for t in R.TEETH])
def test_tolerance_rejects_mutated_reference(mut, stages, names):
    """Every wrong variant of the reference, compared with the unmutated fp32 output, leaves the bound in each stage named for it
    on EVERY case named for it (the GPU test repeats this on the kernels' output)."""
    assert mut in R.MUTATIONS
    for name in names:
        case = _named(name)
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


def test_hmc_oracle_condition():
    """The sampler's comparison is only meaningful when no accept / reject decision can flip: every |u - alpha| of the chosen
    seed exceeds HMC_MARGIN in float64, with moves both accepted and rejected; and C_HMC is 4x the fp32 sampler's drift."""
    z, margin, accepted = R.hmc_run(F64)
    n = R.HMC["n_data"] * R.HMC["K"] * R.HMC["mcmc_steps"]
    assert margin > R.HMC_MARGIN, margin
    assert 0 < accepted < n, accepted
    z32, margin32, accepted32 = R.hmc_run(torch.float32)
    assert accepted32 == accepted and abs(margin32 - margin) < 1e-4
    v = R.worst_ratio(z32, z, R.hmc_base(z))
    print("hmc: margin", margin, "accepted", accepted, "of", n, "fp32 drift", v)
    assert 4 * v <= R.C_HMC <= 4 * v * 1.25 + 1
    # the log-density's gradient is the autograd gradient of its value, and the prior term is the reference's
    flows, post, (start_mod, start_noise, gamma, acc) = R.hmc_setup(F64)
    ln, g = R.poe_logdensity(flows, post, start_noise)
    ln0 = R.poe_logdensity(flows, post, start_noise, divide_prior=False, grad=False)
    assert torch.allclose(ln - ln0, (0.5 * (start_noise ** 2 + R.LOG_2PI)).sum(1), rtol=0, atol=1e-12)
    h = 1e-6 * torch.ones_like(start_noise)
    num = (R.poe_logdensity(flows, post, start_noise + h, grad=False) - R.poe_logdensity(flows, post, start_noise - h, grad=False)) / 2e-6
    assert torch.allclose(num, g.sum(1), rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("case", R.JNF_CASES)
def test_float64_reference_matches_golden(case):
    cfg, a = G.load_case(case)
    assert {k: cfg[k] for k in R.CASE_CONFIGS[case]} == R.CASE_CONFIGS[case]
    out, grads = R.reference_grads(cfg, a)
    stage2 = cfg["epoch"] > cfg["warmup"]
    assert list(out) == ["loss", "loss_sum", "metrics"]
    for k in ("loss", "loss_sum"):
        assert abs(float(out[k]) - float(a[k])) <= 1e-6 * max(1.0, abs(float(a[k]))), (k, float(out[k]), float(a[k]))
    names = {k[len("metric/"):] for k in a if k.startswith("metric/")}
    assert names == set(out["metrics"]) == {"kld_prior", "recon_loss", "ljm"}
    for k in names:
        ref = float(a["metric/" + k])
        assert abs(float(out["metrics"][k]) - ref) <= 1e-6 * max(1.0, abs(ref)), (k, float(out["metrics"][k]), ref)
    assert (float(a["metric/ljm"]) == 0.0) == (not stage2)
    assert sorted(k for k, g in grads.items() if g is None) == sorted(cfg["nograd"])
    with_grad = {k: g for k, g in grads.items() if g is not None}
    assert {"gsum/" + k for k in with_grad} == {k for k in a if k.startswith("gsum/")}
    G.check_grads(a, with_grad, rtol=1e-5, atol_frac=1e-6)
    if stage2:  # the unimodal encoders and the flows train; the joint model is frozen
        assert all(k.startswith(("encoders.", "flows.")) for k in with_grad) and cfg["frozen"] == cfg["nograd"]
        assert any(k.startswith("flows.") for k in with_grad)
    else:
        assert cfg["frozen"] == [] and all(k in cfg["nograd"] for k in grads if k.startswith(("encoders.", "flows.")))


# ---- the model on the host --------------------------------------------------------------------------------------------------------------
def _config(**kw):
    from multivae_amd.models import JNFConfig

    base = dict(n_modalities=3, latent_dim=4, input_dims=dict(m1=(2,), m2=(3,), m3=(2, 2)), warmup=3)
    base.update(kw)
    return JNFConfig(**base)


def test_config_json_round_trip(tmp_path):
    from multivae_amd.models import AutoConfig, JNFConfig

    d = JNFConfig(n_modalities=2, latent_dim=3)
    assert (d.warmup, d.beta, d.uses_likelihood_rescaling, d.custom_architectures) == (10, 1, False, [])
    for i, cfg in enumerate((_config(), _config(beta=2.5, uses_likelihood_rescaling=True,
                                               decoders_dist=dict(m1="normal", m2="laplace", m3="bernoulli"),
                                               decoder_dist_params=dict(m1=dict(scale=0.75))))):
        cfg.save_json(str(tmp_path), f"c{i}")
        back = JNFConfig.from_json_file(str(tmp_path / f"c{i}.json"))
        assert back == cfg and back.name == "JNFConfig" and back.input_dims["m3"] == (2, 2)
        assert AutoConfig.from_json_file(str(tmp_path / f"c{i}.json")) == cfg
    theirs = AutoConfig.from_json_file(os.path.join(G.GOLDEN, R.FOLDER, "model_config.json"))  # the file the reference wrote
    assert type(theirs) is JNFConfig and theirs.warmup == R.FOLDER_CONFIG["warmup"] and theirs.beta == R.FOLDER_CONFIG["beta"]
    assert theirs.custom_architectures == []


def test_constructor_flows_and_stage_hooks():
    from multivae_amd.models import JNF, BaseJointModel
    from multivae_amd.models.nn.flows import MAF, BaseNF, MAFConfig

    plain = JNF(_config(beta=0.5))
    assert isinstance(plain, BaseJointModel) and plain.model_name == "JNF" and plain.model_config.custom_architectures == []
    assert plain.warmup == 3 and plain.beta == 0.5 and plain.reset_optimizer_epochs == [4]  # `warmup + 1`, not TELBO's `warmup`
    assert list(plain.flows.keys()) == ["m1", "m2", "m3"]
    for f in plain.flows.values():
        assert type(f) is MAF and f.input_dim == (4,) and len(f.net) == 2 and f.hidden_size == 128
    keys = [k.split(".")[0] for k, _ in plain.named_parameters()]
    assert sorted(set(keys), key=keys.index) == ["decoders", "encoders", "joint_encoder", "flows"]  # the reference's order
    assert "flows.m2.net.1.net.6.mask" in plain.state_dict() and plain.state_dict()["flows.m2.net.1.net.6.mask"].shape == (8, 128)
    # the stages, as a trainer sees them
    assert plain.graph_key(epoch=3) == 1 and plain.graph_key(epoch=4) == 2 and plain.graph_key() == 1
    names = {id(p): k for k, p in plain.named_parameters()}
    one = [names[id(p)] for p in plain.stage_parameters(3)]
    assert one and not any(k.startswith(("encoders.", "flows.")) for k in one) and all(p.requires_grad for p in plain.parameters())
    two = [names[id(p)] for p in plain.stage_parameters(4)]
    assert two == [k for k, _ in plain.named_parameters() if k.startswith(("encoders.", "flows."))]
    assert all(p.requires_grad == k.startswith(("encoders.", "flows.")) for k, p in plain.named_parameters())
    # custom flows
    mine = {m: MAF(MAFConfig(input_dim=(4,), n_made_blocks=1, hidden_size=8)) for m in ("m1", "m2", "m3")}
    custom = JNF(_config(), flows=mine)
    assert custom.model_config.custom_architectures == ["flows"] and custom.flows["m2"] is mine["m2"]

    class Shift(BaseNF):
        def __init__(self):
            super().__init__()
            self.input_dim = (4,)
            self.shift = torch.nn.Parameter(torch.zeros(4))

        def forward(self, x, **kwargs):
            from multivae_amd.models import ModelOutput

            return ModelOutput(out=x + self.shift, log_abs_det_jac=torch.zeros(x.shape[0]))

    odd = JNF(_config(), flows=dict(m1=Shift(), m2=mine["m2"], m3=mine["m3"]))
    assert odd._binding(["m1", "m2", "m3"]) is None and odd._binding(["m1"]) is None
    with pytest.raises(AttributeError, match="keys of provided flows"):
        JNF(_config(), flows={m: mine[m] for m in ("m1", "m2")})
    with pytest.raises(AttributeError, match="BaseNF"):
        JNF(_config(), flows=dict(m1=torch.nn.Linear(4, 4), m2=mine["m2"], m3=mine["m3"]))
    with pytest.raises(AttributeError, match="BaseNF"):
        JNF(_config(), flows=dict(m1=MAF(MAFConfig(input_dim=(5,))), m2=mine["m2"], m3=mine["m3"]))


def test_state_dict_layout_equals_the_goldens():
    from multivae_amd.models import JNF, JNFConfig

    cfg, _ = G.load_case("jnf_tiny_stage2_beta_rescale")
    model = JNF(JNFConfig(**R.config_kwargs(cfg)))
    assert [(k, tuple(v.shape)) for k, v in model.named_parameters()] == \
        [(k, tuple(v.shape)) for k, v in R.case_state_dict(cfg).items()]
    assert [k for k, _ in model.named_parameters() if not k.startswith(("encoders.", "flows."))] == cfg["frozen"]
    assert {float(v) for v in model.rescale_factors.values()} == set(R.rescale_factors(cfg).values())
