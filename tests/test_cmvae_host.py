"""CMVAE without a GPU: the license for the kernel's closed form (logsumexp against the reference's literal expectation over
q(c|u) = softmax + 1e-20, float64, values and every gradient, over the kernel's case table), the error constants of
tests/cmvae_ref.py re-derived from plain torch fp32, and the host side of the model (configuration, parameter names and flags
against the list recorded from the reference, argument errors, the majority vote's ties, the pruning bookkeeping)."""
import json
import math
import os

import numpy as np
import pytest
import torch

import cmvae_ref as R
import golden_cases as G

_EVAL = {}


def evaluated(case):
    """(inputs, literal float64, closed float64, closed fp32, bases, assign float64, assign fp32, assign bases): once per session."""
    if case.name not in _EVAL:
        I = R.make_inputs(case)
        ref = R.reference(case, I)
        aref = R.assign(case, I)
        _EVAL[case.name] = (I, ref, R.closed_form(case, I), R.closed_form(case, I, torch.float32), R.bases(case, I, ref), aref,
                            R.assign(case, I, torch.float32), R.assign_bases(case, I, aref))
    return _EVAL[case.name]


def test_case_table_covers_every_option():
    for field, values in (("Ls", R.LS), ("S", R.SS), ("C", R.CS), ("M", R.MS), ("K", R.KS), ("B", R.BS), ("family", R.FAMILIES),
                          ("dreg", (0, 1)), ("masked", (False, True)), ("pruned", (False, True)), ("spread", R.SPREADS)):
        assert {getattr(c, field) for c in R.CASES} == set(values), field
    for fam in R.FAMILIES:  # both families meet both losses, masks, a pruned cluster, the wide spread and the two-cluster lane
        for field, value in (("dreg", 0), ("dreg", 1), ("masked", True), ("pruned", True), ("spread", 6.0), ("C", 65), ("Ls", 70), ("B", 260)):
            assert any(c.family == fam and getattr(c, field) == value for c in R.CASES), (fam, field, value)
    from multivae_amd import _lib

    header = open(os.path.join(os.path.dirname(R.HERE), "include", "mvk.h")).read()
    assert f"#define MVK_CMVAE_MAX_CLUSTERS {_lib.CMVAE_MAX_CLUSTERS}" in header and max(R.CS) >= 65 > 64
    assert f"#define MVK_CMVAE_MAX_LDS_FLOATS {_lib.CMVAE_MAX_LDS_FLOATS}" in header


def test_no_sample_sits_on_a_kink():
    """No u_l == mean_jl (nor any other sample on the location it is scored against): the Laplace gradient is discontinuous there.
    Exactly, in fp32 and in float64, and with the margin that keeps the fp32 rounding of the sample on the same side."""
    for case in R.CASES:
        I = R.make_inputs(case)
        assert R.kink_distance(case, I) >= 0.5 * R.KINK_MARGIN, case.name
        for c in range(case.M):
            z64 = R._sample(I, c)
            z32 = I["mu"][c] + I["sd"][c] * R.t_of(case.family, I["noise"][c])
            for z in (z64, z32.to(R.F64)):
                assert not bool((z[..., : case.Ls].unsqueeze(-2) == I["cmean"].to(R.F64)).any()), case.name
        assert not bool((I["assign_z"].unsqueeze(-2) == I["cmean"]).any())
        if case.masked:
            av, nav = R.avail_of(case, I)
            assert int(nav.min()) >= 1 and int(nav[0]) == 1
        if case.pruned:
            assert int(torch.isinf(I["logits"]).sum()) == 1


def test_closed_form_equals_the_literal_form():
    """Float64: logsumexp_c a_c against the cluster loop over q = softmax + 1e-20 with q log q, every value and every gradient, within
    1e-6 of the fp32 error model's base (i.e. 1e-13 relative to the sum of the terms' magnitudes), plus, for the cluster means and
    logits, the literal form's own 1e-20 on clusters whose responsibility underflows."""
    worst = {}
    for case in R.CASES:
        I, ref, closed, _, base, _, _, _ = evaluated(case)
        lic = {"literal_1e-20": base["literal_1e-20"]}
        for k in R.FWD_STAGES + R.BWD_STAGES:
            lic[k] = [1e-6 * b for b in base[k]] if isinstance(base[k], list) else 1e-6 * base[k]
        for k, v in R.ratios(closed, ref, lic, R.FWD_STAGES + R.BWD_STAGES).items():
            worst[k] = max(worst.get(k, 0.0), v)
            assert v <= 1.0, (case.name, k, v)
    print("closed against literal, in units of 1e-6 base:", {k: f"{v:.2e}" for k, v in worst.items()})


def test_error_constants():
    """C_STAGE is 4x the largest |err| / base of the closed form in torch fp32 (backward: fp32 autograd) over the case table,
    rounded up."""
    worst = {}
    for case in R.CASES:
        I, ref, _, f32, base, aref, a32, abase = evaluated(case)
        r = R.ratios(f32, ref, base, R.FWD_STAGES + R.BWD_STAGES)
        r.update(R.ratios(a32, aref, abase, R.ASSIGN_STAGES))
        assert torch.equal(a32["argmax"], aref["argmax"]), case.name
        for k, v in r.items():
            if v > worst.get(k, (0.0, ""))[0]:
                worst[k] = (v, case.name)
    for k in R.STAGES:
        print(f"{k:10s} torch fp32 {worst[k][0]:.2f}  C {R.C_STAGE[k]:g}  set by {worst[k][1]}")
    assert {k: float(math.ceil(4.0 * worst[k][0])) for k in R.STAGES} == R.C_STAGE


@pytest.mark.parametrize("mut,stages,names", R.TEETH, ids=[t[0] for t in R.TEETH])
def test_tolerance_rejects_mutated_reference(mut, stages, names):
    """Against torch fp32 (the GPU test repeats it on the kernel's output): each deliberate mistake of the reference exceeds the bound."""
    for name in names:
        case = R.CASE_BY_NAME[name]
        I, _, _, f32, base, _, _, _ = evaluated(case)
        bad = R.ratios(f32, R.reference(case, I, mut=(mut,)), base, stages)
        for s in stages:
            assert bad[s] > R.C_STAGE[s], (mut, name, s, bad[s])


# ---- the model's host side ------------------------------------------------------------------------------------------------------------
def test_config_defaults_and_json_round_trip(tmp_path):
    from multivae_amd.models import AutoConfig, CMVAEConfig

    c = CMVAEConfig(n_modalities=2, latent_dim=5, input_dims=dict(a=(2,), b=(3,)), modalities_specific_dim=3)
    assert (c.K, c.prior_and_posterior_dist, c.learn_modality_prior, c.beta, c.reconstruction_option, c.loss,
            c.number_of_clusters) == (10, "laplace_with_softmax", True, 1.0, "joint_prior", "dreg_looser", 10)
    assert CMVAEConfig().modalities_specific_dim is None
    c2 = CMVAEConfig(n_modalities=2, latent_dim=5, input_dims=dict(a=(2,), b=(3,)), modalities_specific_dim=3, number_of_clusters=7,
                     beta=2.5, loss="iwae_looser", reconstruction_option="single_prior", K=3)
    c2.save_json(str(tmp_path), "model_config")
    blob = json.load(open(tmp_path / "model_config.json"))
    assert blob["name"] == "CMVAEConfig" and blob["number_of_clusters"] == 7
    back = AutoConfig.from_json_file(str(tmp_path / "model_config.json"))
    assert type(back) is CMVAEConfig and back.to_dict() == c2.to_dict()
    ref = json.load(open(os.path.join(R.GOLDEN, "cmvae_reference_folder", "model_config.json")))  # written by the reference
    assert set(ref) == set(blob)


@pytest.mark.parametrize("name", ["cmvae_tiny_normal_iwae", "cmvae_mnistsvhn_mlp_k2"])
def test_parameter_names_and_flags_match_the_reference(name):
    from multivae_amd.models import CMVAE, CMVAEConfig

    cfg, _ = G.load_case(name)
    dims = R.case_dims(cfg)
    for learn in (True, False):
        model = CMVAE(CMVAEConfig(n_modalities=len(dims), latent_dim=cfg["L"], input_dims=dict(dims), modalities_specific_dim=cfg["S"],
                                  number_of_clusters=cfg["C"], learn_modality_prior=learn))
        got = [[k, list(p.shape), bool(p.requires_grad)] for k, p in model.named_parameters()]
        want = [[k, s, (f and learn) if k.startswith("r_logvars_priors.") else f] for k, s, f in cfg["params"]]
        assert got == want
    model.load_state_dict({k: G.t(v) for k, v in R.case_state_dict(cfg).items()}, strict=True)
    for p in model.mean_clusters:
        assert float(p.detach().abs().max()) <= 1.0
    fresh = CMVAE(CMVAEConfig(n_modalities=len(dims), latent_dim=cfg["L"], input_dims=dict(dims), modalities_specific_dim=cfg["S"]))
    init = torch.cat(list(fresh.mean_clusters))
    assert init.shape == (10, cfg["L"]) and float(init.min()) >= -1 and float(init.max()) <= 1 and float(init.std()) > 0.3
    assert bool((fresh._pc_params == 0).all()) and torch.allclose(fresh.pc_params, torch.full((10,), 0.1))
    assert fresh.n_clusters == 10 and fresh.multiple_latent_spaces and fresh.model_name == "CMVAE"


def test_attribute_errors():
    from multivae_amd.models import CMVAE, CMVAEConfig

    dims = dict(a=(2,), b=(3,))
    with pytest.raises(AttributeError, match="modalities_specific_dim"):
        CMVAE(CMVAEConfig(n_modalities=2, latent_dim=5, input_dims=dims))
    cfg = CMVAEConfig(n_modalities=2, latent_dim=5, input_dims=dims, modalities_specific_dim=3)
    cfg.prior_and_posterior_dist = "cauchy"
    with pytest.raises(AttributeError, match="posterior_dist"):
        CMVAE(cfg)
    with pytest.raises(AttributeError, match="number_of_clusters"):
        CMVAE(CMVAEConfig(n_modalities=2, latent_dim=5, input_dims=dims, modalities_specific_dim=3, number_of_clusters=129))
    # the cluster table of the latent kernel (include/mvk.h): refused when the model is built, not at the first forward
    with pytest.raises(AttributeError, match="cluster table"):
        CMVAE(CMVAEConfig(n_modalities=2, latent_dim=64, input_dims=dims, modalities_specific_dim=3, number_of_clusters=128))
    assert CMVAE(CMVAEConfig(n_modalities=2, latent_dim=45, input_dims=dims, modalities_specific_dim=3, number_of_clusters=128)).n_clusters == 128


def test_vote_ties_go_to_the_smallest_cluster():
    """predict_clusters votes with torch.mode over the modalities' assignments: among equally frequent clusters the smallest index."""
    votes = torch.tensor([[3, 1], [1, 3], [2, 2], [4, 0], [5, 5], [0, 7]]).t()  # [M = 2, B]
    assert torch.mode(votes.t(), dim=-1)[0].tolist() == [1, 1, 2, 0, 5, 0]
    three = torch.tensor([[2, 2, 1], [0, 3, 3], [4, 1, 0], [6, 5, 6]])
    assert torch.mode(three, dim=-1)[0].tolist() == [2, 3, 0, 6]


def _np_entropy(pc):
    """scipy.stats.entropy(pc, axis=0) / log(count_nonzero(pc, axis=0)), written out with numpy."""
    p = pc / pc.sum(0, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        h = -np.where(p > 0, p * np.log(p), 0.0).sum(0)
    return h / np.log(np.count_nonzero(pc, axis=0))


def test_prune_bookkeeping_on_a_hand_made_sequence():
    """prune_clusters with predict_clusters replaced by a hand-made sequence: cluster mass from the votes, the penalised normalised
    entropy per pass, removal of the lightest live cluster, the restored logits and the plain-int cluster count."""
    from multivae_amd.data.datasets.base import MultimodalBaseDataset
    from multivae_amd.models import CMVAE, CMVAEConfig
    from multivae_amd.models.base.base_utils import ModelOutput
    from multivae_amd.models.cmvae.cmvae_model import prune_entropy

    pc = np.array([[0.7, 0.25, 0.0], [0.2, 0.25, 0.5], [0.1, 0.5, 0.5]])
    assert np.allclose(prune_entropy(torch.tensor(pc)).numpy(), _np_entropy(pc))
    assert np.isclose(prune_entropy(torch.tensor(pc))[2].item(), 1.0)  # two non-zero entries, uniform: log 2 / log 2
    torch.manual_seed(0)
    dims = dict(a=(2,), b=(3,))
    model = CMVAE(CMVAEConfig(n_modalities=2, latent_dim=3, input_dims=dims, modalities_specific_dim=2, number_of_clusters=4, beta=2.0))
    with torch.no_grad():
        model._pc_params.copy_(torch.tensor([0.1, 0.2, 0.3, 0.4]))
    ds = MultimodalBaseDataset(data={m: torch.rand(5, *d) for m, d in dims.items()})
    g = np.random.default_rng(0)
    # pass 0 (4 clusters): votes leave cluster 2 the lightest; pass 1 (3): cluster 0; pass 2 (2): cluster 3
    votes = [[[0, 0, 1], [3, 3]], [[1, 1, 3], [3, 0]], [[1, 1, 1], [3, 1]]]
    script, calls = [], []
    for p in range(3):
        for i, v in enumerate(votes[p]):
            n = len(v)
            pcs = {m: g.random((4, n)) + 0.05 for m in dims}
            script.append(ModelOutput(clusters=torch.tensor(v), pc_zs={m: torch.tensor(x, dtype=torch.float32) for m, x in pcs.items()},
                                      norm_lliks=torch.tensor(g.random(n), dtype=torch.float32)))

    def fake(batch, compute_lliks=False, noise=None):
        assert compute_lliks and len(batch.data["a"]) == len(script[len(calls)].clusters)
        calls.append(model._pc_params.detach().clone())
        return script[len(calls) - 1]

    model.predict_clusters = fake
    h = model.prune_clusters(ds, batch_size=3)
    assert len(calls) == 6 and len(h) == 5 and h[0] == math.inf and h[1] == math.inf
    want = []
    for p in range(3):
        rows = []
        for out in script[2 * p : 2 * p + 2]:
            ent = np.mean([_np_entropy(x.double().numpy()) for x in out.pc_zs.values()], axis=0)
            rows.append(2.0 * ent - out.norm_lliks.double().numpy())
        want.append(float(np.concatenate(rows).mean()))
    for n, w in zip((4, 3, 2), want):
        assert abs(float(h[n]) - w) <= 1e-5 * abs(w), (n, float(h[n]), w)
    inf = -math.inf
    assert calls[0].tolist() == calls[1].tolist() == pytest.approx([0.1, 0.2, 0.3, 0.4])
    assert calls[2].tolist() == pytest.approx([0.1, 0.2, inf, 0.4]) and calls[4].tolist() == pytest.approx([inf, 0.2, inf, 0.4])
    best = (4, 3, 2)[int(np.argmin(want))]
    assert type(model.n_clusters) is int and model.n_clusters == best
    final = {4: [0.1, 0.2, 0.3, 0.4], 3: [0.1, 0.2, inf, 0.4], 2: [inf, 0.2, inf, 0.4]}[best]
    assert model._pc_params.tolist() == pytest.approx(final) and isinstance(model._pc_params, torch.nn.Parameter)
