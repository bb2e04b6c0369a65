"""CPU checks behind test_gpu_gmm.py: that tests/gmm_ref.py IS scikit-learn's EM, that every case of its tables can be decided
(iteration counts cannot differ by rounding; the fp32-rows / fp64-sums error model sits well inside the bar), and the host
surface of multivae_amd.samplers that needs no GPU."""
import json
import os

import numpy as np
import pytest
import torch

import gmm_ref as R


@pytest.mark.parametrize("case", R.FIT_CASES[:5], ids=lambda c: c.name)
def test_restatement_is_sklearn(case):
    """From weights_init / means_init / precisions_init on the same float64 data: the same n_iter_, parameters within 1e-12."""
    from sklearn.mixture import GaussianMixture

    X, w, mu, pr = case.make()
    sk = GaussianMixture(n_components=case.C, covariance_type="full", tol=R.TOL, max_iter=2000, reg_covar=R.REG, weights_init=w,
                         means_init=mu, precisions_init=pr).fit(X)
    ref = R.em64(X, w, mu, R.prec_chol_from_precisions(pr), nk_eps=R.DBL_EPS)
    assert ref["n_iter"] == sk.n_iter_ and ref["converged"] == sk.converged_
    for got, want in ((ref["weights"], sk.weights_), (ref["means"], sk.means_), (ref["covs"], sk.covariances_),
                      (ref["prec_chol"], sk.precisions_cholesky_)):
        assert R.rel(got, want) <= 1e-12
    assert abs(ref["lower_bound"] - sk.lower_bound_) <= 1e-12 * abs(sk.lower_bound_)


@pytest.mark.parametrize("case", R.FIT_CASES, ids=lambda c: c.name)
def test_fit_cases_can_be_decided(case):
    (X, w, mu, pr), ref = R.fit_reference(case)
    assert ref["converged"]
    # (a) no component of a case that is not labelled degenerate is a singleton; a degenerate one really holds <= L points
    counts = np.bincount(ref["resp"].argmax(1), minlength=case.C)
    if case.degenerate:
        assert counts.min() <= case.L, counts
    else:
        assert counts.min() >= 2, counts
    # (b) the margin: the stopping test is not within rounding of flipping at the last or the last-but-one iteration
    ch = np.abs(ref["changes"])
    assert ch[-1] < R.TOL / 2 and ch[-2] > 2 * R.TOL, ch[-3:]
    # (c) the error model stays within a quarter of the bar, with the same iteration count
    em = R.em_emul(X, w, mu, R.prec_chol_from_precisions(pr))
    assert em["n_iter"] == ref["n_iter"] and em["converged"]
    d = {k: R.rel(em[k], ref[k]) for k in ("weights", "means", "covs")}
    d["lower_bound"] = abs(em["lower_bound"] - ref["lower_bound"])
    print(case.name, ref["n_iter"], d)
    assert max(d.values()) <= R.BAR / 4, d


@pytest.mark.parametrize("case", R.STEP_CASES, ids=lambda c: c.name)
def test_step_cases_error_model(case):
    """One E-step and one M-step of the error model against float64, entry-wise, within a quarter of the bar; a component without
    responsibility has mean 0 and covariance reg_covar I."""
    X, w, mu, P = case.make()
    r64, lse64, lb64 = R.estep64(X, w, mu, P)
    r32, lse32, lb32 = R.estep_emul(X, w, mu, P)
    assert np.max(np.abs(r32 - r64)) <= R.BAR / 4 and R.rel(lse32, lse64) <= R.BAR / 4 and abs(lb32 - lb64) <= R.BAR / 4
    resp = case.resp(X, w, mu, P)
    m64, m32 = R.mstep64(X, resp, case.reg), R.mstep_emul(X, resp, case.reg)
    c64, c32 = R.finish64(m64["covs"]), R.finish64(m32["covs"])
    for k in m64:
        assert R.rel(m32[k], m64[k]) <= R.BAR / 4, (k, R.rel(m32[k], m64[k]))
    for a, b, k in zip(c32, c64, ("cov_chol", "prec_chol", "logdet")):
        assert R.rel(a, b) <= R.BAR / 4, (k, R.rel(a, b))
    if case.empty is not None and case.C > 1:
        assert np.all(m64["means"][case.empty] == 0) and np.array_equal(m64["covs"][case.empty], case.reg * np.eye(case.L))


def test_lloyd_case_has_clear_labels():
    """The data of the Lloyd test: in every round the second-nearest centre of every row is at least 1.5x as far (squared
    distance) as the nearest, so fp32 distances give the float64 labels."""
    X, idx = R.lloyd_case()
    labels, _, rounds, gap = R.lloyd64(X, idx)
    assert gap >= 1.5 and 1 <= rounds < 100 and len(np.unique(labels)) == len(idx)


def test_mutations_are_outside_the_bar():
    """Each mutation of the reference (test_gpu_gmm.py asserts the same on the kernel's output) is rejected by the bar when the
    comparison is against the error model."""
    case = R.MUTATION_CASE
    X, w, mu, P = case.make()
    resp = case.resp(X, w, mu, P)
    good = R.mstep_emul(X, resp, case.reg)
    assert R.rel(good["covs"], R.mstep64(X, resp, case.reg, no_recentre=True)["covs"]) > R.BAR
    assert R.rel(good["covs"], R.mstep64(X, resp, case.reg, no_reg=True)["covs"]) > R.BAR
    assert R.rel(R.estep_emul(X, w, mu, P)[1], R.estep64(X, w, mu, P, drop_logw=True)[1]) > R.BAR  # the logsumexp rows


def test_config_round_trip_and_unfitted_sampler(tmp_path):
    from multivae_amd.models import MoPoE, MoPoEConfig
    from multivae_amd.samplers import BaseSamplerConfig, GaussianMixtureSampler, GaussianMixtureSamplerConfig

    cfg = GaussianMixtureSamplerConfig(n_components=7)
    assert cfg.name == "GaussianMixtureSamplerConfig" and GaussianMixtureSamplerConfig().n_components == 10
    assert BaseSamplerConfig().to_dict() == {"name": "BaseSamplerConfig"}
    model = MoPoE(MoPoEConfig(n_modalities=2, latent_dim=4, input_dims=dict(a=(6,), b=(2, 5))))
    sampler = GaussianMixtureSampler(model, cfg)
    assert sampler.name == "GaussianMixtureSampler" and sampler.n_components == 7 and sampler.is_fitted is False
    assert not model.training
    with pytest.raises(ArithmeticError):
        sampler.sample(3)
    sampler.save(str(tmp_path / "s"))
    path = os.path.join(str(tmp_path / "s"), "sampler_config.json")
    assert json.load(open(path)) == {"name": "GaussianMixtureSamplerConfig", "n_components": 7}  # the reference's file
    assert GaussianMixtureSamplerConfig.from_json_file(path) == cfg
    assert GaussianMixtureSampler(model).n_components == 10


def test_state_block_mirror():
    """The device state block is 8 doubles, not a struct: the indices _lib names are the header's MVK_GMM_STATE_* values."""
    import re

    from multivae_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "mvk.h")).read()
    defs = {k.lower(): int(v) for k, v in re.findall(r"#define MVK_GMM_STATE_(\w+) (\d+)", header)}
    assert defs.pop("doubles") == _lib.GMM_STATE_DOUBLES == 8
    assert defs == _lib.GMM_STATE and len(set(defs.values())) == len(defs) and max(defs.values()) < 8
    assert torch.zeros(_lib.GMM_STATE_DOUBLES, dtype=torch.float64).numel() * 8 == 64
