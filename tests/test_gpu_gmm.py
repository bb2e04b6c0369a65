"""The Gaussian-mixture EM of csrc/gmm.hip on the GPU: the mvk_gmm_* entry points through the C ABI, entry-wise against the
float64 restatement of tests/gmm_ref.py, and multivae_amd.samplers.GaussianMixtureSampler end to end.

The bar (gmm_ref.BAR) is the project's parity bar, 1e-4: max|got - ref| / max|ref| per tensor, absolute for the lower bound (and
for the log-determinants, which enter log p additively like it: max|got - ref| <= 1e-4 max(1, max|ref|)).  test_gmm_host.py shows
that gmm_ref IS scikit-learn's EM, that the iteration count of every fit case cannot differ from the reference's by rounding,
and that the CPU emulation of the kernels' precision split stays within a quarter of the bar on every case used here.

1. test_step_cases: one soft E-step, one hard E-step and one M-step per case of gmm_ref.STEP_CASES (N in {1, 37, 257, 1003, 4099} x
   L in {1, 2, 20, 33, 64} x C in {1, 3, 10, 64}, pruned; C > N and a component without responsibility included), outputs
   pre-filled with NaN, every entry compared, a second launch bit-identical.
2. test_fit_cases: the whole fit from a given initial state on gmm_ref.FIT_CASES, the two `degenerate` cases (a component with no
   more than L points: an all-fp32 EM meets a non-positive pivot there) among them: n_iter_, converged_, weights_, means_,
   covariances_, lower_bound_.
3. check_every 1 and 8 give the same bits; steps enqueued after convergence change nothing.
4. Lloyd from given rows: the float64 labels; seeded default seeding: reproducible, distinct rows.
5. Sampling with given components and noise; chunking; grouping by component.
6. Errors: NaN embeddings, a singular covariance, every MVK_EINVAL branch, N = 0.
7. End to end on a tiny MoPoE (one latent space) and a tiny DMVAE (private latent spaces).
8. Mutations of the reference (means not re-centred, reg_covar dropped, ln w_c dropped) are rejected by the same bar.

Largest distance of the HIP kernels from float64 on an MI355X, per tensor, with the case that set it (test_zz_report prints
HIP_MEASURED; the bar is 1e-4):
    step: cov_chol 5.89e-08 (n1-l20-c3), covs 5.64e-08 (n1-l20-c3), hard_d2 3.54e-07 (n1003-l64-c3), lb 3.93e-05 (n1-l64-c64),
        logdet 4.83e-08 (n1003-l33-c10-empty9), lse 3.48e-07 (n1003-l64-c3), means 4.37e-08 (n1003-l2-c64), prec_chol 4.03e-08
        (n1003-l1-c10), resp 3.50e-05 (n1003-l64-c3), weights 4.76e-08 (n257-l2-c3-empty0)
    fit: covs 5.87e-07 (n600-l33-c4-s0), lower_bound 1.84e-06 (n900-l64-c5-s0), means 7.24e-07 (n600-l33-c4-s0), weights
        5.88e-07 (n600-l33-c4-s0)
    sample: z 2.32e-07 (n4099-l64-c64-empty63)
Factor by which each mutated reference exceeded the bar on the kernel's output (HIP_TEETH): no_recentre 9.64e+03, no_reg 662, drop_logw 132.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import gmm_ref as R

pytestmark = pytest.mark.gpu
D = torch.device("cuda:0")
MEASURED = {}


def _mods():
    from multivae_amd import _lib, kernels

    return _lib, kernels


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=D, dtype=dtype).contiguous()


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=D)


def host(t):
    return t.detach().cpu().double().numpy()


def note(key, value, name):
    if value > MEASURED.get(key, (-1.0, ""))[0]:
        MEASURED[key] = (value, name)


def params_on_device(w, mu, P, L, C):
    _, K = _mods()
    p = K.gmm_new_params(L, C, D)
    for t in p.values():
        t.fill_(float("nan"))
    p["weights"].copy_(dev(w))
    p["means"].copy_(dev(mu))
    p["prec_chol"].copy_(dev(P))
    p["logdet"].copy_(dev(np.log(np.diagonal(P, axis1=1, axis2=2)).sum(1)))
    return p


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def logdet_dist(got, ref):
    return float(np.max(np.abs(got - ref)) / max(1.0, np.max(np.abs(ref))))


def step_launches(case):
    """Every output of one soft E-step, one hard E-step and one M-step of the case, from NaN-filled buffers."""
    _, K = _mods()
    X, w, mu, P = case.make()
    N, L, C = case.N, case.L, case.C
    x = dev(X)
    scratch = K.gmm_scratch(L, C, D)
    scratch.fill_(float("nan"))
    p = params_on_device(w, mu, P, L, C)
    resp, lse, lb = nan(N, C), nan(N), torch.full((1,), float("nan"), dtype=torch.float64, device=D)
    K.gmm_estep(x, p, resp, scratch, row_out=lse, lb=lb)
    hresp, hd2 = nan(N, C), nan(N)
    labels, changed = torch.full((N,), -1, dtype=torch.int32, device=D), torch.full((1,), 77, dtype=torch.int32, device=D)
    K.gmm_estep_hard(x, p["means"], hresp, scratch, row_out=hd2, labels=labels, changed=changed)
    q = K.gmm_new_params(L, C, D)
    for t in q.values():
        t.fill_(float("nan"))
    K.gmm_mstep(x, dev(case.resp(X, w, mu, P)), q, case.reg, scratch)
    torch.cuda.synchronize()
    return dict(resp=resp, lse=lse, lb=lb, hresp=hresp, hd2=hd2, labels=labels, changed=changed, **q)


@pytest.mark.parametrize("case", R.STEP_CASES, ids=lambda c: c.name)
def test_step_cases(case):
    X, w, mu, P = case.make()
    got, again = step_launches(case), step_launches(case)
    for k in got:
        assert not bool(torch.isnan(got[k].double()).any()), f"{k} holds a NaN"
        assert torch.equal(got[k], again[k]) and (got[k].dtype != torch.float32 or same_bits(got[k], again[k])), f"{k}: a second launch differs"
    # soft E-step
    r64, lse64, lb64 = R.estep64(X, w, mu, P)
    d = dict(resp=R.rel(host(got["resp"]), r64), lse=R.rel(host(got["lse"]), lse64), lb=abs(float(got["lb"]) - lb64))
    # hard E-step
    lab64, d1, d2 = R.hard64(X, mu)
    clear = d2 >= 1.001 * d1
    lab = got["labels"].cpu().numpy()
    assert np.array_equal(lab[clear], lab64[clear]) and int(got["changed"]) == case.N
    assert np.array_equal(host(got["hresp"]), np.eye(case.C)[lab])
    d["hard_d2"] = R.rel(host(got["hd2"]), d1) if d1.max() > 0 else float(np.max(np.abs(host(got["hd2"]))))
    # M-step
    m64 = R.mstep64(X, case.resp(X, w, mu, P), case.reg)
    chol64, prec64, logdet64 = R.finish64(m64["covs"])
    d.update(weights=R.rel(host(got["weights"]), m64["weights"]), means=R.rel(host(got["means"]), m64["means"]),
             covs=R.rel(host(got["covs"]), m64["covs"]), cov_chol=R.rel(host(got["cov_chol"]), chol64),
             prec_chol=R.rel(host(got["prec_chol"]), prec64), logdet=logdet_dist(host(got["logdet"]), logdet64))
    print(case.name, {k: f"{v:.2e}" for k, v in d.items()})
    for k, v in d.items():
        note("step " + k, v, case.name)
    for k, v in d.items():
        assert v <= R.BAR, f"{case.name}: {k} is {v:.3g} from float64"
    if case.empty is not None and case.C > 1:
        e = case.empty
        assert bool((got["means"][e] == 0).all())
        assert torch.equal(got["covs"][e], torch.eye(case.L, device=D) * torch.tensor(case.reg, dtype=torch.float32, device=D))
    tri = torch.ones(case.L, case.L, device=D).tril(-1).bool()
    assert bool((got["prec_chol"][:, tri] == 0).all()) and bool((got["cov_chol"][:, tri.T] == 0).all())


_FITS = {}


def device_fit(case, check_every=8):
    """The fit of a case from its given initial state: run once per (case, check_every), shared, left unchanged."""
    from multivae_amd.samplers.gaussian_mixture import DeviceGaussianMixture

    key = (case.name, check_every)
    if key not in _FITS:
        X, w, mu, pr = case.make()
        _FITS[key] = DeviceGaussianMixture(case.C, check_every=check_every).fit(dev(X), weights_init=w, means_init=mu,
                                                                                precisions_init=pr)
    return _FITS[key]


@pytest.mark.parametrize("case", R.FIT_CASES, ids=lambda c: c.name)
def test_fit_cases(case):
    _, ref = R.fit_reference(case)
    g = device_fit(case)
    for t in (g.weights_, g.means_, g.covariances_, g.precisions_cholesky_, g.covariances_cholesky_):
        assert bool(torch.isfinite(t).all())
    assert math.isfinite(g.lower_bound_)
    d = dict(weights=R.rel(host(g.weights_), ref["weights"]), means=R.rel(host(g.means_), ref["means"]),
             covs=R.rel(host(g.covariances_), ref["covs"]), lower_bound=abs(g.lower_bound_ - ref["lower_bound"]))
    print(case.name, "n_iter", g.n_iter_, ref["n_iter"], {k: f"{v:.2e}" for k, v in d.items()})
    for k, v in d.items():
        note("fit " + k, v, case.name)
    assert g.n_iter_ == ref["n_iter"] and g.converged_ == ref["converged"]
    for k, v in d.items():
        assert v <= R.BAR, f"{case.name}: {k} is {v:.3g} from float64"


def test_check_every_and_steps_after_convergence():
    _, K = _mods()
    case = R.FIT_CASES[3]
    a, b = device_fit(case, 8), device_fit(case, 1)
    assert a.n_iter_ == b.n_iter_ and a.converged_ and b.converged_ and a.lower_bound_ == b.lower_bound_
    for k in ("weights_", "means_", "covariances_", "precisions_cholesky_", "covariances_cholesky_"):
        assert same_bits(getattr(a, k), getattr(b, k)), k
    # the same fit by hand: steps enqueued after convergence leave the state block and every buffer as they are
    X, w, mu, pr = case.make()
    x = dev(X)
    p = params_on_device(w, mu, R.prec_chol_from_precisions(pr), case.L, case.C)
    p["covs"].zero_(), p["cov_chol"].zero_()
    resp, state, scratch = nan(case.N, case.C), K.gmm_new_state(D), K.gmm_scratch(case.L, case.C, D)
    for _ in range(a.n_iter_):
        K.gmm_em_step(x, p, resp, state, R.REG, R.TOL, scratch)
    before = {k: v.clone() for k, v in p.items()}
    st, r0 = state.clone(), resp.clone()
    from multivae_amd._lib import GMM_STATE as S
    assert st[S["converged"]] == 1 and st[S["iter"]] == a.n_iter_ and st[S["status"]] == 0
    for _ in range(3):
        K.gmm_em_step(x, p, resp, state, R.REG, R.TOL, scratch)
    assert torch.equal(state, st) and same_bits(resp, r0)
    for k in p:
        assert same_bits(p[k], before[k]), k
    assert same_bits(p["means"], a.means_) and same_bits(p["covs"], a.covariances_)


def test_lloyd_and_seeding():
    from multivae_amd.samplers.gaussian_mixture import DeviceGaussianMixture

    X, idx = R.lloyd_case()
    labels, means, rounds, _ = R.lloyd64(X, idx)
    g = DeviceGaussianMixture(len(idx)).fit(dev(X), init_indices=idx)
    assert np.array_equal(g.kmeans_labels_.cpu().numpy(), labels) and g.kmeans_n_iter_ == rounds
    assert g.converged_ and bool(torch.isfinite(g.covariances_).all())
    gens = [torch.Generator(device=D).manual_seed(123) for _ in range(2)]
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        s = [DeviceGaussianMixture(len(idx), max_iter=1).fit(dev(X), generator=gen).init_indices_.cpu().numpy() for gen in gens]
    assert np.array_equal(s[0], s[1]) and len(set(s[0].tolist())) == len(idx)


def _fitted(case):
    """A mixture with the float64 M-step's parameters of a step case, as the sampler holds it."""
    from multivae_amd.samplers.gaussian_mixture import DeviceGaussianMixture

    X, w, mu, P = case.make()
    m64 = R.mstep64(X, case.resp(X, w, mu, P), case.reg)
    chol64, prec64, _ = R.finish64(m64["covs"])
    g = DeviceGaussianMixture(case.C)
    g.weights_, g.means_, g.covariances_ = dev(m64["weights"]), dev(m64["means"]), dev(m64["covs"])
    g.precisions_cholesky_, g.covariances_cholesky_ = dev(prec64), dev(chol64)
    return g, m64, chol64


@pytest.mark.parametrize("case", [R.STEP_CASES[i] for i in (0, 4, 8, 15)], ids=lambda c: c.name)
def test_sample_kernel(case):
    g, m64, chol64 = _fitted(case)
    rng = np.random.default_rng(5)
    n = 131
    comp = rng.integers(0, case.C, n)
    eps = rng.standard_normal((n, case.L)).astype(np.float32).astype(np.float64)
    z, c = g.sample(n, components=comp, noise=eps)
    want = R.sample64(host(g.means_), host(g.covariances_cholesky_), comp, eps)
    v = R.rel(host(z), want)
    note("sample z", v, case.name)
    assert v <= R.BAR and np.array_equal(c.cpu().numpy(), comp)
    z2, _ = g.sample(n, components=comp, noise=eps)
    assert same_bits(z, z2)
    _, drawn = g.sample(500, generator=torch.Generator(device=D).manual_seed(1))
    drawn = drawn.cpu().numpy()
    assert np.all(np.diff(drawn) >= 0) and drawn.min() >= 0 and drawn.max() < case.C  # grouped by component
    with pytest.raises(ValueError):
        g.sample(2, components=[0, case.C], noise=np.zeros((2, case.L)))


def test_errors_and_argument_checks():
    L_, K = _mods()
    from multivae_amd.samplers.gaussian_mixture import DeviceGaussianMixture

    X, _, _ = R.blobs(300, 5, 3, 1)
    bad = dev(X)
    bad[17, 2] = float("nan")
    with pytest.raises(ValueError):
        DeviceGaussianMixture(3).fit(bad)
    # the device's own guard: a NaN row makes the lower bound NaN, status 2, and the step stops before the covariances
    p = params_on_device(np.full(3, 1 / 3), X[:3], np.stack([np.eye(5)] * 3), 5, 3)
    p["covs"].fill_(7.0)
    state, scratch, resp = K.gmm_new_state(D), K.gmm_scratch(5, 3, D), nan(300, 3)
    K.gmm_em_step(bad, p, resp, state, R.REG, R.TOL, scratch)
    K.gmm_em_step(bad, p, resp, state, R.REG, R.TOL, scratch)
    S = L_.GMM_STATE
    assert state[S["status"]] == 2 and state[S["iter"]] == 0 and state[S["converged"]] == 0 and bool((p["covs"] == 7.0).all())
    assert same_bits(p["means"], dev(X[:3]))
    # identical rows without regularisation: a zero pivot, scikit-learn's ValueError
    with pytest.raises(ValueError, match="ill-defined empirical covariance"):
        DeviceGaussianMixture(1, reg_covar=0.0).fit(torch.ones(50, 4, device=D))
    # MVK_EINVAL without a launch; N = 0 is MVK_OK and writes nothing
    lib, sp, ptr = L_.load(), L_.stream_ptr, L_.ptr
    x = dev(X)
    q = params_on_device(np.full(3, 1 / 3), X[:3], np.stack([np.eye(5)] * 3), 5, 3)
    resp, lb = nan(300, 3), torch.zeros(1, dtype=torch.float64, device=D)
    z, comp, eps = nan(4, 5), torch.zeros(4, dtype=torch.int32, device=D), torch.zeros(4, 5, device=D)

    def estep(N=300, L=5, C=3, x=x, w=q["weights"], mu=q["means"], P=q["prec_chol"], ld=q["logdet"], hard=0, resp=resp, sc=scratch):
        return lib.mvk_gmm_estep(ptr(x), N, L, C, ptr(w), ptr(mu), ptr(P), ptr(ld), hard, ptr(resp), None, None, None, ptr(lb), ptr(sc),
                                 sp())

    def mstep(N=300, L=5, C=3, x=x, resp=resp, mu=q["means"], covs=q["covs"], only=0, sc=scratch):
        return lib.mvk_gmm_mstep(ptr(x), ptr(resp), N, L, C, 1e-6, only, ptr(q["weights"]), ptr(mu), ptr(covs), ptr(q["cov_chol"]),
                                 ptr(q["prec_chol"]), ptr(q["logdet"]), ptr(sc), sp())

    def em(N=300, L=5, C=3, x=x, state=state, sc=scratch):
        return lib.mvk_gmm_em_step(ptr(x), N, L, C, 1e-6, 1e-3, ptr(q["weights"]), ptr(q["means"]), ptr(q["covs"]), ptr(q["cov_chol"]),
                                   ptr(q["prec_chol"]), ptr(q["logdet"]), ptr(resp), ptr(state), ptr(sc), sp())

    def sample(n=4, L=5, C=3, mu=q["means"], ch=q["cov_chol"], comp=comp, eps=eps, z=z):
        return lib.mvk_gmm_sample(ptr(mu), ptr(ch), ptr(comp), ptr(eps), n, L, C, ptr(z), sp())

    n64 = ctypes.c_int64(-5)
    EINVAL = -1
    assert lib.mvk_gmm_scratch_bytes(65, 3, ctypes.byref(n64)) == EINVAL and lib.mvk_gmm_scratch_bytes(5, 65, ctypes.byref(n64)) == EINVAL
    assert lib.mvk_gmm_scratch_bytes(0, 3, ctypes.byref(n64)) == EINVAL and lib.mvk_gmm_scratch_bytes(5, 3, None) == EINVAL and n64.value == -5
    assert lib.mvk_gmm_scratch_bytes(64, 64, ctypes.byref(n64)) == 0 and 0 < n64.value < 64 << 20
    for f in (estep, mstep, em, sample):
        assert f(L=65) == EINVAL and f(C=65) == EINVAL and f(L=0) == EINVAL and f(C=0) == EINVAL, f.__name__
    assert estep(N=-1) == EINVAL and mstep(N=-1) == EINVAL and em(N=-1) == EINVAL and sample(n=-1) == EINVAL
    assert estep(x=None) == EINVAL and estep(mu=None) == EINVAL and estep(resp=None) == EINVAL and estep(sc=None) == EINVAL
    assert estep(w=None) == EINVAL and estep(P=None) == EINVAL and estep(ld=None) == EINVAL
    assert mstep(x=None) == EINVAL and mstep(resp=None) == EINVAL and mstep(mu=None) == EINVAL and mstep(sc=None) == EINVAL
    assert mstep(covs=None) == EINVAL and em(x=None) == EINVAL and em(state=None) == EINVAL and em(sc=None) == EINVAL
    assert sample(mu=None) == EINVAL and sample(ch=None) == EINVAL and sample(comp=None) == EINVAL and sample(eps=None) == EINVAL
    assert sample(z=None) == EINVAL
    assert estep(N=0) == 0 and mstep(N=0) == 0 and em(N=0) == 0 and sample(n=0) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(resp).all()) and bool(torch.isnan(z).all()) and bool(torch.isnan(q["covs"]).all()) and float(lb) == 0.0


def _two_modalities(n, seed=0):
    from multivae_amd.data.datasets.base import MultimodalBaseDataset

    g = torch.Generator().manual_seed(seed)
    return MultimodalBaseDataset(data=dict(a=torch.rand(n, 12, generator=g), b=torch.rand(n, 2, 5, generator=g)))


@pytest.mark.parametrize("private", [False, True], ids=["mopoe", "dmvae"])
def test_end_to_end(private, caplog):
    from multivae_amd.models import DMVAE, DMVAEConfig, MoPoE, MoPoEConfig
    from multivae_amd.samplers import GaussianMixtureSampler, GaussianMixtureSamplerConfig

    torch.manual_seed(0)
    dims = dict(a=(12,), b=(2, 5))
    if private:
        model = DMVAE(DMVAEConfig(n_modalities=2, latent_dim=6, input_dims=dims, modalities_specific_dim=dict(a=2, b=3)))
    else:
        model = MoPoE(MoPoEConfig(n_modalities=2, latent_dim=6, input_dims=dims))
    sampler = GaussianMixtureSampler(model, GaussianMixtureSamplerConfig(n_components=3))
    sampler.fit(_two_modalities(230), generator=torch.Generator(device=D).manual_seed(3))
    assert sampler.is_fitted and sampler.gmm.means_.shape == (3, 6) and sampler.gmm.n_iter_ >= 1
    out = sampler.sample(7, batch_size=3)
    assert out.z.shape == (7, 6) and out.z.is_cuda and out.one_latent_space == (not private)
    assert bool(torch.isfinite(out.z).all())
    if private:
        assert set(sampler.mod_gmms) == {"a", "b"} and out.modalities_z["a"].shape == (7, 2) and out.modalities_z["b"].shape == (7, 3)
        assert all(bool(torch.isfinite(v).all()) for v in out.modalities_z.values())
    rec = model.decode(out)
    assert rec["a"].shape == (7, 12) and rec["b"].shape == (7, 2, 5)
    assert all(bool(torch.isfinite(v).all()) for v in rec.values())
    # the reference's chunking: 3 + 3 + 1 rows, each chunk one launch on its slice of the given components and noise
    comp = torch.tensor([0, 0, 1, 2, 2, 2, 1])
    eps = torch.randn(7, 6, generator=torch.Generator().manual_seed(1))
    z = sampler.sample(7, batch_size=3, components=comp, noise=eps).z
    whole, _ = sampler.gmm.sample(7, components=comp, noise=eps)
    assert same_bits(z, whole)
    # more components than embeddings: clamped, with the reference's warning
    small = GaussianMixtureSampler(model, GaussianMixtureSamplerConfig(n_components=10))
    with caplog.at_level("WARNING"):
        small.fit(_two_modalities(4, seed=1), generator=torch.Generator(device=D).manual_seed(4))
    assert small.n_components == 4 and small.gmm.means_.shape[0] == 4 and "Setting the number of component to 4" in caplog.text
    assert bool(torch.isfinite(small.sample(5).z).all())


def test_tolerance_rejects_mutated_reference():
    """The comparisons of test_step_cases with one deliberate mistake in the REFERENCE must fail on the kernel's output."""
    case = R.MUTATION_CASE
    X, w, mu, P = case.make()
    got = step_launches(case)
    resp = case.resp(X, w, mu, P)
    covs = host(got["covs"])
    teeth = dict(no_recentre=R.rel(covs, R.mstep64(X, resp, case.reg, no_recentre=True)["covs"]),
                 no_reg=R.rel(covs, R.mstep64(X, resp, case.reg, no_reg=True)["covs"]),
                 drop_logw=R.rel(host(got["lse"]), R.estep64(X, w, mu, P, drop_logw=True)[1]))
    assert R.rel(covs, R.mstep64(X, resp, case.reg)["covs"]) <= R.BAR
    for k, v in teeth.items():
        print("HIP_TEETH", k, f"{v / R.BAR:.3g}x the bar")
        assert v > R.BAR, k


def test_zz_report():
    for k in sorted(MEASURED):
        print("HIP_MEASURED", k, f"{MEASURED[k][0]:.2e}", MEASURED[k][1])
