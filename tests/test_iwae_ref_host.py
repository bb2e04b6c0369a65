"""CPU checks of tests/iwae_ref.py, the references behind tests/test_gpu_iwae.py:

- the references are pinned to independent definitions: z to oracle.elbo.latent_rsample, the log-densities to
  torch.distributions.Normal / Laplace and oracle.elbo.latent_log_prob, the mixture and the reduction to torch.logsumexp, all in
  float64; the derivative magnitudes of the end-to-end base to float64 autograd;
- the non-finite cases have the classes the issue names: the NaN expert density gives NaN on row 1 alone, an expert at -inf leaves
  everything finite, all experts at -inf give +inf;
- the constants of the measured stages are 4x what the plain fp32 evaluation shows, rounded up; the derived one holds;
- every `check_*` routine of the GPU file passes on every case with a stand-in backend (the same formulas in plain torch fp32);
- every wrong variant of iwae_ref.TEETH leaves the bound on each of its named cases.
"""
import math

import pytest
import torch

import iwae_ref as R
import test_gpu_iwae as G
from oracle import elbo

F64 = torch.float64


class Standin:
    @staticmethod
    def _fam(fam):
        return "laplace" if fam == 1 else "normal"

    def sample(self, fam, loc, sd, noise):
        return dict(z=loc + sd * R.t32(self._fam(fam), noise), guards=True)

    def logw(self, fam, z, rows, locs, sds, ploc, psd):
        return dict(lw=R.lw32(self._fam(fam), z, rows, locs, sds, ploc, psd), guards=True)

    def reduce(self, lws):
        return dict(ll=R.ll32(lws), guards=True)


BE = Standin()


# ---- independent definitions ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in R.CASES if c.finite], ids=[c.name for c in R.CASES if c.finite])
def test_reference_is_torch_distributions_and_logsumexp(case):
    inp = R.make_inputs(case)
    fam = G.ref_family(case)
    ofam = "normal" if fam == "normal" else "laplace_with_softmax"
    d = lambda t: t.double()  # noqa: E731
    z, zb = R.z_of(fam, inp["sloc"], inp["ssd"], inp["noise"])
    want_z = elbo.latent_rsample(ofam, d(inp["sloc"]), d(inp["ssd"]), d(inp["noise"]))
    assert float((z - want_z).abs().max()) <= 1e-15 * float(zb.max())
    dist = torch.distributions.Laplace if fam == "laplace" else torch.distributions.Normal
    L = case.L
    ploc = torch.zeros(L, dtype=F64) if inp["ploc"] is None else d(inp["ploc"])
    psd = torch.ones(L, dtype=F64) if inp["psd"] is None else d(inp["psd"])
    lpz = dist(ploc, psd).log_prob(z).sum(-1)
    assert float((lpz - elbo.latent_log_prob(ofam, z, ploc, psd).sum(-1)).abs().max()) <= 1e-12 * float(lpz.abs().max())
    finite = [e for e in range(case.E) if bool(torch.isfinite(inp["sds"][e]).all())]
    lq = torch.stack([dist(d(inp["locs"][e]), d(inp["sds"][e])).log_prob(z).sum(-1) if e in finite else torch.full(lpz.shape, -math.inf, dtype=F64)
                      for e in range(case.E)])
    got_lq = R.lq_e_of(fam, z, inp["locs"], inp["sds"])[0]
    assert torch.equal(torch.isfinite(got_lq), torch.isfinite(lq))
    assert float(torch.nan_to_num(got_lq - lq, nan=0.0).abs().max()) <= 1e-12 * float(lq[finite].abs().max())
    want = -sum(d(r) for r in inp["rows"]) + lpz - (torch.logsumexp(lq, 0) - math.log(case.E)) if inp["rows"] else lpz - (torch.logsumexp(lq, 0) - math.log(case.E))
    lw, base, td = R.lw_of(fam, z, inp["rows"], inp["locs"], inp["sds"], inp["ploc"], inp["psd"], zmag=zb)
    assert bool(((lw - want).abs() <= 1e-13 * base).all())
    assert bool((base >= lw.abs() * (1 - 1e-12)).all())  # a sum of magnitudes is never below the magnitude of the sum
    ll, lb = R.ll_of([lw])
    assert bool(((ll - (torch.logsumexp(want, 0) - math.log(case.K))).abs() <= 1e-13 * lb).all())
    # the end-to-end base: |d lw / d z| zmag summed over l, by autograd through the independent definition
    if case.special == "":
        zz = z.clone().requires_grad_(True)
        lq2 = torch.stack([dist(d(inp["locs"][e]), d(inp["sds"][e])).log_prob(zz).sum(-1) for e in range(case.E)])
        (dist(ploc, psd).log_prob(zz).sum(-1) - torch.logsumexp(lq2, 0)).sum().backward()
        assert bool(((zz.grad.abs() * zb).sum(-1) <= td * (1 + 1e-9) + 1e-300).all())


@pytest.mark.parametrize("case", R.REDUCE_CASES, ids=[c.name for c in R.REDUCE_CASES])
def test_reduce_reference_is_torch_logsumexp(case):
    lws = R.reduce_inputs(case)
    x = torch.cat([t.double() for t in lws], 0)
    want = torch.logsumexp(x, 0) - math.log(case.n * case.K)
    ll, base = R.ll_of(lws)
    nan = torch.isnan(x).any(0)
    assert torch.equal(torch.isnan(ll), nan)  # torch.logsumexp itself loses a NaN next to +inf; the reference does not
    assert torch.equal(R.klass(ll)[~nan], R.klass(want)[~nan])
    fin = torch.isfinite(ll)
    assert bool(((ll - want)[fin].abs() <= 1e-13 * base[fin]).all()) and (fin.all() == case.finite)
    if case.kind == "big":
        assert float(x.abs().min()) > 2.8e3 and float((x.max(0).values - x.min(0).values).min()) > 90


def test_non_finite_cases_have_the_named_classes():
    for name, cls_row1 in (("iw-nan-expert-k4-b3-l5-e3-r1", 1), ("iw-nan-first-expert-k4-b3-l5-e3-r1", 1), ("iw-all-experts-minf-k4-b3-l5-e2-r1", 2),
                           ("iw-one-expert-minf-k4-b3-l5-e3-r1", 0)):
        case = R.BY_NAME[name]
        inp = R.make_inputs(case)
        z, _ = R.z_of("normal", inp["sloc"], inp["ssd"], inp["noise"])
        lw, _, _ = R.lw_of("normal", z, inp["rows"], inp["locs"], inp["sds"], inp["ploc"], inp["psd"])
        cls = R.klass(lw)
        assert bool((cls[:, 1] == cls_row1).all()) and bool((cls[:, [0, 2]] == 0).all()), name
        assert R.klass(R.ll_of([lw])[0]).tolist() == [0, cls_row1, 0]
        if cls_row1 == 1:
            assert float(z[2, 1, 2]) == float(inp["locs"][1 if case.special == "nan" else 0][1, 2])  # z == loc where sd = 0


# ---- the constants ------------------------------------------------------------------------------------------------------------------------------
def measure():
    worst = {}
    for case in R.CASES:
        inp, out = G.run_case(case, BE)
        for k, v in G.case_ratios(case, inp, out[0]).items():
            G.note(worst, k, v, case.name)
    for case in R.REDUCE_CASES:
        lws, got, _ = G.run_reduce(case, BE)
        for k, v in G.reduce_ratios(case, lws, got).items():
            G.note(worst, k, v, case.name)
    return worst


def test_error_constants():
    """Measured stages: C = 4x the largest |err| / (U base) of the stand-in against the float64 reference over the case tables,
    rounded up: never below 4x the measured value, never above 8x (or 1).  The derived stage: the stand-in stays inside.  The
    figures and the cases that set them are in the docstring of tests/test_gpu_iwae.py."""
    worst = measure()
    print({k: (round(v, 3), n) for k, (v, n) in sorted(worst.items())})
    assert set(worst) == set(R.C_STAGE)
    for k in R.MEASURED_STAGES:
        v, name = worst[k]
        assert 4 * v <= R.C_STAGE[k], f"{k}: fp32 on the CPU shows {v:.3g} on {name}; C = {R.C_STAGE[k]} is less than 4x that"
        assert R.C_STAGE[k] <= max(8 * v, 1), f"{k}: C = {R.C_STAGE[k]} is more than 8x the measured {v:.3g}"
    for k in R.DERIVED:
        assert worst[k][0] <= R.C_STAGE[k], (k, worst[k])


# ---- the GPU file's comparison routines on the stand-in ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
def test_check_case(case):
    G.check_case(case, BE)


@pytest.mark.parametrize("case", R.REDUCE_CASES, ids=[c.name for c in R.REDUCE_CASES])
def test_check_reduce(case):
    G.check_reduce(case, BE)


@pytest.mark.parametrize("mut,stages,name", G.TEETH_IDS, ids=[f"{t[0]}-{t[2]}" for t in G.TEETH_IDS])
def test_tolerance_rejects_mutated_reference(mut, stages, name):
    f = G.teeth_factor(mut, stages, name, BE)
    print(mut, name, f"{f:.3g}x the bound")
    assert f > 1.0, f"{mut} passes on {name}: {f:.3g}x the bound"


def test_case_tables_hold_the_edges():
    """The shapes of the issue, read off the launch code of the three entries."""
    cs, rc = R.CASES, R.REDUCE_CASES
    assert all(c.why for c in cs + rc)
    assert {c.R for c in cs} >= {0, 8} and {c.prior for c in cs} == {"none", "loc", "sd", "both"} and {c.L for c in cs} >= {1, 64, 130}
    assert {c.E for c in cs} >= {1, R.MAXE} and {c.family for c in cs} == {"normal", "laplace", "softplus"}
    assert any((c.K * c.B * c.L) % 256 for c in cs if c.K * c.B * c.L > 256) and any((c.K * c.B) % 256 for c in cs if c.K * c.B > 256)
    assert {c.special for c in cs} == {"", "nan", "nan0", "minf1", "minf"} and any(c.noise == "edges" for c in cs)
    assert {c.K for c in rc} >= {1, 63, 64, 65, 1000} and {c.B for c in rc} >= {1, 3, 4, 5} and {c.n for c in rc} >= {1, 8}
    assert {c.kind for c in rc} == {"plain", "big", "minf", "pinf", "nan"}
    inp = R.make_inputs(R.BY_NAME["iw-laplace-edges-k5-b3-l7-e2-r1"])
    n = inp["noise"].reshape(-1)[:16].tolist()
    assert {0.0, 1.0 - 2.0 ** -24, -(1.0 - 2.0 ** -24), 2.0 ** -126, -(2.0 ** -149)} <= set(n) and bool((inp["noise"].abs() < 1).all())
