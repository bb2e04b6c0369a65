"""CPU checks of tests/nll_ref.py, the float64 reference behind tests/test_gpu_recon_nll.py:

- on every case the reference gives the rows and the autograd gradient of oracle.elbo._row_nll evaluated in float64;
- the error constants C_STAGE are 4x what oracle.elbo in plain torch fp32 (backward: fp32 autograd) shows against the float64
  reference over the case table;
- every mutation of nll_ref.TEETH leaves the bound on a named case while the unmutated reference stays inside, against the torch
  fp32 evaluation; the log_softmax shift of 1e-6 is shown NOT to be rejected, because it cannot be;
- the comparison routine of the GPU file (check_case: bounds, NaN, exact properties, NULL forms, determinism) passes on every
  case with a stand-in launcher that returns the fp32 oracle's outputs;
- the case table holds the shape edges it is meant to hold, read off launch_recon and recon_vec_body.
"""
import dataclasses

import pytest
import torch

import nll_ref as R
import test_gpu_recon_nll as G

F64 = torch.float64
IDS = [c.name for c in R.CASES]
_CACHE = {}


def torch32(case):
    """(inputs, oracle.elbo in fp32, float64 reference, bases) of a case, computed once and left unchanged."""
    if case.name not in _CACHE:
        inp = R.make_inputs(case)
        _CACHE[case.name] = (inp, R.run_torch32(case, inp), R.reference(case, inp), R.bases(case, inp))
    return _CACHE[case.name]


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_reference_is_the_oracle_in_float64(case):
    """Both sides are float64 evaluations of the same formulas in different operation orders, so they differ by rounding alone:
    n 2^-53 times the sum of the absolute values of the terms of an entry, n the number of operations behind it.  base / u is
    that sum, and n < 4500 = 1e-12 / 2^-53 for every entry here (the longest chain: a row sum over 4770 addends, whose pairwise
    summation in torch has depth < 20), hence |a - b| <= 1e-12 * base / u entry by entry."""
    inp, _, ref, base = torch32(case)
    orc = R.oracle_eval(case, inp, F64)
    for k in ("rows", "drecon"):
        assert (ref[k] is None) == (orc[k] is None) == (not case.drecon and k == "drecon")
        if ref[k] is not None:
            assert ref[k].dtype == F64 and orc[k].dtype == F64
            r = R.worst_ratio(ref[k], orc[k], 1e-12 * base[k] / R.U)
            assert r <= 1.0, f"{case.name}: {k} differs from the float64 oracle by {r:.3g} x 1e-12 of its term magnitude"


def measure():
    worst = {}
    for case in R.CASES:
        inp, got, ref, base = torch32(case)
        for k, v in R.ratios(case, got, ref, base).items():
            if v > worst.get(k, (-1.0, ""))[0]:
                worst[k] = (v, case.name)
    return worst


def test_error_constants():
    """C_STAGE = 4x the largest |err| / base of oracle.elbo in plain torch fp32 (backward: fp32 autograd) against the float64
    reference, rounded up, over the whole case table: never below the measured value, never more than 8x above it.  The measured
    values and the cases that set them are in the docstring of tests/test_gpu_recon_nll.py."""
    worst = measure()
    print({k: (round(v, 3), n) for k, (v, n) in sorted(worst.items())})
    assert set(worst) == set(R.C_STAGE)
    for k, (v, name) in worst.items():
        assert 4 * v <= R.C_STAGE[k], f"{k}: torch fp32 shows {v:.3g} on {name}; C = {R.C_STAGE[k]} is less than 4x that"
        assert R.C_STAGE[k] <= 8 * v, f"{k}: C = {R.C_STAGE[k]} is more than 8x the measured {v:.3g}"


@pytest.mark.parametrize("mut,kind,names", R.TEETH, ids=[t[0] for t in R.TEETH])
def test_tolerance_rejects_mutated_reference(mut, kind, names):
    """Every wrong variant of the reference, compared with the unmutated fp32 oracle output, leaves the bound of its stage on
    every case named for it; the factors are printed."""
    for name in names:
        case = R.CASE_BY_NAME[name]
        inp, got, ref, base = torch32(case)
        clean = R.ratios(case, got, ref, base)
        assert all(v <= R.C_STAGE[k] for k, v in clean.items()), clean
        bad = R.ratios(case, got, R.reference(case, inp, mut=(mut,)), base)
        st = f"{case.dist}.{kind}"
        f = bad[st] / R.C_STAGE[st]
        print(mut, name, st, f"{f:.3g}x the bound")
        assert f > 1.0, f"{mut} passes {st} on {name}: {f:.3g}x the bound"


def test_softmax_shift_is_not_rejected_and_cannot_be():
    """log_softmax(r + 1e-6) == log_softmax(r) as functions: the shift moves every logit of a position by the same amount.  What
    the fp32 kernel and the fp32 oracle see of it is the rounding of r + 1e-6 (half an ulp of r per logit, not uniform), which
    the base already carries in EL and in sum|x v|.  A reference without the shift therefore stays inside every bound; no case can
    separate the two, and none should be added to try."""
    worst = 0.0
    for case in R.CASES:
        if case.dist != "categorical":
            continue
        inp, got, ref, base = torch32(case)
        noshift = R.reference(case, inp, mut=(R.NOOP_MUT,))
        for k, v in R.ratios(case, got, noshift, base).items():
            assert v <= R.C_STAGE[k], (case.name, k, v)
        for k in ("rows", "drecon"):
            if ref[k] is not None:
                worst = max(worst, R.worst_ratio(noshift[k], ref[k], base[k]))
    print(f"reference without the shift against the reference: at most {worst:.3g} of base")
    assert worst < 0.01


def standin_launch(case, recon, x, mask, rowcoef, drecon, coef, via):
    """The fp32 oracle in the place of the HIP launch."""
    c = dataclasses.replace(case, drecon=drecon, coef=coef)
    out = R.oracle_eval(c, dict(recon=recon, x=x, mask=mask, rowcoef=rowcoef), torch.float32)
    return dict(rows=out["rows"] if via == "fwd" else None, drecon=out["drecon"], guards=True)


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_gpu_comparison_routine_on_the_oracle(case):
    G.check_case(case, standin_launch)


def test_laplace_ties_and_masked_rows_have_zero_gradient():
    hit = 0
    for case in R.CASES:
        inp, _, ref, _ = torch32(case)
        if ref["drecon"] is None:
            continue
        if case.dist == "laplace":
            tie = inp["recon"] == inp["x"].unsqueeze(0)
            assert bool(tie.any()) and bool((ref["drecon"][tie] == 0).all())
            hit += 1
        if inp["mask"] is not None:
            assert bool((~inp["mask"]).any()) and bool((ref["drecon"][:, ~inp["mask"]] == 0).all())
            hit += 1
    assert hit >= 10


def test_case_table_holds_the_edges():
    """The shapes of the issue, read off launch_recon / recon_vec_body; large rows only in small launches."""
    cs = R.CASES
    vec = {c.D for c in cs if c.dist != "categorical" and c.D % 4 == 0 and not c.misalign}
    assert vec >= {4, 1020, 1024, 1028, 3072, 3076, 4100}
    assert {c.D for c in cs if c.dist != "categorical" and c.D % 4} >= {1, 3, 255, 257, 1023, 4099}
    assert {c.misalign for c in cs if c.D == 784} >= {"recon", "x", "drecon"}
    assert {c.K for c in cs} >= {1, 10, 16, 17, 33} and {c.B for c in cs} >= {1, 3, 5, 9}
    assert {c.scale for c in cs if c.dist == "normal"} >= {1.0, 0.75, R.f32(0.4), R.f32(0.01)}
    assert {c.regime for c in cs if c.dist == "bernoulli"} == {"hard", "soft"}
    cat = [c for c in cs if c.dist == "categorical"]
    assert {c.C for c in cat} >= {1, 2, 63, 64, 65, 130, 1590} and {c.D // c.C for c in cat} >= {1, 3, 4, 5, 32}
    assert {c.regime for c in cat} == {"onehot", "soft", "zeros"}
    assert {c.mask for c in cs} == {"none", "random", "all", "last"}
    for dist in R.DISTS:
        mine = [c for c in cs if c.dist == dist]
        assert {c.drecon for c in mine} == {True, False} and {c.rowcoef for c in mine} == {True, False}
        assert any(c.rescale != 1 for c in mine) and any(c.coef != 1 for c in mine) and any(c.mask != "none" for c in mine)
    for c in cs:
        assert c.why and (c.D <= 1024 or c.K * c.B <= 51), c.name
        assert c.dist != "categorical" or c.D % c.C == 0
        inp = R.make_inputs(c)
        if c.dist == "bernoulli":
            assert float(inp["recon"].max()) == 90.0 and float(inp["recon"].min()) == -90.0
        if c.dist == "categorical" and c.C > 1:
            assert float(inp["recon"].abs().max()) > 30.0
        if c.regime == "zeros":
            assert bool((inp["x"].reshape(c.B, -1, c.C).sum(-1) == 0).any())
    assert len(R.ONE_LAUNCH) == 8 and {c.dist for c in R.ONE_LAUNCH} == set(R.DISTS)
