"""CPU checks of tests/base_utils_ref.py, the float64 reference behind tests/test_gpu_base_utils.py:

- on every case the reference gives the values and the autograd gradients of oracle.elbo (poe, stable_poe, kl_divergence,
  recon_log_prob) evaluated in float64;
- the error constants C_STAGE are 4x what oracle.elbo in plain torch fp32 (backward: fp32 autograd) shows against the float64
  reference over the case table;
- every mutation of base_utils_ref.TEETH leaves the bound on a named case while the unmutated reference stays inside;
- the comparison routine of the GPU file passes on every case with a stand-in launcher that returns the fp32 oracle's outputs;
- the case table holds the shape edges it is meant to hold.
"""
import pytest
import torch

import base_utils_ref as R
import test_gpu_base_utils as G

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
    n 2^-53 times the sum of the absolute values of the terms of an entry, with n < 4500 = 1e-12 / 2^-53 operations behind every
    entry here (the longest chain: a KL row over 130 columns of ~10 operations); base / u is that sum, hence
    |a - b| <= 1e-12 * base / u entry by entry."""
    inp, _, ref, base = torch32(case)
    orc = R.oracle_eval(case, inp, F64)
    assert set(orc) == set(ref)
    for k in ref:
        assert ref[k].dtype == F64 and orc[k].dtype == F64 and ref[k].shape == orc[k].shape
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
    """C_STAGE = 4x the largest |err| / base of oracle.elbo in plain torch fp32 against the float64 reference, rounded up, over the
    whole case table: never below the measured value, never more than 8x above it."""
    worst = measure()
    print({k: (round(v, 3), n) for k, (v, n) in sorted(worst.items())})
    assert set(worst) == set(R.C_STAGE)
    for k, (v, name) in worst.items():
        assert 4 * v <= R.C_STAGE[k], f"{k}: torch fp32 shows {v:.3g} on {name}; C = {R.C_STAGE[k]} is less than 4x that"
        assert R.C_STAGE[k] <= 8 * v, f"{k}: C = {R.C_STAGE[k]} is more than 8x the measured {v:.3g}"


@pytest.mark.parametrize("mut,stages,names", R.TEETH, ids=[t[0] for t in R.TEETH])
def test_tolerance_rejects_mutated_reference(mut, stages, names):
    """Every wrong variant of the reference, compared with the unmutated fp32 oracle output, leaves the bound in each stage
    named for it on at least one of its cases (a stage of another family than the case's does not apply to it)."""
    best = {s: 0.0 for s in stages}
    for name in names:
        case = R.CASE_BY_NAME[name]
        inp, got, ref, base = torch32(case)
        clean = R.ratios(case, got, ref, base)
        assert all(v <= R.C_STAGE[k] for k, v in clean.items()), clean
        bad = R.ratios(case, got, R.reference(case, inp, mut=(mut,)), base)
        for s in stages:
            if s in bad:
                f = bad[s] / R.C_STAGE[s]
                print(mut, name, s, f"{f:.3g}x the bound")
                best[s] = max(best[s], f)
    for s, f in best.items():
        assert f > 1.0, f"{mut} passes {s} on all of {names}: at most {f:.3g}x the bound"


def standin_launch(case, inp, null=frozenset()):
    """The fp32 oracle in the place of the HIP launch (an input named in `null` is left out, one not named is zeros)."""
    inp = dict(inp)
    for k in ("gmu", "glv"):
        if k in inp and inp[k] is None and k not in null:
            inp[k] = torch.zeros(case.n)
    out = {k: v + 0.0 for k, v in R.run_torch32(case, inp).items() if k not in null}  # + 0.0: autograd's -0.0 for a zero seed
    out["guards"] = True
    return out


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_gpu_comparison_routine_on_the_oracle(case):
    G.check_case(case, standin_launch)


def test_case_table_holds_the_edges():
    cs = R.CASES
    for fam in ("poe", "spoe"):
        mine = [c for c in cs if c.fam == fam]
        assert {c.n for c in mine} >= {1, 255, 256, 257, 1300} and {c.E for c in mine} >= {1, 2, 3, 8}
        assert {x for c in mine for x in c.null} == {"gmu", "glv"}
    assert any(c.fam == "poe" and c.regime == "eps" for c in cs) and any(c.fam == "spoe" and c.regime == "inf" for c in cs)
    kl = [c for c in cs if c.fam == "kl"]
    assert {c.K * c.B for c in kl} >= {1, 255, 257} and {c.L for c in kl} >= {1, 5, 130}
    for j in range(4):  # each operand at each size, under a shape where the four sizes differ
        assert {c.sizes[j] for c in kl if c.K > 1 and c.L > 1} == {"full", "bl", "l", "one"}
    lp = [c for c in cs if c.fam == "logprob"]
    assert {c.dist for c in lp} == set(R.DISTS)
    for dist in R.DISTS:
        assert {c.K > 1 for c in lp if c.dist == dist} == {True, False}
    cat = [c for c in lp if c.dist == "categorical"]
    assert {c.C for c in cat} >= {1, 64, 65, 130} and {c.K * c.nx // c.C for c in cat} >= {1, 3, 5, 9}
    for c in cs:
        assert c.why
        inp = R.make_inputs(c)
        if c.fam == "spoe":
            assert float(inp["lv"].min()) >= -80 and bool(torch.isfinite(inp["lv"]).any(0).all())
            assert (c.regime == "inf") == bool(torch.isinf(inp["lv"]).any())
        if c.fam == "poe" and c.regime == "eps":
            assert float(inp["lv"].min()) < -16
        if c.dist == "bernoulli" and c.nx > 1:
            assert float(inp["r"].max()) == 90.0 and float(inp["r"].min()) == -90.0
