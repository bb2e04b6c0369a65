"""CPU checks of tests/elbo_ref.py, the float64 reference behind tests/test_gpu_elbo_posterior.py:

- on every case the reference gives the forward values and the autograd gradients of oracle.elbo evaluated in float64
  (mopoe_inference + mopoe_joint_divergence + rsample; mvtcae_forward; stable_poe + rsample with mvae_forward's KL;
  jmvae_forward; rsample + the style KL), to 1e-12;
- the error constants C_STAGE are 4x what oracle.elbo in plain torch fp32 (backward: fp32 autograd) shows against the float64
  reference over the case table;
- every mutation of elbo_ref.TEETH leaves the bound on a named case while the unmutated reference stays inside, against the torch
  fp32 evaluation (the GPU test repeats this on the kernels' output);
- exact properties of the reference: an MVAE subset with nothing present gives KL = 0 and z = eps; the gradients of a missing
  modality's rows are 0; the subset lists are oracle.elbo's.
"""
import pytest
import torch

import elbo_ref as R
from oracle import elbo

F64 = torch.float64
IDS = [c.name for c in R.CASES]
_CACHE = {}


def torch32(case):
    """(inputs, oracle.elbo in fp32, float64 reference, bases) of a case, computed once and left unchanged."""
    if case.name not in _CACHE:
        inp = R.make_inputs(case)
        _CACHE[case.name] = (inp, R.run_torch32(case, inp), R.reference(case, inp), R.bases(case, inp))
    return _CACHE[case.name]


def _pairs(a, b):
    for k in a:
        xs, ys = (a[k], b[k]) if isinstance(a[k], list) else ([a[k]], [b[k]])
        for i, (x, y) in enumerate(zip(xs, ys)):
            if x is not None:
                yield f"{k}[{i}]", x, y


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_reference_is_the_oracle_in_float64(case):
    """Both sides are float64 evaluations of the same formulas in different operation orders, so they differ by rounding alone:
    n 2^-53 times the sum of the absolute values of the terms of an entry, n the number of operations behind it.  base / u is
    that sum (the error model's term magnitudes), and n < 4500 = 1e-12 / 2^-53 for every entry here (the longest chain: the
    MoPoE KL rows, 31 subsets x 5 latent dims x ~10 operations), hence |a - b| <= 1e-12 * base / u entry by entry: 1e-12
    relative to the magnitude of what is summed, which is the only meaning "relative" has for the cancelling entries."""
    inp, _, ref, base = torch32(case)
    orc = R.oracle_eval(case, inp, F64)
    assert set(orc) == set(ref)
    for (k, x, y), (_, _, b) in zip(_pairs(ref, orc), _pairs(ref, base)):
        assert x.dtype == F64 and y.dtype == F64 and x.shape == y.shape
        r = R.worst_ratio(x, y, 1e-12 * b / R.U)
        assert r <= 1.0, f"{case.name}: {k} differs from the float64 oracle by {r:.3g} x 1e-12 of its term magnitude"


def measure():
    worst = {}
    for case in R.CASES:
        inp, got, ref, base = torch32(case)
        for k, (v, arr) in R.ratios(case, inp, got, ref=ref, base=base).items():
            if v > worst.get(k, (-1.0, ""))[0]:
                worst[k] = (v, case.name)
    return worst


def test_error_constants():
    """C_STAGE = 4x the largest |err| / base of oracle.elbo in plain torch fp32 (backward: fp32 autograd) against the float64
    reference, rounded up, over the whole case table.  The measured values and the cases that set them are in the docstring of
    tests/test_gpu_elbo_posterior.py."""
    worst = measure()
    print({k: (round(v, 2), n) for k, (v, n) in sorted(worst.items())})
    assert set(worst) == set(R.C_STAGE)
    for k, (v, name) in worst.items():
        assert 4 * v <= R.C_STAGE[k], f"{k}: torch fp32 shows {v:.3g} on {name}; C = {R.C_STAGE[k]} is less than 4x that"
        assert R.C_STAGE[k] <= 4 * v * 1.25 + 1, f"{k}: C = {R.C_STAGE[k]} is looser than 4 x {v:.3g} rounded up"


@pytest.mark.parametrize("mut,stages,names", R.TEETH, ids=[t[0] for t in R.TEETH])
def test_tolerance_rejects_mutated_reference(mut, stages, names):
    """Every wrong variant of the reference, compared with the unmutated fp32 oracle output, leaves the bound in each stage
    named for it on at least one of its cases (a stage of another family than the case's does not apply to it); the factors are
    recorded in the GPU test's docstring."""
    best = {s: 0.0 for s in stages}
    for name in names:
        case = R.CASE_BY_NAME[name]
        inp, got, ref, base = torch32(case)
        clean = R.ratios(case, inp, got, ref=ref, base=base)
        assert all(v <= R.C_STAGE[k] for k, (v, _) in clean.items()), clean
        bad = R.ratios(case, inp, got, mut=(mut,), base=base)
        for s in stages:
            if s in bad:
                f = bad[s][0] / R.C_STAGE[s]
                print(mut, name, s, f"{f:.3g}x the bound")
                best[s] = max(best[s], f)
    for s, f in best.items():
        assert f > 1.0, f"{mut} passes {s} on all of {names}: at most {f:.3g}x the bound"


def test_mvae_subset_with_nothing_present_is_the_prior():
    case = R.CASE_BY_NAME["mvae-m3-b9-l20-empty-graded"]
    inp, _, ref, _ = torch32(case)
    hit = 0
    for s, bt in enumerate(inp["bits"]):
        members = [m for m in range(case.M) if (bt >> m) & 1]
        gone = ~torch.stack([inp["masks"][m] for m in members]).any(0)
        if not bool(gone.any()):
            continue
        hit += 1
        assert bool((ref["kld"][s][gone] == 0).all())
        assert bool((ref["sub_mu"][s][gone] == 0).all()) and bool((ref["sub_lv"][s][gone] == 0).all())
        for m in members:
            slab = sum(1 for t in inp["bits"][:s] if (t >> m) & 1)
            assert torch.equal(ref["zm"][m][slab][gone], inp["eps"][s][gone].double())
    assert hit == 2  # the unimodal subsets of modalities 1 and 2 (the joint one always holds modality 0)


@pytest.mark.parametrize("name", ["mvtcae-m3-k4-b9-l5-one", "mvtcae-m2-k5-b9-l20-tail-graded", "mvae-m3-b9-l5-one",
                                  "mvae-m3-b9-l20-empty-graded"])
def test_missing_rows_have_zero_gradient(name):
    case = R.CASE_BY_NAME[name]
    inp, _, ref, base = torch32(case)
    for m in range(case.M):
        gone = ~inp["masks"][m]
        assert bool(gone.any()) or m == 0
        for k in ("dmu", "dlv"):
            assert bool((ref[k][m][gone] == 0).all()) and bool((base[k][m][gone] == 0).all())


def test_case_table_follows_the_oracle():
    """sel follows mopoe_row_bounds where weights is NULL; the MVAE lists are mvae_subsets; every case names its edge; the table
    holds the shape edges of the issue and nothing larger."""
    names = lambda M: [f"m{i}" for i in range(M)]
    for case in R.CASES:
        assert case.why and case.B <= 260 and case.L <= 130 and case.K <= 11 and case.M <= 8
        inp = R.make_inputs(case)
        if case.fam == "mopoe" and inp["weights"] is None:
            bnd = elbo.mopoe_row_bounds(case.B, len(inp["bits"]))
            for k in range(len(inp["bits"])):
                assert bool((inp["sel"][bnd[k]:bnd[k + 1]] == k).all())
        if case.fam == "mopoe" and case.sub != "chosen":
            assert len(inp["bits"]) == len(elbo.mopoe_subsets(names(case.M))) == 2 ** case.M - 1
        if case.fam == "mvae":
            assert inp["bits"][0] == (1 << case.M) - 1 and len(inp["bits"]) <= R.MAX_SUBSETS
            if case.sub != "joint":
                assert inp["bits"][1:case.M + 1] == [1 << m for m in range(case.M)]
            assert all(float(lv.min()) >= -80 for lv in inp["lvs"])
        if inp["masks"] is not None:
            assert bool(torch.stack(inp["masks"]).any(0).all())
    for fam in ("mopoe", "mvtcae", "mvae", "jmvae", "gauss"):
        cs = [c for c in R.CASES if c.fam == fam]
        assert {c.B for c in cs} >= {1, 3, 4, 5, 9, 260} and {c.L for c in cs} >= {1, 5, 63, 64, 65, 130}
        if fam != "mvae":
            assert {c.K for c in cs} >= {1, 4, 5, 7, 11}
        if fam != "gauss":
            assert {c.M for c in cs} >= {1, 2, 3, 8}
    assert max(len(R.make_inputs(c)["bits"]) for c in R.CASES if c.fam == "mvae") == R.MAX_SUBSETS
