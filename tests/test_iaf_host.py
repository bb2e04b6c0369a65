"""The inverse autoregressive flow on the host.  The `IAF` module (multivae_amd/models/nn/flows.py) against the float64 restatement
of tests/iaf_ref.py and against its own definition (inverse o forward, opposite log-determinants, the log-determinant against
slogdet of the autograd Jacobian), its state-dict layout and refusals, `fused_layout`; the reverse-sweep backward of
tests/iaf_ref.py against float64 autograd through the module; the error constants and the mutation checks of tests/iaf_ref.py (the
reference and error model behind tests/test_gpu_iaf.py) against the same formulas in plain torch fp32."""
import pytest
import torch

import iaf_ref as R

F64 = torch.float64
_CACHE = {}
SHAPES = [(2, 3, 1, 1), (3, 5, 1, 2), (5, 7, 3, 2), (20, 128, 3, 2)]  # (D, H, hidden layers, blocks)


def torch32(case):
    """(inputs, the formulas in torch fp32, float64 reference, bases) of a case, computed once and left unchanged."""
    if case.name not in _CACHE:
        inp = R.make_inputs(case)
        ref = R.reference(case, inp)
        _CACHE[case.name] = (inp, R.run_torch32(case, inp), ref, R.bases(case, inp, ref))
    return _CACHE[case.name]


def _iaf(D, H, nh, nb, seed=0, scale=1.0):
    from multivae_amd.models.nn.flows import IAF, IAFConfig

    torch.manual_seed(seed)
    flow = IAF(IAFConfig(input_dim=(D,), n_made_blocks=nb, n_hidden_in_made=nh, hidden_size=H)).double()
    with torch.no_grad():
        for p in flow.parameters():
            p.mul_(scale)
    return flow


def _params(flow):
    """W[blk][l], b[blk][l] of a flow module."""
    from multivae_amd.models.nn.flows import MaskedLinear

    W = [[mod.weight for mod in made.net if isinstance(mod, MaskedLinear)] for made in flow.net]
    b = [[mod.bias for mod in made.net if isinstance(mod, MaskedLinear)] for made in flow.net]
    return W, b


# ---- the module ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,H,nh,nb", SHAPES)
def test_module_matches_the_float64_restatement(D, H, nh, nb):
    flow = _iaf(D, H, nh, nb, seed=D)
    W, b = _params(flow)
    g = torch.Generator().manual_seed(21 + D)
    x = torch.randn(6, D, generator=g, dtype=F64)
    with torch.no_grad():
        out = flow(x)
        z0, ladj = R.iaf_forward(W, b, x)
        assert torch.allclose(out.out, z0, rtol=0, atol=1e-13) and torch.allclose(out.log_abs_det_jac, ladj, rtol=0, atol=1e-13)
        inv = flow.inverse(x)
        xi, li = R.iaf_inverse(W, b, x)
        assert torch.allclose(inv.out, xi, rtol=0, atol=1e-13) and torch.allclose(inv.log_abs_det_jac, li, rtol=0, atol=1e-13)


@pytest.mark.parametrize("D,H,nh,nb", SHAPES)
def test_inverse_of_forward_and_opposite_log_determinants(D, H, nh, nb):
    flow = _iaf(D, H, nh, nb, seed=3 + D)
    g = torch.Generator().manual_seed(5 + D)
    x = torch.randn(7, D, generator=g, dtype=F64)
    with torch.no_grad():
        fwd = flow(x)
        back = flow.inverse(fwd.out)
    assert fwd.out.shape == (7, D) and fwd.log_abs_det_jac.shape == (7,)
    assert torch.allclose(back.out, x, rtol=0, atol=1e-10)
    assert torch.allclose(back.log_abs_det_jac, -fwd.log_abs_det_jac, rtol=0, atol=1e-10)


def test_log_determinant_is_that_of_the_jacobian():
    flow = _iaf(4, 9, 2, 3, seed=1)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(3, 4, generator=g, dtype=F64)
    ladj = flow(x).log_abs_det_jac
    for r in range(3):
        J = torch.autograd.functional.jacobian(lambda v: flow(v.unsqueeze(0)).out[0], x[r])
        assert torch.allclose(torch.linalg.slogdet(J)[1], ladj[r], rtol=0, atol=1e-10)


def test_state_dict_keys_and_fused_layout():
    from multivae_amd.models.nn.flows import IAF, MAF, MAFConfig, fused_layout

    flow = _iaf(5, 7, 3, 2)
    keys = set(flow.state_dict())
    want = {f"net.{k}.net.{2 * l}.{n}" for k in range(2) for l in range(4) for n in ("weight", "bias", "mask")}
    assert keys == want
    assert flow.model_name == "IAF" and flow.input_dim == (5,)
    lay = fused_layout(flow, IAF)
    assert lay is not None and lay[:4] == (5, 7, 3, 2) and len(lay[4]) == 8
    assert fused_layout(flow) is None and fused_layout(flow, MAF) is None  # an IAF is never taken for a MAF
    maf = MAF(MAFConfig(input_dim=(5,), n_made_blocks=2, n_hidden_in_made=3, hidden_size=7))
    assert fused_layout(maf, IAF) is None and fused_layout(maf) is not None
    with torch.no_grad():
        flow.net[1].net[2].mask[0, 0] = 1 - flow.net[1].net[2].mask[0, 0]
    assert fused_layout(flow, IAF) is None  # a mask the kernels would not compute


def test_refusals():
    from multivae_amd.models.nn.flows import IAF, IAFConfig, MAFConfig

    with pytest.raises(NotImplementedError, match="include_batch_norm"):
        IAF(IAFConfig(input_dim=(4,), include_batch_norm=True))
    with pytest.raises(AttributeError, match="input_dim"):
        IAF(IAFConfig())
    a, b = IAFConfig(input_dim=(4,)).to_dict(), MAFConfig(input_dim=(4,)).to_dict()
    a.pop("name"), b.pop("name")
    assert a == b  # the same fields and defaults


# ---- the reverse sweep ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,H,nh,nb", SHAPES)
def test_sweep_backward_equals_float64_autograd_through_the_module(D, H, nh, nb):
    flow = _iaf(D, H, nh, nb, seed=7 + D)
    W, b = _params(flow)
    g = torch.Generator().manual_seed(9 + D)
    B = 5
    x = torch.randn(B, D, generator=g, dtype=F64).requires_grad_(True)
    I = dict(grows=torch.randn(B, generator=g, dtype=F64), dz0=torch.randn(B, D, generator=g, dtype=F64),
             dladj=torch.randn(B, generator=g, dtype=F64))
    out = flow(x)
    z0, ladj = out.out, out.log_abs_det_jac
    total = (R.nll_rows(z0, ladj) * I["grows"]).sum() + (z0 * I["dz0"]).sum() + (ladj * I["dladj"]).sum()
    flatW, flatb = [w for Wb in W for w in Wb], [v for bb in b for v in bb]
    gs = torch.autograd.grad(total, [x] + flatW + flatb)
    with torch.no_grad():
        saved = []
        z0r, _ = R.iaf_forward(W, b, x.detach(), keep=saved)
        gz0, gl = R.upstream(I, z0r, F64)
        dx, dW, db = R.sweep_backward(W, b, saved, gz0, gl)
    masked = [m.mask for made in flow.net for m in made.net if hasattr(m, "mask")]
    for got, want, mask in zip([dx] + dW + db, gs, [None] + masked + [None] * len(db)):
        scale = float(want.abs().max()) + 1e-300
        assert float((got - want).abs().max()) <= 1e-12 * scale + 1e-14
        if mask is not None:
            assert float((got * (1 - mask)).abs().max()) == 0.0  # a masked weight has no gradient


# ---- the error model ------------------------------------------------------------------------------------------------------------------------
def test_case_table():
    names = [c.name for c in R.CASES]
    assert len(set(names)) == len(names) == 4 * 3 * 2 * 3 * 3 + 1
    assert {(c.D, c.H, c.nh, c.nb, c.B) for c in R.CASES if c.backward} == {
        (D, H, nh, nb, B) for D in (2, 3, 20, 65) for H in (3, 64, 130) for nh in (1, 3) for nb in (1, 2, 3) for B in (1, 3, 70)}
    last = R.CASES[-1]
    assert last.D == 512 and not last.backward
    for n in R.NULLS:
        assert any(c.null == n for c in R.CASES)


def test_error_constants():
    """C_STAGE = 4x the largest |err| / base of the formulas in plain torch fp32 (backward: fp32 autograd through the forward sweep)
    against the float64 reference, rounded up, over the whole case table; every |s| of the table stays below LV_MAX (asserted inside
    `bases`)."""
    worst = {}
    for case in R.CASES:
        inp = R.make_inputs(case)  # not cached: 217 cases
        ref = R.reference(case, inp)
        base = R.bases(case, inp, ref)
        for k, v in R.ratios(case, inp, R.run_torch32(case, inp), ref=ref, base=base).items():
            if v > worst.get(k, (-1.0, ""))[0]:
                worst[k] = (v, case.name)
    print({k: (round(v, 3), n) for k, (v, n) in sorted(worst.items())})
    assert set(worst) == set(R.C_STAGE)
    for k, (v, name) in worst.items():
        assert 4 * v <= R.C_STAGE[k], f"{k}: torch fp32 shows {v:.3g} on {name}; C = {R.C_STAGE[k]} is less than 4x that"
        assert R.C_STAGE[k] <= 4 * v * 1.25 + 0.1, f"{k}: C = {R.C_STAGE[k]} is looser than 4 x {v:.3g} rounded up"


@pytest.mark.parametrize("mut,stages,names", R.TEETH, ids=[t[0] for t in R.TEETH])
def test_tolerance_rejects_mutated_reference(mut, stages, names):
    """Every wrong variant of the reference, compared with the unmutated fp32 output, leaves the bound in each stage named for it
    on EVERY case named for it (the GPU test repeats this on the kernels' output)."""
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
    assert {t[0] for t in R.TEETH} == set(R.MUTATIONS)
    for _, stages, names in R.TEETH:
        assert set(stages) <= set(R.STAGES) and all(n in R.CASE_BY_NAME for n in names)
