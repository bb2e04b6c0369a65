"""MAFSampler, IAFSampler and samplers/flow_fit.py on the GPU: the fused fit (mvk_maf_fwd/bwd or mvk_iaf_fwd/bwd and one fused Adam
launch per step) against the torch-module fit, the learning condition of tests/flow_samplers_ref.py on the fused path, the
fused `sample` (mvk_maf_inverse / mvk_iaf_inverse) against float64, save and reload on the device, and MVAE / DMVAE (style spaces
of different dimensions) end to end through both paths.

Bounds.  The NLL rows of a flow carry the `rows` bound of the float64 error models (tests/jnf_ref.py for the MAF with mu0 = lv0 = 0,
tests/iaf_ref.py for the IAF): |row - float64| <= C_STAGE["rows"] * base.  A step's loss is the sum of its batch's rows: two fits
from the same parameters and batches must agree within the batch's summed bound plus the rounding of the sum itself (depth(B) u
sum |row|).  Compared are the losses of three steps, not the parameters behind Adam: its first steps are sign-like and
ill-conditioned where a gradient is near zero.  A sample z = inverse(u) is within C_STAGE["x_inv"] * base of the float64 inverse, and
`flow.forward(z)` (the torch module, fp32) recovers u within the forward bound C_STAGE["z0"] * base at z plus the inverse bound
carried through the forward's float64 Jacobian (first order).

Shown on an MI355X (test_zz_report prints HIP_MEASURED; recorded, not bounds), as fractions of those bounds: the fits' step losses
differ by at most 0.001 (MAF) and 0.013 (IAF), a sample is within 0.008 (MAF) and 0.022 (IAF) of the inverse bound, the round trip
within 0.002 and 0.004.  The learning condition on the fused path: eval NLL 5.86 -> 2.725 (MAF) and 5.819 -> 2.711 (IAF) against
6.123 under N(0, I), best epoch 27 of 40, the same figures as the module path on the host."""
import os

import pytest
import torch

import iaf_ref as RI
import jnf_ref as RM
from flow_samplers_ref import DIMS, KINDS, check_learning, classes, eval_nll, fit_config, learning_setup, two_modalities

pytestmark = pytest.mark.gpu
D0 = torch.device("cuda:0")
MEASURED = {}


def note(key, value, what):
    if value > MEASURED.get(key, (-1.0, ""))[0]:
        MEASURED[key] = (value, what)


def nested(flow):
    """W[blk][l], b[blk][l] of a flow module, fp32 on the CPU."""
    from multivae_amd.models.nn.flows import MaskedLinear

    W = [[mod.weight.detach().cpu().clone() for mod in made.net if isinstance(mod, MaskedLinear)] for made in flow.net]
    b = [[mod.bias.detach().cpu().clone() for mod in made.net if isinstance(mod, MaskedLinear)] for made in flow.net]
    return W, b


def error_model(kind, flow, x, y):
    """-> (float64 reference, bases) of the flow's forward at x [B,D] (z0, ladj, rows) and inverse at y [B,D] (x_inv), from the
    float64 restatements, under the stage names of iaf_ref."""
    W, b = nested(flow)
    B, Dm = x.shape
    H, nh, nb = W[0][0].shape[0], len(W[0]) - 1, len(W)
    x, y = x.detach().cpu().float(), y.detach().cpu().float()
    if kind == "iaf":
        case = RI.Case("flow", Dm, H, nh, nb, B, (), 0, backward=False)
        I = dict(W=W, b=b, x=x, y=y, grows=None, dz0=None, dladj=None)
        ref = RI.reference(case, I)
        return ref, RI.bases(case, I, ref), RI.C_STAGE
    case = RM.Case("flow", Dm, H, nh, nb, B, 1, (), 0, backward=False)
    zeros = torch.zeros(1, B, Dm)
    I = dict(W=[W], b=[b], z=x, y=y, mu0=zeros, lv0=zeros, grows=None, dz0=None, dladj=None)
    ref = RM.reference(case, I)
    base = RM.bases(case, I, ref)
    ref = dict(z0=ref["z0"][0], ladj=ref["ladj"][0], rows=ref["rows"][0], x_inv=ref["x_inv"])
    base = dict(z0=base["z0"][0], ladj=base["ladj"][0], rows=base["rows"][0], x_inv=base["x_inv"])
    return ref, base, RM.C_STAGE


def new_flow(kind, Dm, H, nh, nb, seed):
    _, _, Flow, FlowConfig = classes(kind)
    torch.manual_seed(seed)
    return Flow(FlowConfig(input_dim=(Dm,), n_made_blocks=nb, n_hidden_in_made=nh, hidden_size=H))


# ---- the fit: fused against the module ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Dm,H,nh,nb", [(2, 16, 1, 2), (5, 33, 2, 3), (20, 128, 3, 2)], ids=["d2", "d5", "d20"])
@pytest.mark.parametrize("kind", KINDS)
def test_fused_and_module_fit_agree(kind, Dm, H, nh, nb):
    from multivae_amd.samplers.flow_fit import batch_order, fit_flow

    g = torch.Generator().manual_seed(40 + Dm)
    codes = (torch.randn(150, Dm, generator=g) * 1.3 + 0.4).to(D0)
    fused, module = new_flow(kind, Dm, H, nh, nb, seed=9).to(D0), new_flow(kind, Dm, H, nh, nb, seed=9).to(D0)
    start = new_flow(kind, Dm, H, nh, nb, seed=9)
    cfg = dict(num_epochs=1, per_device_train_batch_size=64, learning_rate=1e-4, seed=11)
    hf = fit_flow(fused, codes, training_config=fit_config(**cfg), fused=True, max_steps=3)
    hm = fit_flow(module, codes, training_config=fit_config(**cfg), fused=False, max_steps=3)
    assert hf["fused"] is True and hm["fused"] is False and len(hf["step_loss"]) == len(hm["step_loss"]) == 3
    order = batch_order(150, 64, torch.Generator().manual_seed(11))
    assert [b.numel() for b in order] == [64, 64, 22]  # the last step runs a partial batch
    for step, idx in enumerate(order):
        xb = codes.cpu()[idx]
        ref, base, C = error_model(kind, start, xb, xb)
        bound = C["rows"] * float(base["rows"].sum()) + RM.depth(idx.numel()) * RM.U * float(ref["rows"].abs().sum())
        lf, lm = float(hf["step_loss"][step]), float(hm["step_loss"][step])
        ratio = abs(lf - lm) / bound
        print("FIT", kind, f"d{Dm}", "step", step, "fused", lf, "module", lm, "float64 at the initial parameters", float(ref["rows"].sum()),
              f"|fused - module| / bound = {ratio:.3g}")
        note(f"fit_{kind}", ratio, f"d{Dm} step {step}")
        assert abs(lf - lm) <= bound, f"step {step}: fused {lf} and module {lm} differ by {ratio:.3g}x the summed rows bound"
        if step == 0:  # the parameters are still the initial ones: each path against float64
            for name, v in (("fused", lf), ("module", lm)):
                assert abs(v - float(ref["rows"].sum())) <= bound, name
    # the fused fit leaves the flow's parameters as ordinary tensors that moved
    assert all(p.is_cuda and p.dtype == torch.float32 for p in fused.parameters())
    assert any(not torch.equal(p.cpu(), q) for p, q in zip(fused.parameters(), start.parameters()))


@pytest.mark.parametrize("kind", KINDS)
def test_learning_condition_fused(kind):
    from multivae_amd.samplers.flow_fit import fit_flow

    flow, train, evals, cfg = learning_setup(kind, D0)
    before = eval_nll(flow, evals)
    hist = fit_flow(flow, train, evals, training_config=cfg, fused=True)
    assert hist["fused"] is True and len(hist["eval_loss"]) == 40
    check_learning(flow, evals, before, hist)
    # the returned parameters are those of the best eval epoch: the eval loss (the mean over eval batches of the summed rows)
    best = hist["eval_loss"][hist["best_epoch"]]
    assert best == min(hist["eval_loss"])
    assert eval_nll(flow, evals) * 64 == pytest.approx(best, rel=1e-4)  # 256 eval codes in batches of 64


# ---- sample ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_fused_sample_against_float64(kind):
    Sampler, Config, _, _ = classes(kind)
    model = mvae()
    sampler = Sampler(model, Config(n_made_blocks=2, n_hidden_in_made=2, hidden_size=24))
    sampler.fit(two_modalities(90), training_config=fit_config(num_epochs=3, learning_rate=1e-2))
    assert sampler.fit_history["shared"]["fused"] is True
    out = sampler.sample(7, batch_size=3, generator=torch.Generator(device=D0).manual_seed(3))
    g = torch.Generator(device=D0).manual_seed(3)
    u = torch.cat([torch.randn(n, 4, generator=g, device=D0) for n in (3, 3, 1)])  # 7 = 3 + 3 + 1: one launch per batch
    flow = sampler.flows_models["shared"]
    z = out.z
    assert z.shape == (7, 4) and z.is_cuda
    ref, base, C = error_model(kind, flow, z, u)
    r_inv = RM.worst_ratio(z.cpu(), ref["x_inv"], base["x_inv"])
    note(f"sample_{kind}", r_inv, "x_inv")
    assert r_inv <= C["x_inv"], f"sample: |z - float64 inverse| is {r_inv:.3g} of the base, C = {C['x_inv']}"
    # flow.forward(z) recovers u: the forward bound at z plus the inverse bound carried through the forward's Jacobian
    with torch.no_grad():
        back = flow(z).out.cpu()
    f64 = type(flow)(flow.model_config).double()
    f64.load_state_dict({k: v.double().cpu() for k, v in flow.state_dict().items()})
    for r in range(7):
        J = torch.autograd.functional.jacobian(lambda v: f64(v.unsqueeze(0)).out[0], z[r].cpu().double())
        bound = C["z0"] * base["z0"][r] + J.abs() @ (C["x_inv"] * base["x_inv"][r])
        ratio = float(((back[r].double() - u[r].cpu().double()).abs() / bound).max())
        note(f"roundtrip_{kind}", ratio, f"row {r}")
        assert ratio <= 1.0, f"row {r}: flow.forward(z) misses u by {ratio:.3g}x the bound"


# ---- the samplers end to end -------------------------------------------------------------------------------------------------------------
def mvae(seed=0):
    from multivae_amd.models import MVAE, MVAEConfig

    torch.manual_seed(seed)
    return MVAE(MVAEConfig(n_modalities=2, latent_dim=4, input_dims=DIMS))


def dmvae(seed=0):
    from multivae_amd.models import DMVAE, DMVAEConfig

    torch.manual_seed(seed)
    return DMVAE(DMVAEConfig(n_modalities=2, latent_dim=4, input_dims=DIMS, modalities_specific_dim=dict(a=2, b=3)))


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "module"])
@pytest.mark.parametrize("private", [False, True], ids=["mvae", "dmvae"])
@pytest.mark.parametrize("kind", KINDS)
def test_end_to_end(kind, private, fused, tmp_path):
    from multivae_amd.metrics.base import Evaluator, EvaluatorConfig

    Sampler, Config, Flow, _ = classes(kind)
    model = dmvae() if private else mvae()
    config = Config(n_made_blocks=2, n_hidden_in_made=1, hidden_size=8)
    sampler = Sampler(model, config)
    with pytest.raises(ArithmeticError, match="needs to be fitted"):
        sampler.sample(3)
    assert sampler.flows_dims == (dict(shared=4, a=2, b=3) if private else dict(shared=4))
    sampler.fit(two_modalities(70), eval_data=two_modalities(30, seed=1), training_config=fit_config(), fused=fused)
    assert sampler.is_fitted
    for key, flow in sampler.flows_models.items():
        h = sampler.fit_history[key]
        assert h["fused"] is fused and len(h["train_loss"]) == len(h["eval_loss"]) == 2
        assert all(p.is_cuda for p in flow.parameters())
    out = sampler.sample(7, batch_size=3, generator=torch.Generator(device=D0).manual_seed(3))
    assert out.z.shape == (7, 4) and out.z.is_cuda and out.one_latent_space == (not private) and bool(torch.isfinite(out.z).all())
    if private:
        assert set(out.keys()) == {"z", "one_latent_space", "modalities_z"}
        assert out.modalities_z["a"].shape == (7, 2) and out.modalities_z["b"].shape == (7, 3)
        assert all(bool(torch.isfinite(v).all()) for v in out.modalities_z.values())
    else:
        assert set(out.keys()) == {"z", "one_latent_space"}
    rec = model.decode(out)
    assert rec["a"].shape == (7, 12) and rec["b"].shape == (7, 2, 5) and all(bool(torch.isfinite(v).all()) for v in rec.values())
    # save -> a new sampler -> load, on the device: identical samples under the same generator
    folder = str(tmp_path / "saved")
    sampler.save(folder)
    assert sorted(os.listdir(folder)) == sorted(["sampler_config.json", *sampler.flows_models])
    again = Sampler(model, config)
    again.load_flows_from_folder(folder)
    assert again.is_fitted and all(type(f) is Flow and next(f.parameters()).is_cuda for f in again.flows_models.values())
    out2 = again.sample(7, batch_size=3, generator=torch.Generator(device=D0).manual_seed(3))
    assert torch.equal(out2.z, out.z)
    if private:
        assert all(torch.equal(out2.modalities_z[m], out.modalities_z[m]) for m in ("a", "b"))
    with pytest.raises(AttributeError, match="Error when trying to load the flows from the folder."):
        Sampler(model, config).load_flows_from_folder(str(tmp_path / "nothing-here"))
    ev = Evaluator(model, two_modalities(6), None, EvaluatorConfig(), sampler=sampler)
    assert ev.sampler is sampler
    ev.finish()


def test_zz_report():
    """Prints what the fused paths showed in this session, as fractions of their bounds."""
    print("HIP_MEASURED", {k: (round(v, 3), n) for k, (v, n) in sorted(MEASURED.items())})
