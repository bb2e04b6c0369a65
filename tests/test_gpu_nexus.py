"""Nexus on the GPU: the public model against the goldens recorded from the reference and against the float64 reference of
tests/nexus_ref.py (every gradient), the two new kernels against float64, the statistics of the device-drawn forced
perceptual dropout, bit-reproducibility, graph replay and the trainer."""
import math
import os

import numpy as np
import pytest
import torch

import golden_cases as G
import nexus_ref as NR

pytestmark = pytest.mark.gpu
D = torch.device("cuda:0")


def _model(cfg):
    from multivae_amd.models import Nexus, NexusConfig

    dims = NR.case_dims(cfg)
    model = Nexus(NexusConfig(n_modalities=len(cfg["names"]), latent_dim=cfg["L"], input_dims=dict(dims),
                              modalities_specific_dim=dict(cfg["S"]), bottom_betas=cfg["bottom_betas"], gammas=cfg["gammas"],
                              dropout_rate=cfg["dropout_rate"], msg_dim=cfg["msg_dim"], top_beta=cfg["top_beta"],
                              warmup=cfg["warmup"], adapt_top_decoder_variance=cfg["adapt"],
                              uses_likelihood_rescaling=cfg["rescaling"], decoders_dist=cfg["dists"]))
    model.load_state_dict({k: G.t(v) for k, v in NR.case_state_dict(cfg).items()})
    return model.to(D).train()


def _inputs(cfg, with_masks=True):
    from multivae_amd.data.datasets.base import DatasetOutput

    _, data, masks = NR.case_inputs(cfg)
    out = dict(data={m: G.t(v).to(D) for m, v in data.items()})
    if masks is not None and with_masks:
        out["masks"] = {m: G.t(v).to(D) for m, v in masks.items()}
    return DatasetOutput(**out)


def _draws(cfg, a):
    noise = {"bottom": {m: G.t(a["eps/" + m]).to(D) for m in cfg["names"]}, "joint": G.t(a["eps_joint"]).to(D)}
    return noise, G.t(a["keep"]).to(D)


@pytest.mark.parametrize("case", NR.NEXUS_CASES)
def test_golden(case):
    cfg, a = G.load_case(case)
    model = _model(cfg)
    noise, keep = _draws(cfg, a)
    model.zero_grad(set_to_none=True)
    out = model(_inputs(cfg), epoch=cfg["epoch"], noise=noise, keep=keep)
    out.loss.backward()
    assert abs(float(out.loss) - float(a["loss"])) <= 1e-4 * abs(float(a["loss"]))
    assert abs(float(out.loss_sum) - float(a["loss_sum"])) <= 1e-4 * abs(float(a["loss_sum"]))
    names = {k[len("metric/"):] for k in a if k.startswith("metric/")}
    assert names == set(out.metrics)
    assert isinstance(out.metrics["annealing"], float)
    for k in names:
        ref = float(a["metric/" + k])
        assert abs(float(out.metrics[k]) - ref) <= 1e-4 * max(1.0, abs(ref)), (k, float(out.metrics[k]), ref)
    assert torch.equal(out.keep.cpu(), G.t(a["keep"]))
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in model.named_parameters()}
    _, g64 = NR.reference_grads(cfg, a)
    for k, g in g64.items():
        err = float((grads[k].double().cpu() - g).abs().max())
        assert err <= 1e-4 * float(g.abs().max()) + 1e-9, (k, err, float(g.abs().max()))
    G.check_grads(a, grads, rtol=1e-4)
    model.eval()
    with torch.no_grad():
        enc = model.encode(_inputs(cfg, with_masks=False), return_mean=True)
        assert torch.allclose(enc.z.cpu(), G.t(a["encode/z"]), rtol=1e-4, atol=1e-5)
        for m in cfg["names"]:
            assert torch.allclose(enc.modalities_z[m].cpu(), G.t(a["encode/z_" + m]), rtol=1e-4, atol=1e-5)
        for flag in (True, False):
            dec = model.decode(enc, use_bottom_z_for_recon=flag)
            for m in cfg["names"]:
                assert torch.allclose(dec[m].cpu(), G.t(a[f"decode/{int(flag)}/{m}"]), rtol=1e-4, atol=1e-5), (m, flag)


def test_top_level_gradient_does_not_reach_the_bottom_encoders():
    """z_m enters the top level detached: the bottom encoders' gradients do not change when every top-level term is weighted
    by 0 (gammas and top_beta)."""
    cfg, a = G.load_case("nexus_tiny_complete")
    noise, keep = _draws(cfg, a)
    res = []
    for gammas, top_beta in ((cfg["gammas"], cfg["top_beta"]), ({m: 0.0 for m in cfg["names"]}, 0.0)):
        c = dict(cfg, gammas=gammas, top_beta=top_beta)
        model = _model(c)
        out = model(_inputs(c), epoch=c["epoch"], noise=noise, keep=keep)
        out.loss.backward()
        res.append({k: p.grad.detach().clone() for k, p in model.named_parameters() if k.startswith("encoders.")})
    for k in res[0]:
        assert torch.allclose(res[0][k], res[1][k], rtol=1e-5, atol=1e-7), k


# -- the new kernels against float64 ---------------------------------------------------------------------------------------
def test_aggregate_kernel_forward_backward():
    from multivae_amd import kernels

    g = torch.Generator().manual_seed(3)
    B, M, Dm = 37, 3, 70
    msgs = [torch.randn(B, Dm, generator=g).to(D).requires_grad_(True) for _ in range(M)]
    keep = (torch.rand(B, M, generator=g) > 0.4).float()
    keep[0] = 0.0  # a row with nothing kept: zero message, zero gradient
    keep[1] = torch.tensor([0.0, 1.0, 0.0])
    agg, used = kernels.NexusAggregateFn.apply(None, keep.to(D), None, 0.0, *msgs)
    assert torch.equal(used.cpu(), keep)
    m64 = torch.stack([t.detach().double().cpu() for t in msgs], 1)  # [B, M, D]
    cnt = keep.double().sum(1, keepdim=True)
    ref = (m64 * keep.double()[:, :, None]).sum(1) / cnt.clamp_min(1)
    assert torch.allclose(agg.detach().double().cpu(), ref, rtol=1e-6, atol=1e-6)
    gout = torch.randn(B, Dm, generator=g)
    grads = torch.autograd.grad(agg, msgs, gout.to(D))
    for i in range(M):
        want = keep[:, i:i + 1].double() / cnt.clamp_min(1) * gout.double()
        got = grads[i].double().cpu()
        assert torch.allclose(got, want, rtol=1e-6, atol=1e-7)
        assert (got[keep[:, i] == 0] == 0).all()
    # the dataset masks give the same keep set and the same mean
    masks = [keep[:, i].bool().to(D) for i in range(M)]
    agg2, used2 = kernels.NexusAggregateFn.apply(masks, None, None, 0.0, *[t.detach() for t in msgs])
    assert torch.equal(used2, used) and torch.equal(agg2, agg.detach())


@pytest.mark.parametrize("adapt", [False, True])
def test_top_nll_kernel_against_float64_autograd(adapt):
    from multivae_amd import kernels

    g = torch.Generator().manual_seed(7)
    B, dims, gammas = 300, (5, 70, 3), (0.5, 2.0, 1.3)
    ad = [adapt, adapt, False]
    zs = [torch.randn(B, d, generator=g) for d in dims]
    rs = [(z + 0.3 * torch.randn(z.shape, generator=g)) for z in zs]
    masks = [torch.rand(B, generator=g) > 0.3 for _ in dims]
    w = torch.randn(len(dims), B, generator=g)
    rg = [r.to(D).requires_grad_(True) for r in rs]
    rows, s2 = kernels.NexusTopNLLFn.apply([m.to(D) for m in masks], list(gammas), ad, *[z.to(D) for z in zs], *rg)
    (rows * w.to(D)).sum().backward()
    r64 = [r.double().requires_grad_(True) for r in rs]
    ref_rows = []
    for i, d in enumerate(dims):
        e2 = (zs[i].double() - r64[i]) ** 2
        v = e2.mean() if ad[i] else torch.tensor(1.0, dtype=torch.float64)
        ref_rows.append(gammas[i] * masks[i].double() * (e2.sum(1) / (2 * v) + 0.5 * d * torch.log(v) + 0.5 * d * math.log(2 * math.pi)))
        assert abs(float(s2[i]) - float(v)) <= 1e-5 * float(v)
    ref_rows = torch.stack(ref_rows)
    (ref_rows * w.double()).sum().backward()
    assert torch.allclose(rows.detach().double().cpu(), ref_rows.detach(), rtol=1e-5, atol=1e-5)
    for i in range(len(dims)):
        got, want = rg[i].grad.double().cpu(), r64[i].grad
        assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max()), (i, adapt)


def test_top_nll_is_bit_reproducible():
    from multivae_amd import kernels

    g = torch.Generator().manual_seed(8)
    B = 4099
    z = torch.randn(B, 33, generator=g).to(D)
    r0 = (z + torch.randn(B, 33, generator=g).to(D))
    outs = []
    for _ in range(2):
        r = r0.clone().requires_grad_(True)
        rows, _ = kernels.NexusTopNLLFn.apply(None, [1.5], [True], z, r)
        rows.sum().backward()
        outs.append((rows.detach().clone(), r.grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# -- forced perceptual dropout drawn on the device -------------------------------------------------------------------------
@pytest.mark.parametrize("M", [2, 3, 5])
@pytest.mark.parametrize("p", [0.0, 0.3, 1.0])
def test_device_dropout_statistics(M, p):
    from multivae_amd import kernels

    B = 65536
    msgs = [torch.randn(B, 4, device=D) for _ in range(M)]

    def draw():
        u = kernels.device_randn((B, M + 1), D, uniform=True, lo=0.0, hi=1.0)
        return kernels.NexusAggregateFn.apply(None, None, u, p, *msgs)[1]

    keep = draw()
    assert ((keep == 0) | (keep == 1)).all()
    k = keep.sum(1)
    dropped = k < M
    frac = float(dropped.double().mean())
    assert abs(frac - p) <= 5 * math.sqrt(p * (1 - p) / B) + 1e-12, (frac, p)
    if p == 0:
        assert bool((k == M).all())
        return
    n = int(dropped.sum())
    sizes = k[dropped].long().cpu()
    assert int(sizes.min()) >= 1 and int(sizes.max()) <= M - 1
    q = 1.0 / (M - 1)
    for s in range(1, M):
        c = int((sizes == s).sum())
        assert abs(c - n * q) <= 5 * math.sqrt(n * q * (1 - q)) + 1e-9, (s, c, n * q)
    # each modality is kept equally often among the dropped rows: P(kept) = E[size] / M = 1 / 2
    per = keep[dropped].double().mean(0).cpu()
    assert (per - 0.5).abs().max() <= 5 * math.sqrt(0.25 / n), per
    assert not torch.equal(draw(), keep)  # two consecutive draws differ


# -- reproducibility, graph replay, trainer --------------------------------------------------------------------------------
def _synthetic(B=256, dropout=0.5, adapt=("mod2",), seed=0):
    from multivae_amd.data.datasets.base import DatasetOutput
    from multivae_amd.models import Nexus, NexusConfig

    torch.manual_seed(seed)
    dims = dict(mod1=(6,), mod2=(2, 5), mod3=(7,))
    model = Nexus(NexusConfig(n_modalities=3, latent_dim=5, input_dims=dims, modalities_specific_dim=dict(mod1=3, mod2=4, mod3=2),
                              dropout_rate=dropout, adapt_top_decoder_variance=list(adapt), warmup=4,
                              gammas=dict(mod1=1.0, mod2=2.0, mod3=0.5))).to(D).train()
    inputs = DatasetOutput(data={m: torch.rand(B, *d).to(D) for m, d in dims.items()})
    return model, inputs


def test_same_rng_state_gives_bit_identical_steps():
    model, inputs = _synthetic()
    res = []
    for _ in range(2):
        torch.cuda.manual_seed(123)
        model.zero_grad(set_to_none=True)
        out = model(inputs, epoch=2)
        out.loss.backward()
        res.append((out.loss.detach().clone(), out.keep.clone(), [p.grad.clone() for p in model.parameters()]))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert all(torch.equal(a, b) for a, b in zip(res[0][2], res[1][2]))
    assert 0 < float((res[0][1].sum(1) < 3).double().mean()) < 1


def test_graph_replay_equals_eager_and_draws_fresh_subsets():
    from multivae_amd import kernels
    from multivae_amd.trainers import FlatParams, GraphedStep

    model, inputs = _synthetic()
    flat = FlatParams(model)
    torch.cuda.manual_seed(5)
    flat.zero_grad()
    out = model(inputs, epoch=2)
    out.loss.backward(gradient=kernels.unit_seed(out.loss))
    eager = (out.loss.detach().clone(), out.keep.clone(), flat.grad.clone())
    gs = GraphedStep(model, flat, inputs, epoch=2)
    torch.cuda.manual_seed(5)
    kernels._rng_state(D)  # re-seed the device generator in place: the captured draws start where the eager step's did
    o = gs(inputs)
    torch.cuda.synchronize()
    assert torch.equal(o.loss.detach(), eager[0]) and torch.equal(o.keep, eager[1])
    assert torch.allclose(flat.grad, eager[2], rtol=1e-5, atol=1e-6 * float(eager[2].abs().max()))
    keep1 = o.keep.clone()
    o2 = gs(inputs)
    torch.cuda.synchronize()
    assert not torch.equal(o2.keep, keep1)
    assert math.isfinite(float(o2.loss))


def test_annealing_follows_the_epoch():
    model, inputs = _synthetic(dropout=0.0)
    for e in (1, 2, 4, 9):
        assert model(inputs, epoch=e).metrics["annealing"] == min(e / 4, 1.0)


@pytest.mark.parametrize("masked", [False, True])
def test_trainer_two_epochs_and_resume(tmp_path, masked):
    from multivae_amd.data.datasets.base import IncompleteDataset, MultimodalBaseDataset
    from multivae_amd.models import AutoModel, Nexus, NexusConfig
    from multivae_amd.trainers import BaseTrainer, BaseTrainerConfig

    torch.manual_seed(0)
    n = 64 * 3
    data = dict(mnist=torch.rand(n, 1, 28, 28), svhn=torch.rand(n, 3, 32, 32))
    if masked:
        masks = dict(mnist=torch.ones(n, dtype=torch.bool), svhn=torch.rand(n) > 0.3)
        ds = IncompleteDataset(data=data, masks=masks)
    else:
        ds = MultimodalBaseDataset(data=data)

    def make():
        torch.manual_seed(1)
        return Nexus(NexusConfig(n_modalities=2, latent_dim=20, input_dims=dict(mnist=(1, 28, 28), svhn=(3, 32, 32)),
                                 modalities_specific_dim=dict(mnist=16, svhn=20), dropout_rate=0.2, warmup=1,
                                 adapt_top_decoder_variance=["svhn"]))

    def cfg(out, epochs):
        return BaseTrainerConfig(output_dir=str(out), per_device_train_batch_size=64, num_epochs=epochs, learning_rate=1e-3,
                                 steps_saving=1, use_hip_graph=not masked)

    t1 = BaseTrainer(make(), train_dataset=ds, training_config=cfg(tmp_path / "a", 2))
    hist = t1.train()
    losses = [h["train_epoch_loss"] for h in hist]
    assert all(np.isfinite(v) for v in losses) and losses[-1] < losses[0], losses
    ck = os.path.join(t1.training_dir, "checkpoint_epoch_1")
    t2 = BaseTrainer(make(), train_dataset=ds, training_config=cfg(tmp_path / "b", 2), checkpoint=ck)
    hist2 = t2.train()
    assert len(hist2) == 1 and np.isfinite(hist2[0]["train_epoch_loss"])
    back = AutoModel.load_from_folder(os.path.join(t1.training_dir, "final_model"))
    assert type(back) is Nexus
