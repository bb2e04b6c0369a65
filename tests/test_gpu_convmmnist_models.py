"""The PolyMNIST convolutional networks end to end on the plugin surface, without goldens.

Every case builds a model twice: once with the package's EncoderConvMMNIST_* / DecoderConvMMNIST (HIP trunks, csrc/polyconv.hip) and
once with plain-torch twins written here — nn.Sequential modules with the same layers and state-dict keys, which travel the generic
user-architecture path (torch's own convolutions and autograd).  Same weights, same seed (so the same device noise), same batch:
loss, metrics and every parameter gradient agree within 1e-4 relative (gradients: of the tensor's largest magnitude).

Trainer: BaseTrainer runs two epochs of two steps eagerly and with hipGraph replay.  A capture warms up with eager passes that draw
from the device generator, so the two trainer runs see different noise and are compared by their epoch losses; with the noise
SUPPLIED (GraphedStep, as tests/test_gpu_trainer.py does for the SVHN networks) the same two epochs of two steps end in bit-identical
parameters.

Evaluator: CoherenceEvaluator.eval() on a model of the new classes with seeded ClassifierPolyMNIST weights returns the reference's
metric keys: the no-grad fused trunks through a public evaluator.
"""
import types

import numpy as np
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

D = torch.device("cuda:0")
MODS = ("m0", "m1")
DIMS = {m: (3, 28, 28) for m in MODS}
TOL = 1e-4


def _pkg():
    from multivae_amd.models.base.base_utils import ModelOutput
    from multivae_amd.models.nn import mmnist as M
    from multivae_amd.models.nn.base_architectures import BaseDecoder, BaseEncoder

    return M, ModelOutput, BaseEncoder, BaseDecoder


def _trunk():
    return [nn.Conv2d(3, 32, 3, 2, 1), nn.ReLU(), nn.Conv2d(32, 64, 3, 2, 1), nn.ReLU(), nn.Conv2d(64, 128, 3, 2, 1), nn.ReLU()]


def twin_encoder(src):
    """A plain-torch module with the layers and state-dict keys of `src` (an EncoderConvMMNIST_adapted / _multilatents / EncoderConvMMNIST)."""
    M, ModelOutput, BaseEncoder, _ = _pkg()

    class Twin(BaseEncoder):
        def __init__(self):
            super().__init__()
            self.latent_dim, L = src.latent_dim, src.latent_dim
            self.style_dim = getattr(src, "style_dim", 0)
            if isinstance(src, M.EncoderConvMMNIST):
                self.shared_encoder = nn.Sequential(*_trunk(), nn.Flatten(), nn.Linear(2048, L), nn.ReLU())
                self.class_mu, self.class_logvar = nn.Linear(L, L, bias=False), nn.Linear(L, L, bias=False)
                self.trunks = [(self.shared_encoder, self.class_mu, self.class_logvar)]
            else:
                name = "shared_encoder" if isinstance(src, M.EncoderConvMMNIST_adapted) else "encoder_class"
                setattr(self, name, nn.Sequential(*_trunk()))
                self.class_mu, self.class_logvar = nn.Conv2d(128, L, 4, 2, 0), nn.Conv2d(128, L, 4, 2, 0)
                self.trunks = [(getattr(self, name), self.class_mu, self.class_logvar)]
                if self.style_dim > 0 and not isinstance(src, M.EncoderConvMMNIST_adapted):
                    self.encoder_style = nn.Sequential(*_trunk())
                    self.style_mu, self.style_logvar = nn.Conv2d(128, self.style_dim, 4, 2, 0), nn.Conv2d(128, self.style_dim, 4, 2, 0)
                    self.trunks.append((self.encoder_style, self.style_mu, self.style_logvar))

        def forward(self, x):
            out = ModelOutput()
            for (seq, mu, lv), names in zip(self.trunks, (("embedding", "log_covariance"), ("style_embedding", "style_log_covariance"))):
                h = seq(x)
                out[names[0]], out[names[1]] = mu(h).flatten(1), lv(h).flatten(1)
            return out

    tw = Twin()
    tw.load_state_dict(src.state_dict())  # same keys, same shapes
    return tw


def twin_decoder(src):
    M, ModelOutput, _, BaseDecoder = _pkg()

    class Twin(BaseDecoder):
        def __init__(self):
            super().__init__()
            self.latent_dim = src.latent_dim
            self.decoder = nn.Sequential(nn.Linear(src.latent_dim, 2048), nn.ReLU(), nn.Unflatten(1, (128, 4, 4)),
                                         nn.ConvTranspose2d(128, 64, 3, 2, 1), nn.ReLU(),
                                         nn.ConvTranspose2d(64, 32, 3, 2, 1, output_padding=1), nn.ReLU(),
                                         nn.ConvTranspose2d(32, 3, 3, 2, 1, output_padding=1))

        def forward(self, z):
            out = self.decoder(z.reshape(-1, z.shape[-1]))
            return ModelOutput(reconstruction=out.reshape(*z.shape[:-1], 3, 28, 28))

    tw = Twin()
    tw.load_state_dict(src.state_dict())
    return tw


def _ns(L, S=0):
    return types.SimpleNamespace(latent_dim=L, style_dim=S)


def _batch(B, seed=3):
    from multivae_amd.data.datasets.base import DatasetOutput

    g = torch.Generator().manual_seed(seed)
    return DatasetOutput(data={m: torch.rand(B, 3, 28, 28, generator=g).to(D) for m in MODS})


def _models(kind):
    """(model on the package's classes, model on the twins), same weights."""
    from multivae_amd import models as MM

    M = _pkg()[0]
    torch.manual_seed(7)
    lap = dict(decoders_dist={m: "laplace" for m in MODS}, decoder_dist_params={m: dict(scale=0.75) for m in MODS})
    if kind == "mvtcae":
        L = 16
        enc = {m: M.EncoderConvMMNIST_adapted(_ns(L)) for m in MODS}
        dec = {m: M.DecoderConvMMNIST(_ns(L)) for m in MODS}
        mk = lambda e, d: MM.MVTCAE(MM.MVTCAEConfig(n_modalities=2, latent_dim=L, input_dims=DIMS, **lap), e, d)  # noqa: E731
    elif kind == "mmvae":
        L = 8
        enc = {"m0": M.EncoderConvMMNIST_adapted(_ns(L)), "m1": M.EncoderConvMMNIST(_ns(L))}
        dec = {m: M.DecoderConvMMNIST(_ns(L)) for m in MODS}
        mk = lambda e, d: MM.MMVAE(MM.MMVAEConfig(n_modalities=2, latent_dim=L, input_dims=DIMS, K=2, **lap), e, d)  # noqa: E731
    else:
        L, S = 6, 3
        enc = {m: M.EncoderConvMMNIST_multilatents(_ns(L, S)) for m in MODS}
        dec = {m: M.DecoderConvMMNIST(_ns(L + S)) for m in MODS}
        mk = lambda e, d: MM.DMVAE(MM.DMVAEConfig(n_modalities=2, latent_dim=L, input_dims=DIMS,  # noqa: E731
                                                  modalities_specific_dim={m: S for m in MODS}, **lap), e, d)
    hip = mk(enc, dec).to(D).train()
    twin = mk({m: twin_encoder(e) for m, e in enc.items()}, {m: twin_decoder(d) for m, d in dec.items()}).to(D).train()
    twin.load_state_dict(hip.state_dict())  # priors and whatever else the model owns
    return hip, twin


def _step(model, inputs, seed):
    torch.manual_seed(seed)
    torch.cuda.manual_seed(seed)
    model.zero_grad(set_to_none=True)
    out = model(inputs, epoch=2)
    out.loss.backward()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("kind", ["mvtcae", "mmvae", "dmvae"])
def test_model_matches_plain_torch_twins(kind):
    hip, twin = _models(kind)
    inputs = _batch(4)
    o1, o2 = _step(hip, inputs, 11), _step(twin, inputs, 11)
    l1, l2 = float(o1.loss.detach()), float(o2.loss.detach())
    print(f"{kind}: loss {l1:.8g} (HIP trunks) {l2:.8g} (torch twins) rel {abs(l1 - l2) / abs(l2):.2e}")
    assert np.isfinite(l1) and abs(l1 - l2) <= TOL * abs(l2)
    for k, v in o2.metrics.items():
        a, b = float(o1.metrics[k]), float(v)
        assert abs(a - b) <= TOL * max(abs(b), 1e-12), (k, a, b)
    g1 = dict(hip.named_parameters())
    worst, n_grads = 0.0, 0
    for name, p in twin.named_parameters():
        if p.grad is None:
            assert g1[name].grad is None or float(g1[name].grad.abs().max()) == 0.0, name
            continue
        assert g1[name].grad is not None, name
        r = float((g1[name].grad - p.grad).abs().max() / (p.grad.abs().max() + 1e-30))
        worst, n_grads = max(worst, r), n_grads + 1
        assert r <= TOL, (name, r)
    print(f"{kind}: {n_grads} parameter gradients, worst |a - b| / max |b| = {worst:.2e}")
    assert n_grads >= 2 * (6 + 4 + 8)


def _mvtcae(L=8):
    from multivae_amd.models import MVTCAE, MVTCAEConfig

    M = _pkg()[0]
    torch.manual_seed(5)
    cfg = MVTCAEConfig(n_modalities=2, latent_dim=L, input_dims=DIMS, decoders_dist={m: "laplace" for m in MODS},
                       decoder_dist_params={m: dict(scale=0.75) for m in MODS})
    return MVTCAE(cfg, {m: M.EncoderConvMMNIST_adapted(_ns(L)) for m in MODS}, {m: M.DecoderConvMMNIST(_ns(L)) for m in MODS}).to(D).train()


def test_base_trainer_eager_and_graph(tmp_path):
    from multivae_amd.data.datasets.base import MultimodalBaseDataset
    from multivae_amd.trainers import BaseTrainer, BaseTrainerConfig

    res = []
    for use_graph in (False, True):
        torch.manual_seed(0)
        torch.cuda.manual_seed(0)
        g = torch.Generator().manual_seed(1)
        ds = MultimodalBaseDataset(data={m: torch.rand(16, 3, 28, 28, generator=g) for m in MODS})
        cfg = BaseTrainerConfig(output_dir=str(tmp_path / str(use_graph)), per_device_train_batch_size=8, num_epochs=2, learning_rate=1e-3,
                                use_hip_graph=use_graph)
        tr = BaseTrainer(_mvtcae(), train_dataset=ds, training_config=cfg)
        hist = tr.train()
        assert tr.optimizer.step_count == 4
        if use_graph:
            graphs = [x for x in tr._graphs.values() if x is not None]
            assert len(graphs) == 1, tr._graphs  # captured, not fallen back to eager
        res.append([h["train_epoch_loss"] for h in hist])
    eager, graphed = res
    print(f"epoch losses eager {eager} graphed {graphed}")
    assert all(np.isfinite(v) for v in eager + graphed)
    for a, b in zip(eager, graphed):  # same data order and initial weights, different noise stream
        assert abs(a - b) <= 0.05 * abs(a), (eager, graphed)


def test_graph_replay_is_bit_identical_to_eager():
    """Two epochs of two steps with supplied noise: zero_grad + forward + backward replayed from one hipGraph against launches
    enqueued from Python.  Every kernel of the convolutional trunks adds in a fixed order: the final parameters are the same bits."""
    from multivae_amd import kernels, schedule
    from multivae_amd.trainers import FlatParams, FusedAdam, GraphedStep

    B, L = 8, 8
    res = []
    for graphed in (False, True):
        model = _mvtcae(L)
        flat = FlatParams(model)
        opt = FusedAdam(flat, lr=1e-3)
        batches = [_batch(B, seed=20 + i) for i in range(2)]
        g = torch.Generator().manual_seed(3)
        gs = GraphedStep(model, flat, batches[0], noise=torch.zeros(1, B, L, device=D)) if graphed else None
        losses = []
        for _epoch in range(2):
            for inputs in batches:
                eps = torch.randn(1, B, L, generator=g).to(D)
                if gs is not None:
                    out = gs(inputs, eps)
                else:  # the step GraphedStep captures, enqueued from Python
                    flat.zero_grad()
                    with schedule.deferred_reductions(flat):
                        out = model(inputs, noise=eps)
                        out.loss.backward(gradient=kernels.unit_seed(out.loss))
                opt.step()
                losses.append(float(out.loss.detach()))
        torch.cuda.synchronize()
        res.append((losses, flat.dense(flat.flat.detach()).cpu().clone()))
    (l0, p0), (l1, p1) = res
    print(f"losses eager {l0} graphed {l1}")
    assert l0 == l1 and torch.equal(p0, p1), float((p0 - p1).abs().max())


def test_coherence_evaluator_on_the_fused_trunks(monkeypatch):
    from multivae_amd import kernels
    from multivae_amd.data.datasets.base import MultimodalBaseDataset
    from multivae_amd.metrics import ClassifierPolyMNIST, CoherenceEvaluator, CoherenceEvaluatorConfig

    calls = dict(enc=0, dec=0)
    for name, key in (("polyenc_forward", "enc"), ("polydec_forward", "dec")):
        orig = getattr(kernels, name)

        def counted(*a, _o=orig, _k=key):
            calls[_k] += 1
            return _o(*a)

        monkeypatch.setattr(kernels, name, counted)
    g = torch.Generator().manual_seed(11)
    ds = MultimodalBaseDataset(data={m: torch.rand(7, 3, 28, 28, generator=g) for m in MODS}, labels=torch.tensor([0, 1, 3, 9, 1, 0, 3]))
    model = _mvtcae().eval()
    clfs = {}
    for m in MODS:
        torch.manual_seed(20)
        clfs[m] = ClassifierPolyMNIST()
    ev = CoherenceEvaluator(model, clfs, ds, None, CoherenceEvaluatorConfig(batch_size=3, num_classes=10, nb_samples_for_cross=2,
                                                                           nb_samples_for_joint=10))
    torch.manual_seed(0)
    got = ev.eval()
    ev.finish()
    want = {"m0_to_m1", "m1_to_m0", "mean_coherence_1", "std_coherence_1", "joint_coherence_prior"}
    assert want <= set(got.keys()), sorted(got.keys())
    for k in want:
        assert 0.0 <= float(got[k]) <= 1.0, (k, got[k])
    assert calls["enc"] > 0 and calls["dec"] > 0  # the evaluator ran the one-launch trunks
