"""Generate the Nexus golden vectors (tests/golden/nexus_*.npz) by running the REAL reference model.

Run in the build container only (needs the reference checkout; see _reference_import.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_nexus_golden.py

For every case the script builds a reference `Nexus` with procedural weights (procedural.py), runs its forward + backward
while recording every draw it consumes -- the bottom eps of each modality, the per-row Bernoulli / randint / randperm outcomes of
the forced perceptual dropout (turned into a [B, M] keep matrix) and the joint eps --, replays those draws into the reference
and checks that the loss is reproduced, checks tests/nexus_ref.py (float64) against it, and stores the draws, the loss, the
metrics, gradient statistics with sampled entries, encode(return_mean=True) / decode outputs and the state_dict key / shape
list.  Fixtures hold arrays and JSON only."""
import sys

sys.dont_write_bytecode = True
import os

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import numpy as np
import torch

import _reference_import as R

R.install()
import procedural as P
from multivae.data.datasets.base import IncompleteDataset, MultimodalBaseDataset
from multivae.models import Nexus, NexusConfig
from multivae.models.nexus import nexus_model as ref_nexus

import nexus_ref
from make_golden import grad_stats, save, t

torch.set_num_threads(4)


class Draws:
    """Wraps the reference's draw functions: records them (replay=None) or serves recorded outcomes (replay=Draws)."""

    def __init__(self, replay=None):
        self.eps, self.bern, self.randint, self.randperm = [], [], [], []
        self.replay = replay
        self.pos = dict(eps=0, bern=0, randint=0, randperm=0)

    def _next(self, kind, fresh):
        if self.replay is None:
            v = fresh()
        else:
            v = getattr(self.replay, kind)[self.pos[kind]]
            self.pos[kind] += 1
        getattr(self, kind).append(v)
        return v

    def __enter__(self):
        draws = self
        self.saved = (ref_nexus.rsample_from_gaussian, ref_nexus.dist, ref_nexus.np, torch.randperm)
        orig_rsample, orig_dist, orig_np, orig_randperm = self.saved

        def rsample(mu, log_var, N=1, return_mean=False, flatten=False):
            if return_mean or N != 1:
                return orig_rsample(mu, log_var, N, return_mean, flatten)
            eps = draws._next("eps", lambda: torch.randn_like(mu).detach().clone())
            return mu + torch.exp(0.5 * log_var) * eps

        class _Bern:
            def __init__(self, p):
                self.p = p

            def sample(self):
                return draws._next("bern", lambda: orig_dist.Bernoulli(self.p).sample())

        class _Dist:
            Bernoulli = _Bern
            Normal = orig_dist.Normal

        class _Random:
            @staticmethod
            def randint(lo, hi):
                return draws._next("randint", lambda: orig_np.random.randint(lo, hi))

        class _Np:
            random = _Random

        ref_nexus.rsample_from_gaussian = rsample
        ref_nexus.dist = _Dist
        ref_nexus.np = _Np
        torch.randperm = lambda n, *a, **k: draws._next("randperm", lambda: orig_randperm(n, *a, **k))
        return self

    def __exit__(self, *exc):
        ref_nexus.rsample_from_gaussian, ref_nexus.dist, ref_nexus.np, torch.randperm = self.saved
        return False

    def keep_matrix(self, B, M):
        keep = np.ones((B, M), dtype=np.float32)
        j = 0
        for b in range(B):
            if int(self.bern[b].item()) == 1:
                size, perm = self.randint[j], self.randperm[j]
                keep[b] = 0.0
                keep[b, perm[:size].numpy()] = 1.0
                j += 1
        return keep


def nexus_case(name, *, arch, names, B, S, L, msg_dim, dropout, betas, gammas, top_beta, warmup, epoch, adapt, rescaling,
               masked, seed, dists=None):
    print(name)
    cfg = dict(model="Nexus", arch=arch, names=names, B=B, S=S, L=L, msg_dim=msg_dim, dropout_rate=dropout,
               bottom_betas=betas, gammas=gammas, top_beta=top_beta, warmup=warmup, epoch=epoch, adapt=adapt,
               rescaling=rescaling, masked=masked, seed=seed, dists=dists)
    dims, data, masks = nexus_ref.case_inputs(cfg)
    ncfg = NexusConfig(n_modalities=len(names), latent_dim=L, input_dims=dict(dims), modalities_specific_dim=dict(S),
                       bottom_betas=betas, gammas=gammas, dropout_rate=dropout, msg_dim=msg_dim, top_beta=top_beta,
                       warmup=warmup, adapt_top_decoder_variance=adapt, uses_likelihood_rescaling=rescaling,
                       decoders_dist=dists)
    model = Nexus(ncfg)
    cfg["sd_shapes"] = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    sd_np = nexus_ref.case_state_dict(cfg)
    model.load_state_dict({k: t(v) for k, v in sd_np.items()})
    d = {m: t(v) for m, v in data.items()}
    inputs = MultimodalBaseDataset(data=d) if masks is None else IncompleteDataset(data=d, masks={m: t(v) for m, v in masks.items()})
    model.train()
    torch.manual_seed(seed)
    np.random.seed(seed)
    with Draws() as rec:
        out = model(inputs, epoch=epoch)
    model.zero_grad()
    out.loss.backward()
    gref = {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in model.named_parameters()}
    M = len(names)
    assert len(rec.eps) == M + 1
    keep = rec.keep_matrix(B, M) if masks is None else np.stack([masks[m] for m in names], 1).astype(np.float32)
    with Draws(replay=rec):
        out2 = model(inputs, epoch=epoch)
    assert float(out2.loss) == float(out.loss), (float(out2.loss), float(out.loss))
    eps = {m: rec.eps[i].numpy() for i, m in enumerate(names)}
    arrays = dict(loss=out.loss.detach(), loss_sum=out.loss_sum.detach(), keep=keep, eps_joint=rec.eps[M].numpy())
    for m in names:
        arrays["eps/" + m] = eps[m]
    for k, v in out.metrics.items():
        arrays["metric/" + k] = np.float64(float(v))
    if masks is not None:
        for m, v in masks.items():
            arrays["mask/" + m] = v
    arrays.update(grad_stats(gref))
    # float64 formulas at the recorded draws
    ref, g64 = nexus_ref.reference_grads(cfg, arrays)
    rel = abs(float(ref["loss"]) - float(out.loss)) / abs(float(out.loss))
    worst = max(float((g64[k] - gref[k].double()).abs().max() / (gref[k].double().abs().max() + 1e-12)) for k in gref)
    print(f"  loss {float(out.loss):.8g}  float64 rel {rel:.2e}  worst grad rel-to-max {worst:.2e}  "
          f"dropped rows {int((keep.sum(1) < M).sum())}/{B}")
    assert rel < 1e-5 and worst < 1e-4
    for k in out.metrics:
        assert abs(float(ref["metrics"][k]) - float(out.metrics[k])) <= 1e-5 * max(1.0, abs(float(out.metrics[k]))), k
    # inference helpers: encode(return_mean=True) on every modality, decode through the bottom and the top latents
    model.eval()
    with torch.no_grad():
        enc = model.encode(inputs if masks is None else MultimodalBaseDataset(data=d), return_mean=True)
        arrays["encode/z"] = enc.z
        for m in names:
            arrays["encode/z_" + m] = enc.modalities_z[m]
        for flag in (True, False):
            dec = model.decode(enc, use_bottom_z_for_recon=flag)
            for m in names:
                arrays[f"decode/{int(flag)}/{m}"] = dec[m]
    save(name, cfg, arrays)


TINY_NAMES3 = ["mod1", "mod2", "mod3"]


def main():
    nexus_case("nexus_tiny_complete", arch="tiny", names=TINY_NAMES3, B=8, S=dict(mod1=3, mod2=4, mod3=2), L=5, msg_dim=6,
               dropout=0.5, betas=dict(mod1=0.5, mod2=1.5, mod3=1.0), gammas=dict(mod1=2.0, mod2=0.5, mod3=1.0),
               top_beta=0.7, warmup=10, epoch=3, adapt=["mod2"], rescaling=False, masked=False, seed=2101)
    nexus_case("nexus_tiny_masked", arch="tiny", names=TINY_NAMES3, B=9, S=dict(mod1=3, mod2=4, mod3=2), L=5, msg_dim=6,
               dropout=0.5, betas=dict(mod1=1.0, mod2=2.0, mod3=0.5), gammas=dict(mod1=1.0, mod2=1.5, mod3=0.5),
               top_beta=1.3, warmup=4, epoch=7, adapt=["mod1", "mod3"], rescaling=True, masked=True, seed=2102,
               dists=dict(mod1="normal", mod2="laplace", mod3="bernoulli"))
    nexus_case("nexus_tiny_m4_drop_all", arch="tiny", names=["mod1", "mod2", "mod3", "mod4"], B=12,
               S=dict(mod1=3, mod2=4, mod3=2, mod4=3), L=4, msg_dim=5, dropout=1.0,
               betas=dict(mod1=1.0, mod2=1.0, mod3=1.0, mod4=1.0), gammas=dict(mod1=1.0, mod2=1.0, mod3=1.0, mod4=1.0),
               top_beta=1.0, warmup=20, epoch=1, adapt=["mod4"], rescaling=False, masked=False, seed=2103)
    nexus_case("nexus_mnistsvhn", arch="mnistsvhn", names=["mnist", "svhn"], B=8, S=dict(mnist=16, svhn=20), L=20,
               msg_dim=10, dropout=0.2, betas=dict(mnist=1.0, svhn=1.0), gammas=dict(mnist=1.0, svhn=1.0), top_beta=1.0,
               warmup=20, epoch=2, adapt=["svhn"], rescaling=True, masked=False, seed=2104)


if __name__ == "__main__":
    main()
