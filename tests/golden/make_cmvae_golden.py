"""Generate the CMVAE golden vectors (tests/golden/cmvae_*.npz and tests/golden/cmvae_reference_folder/) by running the REAL
reference model.

Run in the build container only (needs the reference checkout; see _reference_import.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_cmvae_golden.py

Every case of tests/cmvae_ref.py (CASE_CONFIGS) builds a reference `CMVAE` with the default multi-latent MLPs and procedural
weights (cmvae_ref.case_state_dict, loaded with strict=True: the parameter names are the reference's), seeds the global generator,
draws the noise in the reference's own order (forward: u, w, then one private-prior draw per other modality, as `mmvaeplus_case`
of make_golden.py; predict_clusters: one draw per modality; compute_joint_nll: the forward's order per data point), re-seeds and
runs the reference, and stores the draws with the reference's results:
  forward cases     loss, lws, us, ws, masks (float32 run) and, from the reference run again in float64 on the same draws,
                    gradient statistics with sampled entries of every parameter;
  cmvae_predict_prune   predict_clusters(compute_lliks=True) on the whole data set (pc_zs, clusters, norm_lliks) and
                    prune_clusters over two batches (h_values, the final _pc_params and n_clusters, the draws of every pass);
                    no p(c|z) may underflow to 0 there (count_nonzero would hinge on a denormal): asserted;
  cmvae_joint_nll   compute_joint_nll;
  cmvae_reference_folder/   what the reference's `model.save` writes for a CMVAE with default architectures (model_config.json and
                    model.pt only; no pickled networks), its parameters overwritten with a per-tensor pattern;
  and in every .npz the reference's parameter names, shapes and requires_grad flags.
Fixtures hold arrays and JSON only."""
import sys

sys.dont_write_bytecode = True
import os
import shutil
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import numpy as np
import torch

import _reference_import as R

R.install()
from multivae.data.datasets.base import IncompleteDataset, MultimodalBaseDataset
from multivae.models import CMVAE, CMVAEConfig

import cmvae_ref
from make_golden import grad_stats, save, t

torch.set_num_threads(4)


def build(cfg):
    dims, data, masks = cmvae_ref.case_inputs(cfg)
    L = cmvae_ref.case_latent_dim(cfg)
    mcfg = CMVAEConfig(n_modalities=len(dims), latent_dim=L, input_dims=dict(dims), K=cfg["K"], modalities_specific_dim=cfg["S"],
                       prior_and_posterior_dist=cfg["family"], loss=cfg["loss"], beta=cfg["beta"],
                       uses_likelihood_rescaling=cfg["rescaling"], learn_modality_prior=True, number_of_clusters=cfg["C"])
    model = CMVAE(mcfg)
    model.load_state_dict({k: t(v) for k, v in cmvae_ref.case_state_dict(cfg).items()}, strict=True)
    d = {m: t(v) for m, v in data.items()}
    inputs = MultimodalBaseDataset(data=d) if masks is None else IncompleteDataset(data=d, masks={m: t(v) for m, v in masks.items()})
    return model, inputs, L


def draw(family, shape):
    if family == "laplace_with_softmax":
        return torch.empty(shape).uniform_(torch.finfo(torch.float32).eps - 1, 1)
    return torch.randn(shape)


def forward_noise(family, mods, K, B, L, S):
    noise = {}
    for c in mods:
        noise[c] = {"u": draw(family, (K, B, L)), "w": draw(family, (K, B, S))}
        for r in mods:
            if r != c:
                noise[c][r] = draw(family, (K, B, S))
    return noise


def param_record(model):
    return [[k, list(p.shape), bool(p.requires_grad)] for k, p in model.named_parameters()]


class Replay:
    """Serves recorded draws to the reference's `latent_dist(...).rsample([K])` calls, in their order, in the dtype of the
    distribution's parameters: the reference run again on the same noise, in float32 (a check of the recorded order) or in float64."""

    def __init__(self, draws, family):
        self.draws, self.family, self.i = draws, family, 0

    def __enter__(self):
        import torch.distributions as td

        replay = self
        self.saved = (td.Normal.rsample, td.Laplace.rsample)

        def rsample(dist, sample_shape=torch.Size()):
            eps = replay.draws[replay.i].to(dist.loc.dtype)
            replay.i += 1
            assert tuple(eps.shape) == tuple(sample_shape) + tuple(dist.loc.shape)
            if replay.family == "laplace_with_softmax":
                return dist.loc - dist.scale * eps.sign() * torch.log1p(-eps.abs())
            return dist.loc + dist.scale * eps

        td.Normal.rsample = td.Laplace.rsample = rsample
        return self

    def __exit__(self, *exc):
        import torch.distributions as td

        td.Normal.rsample, td.Laplace.rsample = self.saved
        assert exc[0] is not None or self.i == len(self.draws)
        return False


def replayed_grads(cfg, noise, mods, dtype):
    """(loss, {name: gradient}) of the reference run on the recorded draws in `dtype`."""
    model, inputs, _ = build(cfg)
    model = model.to(dtype).train()
    inputs.data = {m: v.to(dtype) for m, v in inputs.data.items()}
    draws = [noise[c][k] for c in mods for k in noise[c]]  # u, w, then the other modalities, per conditioning modality
    with Replay(draws, cfg["family"]):
        out = model(inputs)
    out.loss.backward()
    return out.loss.detach(), {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in model.named_parameters()}


def forward_case(name):
    print(name)
    cfg = dict(cmvae_ref.CASE_CONFIGS[name], model="CMVAE")
    model, inputs, L = build(cfg)
    model.train()
    K, B, S, seed = cfg["K"], cfg["B"], cfg["S"], cfg["seed"]
    mods = [m for m in inputs.data if not hasattr(inputs, "masks") or bool(inputs.masks[m].any())]
    torch.manual_seed(seed)
    noise = forward_noise(cfg["family"], mods, K, B, L, S)
    dreg = cfg["loss"] == "dreg_looser"
    torch.manual_seed(seed)
    post, emb, rec = model._compute_posteriors_and_embeddings(inputs, detach=dreg)
    lws, emb, n_mods = model._compute_k_lws(post, emb, rec, inputs)
    arrays = {}
    for c in mods:
        arrays["lws/" + c] = lws[c].detach().clone()
        arrays["us/" + c] = emb[c]["u"].detach().clone()
        arrays["ws/" + c] = emb[c]["w"].detach().clone()
    out = model._dreg_looser(lws, emb, n_mods) if dreg else model._iwae_looser(lws, n_mods)
    model.zero_grad()
    out.loss.backward()
    gref = {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in model.named_parameters()}
    torch.manual_seed(seed)
    again = model(inputs)
    assert float(again.loss) == float(out.loss), (float(again.loss), float(out.loss))
    print(f"  loss {float(out.loss):.8g}")
    arrays["loss"] = out.loss.detach()
    for c in mods:
        for k, v in noise[c].items():
            arrays[f"noise/{c}/{k}"] = v
    if hasattr(inputs, "masks"):
        for m, v in inputs.masks.items():
            arrays["mask/" + m] = v
    # the same draws replayed: float32 reproduces the run above (the recorded order is the reference's), float64 gives the
    # gradients that are stored: the importance weights are a softmax of log-weights of magnitude 1e2 ... 1e4, so the float32
    # gradients carry the float32 rounding of those (printed below) and would be a poorer yardstick than the bar they are held to
    l32, g32 = replayed_grads(cfg, noise, mods, torch.float32)
    assert abs(float(l32) - float(out.loss)) <= 1e-6 * abs(float(out.loss)), (float(l32), float(out.loss))
    l64, g64 = replayed_grads(cfg, noise, mods, torch.float64)
    assert abs(float(l64) - float(out.loss)) <= 1e-4 * abs(float(out.loss)), (float(l64), float(out.loss))  # the parity bar
    own = max(float((gref[k].double() - g64[k]).abs().max() / (g64[k].abs().max() + 1e-30)) for k in g64)
    print(f"  float64 loss {float(l64):.10g}; the reference's float32 gradients are within {own:.1e} of its float64 ones (of each tensor's largest entry)")
    arrays["loss64"] = l64
    arrays.update(grad_stats(g64))
    cfg.update(L=L, names=list(model.encoders.keys()), params=param_record(model), ref_fp32_grad_distance=own)
    save(name, cfg, arrays)


def predict_prune_case(name="cmvae_predict_prune"):
    print(name)
    cfg = dict(cmvae_ref.CASE_CONFIGS[name], model="CMVAE")
    model, inputs, L = build(cfg)
    model.eval()
    B, bs, seed, C = cfg["B"], cfg["batch_size"], cfg["seed"], cfg["C"]
    mods = list(inputs.data)
    arrays = {}
    torch.manual_seed(seed)
    for m in mods:
        arrays["predict_noise/" + m] = torch.randn(B, L)
    torch.manual_seed(seed)
    pred = model.predict_clusters(inputs, compute_lliks=True)
    arrays["clusters"], arrays["norm_lliks"] = pred.clusters, pred.norm_lliks
    for m in mods:
        assert int(torch.count_nonzero(pred.pc_zs[m])) == pred.pc_zs[m].numel()
        arrays["pc_zs/" + m] = pred.pc_zs[m]
    # prune: passes with C, C - 1, ..., 2 clusters, each over ceil(B / bs) batches, one draw per modality and batch.  The draws
    # are recorded as the reference makes them (its DataLoader takes a number from the same generator at the start of every pass)
    n_batches = (B + bs - 1) // bs
    import torch.distributions as td

    drawn, saved = [], td.Normal.sample

    def sample(dist, sample_shape=torch.Size()):
        assert len(sample_shape) == 0
        eps = torch.randn(dist.loc.shape)
        drawn.append(eps)
        return (dist.loc + dist.scale * eps).detach()

    orig, smallest = model.predict_clusters, [1.0]

    def checked(batch, **kw):
        out = orig(batch, **kw)
        for m, pc in out.pc_zs.items():
            assert int(torch.count_nonzero(pc)) == pc.numel(), "a p(c|z) underflowed to 0"  # pruned clusters (log 1e-20) included
            smallest[0] = min(smallest[0], float(pc.min()))
        return out

    model.predict_clusters = checked
    torch.manual_seed(seed + 1)
    td.Normal.sample = sample
    try:
        h_values = model.prune_clusters(inputs, batch_size=bs)
    finally:
        td.Normal.sample = saved
    assert len(drawn) == (C - 1) * n_batches * len(mods)
    for p in range(C - 1):
        for i in range(n_batches):
            for j, m in enumerate(mods):
                arrays[f"prune_noise/{p}/{i}/{m}"] = drawn[(p * n_batches + i) * len(mods) + j]
    print("  h_values", [float(h) for h in h_values], "n_clusters", int(model.n_clusters), "smallest p(c|z)", smallest[0])
    arrays["h_values"] = np.array([float(h) for h in h_values], dtype=np.float64)
    arrays["pc_params_final"] = model._pc_params.detach()
    arrays["n_clusters_final"] = np.int64(int(model.n_clusters))
    cfg.update(L=L, names=mods, n_passes=C - 1, n_batches=n_batches)
    save(name, cfg, arrays)


def joint_nll_case(name="cmvae_joint_nll"):
    print(name)
    cfg = dict(cmvae_ref.CASE_CONFIGS[name], model="CMVAE")
    model, inputs, L = build(cfg)
    B, S, seed, K = cfg["B"], cfg["S"], cfg["seed"], cfg["nll_K"]
    mods = list(inputs.data)
    k = K // len(mods)
    torch.manual_seed(seed)
    per_point = [forward_noise(cfg["family"], mods, k, 1, L, S) for _ in range(B)]  # the reference walks the data points
    arrays = {}
    for c in mods:
        for key in per_point[0][c]:
            arrays[f"noise/{c}/{key}"] = torch.cat([per_point[i][c][key] for i in range(B)], dim=1)
    torch.manual_seed(seed)
    nll = model.compute_joint_nll(inputs, K=K)
    assert model.model_config.beta == cfg["beta"]
    print(f"  joint nll {float(nll):.8g}")
    arrays["joint_nll"] = nll.detach()
    cfg.update(L=L, names=mods)
    save(name, cfg, arrays)


def reference_folder(name="cmvae_reference_folder"):
    """The reference's `model.save` of a CMVAE with default architectures; parameters overwritten with a per-tensor periodic
    pattern (distinct for every tensor), as make_checkpoint_golden.py does."""
    print(name)
    dims = dict(mod1=(2,), mod2=(3,))
    mcfg = CMVAEConfig(n_modalities=2, latent_dim=5, input_dims=dims, K=2, modalities_specific_dim=3, beta=2.5,
                       number_of_clusters=4, prior_and_posterior_dist="normal", loss="iwae_looser", reconstruction_option="single_prior")
    torch.manual_seed(0)
    model = CMVAE(mcfg)
    with torch.no_grad():
        for i, p in enumerate(model.parameters()):
            n = p.numel()
            v = ((torch.arange(n, dtype=torch.float64) + 13 * i) % 127) / 32 - 2 + i / 4096
            p.copy_(v.reshape(p.shape).to(p.dtype))
    out = os.path.join(HERE, name)
    shutil.rmtree(out, ignore_errors=True)
    os.makedirs(out)
    with tempfile.TemporaryDirectory() as tmp:
        model.save(tmp)
        written = sorted(os.listdir(tmp))
        assert "model.pt" in written and "model_config.json" in written and not [f for f in written if f.endswith(".pkl")], written
        for f in ("model_config.json", "model.pt"):  # model.pt: a torch.save file of tensors in plain containers
            shutil.copy(os.path.join(tmp, f), os.path.join(out, f))
    print("  wrote", sorted(os.listdir(out)), [os.path.getsize(os.path.join(out, f)) for f in sorted(os.listdir(out))])


def main():
    for name in cmvae_ref.CMVAE_CASES:
        forward_case(name)
    predict_prune_case()
    joint_nll_case()
    reference_folder()


if __name__ == "__main__":
    main()
