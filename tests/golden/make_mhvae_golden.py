"""Generate the MHVAE golden vectors (tests/golden/mhvae_*.npz, tests/golden/mhvae_reference_folder/) by running the REAL reference
model.

Run in the build container only (needs the reference checkout; see _reference_import.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_mhvae_golden.py

For every case of tests/mhvae_ref.py (CASE_CONFIGS) the script builds a reference `MHVAE` from the Linear / SiLU / sigmoid blocks of
`mhvae_ref.build_blocks` (instantiated on the reference's base classes) with procedural weights (procedural.py), runs its forward
and backward while recording every draw of the reparameterisation (the reference draws subset-major, level L down to 1 inside a
subset) and every level's z of every subset, replays the draws and checks that the loss is reproduced bit for bit, then reruns
the reference in float64 on the recorded draws.  Stored: the draws re-packed as {"z_l": [S, B, *shape]}, every level's z, the loss,
the metrics, the float64 loss and every float64 parameter gradient, gradient statistics of the fp32 run, and `grad_bound` = 2 x
the largest distance, relative to the tensor's largest entry, that the reference's own fp32 gradients show from its float64 run:
the tolerance of the GPU test.  tests/mhvae_ref.py (float64 literal form, batched and per subset) is checked against the
reference on the way.  The first case is also saved the way the reference saves a model; only `model.pt` and `model_config.json`
are kept (the pickled architectures would carry the reference's program text).  Fixtures hold arrays and JSON only."""
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
from multivae.models import MHVAE, MHVAEConfig
from multivae.models.base import base_utils as ref_utils
from multivae.models.base import ModelOutput
from multivae.models.nn.base_architectures import BaseDecoder, BaseEncoder

import mhvae_ref
from make_golden import grad_stats, save, t

torch.set_num_threads(4)


class Draw:
    """Wraps the reference's `dist.Normal(...).rsample()`: records the eps behind it (replay=None) or serves recorded ones."""

    def __init__(self, replay=None, dtype=torch.float32):
        self.eps, self.replay, self.dtype = [], replay, dtype

    def __enter__(self):
        draw = self
        self.saved = ref_utils.dist

        class _Normal(self.saved.Normal):  # log_prob and the rest stay the reference's
            def rsample(self, sample_shape=()):
                assert len(sample_shape) == 0
                if draw.replay is None:
                    eps = torch.randn_like(self.loc).detach().clone()
                else:
                    eps = draw.replay[len(draw.eps)].to(draw.dtype)
                draw.eps.append(eps)
                return self.loc + self.scale * eps

        class _Dist:
            Normal = _Normal

            def __getattr__(self, item):
                return getattr(draw.saved, item)

        ref_utils.dist = _Dist()
        return self

    def __exit__(self, *exc):
        ref_utils.dist = self.saved
        return False


class Latents:
    """Records the z_dict of every `subset_encode` call of a model."""

    def __init__(self, model):
        self.model, self.z = model, []

    def __enter__(self):
        orig = self.model.subset_encode

        def wrapped(*a, **k):
            z_dict, kl_dict = orig(*a, **k)
            self.z.append({n: v.detach().clone() for n, v in z_dict.items()})
            return z_dict, kl_dict

        self.model.subset_encode = wrapped
        return self

    def __exit__(self, *exc):
        del self.model.subset_encode
        return False


def build(cfg):
    blocks = mhvae_ref.build_blocks(cfg, torch.nn, BaseEncoder, BaseDecoder, ModelOutput)
    return MHVAE(MHVAEConfig(**mhvae_ref.config_kwargs(cfg)), **blocks)


def dataset(data, masks, dtype):
    d = {m: t(v).to(dtype) for m, v in data.items()}
    if masks is None:
        return MultimodalBaseDataset(data=d)
    return IncompleteDataset(data=d, masks={m: t(v) for m, v in masks.items()})


def mhvae_case(name, folder=False):
    print(name)
    cfg = dict(mhvae_ref.CASE_CONFIGS[name], model="MHVAE")
    dims, data, masks = mhvae_ref.case_inputs(cfg)
    model = build(cfg)
    cfg["sd_shapes"] = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    sd = {k: t(v) for k, v in mhvae_ref.case_state_dict(cfg).items()}
    model.load_state_dict(sd)
    model.train()
    inputs = dataset(data, masks, torch.float32)
    torch.manual_seed(cfg["seed"])
    with Draw() as rec, Latents(model) as lat:
        out = model(inputs)
    model.zero_grad()
    out.loss.backward()
    gref = {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in model.named_parameters()}
    with Draw(replay=rec.eps):
        out2 = model(dataset(data, masks, torch.float32))
    assert float(out2.loss.detach()) == float(out.loss.detach())
    noise = mhvae_ref.repack_draws(cfg, [e.numpy() for e in rec.eps])
    arrays = dict(loss=out.loss.detach())
    for k, v in noise.items():
        arrays["noise/" + k] = v
    for k in noise:
        arrays["z/" + k] = np.stack([z[k].numpy() for z in lat.z])
    for k, v in out.metrics.items():
        arrays["metric/" + k] = np.float64(float(v))
    arrays.update(grad_stats(gref))
    # the reference itself in float64 on the recorded draws
    m64 = build(cfg)
    m64.load_state_dict(sd)
    m64 = m64.double().train()
    with Draw(replay=rec.eps, dtype=torch.float64):
        o64 = m64(dataset(data, masks, torch.float64))
    o64.loss.backward()
    g64 = {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in m64.named_parameters()}
    worst = max(float((g64[k] - gref[k].double()).abs().max() / (g64[k].abs().max() + 1e-300)) for k in gref)
    rel = abs(float(o64.loss) - float(out.loss)) / abs(float(o64.loss))
    arrays["loss64"] = np.float64(float(o64.loss))
    arrays["grad_bound"] = np.float64(2.0 * worst)
    for k, g in g64.items():
        arrays["g64/" + k] = g.numpy()
    print(f"  loss {float(out.loss):.8g}  fp32 vs float64: loss rel {rel:.2e}, worst grad rel-to-max {worst:.2e}"
          f"  -> grad_bound {2 * worst:.2e}")
    assert rel < 1e-5
    # tests/mhvae_ref.py in float64, subsets walked and batched, against the reference in float64
    n64 = {k: t(v).double() for k, v in noise.items()}
    d64 = {m: t(v).double() for m, v in data.items()}
    mk = None if masks is None else {m: t(v) for m, v in masks.items()}
    for batched in (False, True):
        m64.zero_grad()
        res = mhvae_ref.mhvae_loss(m64, d64, mk, n64, batched)
        res["loss"].backward()
        assert abs(float(res["loss"]) - float(o64.loss)) <= 1e-12 * abs(float(o64.loss)), (batched, float(res["loss"]))
        for k, p in m64.named_parameters():
            g = p.grad if p.grad is not None else torch.zeros_like(p)
            assert float((g - g64[k]).abs().max()) <= 1e-10 * float(g64[k].abs().max()) + 1e-300, (batched, k)
        for k in out.metrics:
            assert abs(float(res["metrics"][k]) - float(o64.metrics[k])) <= 1e-12 * max(1.0, abs(float(o64.metrics[k]))), k
        for k in noise:
            assert torch.allclose(res["z"][k].float(), t(arrays["z/" + k]), rtol=1e-4, atol=1e-5), k
    save(name, cfg, arrays)
    if folder:
        dst = os.path.join(HERE, "mhvae_reference_folder")
        os.makedirs(dst, exist_ok=True)
        with tempfile.TemporaryDirectory() as tmp:
            model.save(tmp)
            for f in ("model.pt", "model_config.json"):
                shutil.copy(os.path.join(tmp, f), os.path.join(dst, f))
        print("  wrote mhvae_reference_folder/", sorted(os.listdir(dst)))


def main():
    for i, name in enumerate(mhvae_ref.MHVAE_CASES):
        mhvae_case(name, folder=i == 0)


if __name__ == "__main__":
    main()
