"""Generate the CVAE golden vectors (tests/golden/cvae_*.npz) by running the REAL reference model.

Run in the build container only (needs the reference checkout; see _reference_import.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_cvae_golden.py

For every case of tests/cvae_ref.py (CASE_CONFIGS) the script builds a reference `CVAE` with procedural weights (procedural.py)
-- the default joint encoder and conditional decoder, and for the cases with a learned prior a MultipleHeadJointEncoder over
the conditioning modalities --, runs its forward + backward while recording the single eps draw of the reparameterisation,
replays that draw into the reference and checks that the loss is reproduced, checks tests/cvae_ref.py (float64) against it,
and stores the draw, the loss, the metrics, gradient statistics with sampled entries, the encode(return_mean=True) / decode
outputs and the state_dict key / shape list.  Fixtures hold arrays and JSON only."""
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
from multivae.data.datasets.base import MultimodalBaseDataset
from multivae.models import CVAE, CVAEConfig
from multivae.models.cvae import cvae_model as ref_cvae
from multivae.models.nn.default_architectures import BaseDictEncoders, MultipleHeadJointEncoder

import cvae_ref
from make_golden import grad_stats, save, t

torch.set_num_threads(4)


class Draw:
    """Wraps the reference's `dist.Normal(...).rsample()`: records the eps behind it (replay=None) or serves a recorded one."""

    def __init__(self, replay=None):
        self.eps, self.replay = [], replay

    def __enter__(self):
        draw, orig = self, ref_cvae.dist
        self.saved = orig

        class _Normal:
            def __init__(self, loc, scale):
                self.loc, self.scale = loc, scale

            def rsample(self, sample_shape=()):
                assert len(sample_shape) == 0
                eps = torch.randn_like(self.loc).detach().clone() if draw.replay is None else draw.replay.eps[len(draw.eps)]
                draw.eps.append(eps)
                return self.loc + self.scale * eps

        class _Dist:
            Normal = _Normal

        ref_cvae.dist = _Dist
        return self

    def __exit__(self, *exc):
        ref_cvae.dist = self.saved
        return False


def cvae_case(name):
    print(name)
    cfg = dict(cvae_ref.CASE_CONFIGS[name], model="CVAE")
    dims, data = cvae_ref.case_inputs(cfg)
    params = {"scale": 1.0} if cfg["dist"] in ("normal", "laplace") else {}
    ccfg = CVAEConfig(conditioning_modalities=list(cfg["cond"]), main_modality=cfg["main"], input_dims=dict(dims),
                      latent_dim=cfg["L"], beta=cfg["beta"], decoder_dist=cfg["dist"], decoder_dist_params=params)
    prior = None
    if cfg["prior"]:
        prior = MultipleHeadJointEncoder(BaseDictEncoders({m: dims[m] for m in cfg["cond"]}, cfg["L"]), args=ccfg)
    model = CVAE(ccfg, prior_network=prior)
    cfg["sd_shapes"] = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    model.load_state_dict({k: t(v) for k, v in cvae_ref.case_state_dict(cfg).items()})
    inputs = MultimodalBaseDataset(data={m: t(v) for m, v in data.items()})
    model.train()
    torch.manual_seed(cfg["seed"])
    with Draw() as rec:
        out = model(inputs)
    model.zero_grad()
    out.loss.backward()
    gref = {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in model.named_parameters()}
    assert len(rec.eps) == 1
    with Draw(replay=rec):
        out2 = model(inputs)
    assert float(out2.loss) == float(out.loss), (float(out2.loss), float(out.loss))
    arrays = dict(loss=out.loss.detach(), eps=rec.eps[0].numpy())
    for k, v in out.metrics.items():
        arrays["metric/" + k] = np.float64(float(v))
    arrays.update(grad_stats(gref))
    # float64 formulas at the recorded draw
    ref, g64 = cvae_ref.reference_grads(cfg, arrays)
    rel = abs(float(ref["loss"]) - float(out.loss)) / abs(float(out.loss))
    worst = max(float((g64[k] - gref[k].double()).abs().max() / (gref[k].double().abs().max() + 1e-12)) for k in gref)
    print(f"  loss {float(out.loss):.8g}  float64 rel {rel:.2e}  worst grad rel-to-max {worst:.2e}")
    assert rel < 1e-5 and worst < 1e-4
    for k in out.metrics:
        assert abs(float(ref["metrics"][k]) - float(out.metrics[k])) <= 1e-5 * max(1.0, abs(float(out.metrics[k]))), k
    # inference helpers: encode(return_mean=True), decode of it
    model.eval()
    with torch.no_grad():
        enc = model.encode(inputs, return_mean=True)
        arrays["encode/z"] = enc.z
        arrays["decode/recon"] = model.decode(enc).reconstruction
    assert torch.allclose(ref["mu"].detach().float(), enc.z, rtol=1e-4, atol=1e-6)
    save(name, cfg, arrays)


def main():
    for name in cvae_ref.CVAE_CASES:
        cvae_case(name)


if __name__ == "__main__":
    main()
