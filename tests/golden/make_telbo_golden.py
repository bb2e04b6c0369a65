"""Generate the TELBO golden vectors (tests/golden/telbo_*.npz, tests/golden/telbo_reference_folder/) by running the REAL reference
model.

Run in the build container only (needs the reference checkout; see _reference_import.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_telbo_golden.py

For every case of tests/telbo_ref.py (CASE_CONFIGS) the script builds a reference `TELBO` with procedural weights (procedural.py;
default MLP encoders / decoders and joint encoder), runs its forward + backward at the case's epoch while recording the eps draws
of `rsample_from_gaussian`, replays the draws into the reference and checks that the loss is reproduced, checks
tests/telbo_ref.py (float64) against it, and stores the draws this package consumes (stage one: the joint draw [B,L]; stage two:
the M unimodal draws [M,B,L] — the reference's joint draw of that stage feeds a decoding it discards), the loss, every output key
and metric, gradient statistics with sampled entries for the parameters that receive a gradient, and in the configuration the
list of the parameters that receive none.  The folder is what the reference's `model.save` writes for a tiny model whose
parameters were overwritten with a periodic pattern (the default joint encoder alone is 1 MB of random bits otherwise), model.pt
xz-packed.  At the end tests/golden/telbo_checkpoint_compat.py runs (folders cross between this package and the live reference).
Fixtures hold arrays and JSON only."""
import sys

sys.dont_write_bytecode = True
import lzma
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
from multivae.data.datasets.base import MultimodalBaseDataset
from multivae.models import TELBO, TELBOConfig
from multivae.models.telbo import telbo_model as ref_telbo

import telbo_ref
from make_golden import grad_stats, save, t

torch.set_num_threads(4)


class Draw:
    """Wraps the reference's `rsample_from_gaussian` inside telbo_model: records the eps behind every call (replay=None) or serves
    the recorded ones."""

    def __init__(self, replay=None):
        self.eps, self.replay = [], replay

    def __enter__(self):
        self.saved = ref_telbo.rsample_from_gaussian

        def rsample(mu, log_var, N=1, return_mean=False, flatten=False):
            assert N == 1 and not return_mean
            eps = torch.randn_like(mu).detach().clone() if self.replay is None else self.replay.eps[len(self.eps)]
            self.eps.append(eps)
            return mu + torch.exp(0.5 * log_var) * eps

        ref_telbo.rsample_from_gaussian = rsample
        return self

    def __exit__(self, *exc):
        ref_telbo.rsample_from_gaussian = self.saved
        return False


def pattern_(t, i):
    """Overwrite `t` in place with values of period 127, shifted by the tensor's index `i` (make_checkpoint_golden.py)."""
    v = ((torch.arange(t.numel(), dtype=torch.float64) + 13 * i) % 127) / 32 - 2 + i / 4096
    t.copy_(v.reshape(t.shape).to(t.dtype))


def build(cfg):
    model = TELBO(TELBOConfig(**telbo_ref.config_kwargs(cfg)))
    sd = telbo_ref.case_state_dict(cfg)
    assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == [(k, tuple(v.shape)) for k, v in sd.items()]
    model.load_state_dict({k: t(v) for k, v in sd.items()})
    return model


def telbo_case(name):
    print(name)
    cfg = dict(telbo_ref.CASE_CONFIGS[name], model="TELBO")
    dims, data = telbo_ref.case_inputs(cfg)
    model = build(cfg)
    inputs = MultimodalBaseDataset(data={m: t(v) for m, v in data.items()})
    model.train()
    torch.manual_seed(cfg["seed"])
    with Draw() as rec:
        out = model(inputs, epoch=cfg["epoch"])
    model.zero_grad()
    out.loss.backward()
    stage2 = cfg["epoch"] > cfg["warmup"]
    assert len(rec.eps) == (1 + len(dims) if stage2 else 1)
    with Draw(replay=rec):
        out2 = build(cfg).train()(inputs, epoch=cfg["epoch"])
    assert float(out2.loss) == float(out.loss), (float(out2.loss), float(out.loss))
    assert list(out.keys()) == (["loss", "loss_sum", "metrics"] if stage2 else ["recon_loss", "KLD", "loss", "metrics"])
    got = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    cfg["nograd"] = [k for k, p in model.named_parameters() if p.grad is None]
    cfg["frozen"] = [k for k, p in model.named_parameters() if not p.requires_grad]
    if stage2:
        assert all(k.startswith("encoders.") for k in got) and cfg["frozen"] == cfg["nograd"], (sorted(got)[:3], cfg["nograd"][:3])
    else:
        # the unimodal encoders do not run; the joint encoder reads its copies' means only (their log_var heads are unused)
        assert all(k.startswith("encoders.") or ".log_var." in k for k in cfg["nograd"]) and not cfg["frozen"]
        assert all(k in cfg["nograd"] for k, _ in model.named_parameters() if k.startswith("encoders."))
    arrays = dict(eps=torch.stack(rec.eps[1:]).numpy() if stage2 else rec.eps[0].numpy())
    for k in out.keys():
        if k != "metrics":
            arrays[k] = np.float64(float(out[k]))
    for k, v in out.metrics.items():
        arrays["metric/" + k] = np.float64(float(v))
    arrays.update(grad_stats(got))
    # float64 formulas at the recorded draw
    ref, g64 = telbo_ref.reference_grads(cfg, arrays)
    rel = abs(float(ref["loss"]) - float(out.loss)) / abs(float(out.loss))
    worst = max(float((g64[k] - got[k].double()).abs().max() / (got[k].double().abs().max() + 1e-12)) for k in got)
    assert sorted(k for k, g in g64.items() if g is None) == sorted(cfg["nograd"])
    print(f"  loss {float(out.loss):.8g}  float64 rel {rel:.2e}  worst grad rel-to-max {worst:.2e}  no gradient: {len(cfg['nograd'])}")
    assert rel < 1e-5 and worst < 1e-4
    for k in out.keys():
        if k != "metrics":
            assert abs(float(ref[k]) - float(out[k])) <= 1e-5 * max(1.0, abs(float(out[k]))), k
    for k in out.metrics:
        assert abs(float(ref["metrics"][k]) - float(out.metrics[k])) <= 1e-5 * max(1.0, abs(float(out.metrics[k]))), k
    save(name, cfg, arrays)


def reference_folder():
    cfg = telbo_ref.FOLDER_CONFIG
    dims = telbo_ref.case_dims(cfg)
    torch.manual_seed(0)
    model = TELBO(TELBOConfig(n_modalities=len(dims), latent_dim=cfg["L"], input_dims=dict(dims), warmup=cfg["warmup"],
                              lambda_factors=dict(m1=0.5, m2=2.0, m3=1.5)))
    with torch.no_grad():
        for i, p in enumerate(model.state_dict().values()):
            pattern_(p, i)
    dst = os.path.join(HERE, telbo_ref.FOLDER)
    shutil.rmtree(dst, ignore_errors=True)
    os.makedirs(dst)
    with tempfile.TemporaryDirectory() as tmp:
        model.save(tmp)
        assert sorted(os.listdir(tmp)) == ["environment.json", "model.pt", "model_config.json"]
        with open(os.path.join(tmp, "model.pt"), "rb") as fi, lzma.open(os.path.join(dst, "model.pt.xz"), "wb", preset=9) as fo:
            fo.write(fi.read())
        shutil.copy(os.path.join(tmp, "model_config.json"), os.path.join(dst, "model_config.json"))
    print("  wrote", telbo_ref.FOLDER, {f: os.path.getsize(os.path.join(dst, f)) for f in sorted(os.listdir(dst))})


def main():
    for name in telbo_ref.TELBO_CASES:
        telbo_case(name)
    reference_folder()
    import telbo_checkpoint_compat

    telbo_checkpoint_compat.main()


if __name__ == "__main__":
    main()
