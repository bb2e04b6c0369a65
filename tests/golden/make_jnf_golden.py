"""Generate the JNF golden vectors (tests/golden/jnf_*.npz, tests/golden/jnf_reference_folder/) by running the REAL reference model.

Run in the build container only (needs the reference checkout; see _reference_import.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_jnf_golden.py

WHAT THESE GOLDENS PIN, AND WHAT THEY DO NOT.  The reference's JNF takes its flows from pythae (`pythae.models.normalizing_flows`),
which is not installed; _reference_import.py fakes that package with empty placeholders.  Before `install()` this script registers
`pythae.models.normalizing_flows`, `.base` and `.maf` in `sys.modules` (consulted before the fake finder) holding THIS PACKAGE'S
OWN `BaseNF`, `MAF` and `MAFConfig` (multivae_amd/models/nn/flows.py; plain torch, they run on the CPU).  So the goldens pin JNF's
LOGIC from the real reference — the two stages, which parameters receive gradients, the loss and metric keys and values, the
on-disk layout — around flows that are this package's.  The flow arithmetic itself is pinned by the definition tests
(tests/test_jnf_host.py: masks, triangular Jacobian, log-determinant against slogdet, inverse o forward; tests/jnf_ref.py restates
it in float64), not by pythae.

For every case of tests/jnf_ref.py (CASE_CONFIGS) the script builds a reference `JNF` with procedural weights (procedural.py;
default MLP encoders / decoders, joint encoder and default flows), runs its forward + backward at the case's epoch while recording
the eps behind the joint posterior's `Normal.rsample` inside jnf_model, replays the draw and checks that the loss is reproduced,
checks tests/jnf_ref.py (float64) against it, and stores the draw [B,L], the loss, every output key and metric, gradient statistics
with sampled entries for the parameters that receive a gradient, and in the configuration the list of the parameters that receive
none.  A stage-two case freezes the joint encoder and the decoders BEFORE the forward pass (`_set_torch_no_grad_on_joint_vae`): the
reference freezes them inside its first stage-two forward, after the joint posterior's sample was taken with autograd on, so in
that one step the joint encoder would still receive a gradient through the sample; every later step, and this package always,
runs with the joint model frozen.  The folder is what the reference's `model.save` writes for a tiny model whose parameters were
overwritten with a periodic pattern (the `mask` buffers keep their values), model.pt xz-packed.  Fixtures hold arrays and JSON
only."""
import sys

sys.dont_write_bytecode = True
import lzma
import os
import shutil
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import numpy as np
import torch

import _reference_import as R
from multivae_amd.models.nn import flows as own_flows


def _register_flows():
    pkg = types.ModuleType("pythae.models.normalizing_flows")
    pkg.__path__ = []
    base = types.ModuleType("pythae.models.normalizing_flows.base")
    maf = types.ModuleType("pythae.models.normalizing_flows.maf")
    for mod in (pkg, base):
        mod.BaseNF = own_flows.BaseNF
    for mod in (pkg, maf):
        mod.MAF, mod.MAFConfig = own_flows.MAF, own_flows.MAFConfig
    pkg.base, pkg.maf = base, maf
    for mod in (pkg, base, maf):
        sys.modules[mod.__name__] = mod


_register_flows()
R.install()
from multivae.data.datasets.base import MultimodalBaseDataset
from multivae.models import JNF, JNFConfig
from multivae.models.jnf import jnf_model as ref_jnf

import jnf_ref
from make_golden import grad_stats, save, t

torch.set_num_threads(4)
assert ref_jnf.MAF is own_flows.MAF and ref_jnf.BaseNF is own_flows.BaseNF


class Draw:
    """Wraps `torch.distributions.Normal.rsample` inside jnf_model (its `dist` name): records the eps behind every call
    (replay=None) or serves the recorded ones.  `log_prob` and everything else is torch's."""

    def __init__(self, replay=None):
        self.eps, self.replay = [], replay

    def __enter__(self):
        self.saved = ref_jnf.dist
        rec = self

        class Normal(torch.distributions.Normal):
            def rsample(self, sample_shape=torch.Size()):
                assert tuple(sample_shape) == ()
                eps = torch.randn_like(self.loc).detach().clone() if rec.replay is None else rec.replay.eps[len(rec.eps)]
                rec.eps.append(eps)
                return self.loc + self.scale * eps

        ref_jnf.dist = types.SimpleNamespace(Normal=Normal)
        return self

    def __exit__(self, *exc):
        ref_jnf.dist = self.saved
        return False


def pattern_(t, i):
    """Overwrite `t` in place with values of period 127, shifted by the tensor's index `i` (make_checkpoint_golden.py)."""
    v = ((torch.arange(t.numel(), dtype=torch.float64) + 13 * i) % 127) / 32 - 2 + i / 4096
    t.copy_(v.reshape(t.shape).to(t.dtype))


def build(cfg):
    model = JNF(JNFConfig(**jnf_ref.config_kwargs(cfg)))
    sd = jnf_ref.case_state_dict(cfg)
    assert [(k, tuple(v.shape)) for k, v in model.named_parameters()] == [(k, tuple(v.shape)) for k, v in sd.items()]
    res = model.load_state_dict({k: t(v) for k, v in sd.items()}, strict=False)
    assert not res.unexpected_keys and all(k.endswith(".mask") for k in res.missing_keys), res
    if cfg["epoch"] > cfg["warmup"]:
        model._set_torch_no_grad_on_joint_vae()  # see the module docstring
    return model


def jnf_case(name):
    print(name)
    cfg = dict(jnf_ref.CASE_CONFIGS[name], model="JNF")
    dims, data = jnf_ref.case_inputs(cfg)
    model = build(cfg)
    inputs = MultimodalBaseDataset(data={m: t(v) for m, v in data.items()})
    model.train()
    torch.manual_seed(cfg["seed"])
    with Draw() as rec:
        out = model(inputs, epoch=cfg["epoch"])
    model.zero_grad()
    out.loss.backward()
    stage2 = cfg["epoch"] > cfg["warmup"]
    assert len(rec.eps) == 1
    with Draw(replay=rec):
        out2 = build(cfg).train()(inputs, epoch=cfg["epoch"])
    assert float(out2.loss) == float(out.loss), (float(out2.loss), float(out.loss))
    assert list(out.keys()) == ["loss", "loss_sum", "metrics"] and list(out.metrics.keys()) == ["kld_prior", "recon_loss", "ljm"]
    got = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    cfg["nograd"] = [k for k, p in model.named_parameters() if p.grad is None]
    cfg["frozen"] = [k for k, p in model.named_parameters() if not p.requires_grad]
    if stage2:
        assert all(k.startswith(("encoders.", "flows.")) for k in got) and cfg["frozen"] == cfg["nograd"]
        assert all(k.startswith(("joint_encoder.", "decoders.")) for k in cfg["frozen"])
    else:
        # the unimodal encoders and the flows do not run; the joint encoder reads its copies' means only
        assert all(k.startswith(("encoders.", "flows.")) or ".log_var." in k for k in cfg["nograd"]) and not cfg["frozen"]
        assert all(k in cfg["nograd"] for k, _ in model.named_parameters() if k.startswith(("encoders.", "flows.")))
    arrays = dict(eps=rec.eps[0].numpy())
    for k in out.keys():
        if k != "metrics":
            arrays[k] = np.float64(float(out[k]))
    for k, v in out.metrics.items():
        arrays["metric/" + k] = np.float64(float(v))
    arrays.update(grad_stats(got))
    # float64 formulas at the recorded draw
    ref, g64 = jnf_ref.reference_grads(cfg, arrays)
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
    cfg = jnf_ref.FOLDER_CONFIG
    dims = jnf_ref.case_dims(cfg)
    torch.manual_seed(0)
    model = JNF(JNFConfig(n_modalities=len(dims), latent_dim=cfg["L"], input_dims=dict(dims), warmup=cfg["warmup"],
                          beta=cfg["beta"]))
    with torch.no_grad():
        for i, p in enumerate(model.parameters()):
            pattern_(p, i)
    dst = os.path.join(HERE, jnf_ref.FOLDER)
    shutil.rmtree(dst, ignore_errors=True)
    os.makedirs(dst)
    with tempfile.TemporaryDirectory() as tmp:
        model.save(tmp)
        assert sorted(os.listdir(tmp)) == ["environment.json", "model.pt", "model_config.json"]
        with open(os.path.join(tmp, "model.pt"), "rb") as fi, lzma.open(os.path.join(dst, "model.pt.xz"), "wb", preset=9) as fo:
            fo.write(fi.read())
        shutil.copy(os.path.join(tmp, "model_config.json"), os.path.join(dst, "model_config.json"))
    print("  wrote", jnf_ref.FOLDER, {f: os.path.getsize(os.path.join(dst, f)) for f in sorted(os.listdir(dst))})


def main():
    for name in jnf_ref.JNF_CASES:
        jnf_case(name)
    reference_folder()


if __name__ == "__main__":
    main()
