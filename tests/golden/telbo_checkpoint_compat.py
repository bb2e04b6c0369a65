"""TELBO model folders cross between this package and the REAL reference (the TELBO case of checkpoint_compat.py, which stays
as it is).  Build container only (needs the reference checkout; see _reference_import.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/telbo_checkpoint_compat.py

  1. a folder written by `multivae_amd.models.TELBO.save` is loaded by the reference's `AutoModel.load_from_folder` and must give
     a reference TELBO with the same configuration fields and a bit-identical state_dict;
  2. the folder the reference wrote (tests/golden/telbo_reference_folder, made by make_telbo_golden.py) is loaded by
     `multivae_amd.models.AutoModel.load_from_folder`, same checks against the reference's own reload of it.
Nothing is written into the repository."""
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

import torch

import _reference_import as R

R.install()
import multivae.models as ref
from multivae.models.auto_model import AutoModel as RefAutoModel

import multivae_amd.models as mine
import telbo_ref

FIELDS = ("n_modalities", "latent_dim", "warmup", "lambda_factors", "gamma_factors", "uses_likelihood_rescaling", "decoders_dist",
          "decoder_dist_params", "rescale_factors", "custom_architectures")


def same(a, b, what):
    assert type(a).__name__ == type(b).__name__ == "TELBO", (what, type(a), type(b))
    for f in FIELDS:
        assert getattr(a.model_config, f) == getattr(b.model_config, f), (what, f)
    assert {m: tuple(d) for m, d in a.model_config.input_dims.items()} == {m: tuple(d) for m, d in b.model_config.input_dims.items()}
    assert (a.warmup, a.reset_optimizer_epochs, dict(a.lambda_factors), dict(a.gamma_factors)) == \
        (b.warmup, b.reset_optimizer_epochs, dict(b.lambda_factors), dict(b.gamma_factors)), what
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb), what
    assert all(torch.equal(sa[k].cpu(), sb[k].cpu()) for k in sa), what


def unpack_reference_folder(dst):
    """tests/golden/telbo_reference_folder with model.pt unpacked, as the reference wrote it."""
    src = os.path.join(HERE, telbo_ref.FOLDER)
    os.makedirs(dst, exist_ok=True)
    shutil.copy(os.path.join(src, "model_config.json"), os.path.join(dst, "model_config.json"))
    with lzma.open(os.path.join(src, "model.pt.xz"), "rb") as fi, open(os.path.join(dst, "model.pt"), "wb") as fo:
        fo.write(fi.read())
    return dst


def main():
    cfg = telbo_ref.CASE_CONFIGS["telbo_tiny_stage2_factors"]
    torch.manual_seed(5)
    ours = mine.TELBO(mine.TELBOConfig(**telbo_ref.config_kwargs(cfg)))
    with tempfile.TemporaryDirectory() as tmp:
        ours.save(os.path.join(tmp, "ours"))
        same(RefAutoModel.load_from_folder(os.path.join(tmp, "ours")), ours, "multivae_amd -> reference")
        folder = unpack_reference_folder(os.path.join(tmp, "theirs"))
        same(mine.AutoModel.load_from_folder(folder), ref.TELBO.load_from_folder(folder), "reference -> multivae_amd")
    print("telbo_checkpoint_compat: ok")


if __name__ == "__main__":
    main()
