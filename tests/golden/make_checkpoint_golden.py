"""Fixtures for the on-disk checkpoint compatibility test (tests/test_host_logic.py): folders written by the REAL reference.

Needs the reference's sources (located by _reference_import.py):  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_checkpoint_golden.py

Writes tests/golden/checkpoint_compat/:
  <Model>/                     what the reference's `model.save` writes for the checkpoint_compat.py cases (MoPoE, MVTCAE,
                               MMVAE, MMVAE+, JMVAE; default architectures): model_config.json, environment.json, model.pt.xz
  trainer_checkpoint_epoch_2/  what the reference's BaseTrainer.save_checkpoint writes after 2 CPU epochs of MVTCAE (the
                               checkpoint_compat.py trainer case): the JSON files, model.pt.xz, optimizer.pt.xz
  cases.json                   the configuration arguments of every case and the file names the reference wrote
model.pt / optimizer.pt are torch.save files of tensors and plain containers only (they load with weights_only=True), xz-packed.
Before saving, every parameter and Adam moment is overwritten in place with a per-tensor periodic pattern (distinct for every
tensor, so a mix-up of two same-shaped tensors shows) that packs to a few KB; the default MLPs would otherwise make 4-20 MB
files of random bits.  The optimizer's step counts, hyper-parameters and the model configurations are the reference's own.
"""
import sys

sys.dont_write_bytecode = True
import json
import lzma
import os
import shutil
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import torch

from checkpoint_compat import CASES, DIMS, ref  # installs the reference (R.install()) on import

OUT = os.path.join(HERE, "checkpoint_compat")


def pattern_(t, i):
    """Overwrite `t` in place with values of period 127, shifted by the tensor's index `i`."""
    n = t.numel()
    v = ((torch.arange(n, dtype=torch.float64) + 13 * i) % 127) / 32 - 2 + i / 4096
    t.copy_(v.reshape(t.shape).to(t.dtype))


def copy_folder(src, dst, packed=("model.pt", "optimizer.pt")):
    os.makedirs(dst)
    names = sorted(os.listdir(src))
    for f in names:
        if f in packed:
            with open(os.path.join(src, f), "rb") as fi, lzma.open(os.path.join(dst, f + ".xz"), "wb", preset=9) as fo:
                fo.write(fi.read())
        else:
            shutil.copy(os.path.join(src, f), os.path.join(dst, f))
    return names


def trainer_checkpoint(tmp):
    from multivae.data.datasets.base import MultimodalBaseDataset
    from multivae.trainers import BaseTrainer as RefTrainer
    from multivae.trainers import BaseTrainerConfig as RefTrainerConfig

    dims = dict(mod1=(2,), mod2=(3,))
    torch.manual_seed(0)
    data = MultimodalBaseDataset(data={m: torch.rand(24, *d) for m, d in dims.items()}, labels=torch.zeros(24))
    model = ref.MVTCAE(ref.MVTCAEConfig(n_modalities=2, latent_dim=4, input_dims=dict(dims)))
    cwd = os.getcwd()
    os.chdir(tmp)  # a relative output_dir: no absolute path in training_config.json
    try:
        cfg = RefTrainerConfig(output_dir="training_out", num_epochs=2, steps_saving=2, per_device_train_batch_size=8,
                               learning_rate=1e-3, no_cuda=True, optimizer_params=dict(betas=(0.8, 0.95)))
        trainer = RefTrainer(model, data, training_config=cfg)
        trainer.train()
        with torch.no_grad():
            for i, p in enumerate(trainer._best_model.parameters()):
                pattern_(p, i)
            for i, p in enumerate(trainer.optimizer.param_groups[0]["params"]):
                st = trainer.optimizer.state[p]
                pattern_(st["exp_avg"], 1000 + 2 * i)
                pattern_(st["exp_avg_sq"], 1001 + 2 * i)
                st["exp_avg_sq"].abs_()
        trainer.save_checkpoint(trainer._best_model, "saved", epoch=2)
        return copy_folder(os.path.join(tmp, "saved", "checkpoint_epoch_2"), os.path.join(OUT, "trainer_checkpoint_epoch_2"))
    finally:
        os.chdir(cwd)


def main():
    shutil.rmtree(OUT, ignore_errors=True)
    files, common = {}, dict(n_modalities=4, latent_dim=5, input_dims=dict(DIMS))
    for name, kw in CASES.items():
        torch.manual_seed(1)
        m = getattr(ref, name)(getattr(ref, name + "Config")(**common, **kw))
        with torch.no_grad():
            for i, p in enumerate(m.state_dict().values()):
                pattern_(p, i)
        with tempfile.TemporaryDirectory() as d:
            m.save(d)
            files[name] = copy_folder(d, os.path.join(OUT, name))
        print(name, files[name])
    with tempfile.TemporaryDirectory() as d:
        files["trainer_checkpoint_epoch_2"] = trainer_checkpoint(d)
    print("trainer_checkpoint_epoch_2", files["trainer_checkpoint_epoch_2"])
    with open(os.path.join(OUT, "cases.json"), "w") as f:
        json.dump(dict(common=common, cases=CASES, files=files), f, indent=1)


if __name__ == "__main__":
    main()
