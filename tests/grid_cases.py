"""What test_grid_host.py and test_gpu_grid.py share: a two-modality plugin model in plain PyTorch (it runs on either device), its
dataset, a callback that records what on_prediction_step hands over, and a recorder of the tensors that the models' predict /
decode return, from which grid_ref rebuilds every picture."""
import numpy as np
import torch

DIMS = dict(a=(1, 5, 7), b=(3, 8, 4))
LATENT = 4


def dataset(n=6, dims=DIMS, seed=5):
    from multivae_amd.data.datasets.base import MultimodalBaseDataset

    g = torch.Generator().manual_seed(seed)
    return MultimodalBaseDataset({m: torch.rand(n, *d, generator=g) for m, d in dims.items()})


def tiny_model(seed=11):
    """A BaseMultiVAE with one linear layer per encoder head and decoder: the posterior of a subset is the mean of its experts."""
    from multivae_amd._output import ModelOutput
    from multivae_amd.models.base.base_ae_model import BaseMultiVAE
    from multivae_amd.models.base.base_config import BaseMultiVAEConfig
    from multivae_amd.models.nn.base_architectures import BaseDecoder, BaseEncoder

    class Enc(BaseEncoder):
        def __init__(self, dim):
            super().__init__()
            self.mu = torch.nn.Linear(int(np.prod(dim)), LATENT)
            self.lv = torch.nn.Linear(int(np.prod(dim)), LATENT)

        def forward(self, x):
            h = x.reshape(x.shape[0], -1)
            return ModelOutput(embedding=self.mu(h), log_covariance=self.lv(h))

    class Dec(BaseDecoder):
        def __init__(self, dim):
            super().__init__()
            self.dim = tuple(dim)
            self.out = torch.nn.Linear(LATENT, int(np.prod(dim)))

        def forward(self, z):
            return ModelOutput(reconstruction=torch.sigmoid(self.out(z)).reshape(z.shape[0], *self.dim))

    class Tiny(BaseMultiVAE):
        def __init__(self):
            torch.manual_seed(seed)
            super().__init__(BaseMultiVAEConfig(n_modalities=2, latent_dim=LATENT, input_dims=dict(DIMS)),
                             {m: Enc(d) for m, d in DIMS.items()}, {m: Dec(d) for m, d in DIMS.items()})
            self.model_name = "Tiny"

        def encode(self, inputs, cond_mod="all", N=1, **kwargs):
            cond_mod = super().encode(inputs, cond_mod, N, **kwargs).cond_mod
            outs = [self.encoders[m](inputs.data[m]) for m in cond_mod]
            mu = torch.stack([o.embedding for o in outs]).mean(0)
            lv = torch.stack([o.log_covariance for o in outs]).mean(0)
            shape = (N,) + tuple(mu.shape) if N > 1 else tuple(mu.shape)
            z = mu + torch.exp(0.5 * lv) * torch.randn(shape, device=mu.device)
            if N > 1 and kwargs.get("flatten", False):
                z = z.reshape(-1, LATENT)
            return ModelOutput(z=z, one_latent_space=True)

        def forward(self, inputs, **kwargs):
            z = self.encode(inputs).z
            s = sum(((self.decoders[m](z).reconstruction - inputs.data[m]) ** 2).sum() for m in self.decoders)
            return ModelOutput(loss=s / z.shape[0], loss_sum=s, metrics={})

    return Tiny()


class Captured:
    """Wraps `cls.predict` and `cls.decode` (on the CLASS: the trainer predicts with a deep copy of the model) and keeps, per call,
    what went in and a CPU copy of every tensor that came out."""

    def __init__(self, monkeypatch, cls):
        self.predicts, self.decodes, self.inside = [], [], 0
        predict, decode, rec = cls.predict, cls.decode, self

        def wrapped_predict(model, inputs, cond_mod="all", *args, **kwargs):
            rec.inside += 1
            try:
                out = predict(model, inputs, cond_mod, *args, **kwargs)
            finally:
                rec.inside -= 1
            rec.predicts.append(dict(cond_mod=cond_mod, data={m: v.detach().cpu().clone() for m, v in inputs.data.items()},
                                     out={m: v.detach().cpu().clone() for m, v in out.items()}))
            return out

        def wrapped_decode(model, *args, **kwargs):
            out = decode(model, *args, **kwargs)
            if not rec.inside:  # a decode of its own (unconditional samples), not the one inside predict
                rec.decodes.append({m: v.detach().cpu().clone() for m, v in out.items()})
            return out

        monkeypatch.setattr(cls, "predict", wrapped_predict)
        monkeypatch.setattr(cls, "decode", wrapped_decode)


def recorder():
    """A TrainingCallback that keeps CPU copies of the images of every on_prediction_step."""
    from multivae_amd.trainers import TrainingCallback

    class Recorder(TrainingCallback):
        def __init__(self):
            self.steps = []

        def on_prediction_step(self, training_config, **kwargs):
            images = kwargs["metrics_media"]["images"]
            self.steps.append(dict(global_step=kwargs["global_step"], devices={k: v.device.type for k, v in images.items()},
                                   images={k: v.detach().cpu().clone() for k, v in images.items()}))

    return Recorder()


def trainer_pictures(calls):
    """The tensors of the pictures of one BaseTrainer.predict, rebuilt from its recorded model.predict calls (one per conditioning
    modality, then the joint one): {key: [true data ..., generated ...]}."""
    want = {}
    for c in calls:
        if c["cond_mod"] == "all":
            want["recon_from_all"] = [c["data"][m] for m in c["data"]] + [c["out"][m] for m in c["out"]]
        else:
            want[f"recon_from_{c['cond_mod']}"] = [c["data"][c["cond_mod"]]] + [c["out"][m] for m in c["out"]]
    return want


def png_pixels(path):
    from PIL import Image

    with Image.open(path) as im:
        assert im.mode == "RGB"
        return torch.from_numpy(np.array(im))
