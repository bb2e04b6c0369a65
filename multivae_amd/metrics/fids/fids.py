"""`multivae/metrics/fids/fids.py`: the Fréchet distance between embedded real data and embedded generations.

The reference appends every batch's activations to a Python list, concatenates, copies all of them to the host and takes `np.mean`,
`np.cov` and `scipy.linalg.sqrtm` there.  Here the two activation streams are folded batch by batch into a device-resident state
(csrc/frechet.hip, kernels.fd_*: a fixed shift per stream, fp64 first and second moments, one launch per batch, no host read), and
the distance is one small piece of float64 linear algebra on the device at the end (`frechet_distance`).  The host reads one
number per `get_frechet_distance`.

The default embedding of the reference, a pretrained InceptionV3, needs torchvision and downloaded weights and is NOT built:
`FIDEvaluator` needs `custom_encoders` (which the reference offers for every modality that is no natural image)."""
from itertools import combinations
from typing import Dict, Optional

import numpy as np
import torch

from ... import _lib
from ... import kernels as K
from ..._output import ModelOutput
from ...data.utils import set_inputs_to_device
from ..base.evaluator_class import Evaluator
from .fids_config import FIDEvaluatorConfig


def frechet_distance(mean0, cov0, mean1, cov1):
    """|mean0 - mean1|^2 + tr cov0 + tr cov1 - 2 sum_i sqrt(max(lambda_i, 0)), lambda the eigenvalues of the symmetrised
    cov0^(1/2) cov1 cov0^(1/2), in float64 on the tensors' device: a 0-d tensor.  cov0^(1/2) comes from `torch.linalg.eigh` with
    negative eigenvalues clamped to 0.  For positive-semidefinite inputs this is the reference's tr sqrtm(cov0 cov1) (the two
    products are similar matrices), without scipy and without its `eps` retry for a singular product."""
    f = torch.float64
    mean0, mean1 = mean0.to(f).reshape(-1), mean1.to(f).reshape(-1)
    D = mean0.shape[0]
    cov0, cov1 = cov0.to(f).reshape(D, D), cov1.to(f).reshape(D, D)
    w, v = torch.linalg.eigh(0.5 * (cov0 + cov0.T))
    root = (v * w.clamp(min=0).sqrt()) @ v.T
    m = root @ cov1 @ root
    lam = torch.linalg.eigvalsh(0.5 * (m + m.T))
    diff = mean0 - mean1
    return diff @ diff + torch.trace(cov0) + torch.trace(cov1) - 2 * lam.clamp(min=0).sqrt().sum()


class DeviceFrechet:
    """Streaming Fréchet statistics of two streams of `D` features (real, generated), the analogue of `DeviceKMeans`: `update`
    is one launch per batch on device-resident state, nothing is kept per row and nothing is read by the host."""

    def __init__(self, D):
        self.D = int(D)
        if self.D < 1:
            raise ValueError("D must be at least 1")
        self.state = None

    def update(self, real, generated=None):
        """real, generated [n, D] fp32 on the GPU (generated may be None: that stream gets no row).  The first call fixes each
        stream's shift to the column mean of its batch."""
        real = self._rows(real, "real activations")
        if generated is not None:
            generated = self._rows(generated, "generated activations")
            if generated.shape != real.shape:
                raise ValueError(f"the two streams take the same number of rows per update, got {tuple(real.shape)} and "
                                 f"{tuple(generated.shape)}")
        if self.state is None:
            self.state = K.fd_new_state(self.D, real.device)
            K.fd_begin(self.state, real, generated)
        K.fd_update(self.state, real, generated)

    def _rows(self, x, name):
        _lib.require_gpu_tensor(x, name)
        x = x.detach().contiguous()
        if x.dim() != 2 or x.shape[1] != self.D or x.shape[0] < 1:
            raise ValueError(f"{name} should have shape [n >= 1, {self.D}], got {tuple(x.shape)}")
        return x

    def statistics(self):
        """(mean [2,D], cov [2,D,D], terms [5] = {|mean0 - mean1|^2, tr cov0, tr cov1, n0, n1}), float64 device tensors; the
        covariances are `np.cov(rowvar=False)` and exactly symmetric."""
        if self.state is None:
            raise ValueError("no update yet")
        return K.fd_finish(self.state, self.D)

    def compute(self):
        """The Fréchet distance of the two streams: a 0-d float64 device tensor."""
        mean, cov, _ = self.statistics()
        return frechet_distance(mean[0], cov[0], mean[1], cov[1])


class AdaptShapeFID(torch.nn.Module):
    """Transform a batched input so that each sample has three channels: (n,), (n, w) and (n, h, w) get a channel axis (and
    height 1), one channel is repeated three times, two channels get a zero plane (on the input's device), more than three
    are cut to three; with `resize`, a bilinear, antialiased resize to 299 x 299 follows (torchvision is no dependency)."""

    def __init__(self, resize=True, **kwargs) -> None:
        super().__init__(**kwargs)
        self.resize = (299, 299) if resize else None

    def forward(self, x):
        if x.dim() > 4:
            raise AttributeError("Can't visualize data with more than 3 dimensions")
        while x.dim() < 4:  # (n,) -> (n, 1, 1, 1), (n, w) -> (n, 1, 1, w), (n, h, w) -> (n, 1, h, w)
            x = x.unsqueeze(1)
        if x.shape[1] == 1:
            x = torch.cat([x for _ in range(3)], dim=1)
        elif x.shape[1] == 2:
            n, _, h, w = x.shape
            x = torch.cat([x, torch.zeros(n, 1, h, w, dtype=x.dtype, device=x.device)], dim=1)
        else:
            x = x[:, :3, :, :]
        if self.resize is None:
            return x
        return torch.nn.functional.interpolate(x, size=self.resize, mode="bilinear", antialias=True, align_corners=False)


class FIDEvaluator(Evaluator):
    """Fréchet distances between the embeddings of the test data and of generated data.

    model, test_dataset, output, eval_config (FIDEvaluatorConfig), sampler (a fitted sampler; None = the latent codes come from
    the prior): as for every evaluator.  custom_encoders {modality: torch.nn.Module}: the embedding network of each modality; it
    may return a tensor [n, D] or a ModelOutput with `.embedding`.  transform: applied to the data before the embedding (as in
    the reference, `AdaptShapeFID()` is the default only when neither transform nor custom_encoders is given, that is on the
    Inception path; with custom_encoders no transform is applied unless one is given).

    The reference's default embedding, the pretrained InceptionV3, is deliberately not built: it needs torchvision and
    downloaded weights.  With `custom_encoders=None` the constructor raises NotImplementedError."""

    def __init__(self, model, test_dataset, output=None, eval_config=FIDEvaluatorConfig(), sampler=None,
                 custom_encoders: Optional[Dict[str, torch.nn.Module]] = None, transform: Optional[torch.nn.Module] = None) -> None:
        if custom_encoders is None:  # before the base class opens its log handlers
            raise NotImplementedError("The default embedding of FIDEvaluator, the pretrained InceptionV3 wrapper, needs torchvision "
                                      "and downloaded weights and is not built here. Provide `custom_encoders`: one embedding "
                                      "network per modality.")
        super().__init__(model, test_dataset, output, eval_config, sampler)
        self.model_fds = {m: custom_encoders[m].to(self.device) for m in custom_encoders}
        self.inception_transform = transform  # AdaptShapeFID() is the default of the Inception path alone

    def _embed(self, mod, data):
        if self.inception_transform is not None:
            data = self.inception_transform(data)
        pred = self.model_fds[mod](data.to(self.device))
        if isinstance(pred, ModelOutput):
            pred = pred.embedding
        return pred.reshape(len(pred), -1).float()

    def get_frechet_distance(self, mod, generate_latent_function):
        """The Fréchet distance between the embedded test data of `mod` and the embedded decodings of the latent codes that
        `generate_latent_function(n, inputs=batch)` returns, batch by batch: a Python float (the one host read)."""
        self.model.eval()
        stats = None
        with torch.no_grad():
            for batch in self.test_loader:
                batch = set_inputs_to_device(batch, self.device)
                pred = self._embed(mod, batch.data[mod])
                n = len(pred)
                latents = generate_latent_function(n, inputs=batch)
                # generate_from_prior(1) returns one code without a batch axis: a one-row last batch gets it back
                latents.z = latents.z.to(self.device).reshape(n, -1)
                if not latents.one_latent_space:
                    for m in latents.modalities_z:
                        latents.modalities_z[m] = latents.modalities_z[m].to(self.device).reshape(n, -1)
                pred_gen = self._embed(mod, self.model.decode(latents, modalities=mod)[mod])
                if stats is None:
                    stats = DeviceFrechet(pred.shape[1])
                stats.update(pred, pred_gen)
        return float(stats.compute())

    def calculate_frechet_distance(self, mu1, sigma1, mu2, sigma2, eps=1e-6):
        r"""The Fréchet distance between two Gaussians :math:`\mathcal{N}(\mu_1, C_1)` and :math:`\mathcal{N}(\mu_2, C_2)`,
        :math:`\lVert \mu_1 - \mu_2\rVert^2 + \mathrm{Tr}(C_1 + C_2 - 2\sqrt{C_1 C_2})`, from numpy arrays or tensors: a Python
        float.  `eps` is accepted for the reference's signature; `frechet_distance` needs no retry."""
        dev = self.device

        def t(a, dims):
            a = torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).to(device=dev, dtype=torch.float64)
            return a.reshape(-1) if dims == 1 else (a.reshape(1, 1) if a.dim() < 2 else a)

        mu1, mu2, sigma1, sigma2 = t(mu1, 1), t(mu2, 1), t(sigma1, 2), t(sigma2, 2)
        assert mu1.shape == mu2.shape, (f"Training and test mean vectors have different lengths. mu1 has shape {tuple(mu1.shape)}"
                                        f"whereas mu2 has shape {tuple(mu2.shape)}")
        assert sigma1.shape == sigma2.shape, "Training and test covariances have different dimensions"
        return float(frechet_distance(mu1, sigma1, mu2, sigma2))

    def unconditional_fids(self):
        """Generate from the prior, or from the sampler fitted in the latent space, and compute the distance of each modality."""
        output = dict()
        generate_function = self.model.generate_from_prior if self.sampler is None else self.sampler.sample
        sampler_name = "prior" if self.sampler is None else self.sampler.name
        for mod in self.model.encoders:
            self.logger.info(f"Start computing FID for modality {mod}")
            fd = self.get_frechet_distance(mod, generate_function)
            output[f"fd_{mod}_sampler_{sampler_name}"] = fd
            self.logger.info(f"The FD for modality {mod} with sampler {sampler_name} is {fd}")
        self.metrics.update(output)
        return ModelOutput(**output)

    def eval(self):
        self.unconditional_fids()
        self.log_to_wandb()
        return ModelOutput(**self.metrics)

    def compute_fid_from_conditional_generation(self, subset, gen_mod):
        """Generate `gen_mod` from the encoding of the modalities in `subset` and compute its Fréchet distance."""

        def generate_function(n_samples, inputs):
            return self.model.encode(inputs=inputs, cond_mod=subset)

        fd = self.get_frechet_distance(gen_mod, generate_function)
        self.logger.info("The FD for modality %s computed from subset=%s is %s", gen_mod, subset, fd)
        subset_name = "_".join(subset)
        self.metrics[f"Conditional FD from {subset_name} to {gen_mod}"] = fd
        return fd

    def compute_all_conditional_fids(self, gen_mod):
        """For every subset of the modalities other than gen_mod, the distance of gen_mod generated from the subset, and the
        running mean over the subsets of each size."""
        modalities = [k for k in self.model.encoders if k != gen_mod]
        for n in range(1, len(modalities) + 1):
            fdn = []
            for s in combinations(modalities, n):
                fdn.append(self.compute_fid_from_conditional_generation(list(s), gen_mod))
                self.metrics[f"Mean FD from {n} modalities to {gen_mod}"] = np.mean(fdn)
        return ModelOutput(**self.metrics)
