"""MMVAE+ (Palumbo et al. 2023) on the HIP kernels.  Mirrors `multivae/models/mmvaePlus/mmvaePlus_model.py`:
_compute_posteriors_and_embeddings :122-187, _compute_k_lws :214-270, _dreg_looser :272-342, _iwae_looser :344-362.

Every modality has a shared latent u (latent_dim) and a private latent w (modalities_specific_dim); the forward pass and
compute_joint_nll are SharedPrivateMultiVAE's (models/base/shared_private_model.py, shared with CMVAE).  Here: the learnable
prior family(mean_priors["shared"], logvars_priors["shared"]) over [u, w] on the MMVAE kernels (csrc/mmvae.hip) and the
learnable private priors of the cross-modal draws.
"""
import torch
from torch import nn

from ... import kernels
from ..base import SharedPrivateMultiVAE
from ..base.base_utils import ModelOutput
from .mmvaePlus_config import MMVAEPlusConfig


class MMVAEPlus(SharedPrivateMultiVAE):
    def __init__(self, model_config: MMVAEPlusConfig, encoders: dict = None, decoders: dict = None):
        super().__init__(model_config, encoders, decoders)
        S, L = model_config.modalities_specific_dim, model_config.latent_dim
        self.mean_priors = nn.ParameterDict()
        self.logvars_priors = nn.ParameterDict()
        for mod in list(self.encoders.keys()):
            self.mean_priors[mod] = nn.Parameter(torch.zeros(1, S), requires_grad=False)
            self.logvars_priors[mod] = nn.Parameter(torch.zeros(1, S), requires_grad=model_config.learn_modality_prior)
        self.mean_priors["shared"] = nn.Parameter(torch.zeros(1, L + S), requires_grad=False)
        self.logvars_priors["shared"] = nn.Parameter(torch.zeros(1, L + S), requires_grad=model_config.learn_shared_prior)
        self.model_name = "MMVAEPlus"

    @property
    def pz_params(self):
        return self.mean_priors["shared"], self._log_var_to_std(self.logvars_priors["shared"])

    def _latent_node(self, state, noises, masks, family, dreg, mus, sds):
        prior_mean, prior_std = self.pz_params
        return kernels.MMVAELatentFn.apply(state, noises, masks, prior_mean.detach(), family, dreg, prior_std, *mus, *sds)

    def _cross_prior_logvar(self, r):
        return self.logvars_priors[r]

    def _joint_nll_modalities(self, inputs, **kwargs):
        """The reference evaluates compute_joint_nll on the inputs WITHOUT their last modality (`inputs.data.popitem()`,
        mmvaePlus_model.py:497, also removes it from the caller's dataset) while the mixture normaliser stays
        ln(n_modalities); the default here returns that number (without touching the caller's inputs).
        kwargs: all_modalities=True conditions on and scores every modality instead."""
        mods = list(inputs.data.keys())
        if not kwargs.get("all_modalities", False):
            mods = mods[:-1]
        if not mods:
            raise AttributeError("compute_joint_nll needs at least two modalities (the reference drops the last one).")
        return mods

    def encode(self, inputs, cond_mod="all", N: int = 1, return_mean=False, **kwargs):
        """mmvaePlus_model.py:364-456: shared latent from a randomly chosen conditioning modality (or the mean of the
        means), private latents from the own posterior for conditioning modalities, from the priors for the others."""
        cond_mod = super().encode(inputs, cond_mod, N, **kwargs).cond_mod
        flatten = kwargs.pop("flatten", False)
        family = self.model_config.prior_and_posterior_dist
        with torch.no_grad():
            outs = {m: self.encoders[m](inputs.data[m]) for m in cond_mod}
            B = len(list(inputs.data.values())[0])
            device = next(iter(outs.values())).embedding.device
            shape = (N,) if N > 1 else ()

            def sample(mu, sd):
                if family == "laplace_with_softmax":
                    return torch.distributions.Laplace(mu, sd).rsample(shape)
                return torch.distributions.Normal(mu, sd).rsample(shape)

            if return_mean:
                emb = torch.mean(torch.stack([o.embedding for o in outs.values()]), dim=0)
                z = torch.stack([emb] * N) if N > 1 else emb
            else:
                pick = cond_mod[int(torch.randint(len(cond_mod), (1,)))]
                z = sample(outs[pick].embedding, self._log_var_to_std(outs[pick].log_covariance))
            style = {}
            for m in self.encoders:
                if m in cond_mod and not return_mean:
                    style[m] = sample(outs[m].style_embedding, self._log_var_to_std(outs[m].style_log_covariance))
                elif m in cond_mod:
                    style[m] = torch.stack([outs[m].style_embedding] * N) if N > 1 else outs[m].style_embedding
                else:
                    mu = torch.cat([self.mean_priors[m]] * B, dim=0).to(device)
                    sd = torch.cat([self._log_var_to_std(self.logvars_priors[m])] * B, dim=0).to(device)
                    style[m] = sample(mu, sd)
            if flatten and N > 1:
                z = z.reshape(-1, z.shape[-1])
                style = {m: v.reshape(-1, v.shape[-1]) for m, v in style.items()}
        return ModelOutput(z=z, one_latent_space=False, modalities_z=style)

    def generate_from_prior(self, n_samples, **kwargs):
        """n samples of the (learnable) prior `prior_dist(*pz_params)` (mmvaePlus_model.py:453-456).  kwargs: noise [n, D]."""
        with torch.no_grad():
            mean, std = self.pz_params
            D = mean.shape[-1]
            n = max(int(n_samples), 1)
            noise = kwargs.get("noise")
            noise = self._noise((n, 1, D), mean.device, None if noise is None else noise.reshape(n, 1, D),
                                uniform=self._family == 1)
            z = kernels.iwae_sample(mean.detach().reshape(1, D), std.detach().reshape(1, D), noise, self._family)
        return ModelOutput(z=z.reshape(n, D).squeeze() if n_samples > 1 else z.reshape(D), one_latent_space=True)
