"""MHVAE, the hierarchical multimodal VAE, on the HIP kernels.  Mirrors `multivae/models/mhvae/mhvae_model.py`: constructor and
its checks :47-77, :346-442, subset_encode :103-186, forward :241-262, encode :264-311, modality_encode :313-344.

Every modality has a bottom-up chain (encoder, n_latent - 1 bottom-up blocks); the latents z_L ... z_1 are sampled top-down, each
from the product of the prior p(z_l | z_>l) (N(0, I) at the top) and the posteriors of the modalities of a subset; the loss is the
mean over ALL non-empty subsets of the negative ELBO.  The reference walks the 2^M - 1 subsets in Python, ~25 elementwise launches
per (subset, level).  Here the subset is a batch axis: one `mvk_mhvae_level_fwd` launch per level for all subsets
(kernels.MHVAELevelFn: product of experts, sample and KL), the top-down, prior and decoder blocks once on [S B, ...] rows, each
modality's posterior block once on the rows of the subsets that hold it, and the loss and its gradients out of ReconLossFn with the
subset axis as its K axis.  The blocks are the user's torch modules and run through torch autograd.

`subset_batching`: batching changes what a batch-statistics layer sees (S B rows in place of B), so it is off when a BatchNorm
layer is found in the top-down, prior or posterior blocks or the decoders, and may be turned off by hand; the model then walks
the subsets in the reference's order with S = 1 launches."""
import logging
from itertools import combinations
from typing import Union

import torch

from ... import kernels
from ..base import BaseMultiVAE
from ..base.base_utils import ModelOutput
from ..nn.base_architectures import BaseEncoder
from .mhvae_config import MHVAEConfig

logger = logging.getLogger(__name__)


class MHVAE(BaseMultiVAE):
    def __init__(self, model_config: MHVAEConfig, encoders: dict, decoders: dict, bottom_up_blocks: dict, top_down_blocks: list,
                 posterior_blocks: Union[list, dict], prior_blocks: list):
        super().__init__(model_config, encoders, decoders)
        self.n_latent = model_config.n_latent
        self.beta = model_config.beta
        self.model_name = "MHVAE"
        if self.n_modalities > kernels._lib.MAX_MODALITIES:
            raise AttributeError(f"MHVAE takes at most {kernels._lib.MAX_MODALITIES} modalities (the experts of one level launch)")

        self.sanity_check_bottom_up(encoders, bottom_up_blocks)
        self.set_bottom_up_blocks(bottom_up_blocks)
        self.sanity_check_top_down_blocks(top_down_blocks)
        self.set_top_down_blocks(top_down_blocks)
        self.sanity_check_prior_blocks(prior_blocks)
        self.prior_blocks = torch.nn.ModuleList(prior_blocks)
        self.check_and_set_posterior_blocks(posterior_blocks)
        self.model_config.custom_architectures.extend(["bottom_up_blocks", "top_down_blocks", "prior_blocks", "posterior_blocks"])

        batch_stats = any(isinstance(layer, torch.nn.modules.batchnorm._BatchNorm)
                          for part in (self.top_down_blocks, self.prior_blocks, self.posterior_blocks, self.decoders)
                          for layer in part.modules())
        self.subset_batching = not batch_stats

    # -- the reference's checks and messages (:346-442) --------------------------------------------------------------------------
    def sanity_check_bottom_up(self, encoders, bottom_up_blocks):
        if self.n_modalities != len(bottom_up_blocks.keys()):
            raise AttributeError(f"The provided number of decoders {len(bottom_up_blocks.keys())} doesn't"
                                 f"match the number of modalities ({self.n_modalities} in model config ")
        if encoders.keys() != bottom_up_blocks.keys():
            raise AttributeError("The names of the modalities in the encoders dict doesn't match the names of the modalities"
                                 " in the bottom_up_blocks dict.")
        for mod in bottom_up_blocks:
            if len(bottom_up_blocks[mod]) != self.n_latent - 1:
                raise AttributeError(f"There must be {self.n_latent - 1} bottom_up_blocks for modality"
                                     f" {mod} but you provided {len(bottom_up_blocks[mod])} layers.")
            if not isinstance(bottom_up_blocks[mod][-1], BaseEncoder):
                raise AttributeError(f"The last layer in bottom_up_blocks for modality {mod}"
                                     " must be an instance of BaseEncoder")

    def sanity_check_top_down_blocks(self, top_down_blocks):
        if len(top_down_blocks) != self.n_latent - 1:
            raise AttributeError(f"There must be {self.n_latent - 1} modules in top_down_blocks.")

    def check_and_set_posterior_blocks(self, posterior_blocks):
        if isinstance(posterior_blocks, (list, torch.nn.ModuleList)):  # shared weights: a list of modules
            logger.info("Shared weights for the posterior blocks")
            self.share_posterior_weights = True
            if len(posterior_blocks) != self.n_latent - 1:
                raise AttributeError(f"There must be {self.n_latent - 1} modules in posterior_blocks.")
            for block in posterior_blocks:
                if not isinstance(block, BaseEncoder):
                    raise AttributeError("The modules in posterior_blocks must be instances of BaseEncoder")
            self.posterior_blocks = torch.nn.ModuleList(posterior_blocks)
            return
        if isinstance(posterior_blocks, (dict, torch.nn.ModuleDict)):  # a list of modules per modality
            logger.info("Not shared weights for the posterior blocks")
            self.share_posterior_weights = False
            if posterior_blocks.keys() != self.encoders.keys():
                raise AttributeError("The keys of posterior_blocks must match the keys of encoders.")
            for m, p in posterior_blocks.items():
                if len(p) != self.n_latent - 1:
                    raise AttributeError(f"There must be {self.n_latent - 1} modules in posterior_blocks[{m}].")
                for block in p:
                    if not isinstance(block, BaseEncoder):
                        raise AttributeError(f"The modules in posterior_blocks[{m}] must be instances of BaseEncoder")
            self.posterior_blocks = torch.nn.ModuleDict()
            for mod in posterior_blocks:
                self.posterior_blocks[mod] = torch.nn.ModuleList(posterior_blocks[mod])
            return
        raise AttributeError("posterior_blocks must be a list or a dict")

    def sanity_check_prior_blocks(self, prior_blocks):
        if len(prior_blocks) != self.n_latent - 1:
            raise AttributeError(f"There must be {self.n_latent - 1} modules in prior.")
        for block in prior_blocks:
            if not isinstance(block, BaseEncoder):
                raise AttributeError("The modules in prior_blocks  must be instances of BaseEncoder")

    def set_top_down_blocks(self, top_down_blocks):
        self.top_down_blocks = torch.nn.ModuleList(top_down_blocks)

    def set_bottom_up_blocks(self, bottom_up_blocks):
        self.bottom_up_blocks = torch.nn.ModuleDict()
        for mod in bottom_up_blocks:
            self.bottom_up_blocks[mod] = torch.nn.ModuleList(bottom_up_blocks[mod])

    def _subsets(self):
        """All the non-empty subsets of the modalities, in the reference's order (by size, the full one last)."""
        subsets = []
        for i in range(1, self.n_modalities + 1):
            subsets += combinations(list(self.encoders.keys()), r=i)
        return subsets

    def _get_posterior_block(self, mod, i):
        if self.share_posterior_weights:
            return self.posterior_blocks[i]
        return self.posterior_blocks[mod][i]

    # -- the hierarchy ---------------------------------------------------------------------------------------------------------
    def modality_encode(self, data: dict):
        """-> ({mod: ModelOutput(embedding, log_covariance)} of the deepest latent, {mod: the n_latent - 1 bottom-up results})."""
        skips = {mod: [] for mod in data}
        z_ls_params = {}
        for mod in data:
            z = self.encoders[mod](data[mod]).embedding
            skips[mod].append(z)
            for i in range(self.n_latent - 2):
                z = self.bottom_up_blocks[mod][i](z)
                skips[mod].append(z)
            z_ls_params[mod] = self.bottom_up_blocks[mod][-1](z)
        return z_ls_params, skips

    def _levels(self, z_ls_params, skips, subsets, masks, noise=None, return_mean=False):
        """The latents and KL rows of every level for the S given subsets (tuples of modality names), the subset a batch axis.
        -> ({"z_l": [S B, *shape_l]}, [kl_rows of level n_latent, ..., 1], each [S, B]).  One level launch per level."""
        mods = [m for m in self.encoders if any(m in s for s in subsets)]  # the experts of the launches, in encoder order
        member = [sum(1 << k for k, m in enumerate(mods) if m in s) for s in subsets]
        S = len(subsets)
        mk = None if masks is None else [masks[m] for m in mods]
        top = [z_ls_params[m] for m in mods]
        B, shape = top[0].embedding.shape[0], tuple(top[0].embedding.shape[1:])
        device = top[0].embedding.device

        def draw(name, F):
            if return_mean:
                return None
            given = None if noise is None else noise[name].reshape(S, B, F)
            return self._noise((S, B, F), device, given)

        F = int(torch.Size(shape).numel())
        name = f"z_{self.n_latent}"
        pairs = [t for o in top for t in (o.embedding, o.log_covariance)]
        z, kl = kernels.MHVAELevelFn.apply(draw(name, F), member, True, mk, B, F, None, None, *pairs)
        z_dict, kls = {name: z.reshape(S * B, *shape)}, [kl]
        for i in range(self.n_latent - 1, 0, -1):
            h = self.top_down_blocks[i - 1](z_dict[f"z_{i + 1}"])
            prior = self.prior_blocks[i - 1](h)
            hv = h.reshape(S, B, *h.shape[1:])
            pairs = []
            for k, m in enumerate(mods):
                rows = [s for s in range(S) if member[s] >> k & 1]
                d = skips[m][i - 1]
                if len(rows) < S:
                    hm = torch.cat([hv[s] for s in rows])
                else:
                    hm = h
                if len(rows) > 1:
                    d = d.repeat(len(rows), *([1] * (d.dim() - 1)))
                out = self._get_posterior_block(m, i - 1)(torch.cat([hm, d], dim=1))  # on the channels
                pairs += [out.embedding, out.log_covariance]
            shape = tuple(prior.embedding.shape[1:])
            F = int(torch.Size(shape).numel())
            name = f"z_{i}"
            z, kl = kernels.MHVAELevelFn.apply(draw(name, F), member, False, mk, B, F, prior.embedding, prior.log_covariance, *pairs)
            z_dict[name] = z.reshape(S * B, *shape)
            kls.append(kl)
        return z_dict, kls

    # -- training -------------------------------------------------------------------------------------------------------------
    def forward(self, inputs, **kwargs) -> ModelOutput:
        """kwargs: noise {"z_l": [S, B, *shape_l]} for every level l (the reparameterisation draws, subsets in `_subsets()` order;
        drawn on the device without it).  Other kwargs are ignored."""
        noise = kwargs.pop("noise", None)
        masks = inputs.masks if hasattr(inputs, "masks") else None
        z_ls_params, skips = self.modality_encode(inputs.data)
        subsets = self._subsets()
        S, names = len(subsets), list(self.decoders.keys())
        B = next(iter(z_ls_params.values())).embedding.shape[0]
        if self.subset_batching:
            z_dict, kls = self._levels(z_ls_params, skips, subsets, masks, noise)
            recons = [self.decoders[m](z_dict["z_1"]).reconstruction for m in names]
        else:
            per_kl, per_rec = [], []
            for s, subset in enumerate(subsets):
                ns = None if noise is None else {k: v[s:s + 1] for k, v in noise.items()}
                z_dict, kl = self._levels(z_ls_params, skips, [subset], masks, ns)
                per_kl.append(kl)
                per_rec.append([self.decoders[m](z_dict["z_1"]).reconstruction for m in names])
            kls = [torch.cat([kl[l] for kl in per_kl]) for l in range(self.n_latent)]
            recons = [torch.cat([r[j] for r in per_rec]) for j in range(len(names))]
        # loss = mean over the subsets of (sum_m sum_b nll_m rescale_m mask_m + beta sum_levels kl); loss_sum = loss (not / B)
        spec = self._recon_spec(names, inputs.data, masks, S, B)
        L = self.n_latent
        spec.update(coef=[1.0] * len(names), lossw=[1.0 / S] * len(names), extra_coef=[1.0] * L,
                    extra_lossw=[float(self.beta) / S] * L, extra_split=[1] * L, loss_sum_scale=1.0)
        loss, _ = kernels.ReconLossFn.apply(spec, len(names), *recons, *kls)
        # the reference reports the KLs of the last subset it walked, the full one
        metrics = {f"kl_{L - j}": kls[j].detach()[S - 1].sum() for j in range(L)}
        return ModelOutput(loss=loss, loss_sum=loss, metrics=metrics)

    # -- inference helpers ----------------------------------------------------------------------------------------------------
    def encode(self, inputs, cond_mod: Union[list, str] = "all", N: int = 1, return_mean=False, **kwargs) -> ModelOutput:
        """The latents of every level given the modalities of cond_mod: z = z_1 and all_z = {"z_l": ...}, [B, *shape_l] for N == 1,
        [N, B, *shape_l] for N > 1 ([N B, *shape_l] with flatten=True).  kwargs: flatten, noise {"z_l": N B F_l elements}."""
        flatten = kwargs.pop("flatten", False)
        noise = kwargs.pop("noise", None)
        cond_mod = super().encode(inputs, cond_mod, N, **kwargs).cond_mod
        z_ls_params, skips = self.modality_encode(inputs.data)
        n_data = len(list(z_ls_params.values())[0].embedding)
        masks = inputs.masks if hasattr(inputs, "masks") else None
        if N > 1:
            for mod, z_l in z_ls_params.items():
                z_l.embedding = torch.cat([z_l.embedding] * N, dim=0)
                z_l.log_covariance = torch.cat([z_l.log_covariance] * N, dim=0)
                skips[mod] = [torch.cat([t] * N, dim=0) for t in skips[mod]]
            if masks is not None:
                masks = {m: torch.cat([masks[m]] * N, dim=0) for m in masks}
        z_dict, _ = self._levels(z_ls_params, skips, [tuple(cond_mod)], masks, noise, return_mean=return_mean)
        if not flatten and N > 1:
            for k in z_dict:
                z_dict[k] = z_dict[k].reshape(N, n_data, *z_dict[k].shape[1:])
        return ModelOutput(z=z_dict["z_1"], all_z=z_dict, one_latent_space=True)
