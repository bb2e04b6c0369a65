"""SharedPrivateMultiVAE: what MMVAE+ and CMVAE have in common.  Every modality has a shared latent u (latent_dim) and a private
latent w (modalities_specific_dim), handled as ONE concatenated latent z = [u, w] by the latent stage of csrc/latent.hpp: the
mixture-of-experts density covers the first latent_dim dimensions, the private ones are scored by the modality's own posterior,
the prior terms are weighted by beta, and cross-modal decoder inputs take their private part from the target modality's prior.

A subclass owns its parameters and supplies the prior through three methods: `_latent_node` (the autograd node of its latent
kernels), `_cross_prior_logvar` (the private prior of the cross-modal draws) and `_detailed_extras` / `_joint_nll_modalities`
(what it adds to a detailed output, which modalities compute_joint_nll scores).  encode and generate_from_prior stay with the
subclasses: they differ in substance."""
import math

import torch
from torch import nn

from ... import _lib, kernels, schedule
from ...data.utils import drop_unused_modalities
from ..nn.default_architectures import BaseDictDecodersMultiLatents, BaseDictEncoders_MultiLatents
from .base_ae_model import BaseMultiVAE
from .base_utils import ModelOutput


class SharedPrivateMultiVAE(BaseMultiVAE):
    def __init__(self, model_config, encoders: dict = None, decoders: dict = None):
        if model_config.modalities_specific_dim is None:
            raise AttributeError("The modalities_specific_dim attribute must be provided in the model config.")
        super().__init__(model_config, encoders, decoders)
        if model_config.prior_and_posterior_dist not in ("laplace_with_softmax", "normal", "normal_with_softplus"):
            raise AttributeError(" The posterior_dist parameter must be  either 'laplace_with_softmax','normal' or "
                                 f"'normal_with_softplus'.  {model_config.prior_and_posterior_dist} was provided.")
        self.beta = model_config.beta
        self.modalities_specific_dim = model_config.modalities_specific_dim
        self.reconstruction_option = model_config.reconstruction_option
        self.multiple_latent_spaces = True
        self.style_dims = {m: self.modalities_specific_dim for m in self.encoders}
        self.objective = model_config.loss

    def default_encoders(self, model_config) -> nn.ModuleDict:
        return BaseDictEncoders_MultiLatents(input_dims=model_config.input_dims, latent_dim=model_config.latent_dim,
                                             modality_dims={m: model_config.modalities_specific_dim
                                                            for m in model_config.input_dims})

    def default_decoders(self, model_config) -> nn.ModuleDict:
        return BaseDictDecodersMultiLatents(input_dims=model_config.input_dims, latent_dim=model_config.latent_dim,
                                            modality_dims={m: model_config.modalities_specific_dim
                                                           for m in model_config.input_dims})

    @property
    def _std_family(self):
        return _lib.FAMILY[self.model_config.prior_and_posterior_dist]

    @property
    def _family(self):  # density / sampling family of the latent kernels
        return 1 if self.model_config.prior_and_posterior_dist == "laplace_with_softmax" else 0

    def _log_var_to_std(self, log_var):
        return kernels.MMVAEStdFn.apply(log_var, self._std_family)

    # -- what a subclass supplies ---------------------------------------------------------------------------------------------
    def _latent_node(self, state, noises, masks, family, dreg, mus, sds):
        """-> z_c [K,B,L+S] for every conditioning modality; fills `state` (kernels.MMVAEState) for MMVAEObjectiveFn."""
        raise NotImplementedError()

    def _cross_prior_logvar(self, r):
        """Log-variance [1,S] of the private prior of modality r that cross-modal decoder inputs are drawn from."""
        raise NotImplementedError()

    def _detailed_extras(self, state, mods):
        """Entries of a detailed output beyond "zss" and "lws"."""
        return {}

    def _joint_nll_modalities(self, inputs, **kwargs):
        """The modalities that compute_joint_nll conditions on and scores."""
        return list(inputs.data.keys())

    # -- the shared forward pass ----------------------------------------------------------------------------------------------
    def forward(self, inputs, **kwargs):
        """kwargs: K, noise = {cond: {"u": [K,B,L], "w": [K,B,S], other modality: [K,B,S]}} (explicit noise in the
        reference's draw order), detailed_output."""
        inputs = drop_unused_modalities(inputs)
        K = int(kwargs.pop("K", self.model_config.K))
        noise = kwargs.pop("noise", None)
        if self.objective not in ("dreg_looser", "iwae_looser"):
            raise NotImplementedError()
        dreg = self.objective == "dreg_looser"
        mods = list(inputs.data.keys())
        M = len(mods)
        L, S = self.latent_dim, self.modalities_specific_dim
        D = L + S
        family = self._family
        uniform = family == 1

        def encode_one(m):
            out = self.encoders[m](inputs.data[m])
            mu = torch.cat([out.embedding, out.style_embedding], dim=-1)
            sd = torch.cat([self._log_var_to_std(out.log_covariance),
                            self._log_var_to_std(out.style_log_covariance)], dim=-1)
            return mu, sd

        order = self._branch_order(inputs, mods)
        enc = schedule.run_branches(order, encode_one, inputs.data[order[0]].device)
        mus = [enc[m][0] for m in mods]
        sds = [enc[m][1] for m in mods]
        B = mus[0].shape[0]
        device = mus[0].device
        noises, cross_noise = [], {}
        for c in mods:  # draw order of the reference: u, w, then one private-prior draw per other modality
            nu = self._noise((K, B, L), device, None if noise is None else noise[c]["u"], uniform=uniform)
            nw = self._noise((K, B, S), device, None if noise is None else noise[c]["w"], uniform=uniform)
            noises.append(torch.cat([nu, nw], dim=-1))
            for r in mods:
                if r != c:
                    cross_noise[(c, r)] = self._noise((K, B, S), device, None if noise is None else noise[c][r],
                                                      uniform=uniform)
        masks = None
        if hasattr(inputs, "masks"):
            masks = [inputs.masks[m].to(torch.bool).contiguous() for m in mods]
        state = kernels.MMVAEState()
        state.shared_dims, state.beta = L, float(self.beta)
        zs = self._latent_node(state, noises, masks, family, int(dreg), mus, sds)
        mod_prior_std = {r: self._log_var_to_std(self._cross_prior_logvar(r)) for r in mods}

        def decode_all(r):  # every conditioning modality's latent through decoder r: ONE pass over the M * K * B stacked rows
            zins = []
            for ci, c in enumerate(mods):
                if r == c:
                    zin = zs[ci]
                else:
                    zin = kernels.MMVAEPlusCrossLatentFn.apply(zs[ci], mod_prior_std[r], cross_noise[(c, r)], L, family)
                zins.append(zin.reshape(-1, D))
            # (the reference decodes every (conditioning, target) pair on its own, mmvaePlus_model.py:172-186: M^2 decoder passes
            # of K * B rows; the rows are independent, so M passes of M * K * B rows give the same reconstructions with 1 / M of
            # the launches and M times longer weight-gradient reductions per launch)
            # — for decoders that declare their rows independent (BaseDecoder.rows_independent: every in-package one); a
            # user-written decoder is run pair by pair like in the reference
            if not getattr(self.decoders[r], "rows_independent", False):
                return [self.decoders[r](zin).reconstruction for zin in zins]
            rec = self.decoders[r](torch.cat(zins, dim=0)).reconstruction
            return list(rec.reshape(M, K * B, *rec.shape[1:]).unbind(0))

        dec = schedule.run_branches(self._branch_order(inputs, mods), decode_all, device)
        recons = [dec[r][c] for c in range(M) for r in mods]
        spec = self._recon_spec(mods, inputs.data, inputs.masks if masks is not None else None, K, B)
        loss = kernels.MMVAEObjectiveFn.apply(state, spec, M, dreg, *recons)
        out = ModelOutput(loss=loss, loss_sum=loss, metrics={})
        if kwargs.pop("detailed_output", False):
            out["zss"] = {m: zs[i] for i, m in enumerate(mods)}
            out["lws"] = {m: state.lw[i] for i, m in enumerate(mods)}
            out.update(self._detailed_extras(state, mods))
        return out

    def compute_joint_nll(self, inputs, K: int = 1000, batch_size_K: int = 100, **kwargs):
        """-sum_b ln p(x_b) from the pooled importance weights of the forward pass (mmvaePlus_model.py:477-531,
        cmvae_model.py:732-788): K // n_modalities samples per conditioning modality of `_joint_nll_modalities`, rescale
        factors and beta forced to 1 (and restored), and ln p(x_b) ~= logsumexp over all conditioning modalities and samples
        - ln(count).  kwargs: noise as in forward() with K -> K // n_modalities; the subclass's own."""
        self.eval()
        if hasattr(inputs, "masks"):
            raise AttributeError(self._NLL_INCOMPLETE)
        from ...data.datasets.base import DatasetOutput

        mods = self._joint_nll_modalities(inputs, **kwargs)
        k = int(K) // self.n_modalities
        noise = kwargs.get("noise")
        B = inputs.data[mods[0]].shape[0]
        device = inputs.data[mods[0]].device
        ll = torch.empty(B, dtype=torch.float32, device=device)
        step = max(1, kernels.IWAE_ROWS_BUDGET // max(k, 1))
        rescale, beta = self.rescale_factors, self.beta
        self.rescale_factors, self.beta = {m: 1.0 for m in rescale}, 1.0
        try:
            with torch.no_grad():
                for b0 in range(0, B, step):
                    b1 = min(B, b0 + step)
                    part = DatasetOutput(data={m: inputs.data[m][b0:b1] for m in mods})
                    nz = None
                    if noise is not None:
                        nz = {c: {key: v[:, b0:b1] for key, v in noise[c].items()} for c in mods}
                    out = self.forward(part, K=k, noise=nz, detailed_output=True)
                    kernels.iwae_reduce([out["lws"][m] for m in mods], out=ll[b0:b1])
        finally:
            self.rescale_factors, self.beta = rescale, beta
        # the latent kernel normalises the mixture of experts by the number of modalities it was given; the reference by
        # n_modalities (mmvaePlus_model.py:239, cmvae_model.py:262): a constant shift of every log-weight
        shift = math.log(self.n_modalities) - math.log(len(mods))
        return -(ll.sum() + B * shift)
