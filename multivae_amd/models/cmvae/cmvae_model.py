"""CMVAE (Palumbo et al. 2023, "Deep Generative Clustering with Multimodal Diffusion Variational Autoencoders", without the
diffusion decoders) on the HIP kernels.  Mirrors `multivae/models/cmvae/cmvae_model.py`: _compute_posteriors_and_embeddings
:147-221, _compute_k_lws :247-345, _iwae_looser / _dreg_looser :347-398, encode :400-505, generate_from_prior :507-544,
predict_clusters :546-619, prune_clusters :621-711, compute_joint_nll :732-788.

The model is MMVAE+ (shared latent u, private latents w_m handled as ONE concatenated latent [u, w]) whose prior of u is a
learnable mixture over `number_of_clusters` clusters and whose prior of w is fixed; the latent stage runs on csrc/cmvae.hip,
everything else (cross-modal private draws, reconstruction NLL, IWAE / DReG objective) on the MMVAE+ kernels.

Deviation from the reference's literal form.  The reference takes an explicit expectation over q(c|u) = softmax_c(a_c) + 1e-20,
a_c = log pi_c + log p(u|c): lw = sum_c q_c (lpx + beta (a_c + log p(w) - log q(u|X) - log q(w|x) - log q_c)).  Up to the 1e-20
(below the resolution of the sums) this is lpx + beta (logsumexp_c a_c + log p(w) - log q(u|X) - log q(w|x)), which is what the
kernel evaluates.  With a pruned cluster (a logit of -inf) the literal form is 1e-20 * (-inf) = -inf for every sample; here
the cluster is simply absent (zero responsibility, no gradient), so a pruned model can still be evaluated and trained.
predict_clusters' norm_lliks is likewise logsumexp_c(.) / latent_dim: finite where a p(c|z) underflows to 0 (literal: 0 * inf)."""
import math

import torch
from torch import nn
from torch.utils.data import DataLoader

from ... import _lib, kernels, schedule
from ...data.utils import drop_unused_modalities, set_inputs_to_device
from ..base import BaseMultiVAE
from ..base.base_utils import ModelOutput
from ..nn.default_architectures import BaseDictDecodersMultiLatents, BaseDictEncoders_MultiLatents
from .cmvae_config import CMVAEConfig


def prune_entropy(pc_z):
    """Normalised entropy of the columns of pc_z [C, R] as the reference computes it with scipy (:661-670): the column is
    normalised by its sum, 0 log 0 = 0, and the entropy is divided by log(count_nonzero) -> [R]."""
    p = pc_z / pc_z.sum(0, keepdim=True)
    h = -torch.special.xlogy(p, p).sum(0)
    return h / torch.log(torch.count_nonzero(pc_z, dim=0).to(h.dtype))


class CMVAE(BaseMultiVAE):
    def __init__(self, model_config: CMVAEConfig, encoders: dict = None, decoders: dict = None):
        if model_config.modalities_specific_dim is None:
            raise AttributeError("The modalities_specific_dim attribute must be provided in the model config.")
        super().__init__(model_config, encoders, decoders)
        if model_config.prior_and_posterior_dist not in ("laplace_with_softmax", "normal", "normal_with_softplus"):
            raise AttributeError(" The posterior_dist parameter must be  either 'laplace_with_softmax','normal' or "
                                 f"'normal_with_softplus'.  {model_config.prior_and_posterior_dist} was provided.")
        S, L = model_config.modalities_specific_dim, model_config.latent_dim
        self.model_name = "CMVAE"
        self.multiple_latent_spaces = True
        self.n_clusters = int(model_config.number_of_clusters)
        if not 1 <= self.n_clusters <= _lib.CMVAE_MAX_CLUSTERS:
            raise AttributeError(f"number_of_clusters must be in 1 .. {_lib.CMVAE_MAX_CLUSTERS}, got {self.n_clusters}")
        table = self.n_clusters * (2 * (L | 1) + 1) + 4 * L  # the latent kernel keeps the cluster means, stds and log pi in LDS
        if table > _lib.CMVAE_MAX_LDS_FLOATS:
            raise AttributeError(f"number_of_clusters = {self.n_clusters} with latent_dim = {L} needs a cluster table of {table} "
                                 f"floats; the CMVAE latent kernel holds at most {_lib.CMVAE_MAX_LDS_FLOATS} (include/mvk.h): "
                                 "use fewer clusters or a smaller latent_dim")
        self.beta = model_config.beta
        self.modalities_specific_dim = S
        self.reconstruction_option = model_config.reconstruction_option
        self.style_dims = {m: S for m in self.encoders}
        self.objective = model_config.loss
        # priors of the private spaces used for cross-modal reconstruction (mean fixed, scale learnable)
        self.r_mean_priors = nn.ParameterDict()
        self.r_logvars_priors = nn.ParameterDict()
        for mod in list(self.encoders.keys()):
            self.r_mean_priors[mod] = nn.Parameter(torch.zeros(1, S), requires_grad=False)
            self.r_logvars_priors[mod] = nn.Parameter(torch.zeros(1, S), requires_grad=model_config.learn_modality_prior)
        # regularising prior p(w_m) of the private spaces: fixed
        self.w_mean_prior = nn.Parameter(torch.zeros(1, S), requires_grad=False)
        self.w_logvar_prior = nn.Parameter(torch.zeros(1, S), requires_grad=False)
        # logits of the cluster weights; one mean (learnable) and one log-variance (fixed) per cluster
        self._pc_params = nn.Parameter(torch.zeros(self.n_clusters), requires_grad=True)
        self.mean_clusters = nn.ParameterList([nn.Parameter(2 * torch.rand(1, L) - 1, requires_grad=True)
                                               for _ in range(self.n_clusters)])
        self.logvar_clusters = nn.ParameterList([nn.Parameter(torch.zeros(1, L), requires_grad=False)
                                                 for _ in range(self.n_clusters)])

    def default_encoders(self, model_config) -> nn.ModuleDict:
        return BaseDictEncoders_MultiLatents(input_dims=model_config.input_dims, latent_dim=model_config.latent_dim,
                                             modality_dims={m: model_config.modalities_specific_dim
                                                            for m in model_config.input_dims})

    def default_decoders(self, model_config) -> nn.ModuleDict:
        return BaseDictDecodersMultiLatents(input_dims=model_config.input_dims, latent_dim=model_config.latent_dim,
                                            modality_dims={m: model_config.modalities_specific_dim
                                                           for m in model_config.input_dims})

    @property
    def pc_params(self):
        """Weights of the prior distribution over the clusters."""
        return torch.softmax(self._pc_params, dim=-1)

    @property
    def _std_family(self):
        return _lib.FAMILY[self.model_config.prior_and_posterior_dist]

    @property
    def _family(self):  # density / sampling family of the latent kernels
        return 1 if self.model_config.prior_and_posterior_dist == "laplace_with_softmax" else 0

    def _log_var_to_std(self, log_var):
        return kernels.MMVAEStdFn.apply(log_var, self._std_family)

    def _cluster_params(self):
        """-> stacked means [C, L], stds [C, L] (no gradient: the log-variances are fixed), logits [C]."""
        means = torch.cat(list(self.mean_clusters), dim=0)
        stds = self._log_var_to_std(torch.cat([p.detach() for p in self.logvar_clusters], dim=0))
        return means, stds, self._pc_params

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
        means, stds, logits = self._cluster_params()
        wstd = self._log_var_to_std(self.w_logvar_prior.detach())
        zs = kernels.CMVAELatentFn.apply(state, noises, masks, family, int(dreg), wstd, stds, means, logits, *mus, *sds)
        mod_prior_std = {r: self._log_var_to_std(self.r_logvars_priors[r]) for r in mods}

        def decode_all(r):  # every conditioning modality's latent through decoder r: ONE pass over the M * K * B stacked rows
            zins = []
            for ci, c in enumerate(mods):
                if r == c:
                    zin = zs[ci]
                else:
                    zin = kernels.MMVAEPlusCrossLatentFn.apply(zs[ci], mod_prior_std[r], cross_noise[(c, r)], L, family)
                zins.append(zin.reshape(-1, D))
            # as in MMVAEPlus.forward: decoders that declare their rows independent take the stacked rows in one pass, a
            # user-written decoder is run pair by pair like in the reference (:177-209)
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
            out["qcs"] = {m: state.resp[i] for i, m in enumerate(mods)}
        return out

    def _sample(self, mu, sd, shape=()):
        if self._family == 1:
            return torch.distributions.Laplace(mu, sd).rsample(shape)
        return torch.distributions.Normal(mu, sd).rsample(shape)

    def _private_prior(self, m):
        """(mean, log-variance) [1, S] of the private prior that `reconstruction_option` selects for modality m."""
        if self.reconstruction_option == "single_prior":
            return self.r_mean_priors[m], self.r_logvars_priors[m]
        if self.reconstruction_option == "joint_prior":
            return self.w_mean_prior, self.w_logvar_prior
        raise NotImplementedError()

    def encode(self, inputs, cond_mod="all", N: int = 1, return_mean=False, **kwargs):
        """:400-505: the shared code from ONE randomly chosen conditioning modality (its mean when return_mean is set: no
        averaging over modalities, unlike MMVAEPlus), private codes from the own posterior for conditioning modalities and
        from the `single_prior` / `joint_prior` prior for the others."""
        cond_mod = super().encode(inputs, cond_mod, N, **kwargs).cond_mod
        flatten = kwargs.pop("flatten", False)
        L, S = self.latent_dim, self.modalities_specific_dim
        with torch.no_grad():
            outs = {m: self.encoders[m](inputs.data[m]) for m in cond_mod}
            pick = cond_mod[int(torch.randint(len(cond_mod), (1,)))]
            mu = outs[pick].embedding.reshape(-1, L)
            n = mu.shape[0]
            shape = (N,) if N > 1 else ()

            def draw(mu_m, lv_m):
                if return_mean:
                    return torch.stack([mu_m] * N) if N > 1 else mu_m
                return self._sample(mu_m, self._log_var_to_std(lv_m), shape)

            z = draw(mu, outs[pick].log_covariance.reshape(-1, L))
            if flatten:
                z = z.reshape(-1, L)
            style = {}
            for m in self.encoders:
                if m in cond_mod:
                    mu_m, lv_m = outs[m].style_embedding.reshape(-1, S), outs[m].style_log_covariance.reshape(-1, S)
                else:
                    pm, plv = self._private_prior(m)
                    mu_m, lv_m = torch.cat([pm] * n, dim=0).to(mu.device), torch.cat([plv] * n, dim=0).to(mu.device)
                style[m] = draw(mu_m, lv_m)
                if flatten:
                    style[m] = style[m].reshape(-1, S)
        return ModelOutput(z=z, one_latent_space=False, modalities_z=style)

    def generate_from_prior(self, n_samples, **kwargs):
        """:507-544: a cluster per sample from Categorical(logits), the shared code from the cluster's distribution, private
        codes from the prior that `reconstruction_option` selects."""
        n = int(n_samples)
        with torch.no_grad():
            means, stds, logits = self._cluster_params()
            clusters = torch.distributions.Categorical(logits=logits).sample([n])
            z = self._sample(means[clusters], stds[clusters])
            style = {}
            for m in self.encoders:
                pm, plv = self._private_prior(m)
                style[m] = self._sample(torch.cat([pm] * n, dim=0), torch.cat([self._log_var_to_std(plv)] * n, dim=0))
        return ModelOutput(z=z, one_latent_space=False, modalities_z=style)

    def predict_clusters(self, inputs, compute_lliks=False, noise=None, **kwargs):
        """:546-619: a sample z_m ~ q(u | x_m) per modality, p(c | z_m) ~ p(z_m | c) (pi_c + 1e-20) and its argmax on
        mvk_cmvae_assign (one launch for all modalities), then a majority vote over the modalities (torch.mode: among tied
        clusters the smallest index).  noise: {modality: [B, L]} (explicit draws).  -> clusters [B], pc_zs {modality: [C, B]}
        and, with compute_lliks, norm_lliks [B] (the mean over modalities of the normalised likelihoods)."""
        L, family = self.latent_dim, self._family
        with torch.no_grad():
            mods = list(inputs.data.keys())
            zs = []
            for m in mods:
                out = self.encoders[m](inputs.data[m])
                mu = out.embedding.reshape(-1, L)
                sd = self._log_var_to_std(out.log_covariance.reshape(-1, L))
                nz = self._noise((1,) + tuple(mu.shape), mu.device, None if noise is None else noise[m].reshape(1, *mu.shape),
                                 uniform=family == 1)
                zs.append(kernels.iwae_sample(mu, sd, nz, family)[0])
            B = zs[0].shape[0]
            means, stds, logits = self._cluster_params()
            pc, assign, lliks = kernels.cmvae_assign(torch.cat(zs, dim=0), means, stds, logits, family, want_lliks=compute_lliks)
            pc_zs = {m: pc[:, i * B : (i + 1) * B] for i, m in enumerate(mods)}
            vote = torch.mode(assign.view(len(mods), B).t(), dim=-1)[0]
            if compute_lliks:
                return ModelOutput(clusters=vote, pc_zs=pc_zs, norm_lliks=lliks.view(len(mods), B).mean(0))
            return ModelOutput(clusters=vote, pc_zs=pc_zs)

    def prune_clusters(self, train_data, batch_size=128, **kwargs):
        """The entropy-based pruning of :621-711.  While at least two clusters are left: one pass over train_data accumulates, on
        the device and without a host read per batch, the mass of every cluster (the votes of predict_clusters) and the
        penalised normalised entropy  beta * mean_m H(p(c | z_m)) / log(count_nonzero) - norm_lliks;  then the cluster with the
        least mass is removed (its logit set to -inf).  At the end `_pc_params` and `n_clusters` (a plain int) are those of the
        pass with the smallest entropy value.  -> h_values, a list indexed by the number of clusters (inf where not computed).
        kwargs: device; noise[pass][batch] = {modality: [B, L]} (explicit draws of predict_clusters)."""
        noise = kwargs.get("noise")
        with torch.no_grad():
            loader = DataLoader(train_data, batch_size=batch_size)
            device = kwargs.get("device") or next(self.parameters()).device
            self.to(device)
            C = self._pc_params.numel()
            saved = [None] * (self.n_clusters + 1)
            h_values = [torch.inf] * (self.n_clusters + 1)
            n_pass = 0
            while self.n_clusters >= 2:
                mass = torch.zeros(C, dtype=torch.float32, device=device)
                h_sum = torch.zeros((), dtype=torch.float32, device=device)
                count = 0
                for i, batch in enumerate(loader):
                    batch = set_inputs_to_device(batch, device)
                    pred = self.predict_clusters(batch, compute_lliks=True, noise=None if noise is None else noise[n_pass][i])
                    mass += torch.bincount(pred.clusters, minlength=C).to(mass.dtype)
                    h = torch.stack([prune_entropy(pc) for pc in pred.pc_zs.values()], dim=0).mean(0)
                    h_sum += (self.beta * h - pred.norm_lliks).sum()
                    count += int(pred.clusters.shape[0])
                h_values[self.n_clusters] = h_sum / count
                saved[self.n_clusters] = self._pc_params.detach().clone()
                # remove the cluster with the least mass among those still present
                self.n_clusters -= 1
                mass[self._pc_params.isinf()] = torch.inf
                lightest = mass == mass.min()
                lightest &= lightest.cumsum(0) == 1  # the FIRST minimum, as torch.argmin on the host; a device argmin may pick any
                self._pc_params.data.masked_fill_(lightest, -torch.inf)
                n_pass += 1
            computed = [n for n, h in enumerate(h_values) if torch.is_tensor(h)]
            if computed:  # ONE host read for all passes
                hs = torch.stack([h_values[n] for n in computed]).cpu()
                for n, h in zip(computed, hs):
                    h_values[n] = h
                self.n_clusters = int(computed[int(torch.argmin(hs))])
                self._pc_params.data.copy_(saved[self.n_clusters])
        return h_values

    def compute_joint_nll(self, inputs, K: int = 1000, batch_size_K: int = 100, **kwargs):
        """-sum_b ln p(x_b) from the pooled importance weights of the forward pass (:732-788): K // n_modalities samples per
        conditioning modality, all modalities, rescale factors and beta forced to 1 (and restored), and
        ln p(x_b) ~= logsumexp over all conditioning modalities and samples - ln(count).  kwargs: noise as in forward() with
        K -> K // n_modalities."""
        self.eval()
        if hasattr(inputs, "masks"):
            raise AttributeError(self._NLL_INCOMPLETE)
        from ...data.datasets.base import DatasetOutput

        mods = list(inputs.data.keys())
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
        # n_modalities (:262): a constant shift of every log-weight
        shift = math.log(self.n_modalities) - math.log(len(mods))
        return -(ll.sum() + B * shift)
