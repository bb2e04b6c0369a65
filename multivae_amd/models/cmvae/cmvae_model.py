"""CMVAE (Palumbo et al. 2023, "Deep Generative Clustering with Multimodal Diffusion Variational Autoencoders", without the
diffusion decoders) on the HIP kernels.  Mirrors `multivae/models/cmvae/cmvae_model.py`: _compute_posteriors_and_embeddings
:147-221, _compute_k_lws :247-345, _iwae_looser / _dreg_looser :347-398, encode :400-505, generate_from_prior :507-544,
predict_clusters :546-619, prune_clusters :621-711, compute_joint_nll :732-788.

The model is MMVAE+ (shared latent u, private latents w_m handled as ONE concatenated latent [u, w]) whose prior of u is a
learnable mixture over `number_of_clusters` clusters and whose prior of w is fixed; the latent stage runs on csrc/cmvae.hip,
everything else (cross-modal private draws, reconstruction NLL, IWAE / DReG objective) on the MMVAE+ kernels.  The forward pass
and compute_joint_nll (all modalities) are SharedPrivateMultiVAE's (models/base/shared_private_model.py, shared with MMVAEPlus).

Deviation from the reference's literal form.  The reference takes an explicit expectation over q(c|u) = softmax_c(a_c) + 1e-20,
a_c = log pi_c + log p(u|c): lw = sum_c q_c (lpx + beta (a_c + log p(w) - log q(u|X) - log q(w|x) - log q_c)).  Up to the 1e-20
(below the resolution of the sums) this is lpx + beta (logsumexp_c a_c + log p(w) - log q(u|X) - log q(w|x)), which is what the
kernel evaluates.  With a pruned cluster (a logit of -inf) the literal form is 1e-20 * (-inf) = -inf for every sample; here
the cluster is simply absent (zero responsibility, no gradient), so a pruned model can still be evaluated and trained.
predict_clusters' norm_lliks is likewise logsumexp_c(.) / latent_dim: finite where a p(c|z) underflows to 0 (literal: 0 * inf)."""
import torch
from torch import nn
from torch.utils.data import DataLoader

from ... import _lib, kernels
from ...data.utils import set_inputs_to_device
from ..base import SharedPrivateMultiVAE
from ..base.base_utils import ModelOutput
from .cmvae_config import CMVAEConfig


def prune_entropy(pc_z):
    """Normalised entropy of the columns of pc_z [C, R] as the reference computes it with scipy (:661-670): the column is
    normalised by its sum, 0 log 0 = 0, and the entropy is divided by log(count_nonzero) -> [R]."""
    p = pc_z / pc_z.sum(0, keepdim=True)
    h = -torch.special.xlogy(p, p).sum(0)
    return h / torch.log(torch.count_nonzero(pc_z, dim=0).to(h.dtype))


class CMVAE(SharedPrivateMultiVAE):
    def __init__(self, model_config: CMVAEConfig, encoders: dict = None, decoders: dict = None):
        super().__init__(model_config, encoders, decoders)
        S, L = model_config.modalities_specific_dim, model_config.latent_dim
        self.model_name = "CMVAE"
        self.n_clusters = int(model_config.number_of_clusters)
        if not 1 <= self.n_clusters <= _lib.CMVAE_MAX_CLUSTERS:
            raise AttributeError(f"number_of_clusters must be in 1 .. {_lib.CMVAE_MAX_CLUSTERS}, got {self.n_clusters}")
        table = self.n_clusters * (2 * (L | 1) + 1) + 4 * L  # the latent kernel keeps the cluster means, stds and log pi in LDS
        if table > _lib.CMVAE_MAX_LDS_FLOATS:
            raise AttributeError(f"number_of_clusters = {self.n_clusters} with latent_dim = {L} needs a cluster table of {table} "
                                 f"floats; the CMVAE latent kernel holds at most {_lib.CMVAE_MAX_LDS_FLOATS} (include/mvk.h): "
                                 "use fewer clusters or a smaller latent_dim")
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

    @property
    def pc_params(self):
        """Weights of the prior distribution over the clusters."""
        return torch.softmax(self._pc_params, dim=-1)

    def _cluster_params(self):
        """-> stacked means [C, L], stds [C, L] (no gradient: the log-variances are fixed), logits [C]."""
        means = torch.cat(list(self.mean_clusters), dim=0)
        stds = self._log_var_to_std(torch.cat([p.detach() for p in self.logvar_clusters], dim=0))
        return means, stds, self._pc_params

    def _latent_node(self, state, noises, masks, family, dreg, mus, sds):
        means, stds, logits = self._cluster_params()
        wstd = self._log_var_to_std(self.w_logvar_prior.detach())
        return kernels.CMVAELatentFn.apply(state, noises, masks, family, dreg, wstd, stds, means, logits, *mus, *sds)

    def _cross_prior_logvar(self, r):
        return self.r_logvars_priors[r]

    def _detailed_extras(self, state, mods):
        return {"qcs": {m: state.resp[i] for i, m in enumerate(mods)}}

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
