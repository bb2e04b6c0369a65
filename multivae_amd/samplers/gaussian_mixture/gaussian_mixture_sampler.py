"""`multivae/samplers/gaussian_mixture/gaussian_mixture_sampler.py`: a Gaussian mixture fitted in the latent space of a trained
model.  The reference copies every training embedding to the host and runs scikit-learn's full-covariance EM there; here the
embeddings stay on the GPU and the fit is the fused EM of csrc/gmm.hip (kernels.gmm_*): per iteration six launches and no host
round trip, the convergence test included (the host reads a 64-byte state block once every `check_every` iterations)."""
import logging
import math
import warnings

import torch
from torch.utils.data import DataLoader

from ... import _lib
from ... import kernels as K
from ..._output import ModelOutput
from ...data.utils import set_inputs_to_device
from ..base import BaseSampler
from .gaussian_mixture_config import GaussianMixtureSamplerConfig

logger = logging.getLogger(__name__)

KMEANS_MAX_ITER = 100


class ConvergenceWarning(UserWarning):
    """EM stopped at max_iter (scikit-learn warns with a class of the same name and goes on)."""


class DeviceGaussianMixture:
    """The fitted state of one mixture, with scikit-learn's attribute names: weights_ [C], means_ [C,L], covariances_ [C,L,L],
    precisions_cholesky_ [C,L,L] (device fp32 tensors), converged_, n_iter_, lower_bound_ (Python scalars).
    covariances_cholesky_ [C,L,L] is the lower factor that `sample` multiplies the noise by."""

    def __init__(self, n_components, tol=1e-3, reg_covar=1e-6, max_iter=2000, check_every=8):
        self.n_components, self.tol, self.reg_covar, self.max_iter = int(n_components), float(tol), float(reg_covar), int(max_iter)
        self.check_every = max(1, int(check_every))
        self.converged_, self.n_iter_, self.lower_bound_ = False, 0, -math.inf

    # ---- initialisation -------------------------------------------------------------------------------------------------
    def _seed(self, x, resp, scratch, generator):
        """k-means++: the first seed uniformly, every next one with probability proportional to the squared distance to the
        nearest seed so far (the per-row distances of the hard E-step).  A row at distance 0 is never drawn: seeds are distinct
        rows unless fewer distinct rows than components exist."""
        N = x.shape[0]
        idx = torch.randint(N, (1,), generator=generator, device=x.device)
        d2 = torch.empty(N, dtype=torch.float32, device=x.device)
        for _ in range(1, self.n_components):
            K.gmm_estep_hard(x, x[idx].contiguous(), resp, scratch, row_out=d2)
            if float(d2.sum()) > 0.0:
                nxt = torch.multinomial(d2, 1, generator=generator)
            else:  # every row coincides with a seed: take the first row that is not one yet
                free = torch.ones(N, dtype=torch.bool, device=x.device)
                free[idx] = False
                nxt = free.nonzero()[:1, 0]
            idx = torch.cat([idx, nxt])
        return idx

    def _kmeans(self, x, p, resp, scratch, generator, init_indices):
        """Lloyd from the seeds until no label changes (at most KMEANS_MAX_ITER rounds); leaves the one-hot labels in resp."""
        if init_indices is None:
            idx = self._seed(x, resp, scratch, generator)
        else:
            idx = torch.as_tensor(init_indices, dtype=torch.int64, device=x.device)
            if idx.numel() != self.n_components:
                raise ValueError(f"init_indices must name {self.n_components} rows, got {idx.numel()}")
        self.init_indices_ = idx
        p["means"].copy_(x[idx])
        labels = torch.full((x.shape[0],), -1, dtype=torch.int32, device=x.device)
        changed = torch.zeros(1, dtype=torch.int32, device=x.device)
        self.kmeans_n_iter_ = 0
        for _ in range(KMEANS_MAX_ITER):
            K.gmm_estep_hard(x, p["means"], resp, scratch, labels=labels, changed=changed)
            if int(changed) == 0:
                break
            K.gmm_mstep(x, resp, p, self.reg_covar, scratch, means_only=True)
            self.kmeans_n_iter_ += 1
        self.kmeans_labels_ = labels

    def _given(self, v, shape, dev, what):
        t = torch.as_tensor(v).to(device=dev, dtype=torch.float64)
        if tuple(t.shape) != shape:
            raise ValueError(f"{what} should have shape {shape}, got {tuple(t.shape)}")
        return t

    # ---- fit ------------------------------------------------------------------------------------------------------------
    def fit(self, x, generator=None, weights_init=None, means_init=None, precisions_init=None, init_indices=None):
        _lib.require_gpu_tensor(x, "embeddings")
        x = x.detach().contiguous()
        N, L = x.shape
        C, dev = self.n_components, x.device
        if not bool(torch.isfinite(x).all()):
            raise ValueError("Input contains NaN or infinity.")
        scratch = K.gmm_scratch(L, C, dev)
        p = K.gmm_new_params(L, C, dev)
        resp = torch.empty(N, C, dtype=torch.float32, device=dev)
        if weights_init is None or means_init is None or precisions_init is None:
            self._kmeans(x, p, resp, scratch, generator, init_indices)
            K.gmm_mstep(x, resp, p, self.reg_covar, scratch)  # scikit-learn's _initialize: one M-step on the one-hot labels
        if weights_init is not None:
            p["weights"].copy_(self._given(weights_init, (C,), dev, "weights_init"))
        if means_init is not None:
            p["means"].copy_(self._given(means_init, (C, L), dev, "means_init"))
        if precisions_init is not None:  # _compute_precision_cholesky_from_precisions: P P^T = precision, P upper triangular
            prec = self._given(precisions_init, (C, L, L), "cpu", "precisions_init")  # C small factorisations, once: on the host
            P = torch.linalg.cholesky(prec.flip(-1, -2)).flip(-1, -2)
            cov = torch.linalg.inv(prec)
            p["prec_chol"].copy_(P)
            p["logdet"].copy_(torch.log(torch.diagonal(P, dim1=-2, dim2=-1)).sum(-1))
            p["covs"].copy_(cov)
            p["cov_chol"].copy_(torch.linalg.cholesky(cov))
        state = K.gmm_new_state(dev)
        S = _lib.GMM_STATE
        done, st = 0, None
        while done < self.max_iter:
            group = min(self.check_every, self.max_iter - done)
            for _ in range(group):
                K.gmm_em_step(x, p, resp, state, self.reg_covar, self.tol, scratch)
            done += group
            st = state.tolist()  # the one host read per group
            if st[S["converged"]] or st[S["status"]]:
                break
        if st is not None:
            if st[S["status"]]:
                raise ValueError("Fitting the mixture model failed because some components have ill-defined empirical covariance "
                                 "(for instance caused by singleton or collapsed samples). Try to decrease the number of components, "
                                 "increase reg_covar, or scale the input data.")
            self.converged_, self.n_iter_, self.lower_bound_ = bool(st[S["converged"]]), int(st[S["iter"]]), float(st[S["lb"]])
            if not self.converged_:
                warnings.warn("EM did not converge within max_iter. Try different init parameters, or increase max_iter, tol, or "
                              "check for degenerate data.", ConvergenceWarning)
        self.weights_, self.means_, self.covariances_ = p["weights"], p["means"], p["covs"]
        self.precisions_cholesky_, self.covariances_cholesky_ = p["prec_chol"], p["cov_chol"]
        return self

    # ---- sample ---------------------------------------------------------------------------------------------------------
    def sample(self, n_samples=1, generator=None, components=None, noise=None):
        """(z [n,L], component indices [n] int32).  Indices are drawn from the weights and grouped by component, the order in
        which scikit-learn stacks its samples; z = mean + covariance factor @ noise in one launch."""
        dev = self.means_.device
        if components is None:
            components = torch.multinomial(self.weights_, n_samples, replacement=True, generator=generator).sort().values
        components = torch.as_tensor(components, device=dev).to(torch.int32).contiguous()
        if bool(((components < 0) | (components >= self.n_components)).any()):
            raise ValueError("component index out of range")
        if noise is None:
            noise = torch.randn(n_samples, self.means_.shape[1], generator=generator, device=dev, dtype=torch.float32)
        noise = torch.as_tensor(noise, dtype=torch.float32, device=dev).contiguous()
        if components.shape[0] != n_samples or tuple(noise.shape) != (n_samples, self.means_.shape[1]):
            raise ValueError("components / noise do not match n_samples")
        return K.gmm_sample(self.means_, self.covariances_cholesky_, components, noise), components


class GaussianMixtureSampler(BaseSampler):
    """Fits a mixture of `n_components` full-covariance Gaussians on the training embeddings `model.encode(...).z` (one more per
    modality on `modalities_z[m]` when the model has private latent spaces).  `fit` must be called before `sample`."""

    def __init__(self, model, sampler_config: GaussianMixtureSamplerConfig = None):
        if sampler_config is None:
            sampler_config = GaussianMixtureSamplerConfig()
        BaseSampler.__init__(self, model=model, sampler_config=sampler_config)
        self.n_components = sampler_config.n_components
        self.name = "GaussianMixtureSampler"

    def fit(self, train_data, **kwargs):
        """kwargs: tol (1e-3), max_iter (2000), reg_covar (1e-6), check_every (8: EM iterations enqueued between two reads of the
        device's convergence state; the result does not depend on it), generator (a device torch.Generator for the seeding),
        weights_init / means_init / precisions_init (scikit-learn's meaning), init_indices (rows used as k-means seeds)."""
        loader = DataLoader(dataset=train_data, batch_size=100, shuffle=False)
        z, mod_z = [], {m: [] for m in self.model.encoders} if self.model.multiple_latent_spaces else {}
        with torch.no_grad():
            for inputs in loader:
                out = self.model.encode(set_inputs_to_device(inputs, self.device))
                z.append(out.z)
                for m in mod_z:
                    mod_z[m].append(out.modalities_z[m])
        z = torch.cat(z).float()
        mod_z = {m: torch.cat(v).float() for m, v in mod_z.items()}
        if self.n_components > z.shape[0]:
            self.n_components = z.shape[0]
            logger.warning(f"Setting the number of component to {z.shape[0]} since n_components > n_samples when fitting the gmm")
        opts = {k: kwargs[k] for k in ("tol", "max_iter", "reg_covar", "check_every") if k in kwargs}
        init = {k: kwargs[k] for k in ("generator", "weights_init", "means_init", "precisions_init", "init_indices") if k in kwargs}
        self.gmm = DeviceGaussianMixture(self.n_components, **opts).fit(z, **init)
        if self.model.multiple_latent_spaces:
            gen = {"generator": init["generator"]} if "generator" in init else {}
            self.mod_gmms = {m: DeviceGaussianMixture(self.n_components, **opts).fit(mod_z[m], **gen) for m in mod_z}
        self.is_fitted = True

    def sample(self, n_samples: int = 1, batch_size: int = 500, **kwargs):
        """A ModelOutput like `encode` returns: z [n_samples, latent_dim], one_latent_space, and modalities_z for a model with
        private latent spaces.  kwargs (for tests): generator; components [n_samples] and noise [n_samples, latent_dim] for z."""
        if not self.is_fitted:
            raise ArithmeticError("The sampler needs to be fitted by calling sampler.fit() method before sampling.")
        generator, components, noise = kwargs.get("generator"), kwargs.get("components"), kwargs.get("noise")
        sizes = [batch_size] * int(n_samples / batch_size)
        if n_samples % batch_size != 0:
            sizes.append(n_samples % batch_size)
        z_list, mod_z, at = [], {m: [] for m in self.model.encoders} if self.model.multiple_latent_spaces else {}, 0
        for b in sizes:
            comp_b = None if components is None else components[at:at + b]
            noise_b = None if noise is None else noise[at:at + b]
            z_list.append(self.gmm.sample(b, generator=generator, components=comp_b, noise=noise_b)[0])
            for m in mod_z:
                mod_z[m].append(self.mod_gmms[m].sample(b, generator=generator)[0])
            at += b
        output = ModelOutput(z=torch.cat(z_list, dim=0))
        if self.model.multiple_latent_spaces:
            output["one_latent_space"] = False
            output["modalities_z"] = {m: torch.cat(mod_z[m]) for m in mod_z}
        else:
            output["one_latent_space"] = True
        return output
