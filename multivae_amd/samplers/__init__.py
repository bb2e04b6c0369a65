"""Samplers that generate from the latent space of a trained model (`multivae/samplers`): they are fitted on the training
embeddings and hand `model.decode` a ModelOutput like the one `encode` / `generate_from_prior` return.  GaussianMixtureSampler fits
a mixture by fused EM; MAFSampler and IAFSampler fit one normalizing flow per latent space (`flow_fit.fit_flow`: on the fused flow
kernels of csrc/maf.hip where they apply, else the torch flow modules) and sample by inverting it."""
from .base import BaseSampler, BaseSamplerConfig
from .flow_fit import fit_flow
from .gaussian_mixture import GaussianMixtureSampler, GaussianMixtureSamplerConfig
from .iaf_sampler import IAFSampler, IAFSamplerConfig
from .maf_sampler import MAFSampler, MAFSamplerConfig

__all__ = ["BaseSampler", "BaseSamplerConfig", "GaussianMixtureSampler", "GaussianMixtureSamplerConfig", "MAFSampler",
           "MAFSamplerConfig", "IAFSampler", "IAFSamplerConfig", "fit_flow"]
