"""Samplers that generate from the latent space of a trained model (`multivae/samplers`): they are fitted on the training
embeddings and hand `model.decode` a ModelOutput like the one `encode` / `generate_from_prior` return.  The flow samplers
(MAFSampler, IAFSampler) need pythae's flow models and trainers and are not built; neither is JNF, the
one model that needs the same flows (TELBO and the multistage trainer it shares with JNF are: `multivae_amd.models.TELBO`,
`multivae_amd.trainers.MultistageTrainer`)."""
from .base import BaseSampler, BaseSamplerConfig
from .gaussian_mixture import GaussianMixtureSampler, GaussianMixtureSamplerConfig

__all__ = ["BaseSampler", "BaseSamplerConfig", "GaussianMixtureSampler", "GaussianMixtureSamplerConfig"]
