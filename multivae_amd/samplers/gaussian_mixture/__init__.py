from .gaussian_mixture_config import GaussianMixtureSamplerConfig
from .gaussian_mixture_sampler import DeviceGaussianMixture, GaussianMixtureSampler

__all__ = ["GaussianMixtureSampler", "GaussianMixtureSamplerConfig", "DeviceGaussianMixture"]
