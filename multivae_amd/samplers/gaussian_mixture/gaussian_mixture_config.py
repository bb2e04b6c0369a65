from pydantic.dataclasses import dataclass

from ..base import BaseSamplerConfig


@dataclass
class GaussianMixtureSamplerConfig(BaseSamplerConfig):
    """`multivae/samplers/gaussian_mixture/gaussian_mixture_config.py`: n_components = the number of Gaussians of the mixture."""

    n_components: int = 10
