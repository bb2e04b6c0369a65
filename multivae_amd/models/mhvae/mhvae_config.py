from pydantic.dataclasses import dataclass

from ..base import BaseMultiVAEConfig


@dataclass
class MHVAEConfig(BaseMultiVAEConfig):
    """`multivae/models/mhvae/mhvae_config.py`: n_latent = the number of latent variables of the hierarchy, beta = the weight of
    the KL divergences.  The fields are the reference's, so a `model_config.json` written by either side loads in the other."""

    n_latent: int = 3
    beta: float = 1.0
