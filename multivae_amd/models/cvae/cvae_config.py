from dataclasses import field
from typing import List, Literal, Optional

from pydantic.dataclasses import dataclass

from ..base import BaseConfig


@dataclass
class CVAEConfig(BaseConfig):
    """`multivae/models/cvae/cvae_config.py` (Sohn et al. 2015): main_modality = the modality that is reconstructed,
    conditioning_modalities = the ones the encoder, the prior and the decoder are conditioned on, beta = the weight of the KL
    to the (learned) prior, decoder_dist / decoder_dist_params = the likelihood of the main modality (bernoulli: logits)."""

    conditioning_modalities: List[str]
    main_modality: str
    input_dims: Optional[dict] = None
    latent_dim: int = 10
    beta: float = 1.0
    decoder_dist: Literal["normal", "laplace", "bernoulli", "categorical"] = "normal"
    decoder_dist_params: dict = field(default_factory=lambda: {})
    custom_architectures: list = field(default_factory=lambda: [])

    def __post_init__(self):
        super().__post_init__()
        if self.input_dims is not None:
            self.input_dims = {k: tuple(self.input_dims[k]) for k in self.input_dims}
