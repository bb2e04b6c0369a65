from typing import Dict, List, Literal, Union

from pydantic.dataclasses import dataclass

from ..base import BaseMultiVAEConfig


@dataclass
class NexusConfig(BaseMultiVAEConfig):
    """`multivae/models/nexus/nexus_config.py` (Vasco et al. 2022): modalities_specific_dim = the first-level latent size of
    every modality, bottom_betas / gammas = per-modality weights of the bottom KL / top-level likelihood, dropout_rate = the
    forced perceptual dropout probability, msg_dim = the size of the messages, top_beta = the weight of the joint KL, warmup =
    epochs of KL annealing, adapt_top_decoder_variance = modalities whose top-level scale is fitted to the batch."""

    modalities_specific_dim: Dict[str, int] = None
    bottom_betas: Union[Dict[str, float], None] = None
    dropout_rate: float = 0
    msg_dim: int = 10
    aggregator: Literal["mean"] = "mean"
    top_beta: float = 1
    gammas: Union[Dict[str, float], None] = None
    warmup: int = 20
    adapt_top_decoder_variance: Union[List[str], None] = None
