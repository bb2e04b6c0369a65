from pydantic.dataclasses import dataclass

from ..base import BaseSamplerConfig


@dataclass
class MAFSamplerConfig(BaseSamplerConfig):
    """`multivae/samplers/maf_sampler/maf_sampler_config.py`: the MADE blocks of every flow, the hidden layers of a MADE and their
    width; include_batch_norm=True is refused (batch-norm flows are not built here)."""

    n_made_blocks: int = 2
    n_hidden_in_made: int = 3
    hidden_size: int = 128
    include_batch_norm: bool = False
