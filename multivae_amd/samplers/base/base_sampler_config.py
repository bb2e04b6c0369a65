from pydantic.dataclasses import dataclass

from ...models.base.base_config import BaseConfig


@dataclass
class BaseSamplerConfig(BaseConfig):
    """`multivae/samplers/base/base_sampler_config.py`: no field of its own; `name` is the class name, as in every config."""
