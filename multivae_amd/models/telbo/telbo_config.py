from typing import Union

from pydantic.dataclasses import dataclass

from ..joint_models.joint_model_config import BaseJointModelConfig


@dataclass
class TELBOConfig(BaseJointModelConfig):
    """`multivae/models/telbo/telbo_config.py`: `warmup` epochs train the joint encoder and the decoders, the epochs after it the
    unimodal encoders against the frozen rest.  lambda_factors / gamma_factors weight the reconstructions of the joint / the
    unimodal ELBOs; None takes the rescale factors (all ones without `uses_likelihood_rescaling`, which defaults to True here)."""

    warmup: int = 10
    lambda_factors: Union[dict, None] = None
    gamma_factors: Union[dict, None] = None
    uses_likelihood_rescaling: bool = True
