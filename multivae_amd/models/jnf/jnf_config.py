from pydantic.dataclasses import dataclass

from ..joint_models.joint_model_config import BaseJointModelConfig


@dataclass
class JNFConfig(BaseJointModelConfig):
    """`multivae/models/jnf/jnf_config.py`: `warmup` epochs train the joint encoder and the decoders on the joint ELBO (its KL
    weighted by `beta`), the epochs after it the unimodal encoders and their flows against the frozen rest."""

    warmup: int = 10
    beta: float = 1
