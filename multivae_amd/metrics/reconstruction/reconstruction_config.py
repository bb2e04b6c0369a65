from typing import Literal

from pydantic.dataclasses import dataclass

from ..base.evaluator_config import EvaluatorConfig


@dataclass
class ReconstructionConfig(EvaluatorConfig):
    """`multivae/metrics/reconstruction/reconstruction_config.py`: metric = 'SSIM' (images only) or 'MSE'."""

    metric: Literal["SSIM", "MSE"] = "SSIM"
