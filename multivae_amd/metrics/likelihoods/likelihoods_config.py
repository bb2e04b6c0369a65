from pydantic.dataclasses import dataclass

from ..base.evaluator_config import EvaluatorConfig


@dataclass
class LikelihoodsEvaluatorConfig(EvaluatorConfig):
    """`multivae/metrics/likelihoods/likelihoods_config.py`: num_samples = importance samples per data point; batch_size_k = how
    the reference batches them (the kernels take the sample axis whole); unified_implementation = False selects a model's
    `compute_joint_nll_paper` where it has one."""

    num_samples: int = 1000
    batch_size_k: int = 100
    unified_implementation: bool = True
