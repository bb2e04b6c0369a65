from pydantic.dataclasses import dataclass

from ...models.base.base_config import BaseConfig


@dataclass
class EvaluatorConfig(BaseConfig):
    """`multivae/metrics/base/evaluator_config.py`: batch_size = the batch size of the evaluation; wandb_path =
    'entity/project/run_id' of the wandb run that receives the metrics, None = no wandb logging."""

    batch_size: int = 512
    wandb_path: str = None
