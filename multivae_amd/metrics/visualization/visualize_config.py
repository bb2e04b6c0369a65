from pydantic.dataclasses import dataclass

from ..base.evaluator_config import EvaluatorConfig


@dataclass
class VisualizationConfig(EvaluatorConfig):
    """`multivae/metrics/visualization/visualize_config.py`: n_samples = the samples generated per modality (and per data point
    in a conditional generation); n_data_cond = the data points a conditional generation starts from."""

    batch_size: int = 20
    n_samples: int = 5
    n_data_cond: int = 5
