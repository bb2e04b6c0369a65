from pydantic.dataclasses import dataclass

from ..base.evaluator_config import EvaluatorConfig


@dataclass
class CoherenceEvaluatorConfig(EvaluatorConfig):
    """`multivae/metrics/coherences/coherences_config.py`: num_classes of the classifiers; include_recon = count the
    reconstructions of the conditioning modalities too; nb_samples_for_joint = samples of the joint coherence;
    nb_samples_for_cross = generations per data point of the cross coherences; give_details_per_class = per-class metrics."""

    num_classes: int = 10
    include_recon: bool = False
    nb_samples_for_joint: int = 10000
    nb_samples_for_cross: int = 1
    give_details_per_class: bool = False
