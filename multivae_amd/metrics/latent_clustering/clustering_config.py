from typing import Literal

from pydantic.dataclasses import dataclass

from ..base.evaluator_config import EvaluatorConfig


@dataclass
class ClusteringConfig(EvaluatorConfig):
    """`multivae/metrics/latent_clustering/clustering_config.py`: clustering_method = 'kmeans' (the only one); n_clusters;
    number_of_runs = fits whose accuracies are averaged; num_samples_for_fit = stop embedding training batches once more than
    this many rows are embedded, None = the whole training set; use_mean = embed with the mean of the encoding distribution
    instead of a sample."""

    clustering_method: Literal["kmeans"] = "kmeans"
    n_clusters: int = 10
    number_of_runs: int = 20
    num_samples_for_fit: int = None
    use_mean: bool = True
