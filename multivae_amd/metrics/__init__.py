"""Evaluators of a trained model (`multivae/metrics`): joint likelihoods, reconstruction error (SSIM / MSE, on the fused kernel of
csrc/ssim.hip) and cross-modal / joint coherences.  FIDEvaluator (needs Inception weights), Visualization (torchvision, PIL),
Clustering and ClassifierPolyMNIST are not built."""
from .base import Evaluator, EvaluatorConfig
from .coherences import CoherenceEvaluator, CoherenceEvaluatorConfig
from .likelihoods import LikelihoodsEvaluator, LikelihoodsEvaluatorConfig
from .reconstruction import Reconstruction, ReconstructionConfig

__all__ = [
    "Evaluator",
    "EvaluatorConfig",
    "LikelihoodsEvaluator",
    "LikelihoodsEvaluatorConfig",
    "Reconstruction",
    "ReconstructionConfig",
    "CoherenceEvaluator",
    "CoherenceEvaluatorConfig",
]
