"""Evaluators of a trained model (`multivae/metrics`): joint likelihoods, reconstruction error (SSIM / MSE, on the fused kernel of
csrc/ssim.hip), cross-modal / joint coherences and the k-means accuracy of the latent space (Clustering, on the batched k-means of
csrc/kmeans.hip), the Fréchet distance of generated data under user-supplied embedding networks (FIDEvaluator with
`custom_encoders`, on the streaming statistics of csrc/frechet.hip) and the PolyMNIST classifiers of the coherence examples
(classifiers.ClassifierPolyMNIST / load_mmnist_classifiers, one fused launch of csrc/clf.hip per batch in eval mode), and the
pictures of unconditional and conditional generations (Visualization: one launch of csrc/grid.hip per picture, PIL for the PNG).
FIDEvaluator's default embedding (the pretrained InceptionV3: torchvision and downloaded weights) is not built (SURVEY.md section
2.1)."""
from .base import Evaluator, EvaluatorConfig
from .classifiers import ClassifierPolyMNIST, load_mmnist_classifiers
from .coherences import CoherenceEvaluator, CoherenceEvaluatorConfig
from .fids import AdaptShapeFID, DeviceFrechet, FIDEvaluator, FIDEvaluatorConfig, frechet_distance
from .latent_clustering import Clustering, ClusteringConfig
from .likelihoods import LikelihoodsEvaluator, LikelihoodsEvaluatorConfig
from .reconstruction import Reconstruction, ReconstructionConfig
from .visualization import Visualization, VisualizationConfig

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
# Clustering, ClusteringConfig, Visualization, VisualizationConfig and the names of .fids and .classifiers are importable from here; __all__ (the star-import surface)
# stays the set that tests/test_metrics_host.py::test_package_surface pins.
