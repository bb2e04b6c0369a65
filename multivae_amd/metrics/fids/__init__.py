from .fids import AdaptShapeFID, DeviceFrechet, FIDEvaluator, frechet_distance
from .fids_config import FIDEvaluatorConfig

__all__ = ["FIDEvaluator", "FIDEvaluatorConfig", "AdaptShapeFID", "DeviceFrechet", "frechet_distance"]
