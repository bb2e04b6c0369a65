from pydantic.dataclasses import dataclass

from ..base.evaluator_config import EvaluatorConfig


@dataclass
class FIDEvaluatorConfig(EvaluatorConfig):
    """`multivae/metrics/fids/fids_config.py`: inception_weights_path = where the state dict of the pretrained InceptionV3 lies;
    dims_inception = the width of the Inception features (the pool_3 layer: 2048).  Both belong to the default Inception path,
    which is not built here (FIDEvaluator needs `custom_encoders`); they are kept so that a reference config round-trips."""

    inception_weights_path: str = "../fid_model/model.pt"
    dims_inception: int = 2048
