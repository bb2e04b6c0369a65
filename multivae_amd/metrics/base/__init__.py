from .evaluator_class import Evaluator
from .evaluator_config import EvaluatorConfig

__all__ = ["Evaluator", "EvaluatorConfig"]
