from .base import BaseTrainer, BaseTrainerConfig, TrainingCallback
from .flat import FlatParams, FusedAdam
from .graph import GraphedStep
from .multistage import MultistageTrainer, MultistageTrainerConfig

__all__ = ["BaseTrainer", "BaseTrainerConfig", "TrainingCallback", "FlatParams", "FusedAdam", "GraphedStep",
           "MultistageTrainer", "MultistageTrainerConfig"]
