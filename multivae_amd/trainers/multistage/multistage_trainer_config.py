from ..base import BaseTrainerConfig


class MultistageTrainerConfig(BaseTrainerConfig):
    """`multivae/trainers/multistage/multistage_trainer_config.py`: the fields of BaseTrainerConfig, for the trainer of the models
    that train in stages (TELBO)."""

    name_trainer = "TwoStepsTrainerConfig"
