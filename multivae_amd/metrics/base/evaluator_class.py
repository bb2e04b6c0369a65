"""`multivae/metrics/base/evaluator_class.py`: what every evaluator shares."""
import datetime
import logging
from pathlib import Path

import torch
from torch.utils.data import DataLoader

from .evaluator_config import EvaluatorConfig


class Evaluator:
    """Holds the model (in eval mode, on the GPU when there is one), the test loader, a logger that also writes `metrics.log`
    into `output`, the optional wandb run and the optional fitted sampler; `metrics` collects what the evaluator computed."""

    def __init__(self, model, test_dataset, output: str = None, eval_config=EvaluatorConfig(), sampler=None) -> None:
        self.device = "cuda" if torch.cuda.is_available() else "cpu"
        self.model = model.to(self.device).eval()
        model.device = self.device
        self.n_data = len(test_dataset)
        self.batch_size = eval_config.batch_size
        self.test_dataset = test_dataset
        self.test_loader = DataLoader(test_dataset, batch_size=eval_config.batch_size)
        if output is not None:
            Path(output).mkdir(parents=True, exist_ok=True)
        self.output = output
        self.set_logger(output)
        self.set_wandb(eval_config.wandb_path)
        self.metrics = {}
        self.sampler = sampler
        if self.sampler is not None and not sampler.is_fitted:
            raise AttributeError("The provided sampler is not fitted."
                                 "Please fit the sampler before using it in the evaluator module.")

    def set_logger(self, output):
        evaluator_id = str(datetime.datetime.now())[0:19].replace(" ", "_").replace(":", "-")
        logger = logging.getLogger(evaluator_id)
        logger.setLevel(logging.INFO)
        self.console_handler = logging.StreamHandler()
        logger.addHandler(self.console_handler)
        if output is not None:
            self.file_handler = logging.FileHandler(str(output) + "/metrics.log")
            logger.addHandler(self.file_handler)
        self.logger = logger

    def set_wandb(self, wandb_path):
        if wandb_path is None:
            self.wandb_run = None
            return
        entity, project, run_id = tuple(wandb_path.split("/"))
        try:
            import wandb
        except ImportError:
            raise ModuleNotFoundError("You provided a wandb_path, but `wandb` package is not installed. Run `pip install wandb`")
        self.wandb_run = wandb.init(entity=entity, project=project, id=run_id, resume="allow", reinit=True)

    def log_to_wandb(self):
        if self.wandb_run is not None:
            self.wandb_run.log(self.metrics)

    def finish(self):
        """Removes the handlers and finishes the wandb run."""
        self.logger.removeHandler(self.console_handler)
        if hasattr(self, "file_handler"):
            self.logger.removeHandler(self.file_handler)
            self.file_handler.close()
        if self.wandb_run is not None:
            self.wandb_run.finish()
