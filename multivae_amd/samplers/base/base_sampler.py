"""`multivae/samplers/base/base_sampler.py`: the surface every sampler shares."""
import logging
import os

import torch

from .base_sampler_config import BaseSamplerConfig

logger = logging.getLogger(__name__)


class BaseSampler:
    """Holds the model (put in eval mode and moved to the GPU when there is one) and the sampler's config; `fit` prepares the
    sampler from training data, `sample` draws latent codes, `save` writes `sampler_config.json`."""

    def __init__(self, model, sampler_config: BaseSamplerConfig = None):
        self.sampler_config = BaseSamplerConfig() if sampler_config is None else sampler_config
        self.model = model
        self.model.eval()
        self.is_fitted = False
        self.device = "cuda" if torch.cuda.is_available() else "cpu"
        self.model.device = self.device
        self.model.to(self.device)
        self.name = "BaseSampler"

    def fit(self, train_data, **kwargs):
        return

    def sample(self, n_samples: int = 1, batch_size: int = 500, return_gen: bool = True):
        raise NotImplementedError()

    def save(self, dir_path):
        logger.info("Saving model in %s.", dir_path)
        os.makedirs(dir_path, exist_ok=True)
        self.sampler_config.save_json(dir_path, "sampler_config")
