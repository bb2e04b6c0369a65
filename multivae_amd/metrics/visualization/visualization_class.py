"""`multivae/metrics/visualization/visualization_class.py`: pictures of unconditional and conditional generations.

The reference adapts every modality (a cat and a pad each), concatenates them, lets torchvision's make_grid copy tile after tile
and quantises the grid in five more tensor operations.  Here the decoders' outputs go as they are to kernels.image_grid: one launch
of csrc/grid.hip writes the uint8 picture, one host read fetches it and PIL encodes the PNG."""
import os
from typing import Union

import torch
from PIL import Image
from torch.utils.data import DataLoader

from ... import kernels
from ..._output import ModelOutput
from ...data.utils import set_inputs_to_device
from ..base.evaluator_class import Evaluator
from .visualize_config import VisualizationConfig


class Visualization(Evaluator):
    """Pictures of the model's generations: `unconditional_samples` (a row of n_samples per modality),
    `conditional_samples_subset(subset, gen_mod)` (a row of the n_data_cond originals of each conditioning modality, then n_samples
    rows per generated modality) and `reconstruction(modality)`.  Each returns a PIL.Image and, with an `output` directory, writes
    `unconditional.png` / `conditional_from_subset_{subset}.png` there.  A dataset's `transform_for_plotting(tensor, modality)` is
    applied to every tensor first, as in the reference."""

    def __init__(self, model, test_dataset, output: str = None, eval_config=VisualizationConfig(), sampler=None) -> None:
        super().__init__(model, test_dataset, output, eval_config, sampler)
        self.n_samples = eval_config.n_samples
        self.n_data_cond = eval_config.n_data_cond

    def _for_plotting(self, tensor, modality):
        if hasattr(self.test_dataset, "transform_for_plotting"):
            return self.test_dataset.transform_for_plotting(tensor, modality)
        return tensor

    def _picture(self, tensors, nrow, name):
        """The tiles of `tensors` in order, `nrow` to a row, as a PIL image: saved as `name`.png and logged to wandb as `name`."""
        _, image = kernels.image_grid(tensors, nrow=nrow, want=("uint8",))
        picture = Image.fromarray(image.cpu().numpy())  # the one host read
        if self.output is not None:
            picture.save(os.path.join(self.output, f"{name}.png"))
        return picture

    def _log_picture(self, key, picture):
        if self.wandb_run is not None:
            import wandb

            self.wandb_run.log({key: wandb.Image(picture)})

    def unconditional_samples(self, **kwargs):
        device = kwargs.pop("device", "cuda" if torch.cuda.is_available() else "cpu")
        if self.sampler is None:
            samples = self.model.generate_from_prior(self.n_samples)
        else:
            samples = self.sampler.sample(self.n_samples)
        samples = set_inputs_to_device(samples, device=device)
        recon = self.model.decode(samples)
        picture = self._picture([self._for_plotting(recon[m], m) for m in recon], self.n_samples, "unconditional")
        self._log_picture("unconditional_generation", picture)
        return picture

    def conditional_samples_subset(self, subset: list, gen_mod: Union[list, str] = "all"):
        data = next(iter(DataLoader(self.test_dataset, batch_size=self.n_data_cond, shuffle=True)))
        data = set_inputs_to_device(data, self.device)
        recon = self.model.predict(data, cond_mod=subset, gen_mod=gen_mod, N=self.n_samples, flatten=True, ignore_incomplete=True)
        # the originals of the conditioning modalities first, then what was generated
        tensors = [self._for_plotting(data.data[m], m) for m in subset] + [self._for_plotting(recon[m], m) for m in recon]
        name = f"conditional_from_subset_{subset}"
        picture = self._picture(tensors, self.n_data_cond, name)
        self._log_picture(name, picture)
        return picture

    def reconstruction(self, modality: str, **kwargs):
        return self.conditional_samples_subset([modality], gen_mod=modality)

    def eval(self):
        image = self.unconditional_samples()
        return ModelOutput(unconditional_generation=image)
