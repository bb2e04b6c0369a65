"""`multivae/metrics/reconstruction/reconstruction.py`: how well a subset of modalities reconstructs itself, as SSIM or MSE.

The reference hands the SSIM to torchmetrics' StructuralSimilarityIndexMeasure (one metric object per call, updated once per
batch and modality) and sums the squared differences in torch.  Here both come from csrc/ssim.hip: an update is mvk_ssim_range,
mvk_ssim_rows and mvk_ssim_accumulate on a device block {ssim_sum, sse_sum, rows}, and nothing is read back before the end."""
from typing import List

from ... import _lib, kernels
from ..._output import ModelOutput
from ...data.utils import set_inputs_to_device
from ..base.evaluator_class import Evaluator
from .reconstruction_config import ReconstructionConfig


class Reconstruction(Evaluator):
    """SSIM = (sum of per-image SSIM over every update) / (images over every update), the data range taken per update; MSE = (sum
    of squared differences) / (sum over updates of batch rows), the reference's normalisation.  One update is one (batch,
    modality) pair and one accumulator spans all modalities of the subset."""

    def __init__(self, model, test_dataset, output=None, eval_config=ReconstructionConfig()) -> None:
        super().__init__(model, test_dataset, output, eval_config)
        self.metric_name = eval_config.metric

    def _update(self, acc, preds, target, scratch):
        preds, target = preds.detach().float().contiguous(), target.detach().float().contiguous()
        if self.metric_name == "MSE":
            kernels.ssim_accumulate(acc, kernels.sse_rows(preds, target))
            return
        key = tuple(preds.shape)
        if key not in scratch:
            scratch[key] = kernels.ssim_scratch(*key, preds.device)
        ssim, sse = kernels.ssim_rows(preds, target, scratch[key])
        kernels.ssim_accumulate(acc, sse, ssim)

    def _check_image(self, preds, target, mod):
        if preds.shape != target.shape:
            raise ValueError(f"modality {mod}: the reconstruction has shape {tuple(preds.shape)}, the data {tuple(target.shape)}")
        if self.metric_name == "SSIM" and (preds.dim() != 4 or preds.shape[-2] < 11 or preds.shape[-1] < 11):
            raise ValueError(f"SSIM needs images [batch, channels, height >= 11, width >= 11]; modality {mod} has shape "
                             f"{tuple(preds.shape)}. Use metric='MSE' for it.")

    def reconstruction_from_subset(self, subset: List[str]):
        """The reconstruction metric of the modalities of `subset`, each reconstructed from the whole subset: a 0-d tensor."""
        if self.metric_name not in ("SSIM", "MSE"):
            raise AttributeError("Unrecognized metric name for reconstruction error. ")
        acc, scratch = None, {}
        for batch in self.test_loader:
            batch = set_inputs_to_device(batch, self.device)
            output = self.model.predict(batch, list(subset), list(subset))
            for mod in subset:
                preds, target = output[mod], batch.data[mod]
                self._check_image(preds, target, mod)
                if acc is None:
                    acc = kernels.ssim_new_acc(preds.device)
                self._update(acc, preds, target, scratch)
        total = acc[_lib.SSIM_ACC["ssim" if self.metric_name == "SSIM" else "sse"]]
        mean_recon_error = (total / acc[_lib.SSIM_ACC["rows"]]).float()
        self.logger.info(f"Subset {subset} reconstruction : {mean_recon_error} ")
        self.metrics.update({f"{subset} reconstruction error ({self.metric_name})": mean_recon_error})
        return mean_recon_error

    def eval(self):
        """The joint subset, then every modality on its own."""
        self.reconstruction_from_subset(list(self.model.encoders.keys()))
        for mod in self.model.encoders.keys():
            self.reconstruction_from_subset([mod])
        self.log_to_wandb()
        return ModelOutput(**self.metrics)
