"""`multivae/metrics/likelihoods/likelihoods.py`: the joint negative log-likelihood of a test set."""
from ..._output import ModelOutput
from ...data.utils import set_inputs_to_device
from ..base.evaluator_class import Evaluator
from .likelihoods_config import LikelihoodsEvaluatorConfig


class LikelihoodsEvaluator(Evaluator):
    """Sums the model's own `compute_joint_nll` (kernels.joint_nll: mvk_recon_nll_fwd rows, mvk_iwae_logw, mvk_iwae_reduce) over
    the batches.  The running sum is a device tensor; the one host read is the log line at the end."""

    def __init__(self, model, test_dataset, output=None, eval_config=LikelihoodsEvaluatorConfig()) -> None:
        super().__init__(model, test_dataset, output, eval_config)
        self.num_samples = eval_config.num_samples
        self.batch_size_k = eval_config.batch_size_k
        self.unified = eval_config.unified_implementation

    def eval(self):
        self.joint_nll()
        self.log_to_wandb()
        return ModelOutput(**self.metrics)

    def joint_nll(self):
        paper = not (self.unified or not hasattr(self.model, "compute_joint_nll_paper"))
        if paper:
            self.logger.info("Using the paper version of the joint nll.")
        estimate = self.model.compute_joint_nll_paper if paper else self.model.compute_joint_nll
        ll = 0
        for batch in self.test_loader:
            batch = set_inputs_to_device(batch, self.device)
            ll += estimate(batch, self.num_samples, self.batch_size_k)
        joint_nll = ll / len(self.test_loader.dataset)
        self.logger.info(f"Mean Joint likelihood : {str(joint_nll)}")
        self.metrics["joint_likelihood"] = joint_nll
        return joint_nll

    def joint_nll_from_subset(self, subset):
        """The joint likelihood with a subset posterior as the importance distribution; None for a model without
        `_compute_joint_nll_from_subset_encoding` (the MoPoE has it)."""
        if not hasattr(self.model, "_compute_joint_nll_from_subset_encoding"):
            return None
        ll = 0
        for batch in self.test_loader:
            batch = set_inputs_to_device(batch, self.device)
            ll += self.model._compute_joint_nll_from_subset_encoding(subset, batch, self.num_samples, self.batch_size_k)
        joint_nll = ll / self.n_data
        self.logger.info("Joint likelihood from subset %s", str(joint_nll))
        self.metrics[f"Joint likelihood from subset {subset}"] = joint_nll
        return joint_nll
