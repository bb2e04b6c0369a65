"""`multivae/metrics/coherences/coherences.py`: do generated modalities carry the label of what they were generated from?

The reference keeps one torchmetrics `MulticlassAccuracy(num_classes, average=None)` per generated modality.  Its per-class accuracy
is fixed here from the definition (torchmetrics was not at hand): correct_c / count_c over everything accumulated, c being the
TRUE class, and 0 for a class that never occurs.  The counts are [num_classes + 1, 2] integers on the device, read once per
subset.  A classifier is a user module in general, and then the counts are updated with torch ops on its logits; where it is
exactly a `ClassifierPolyMNIST` (num_classes = 10, CUDA fp32 [n,3,28,28] generations) the fused launch of csrc/clf.hip classifies
the batch and adds straight into the counts (cross coherences) or writes the argmax (joint coherence): one launch per generated
modality and batch, no logits tensor.  Both paths give the same counts."""
from itertools import combinations
from typing import Dict, List, Optional

import numpy as np
import torch

from ..._output import ModelOutput
from ...data.utils import set_inputs_to_device
from ..base.evaluator_class import Evaluator
from ..classifiers.mmnist import ClassifierPolyMNIST
from .coherences_config import CoherenceEvaluatorConfig


class ClassCounts:
    """counts[c] = (correct predictions among the rows of true class c, rows of true class c), accumulated on the device."""

    def __init__(self, num_classes, device):
        self.num_classes = num_classes
        # one more row than classes: labels outside [0, num_classes) are counted there and reported nowhere
        self.counts = torch.zeros(num_classes + 1, 2, dtype=torch.int64, device=device)

    def update(self, logits, labels):
        """logits [n, num_classes], labels [n].  A bincount of 2 label + correct, written as a
        scatter-add into the running counts so that no size is read back from the device."""
        pred = torch.argmax(logits, dim=1)
        labels = labels.to(pred.device).long().reshape(-1)
        correct = (pred.reshape(-1) == labels).long()
        inside = (labels >= 0) & (labels < self.num_classes)
        row = torch.where(inside, labels, torch.full_like(labels, self.num_classes))
        flat = self.counts.view(-1)
        flat.scatter_add_(0, 2 * row, correct)
        flat.scatter_add_(0, 2 * row + 1, torch.ones_like(row))

    def compute(self):
        """Per-class accuracy [num_classes], float32: correct_c / count_c, 0 where count_c is 0."""
        c = self.counts[: self.num_classes].to(torch.float32)
        return torch.where(c[:, 1] > 0, c[:, 0] / c[:, 1].clamp(min=1), torch.zeros_like(c[:, 0]))


class CoherenceEvaluator(Evaluator):
    """Cross-modal coherences (classify what `predict` generates from every subset of the modalities) and the joint coherence
    (generate every modality from one latent code, drawn from the prior or from a fitted sampler, and count the codes on whose
    label all classifiers agree)."""

    def __init__(self, model, classifiers: Dict[str, torch.nn.Module], test_dataset, output: Optional[str] = None,
                 eval_config=CoherenceEvaluatorConfig(), sampler=None) -> None:
        super().__init__(model, test_dataset, output, eval_config, sampler)
        self.clfs = classifiers
        self.include_recon = eval_config.include_recon
        self.nb_samples_for_joint = eval_config.nb_samples_for_joint
        self.nb_samples_for_cross = eval_config.nb_samples_for_cross
        self.num_classes = eval_config.num_classes
        self.give_details_per_classes = eval_config.give_details_per_class
        assert self.num_classes is not None, "Please provide the number of classes"
        for k in self.clfs:
            self.clfs[k] = self.clfs[k].to(self.device).eval()

    def _fused(self, m, x):
        """The modality's classifier when the fused launch can classify x, else None (the general path)."""
        clf = self.clfs[m]
        if type(clf) is ClassifierPolyMNIST and self.num_classes == 10 and clf.kernel_ok(x):
            return clf
        return None

    def cross_coherences(self):
        """Every coherence from a subset of the modalities to another modality; returns the means and standard deviations over
        the subsets of each size."""
        modalities = list(self.model.encoders.keys())
        accs, accs_per_class = [], []
        for n in range(1, self.model.n_modalities):
            accs.append([])
            accs_per_class.append([])
            for s in combinations(modalities, n):
                subset_dict, mean_acc, mean_acc_per_class = self.coherence_from_subset(list(s), return_accuracies_per_labels=True)
                self.metrics.update(subset_dict)
                accs[-1].append(mean_acc)
                accs_per_class[-1].append(mean_acc_per_class)
        mean_accs = [np.mean(l) for l in accs]
        std_accs = [np.std(l) for l in accs]
        mean_accs_per_class = [np.mean(np.stack(l), axis=0) for l in accs_per_class]
        for i, (m, s) in enumerate(zip(mean_accs, std_accs)):
            self.logger.info("Conditional accuracies for %s modalities : %s +- %s", i + 1, m, s)
            self.metrics.update({f"mean_coherence_{i + 1}": m, f"std_coherence_{i + 1}": s})
            if self.give_details_per_classes:
                for c in range(self.num_classes):
                    self.logger.info("Conditional accuracies for %s modalities in class %s: %s", i + 1, c, mean_accs_per_class[i][c])
                    self.metrics.update({f"mean_coherence_{i + 1}_class_{c}": mean_accs_per_class[i][c]})
        return mean_accs, std_accs

    def coherence_from_subset(self, subset: List[str], return_accuracies_per_labels=False):
        """The coherences of every modality generated from `subset` (those outside it, or all with include_recon): the dict
        {f"{subset}_to_{m}": accuracy}, their mean, and with return_accuracies_per_labels the per-class accuracies averaged
        over the generated modalities."""
        pred_mods = [m for m in self.model.encoders if (m not in subset) or self.include_recon]
        subset_name = "_".join(subset)
        counts = {m: ClassCounts(self.num_classes, self.device) for m in pred_mods}
        for batch in self.test_loader:
            if not hasattr(batch, "labels"):
                raise AttributeError("Cross-modal coherence can not be computed  on a dataset without labels")
            elif batch.labels is None:
                raise AttributeError("Cross-modal coherence can not be computed  on a dataset without labels, but the provided "
                                     "dataset has None instead of tensor labels")
            batch = set_inputs_to_device(batch, device=self.device)
            with torch.no_grad():
                output = self.model.predict(batch, list(subset), pred_mods, N=self.nb_samples_for_cross, flatten=True)
                labels = batch.labels
                if self.nb_samples_for_cross > 1:  # the generations are stacked sample-major: [N * batch, ...]
                    labels = torch.stack([labels] * self.nb_samples_for_cross, dim=0).reshape(-1, *labels.shape[1:])
                flat_labels = None
                for pred_m in pred_mods:
                    clf = self._fused(pred_m, output[pred_m])
                    if clf is None:
                        counts[pred_m].update(self.clfs[pred_m](output[pred_m]), labels)
                        continue
                    if flat_labels is None:  # the kernel stacks the batch's labels itself: row i has labels[i % rows]
                        flat_labels = batch.labels.to(self.device).long().reshape(-1).contiguous()
                    clf.classify(output[pred_m], labels=flat_labels, counts=counts[pred_m].counts)
        acc_per_class = {f"{subset_name}_to_{m}": counts[m].compute().cpu() for m in counts}
        acc = {m: acc_per_class[m].mean() for m in acc_per_class}
        self.logger.info("Subset %s accuracies ", subset)
        self.logger.info(str(acc))
        mean_pair_acc = np.mean([float(v) for v in acc.values()])
        self.logger.info("Mean subset %s accuracies : %s", subset, str(mean_pair_acc))
        mean_acc_per_class = np.mean(np.stack([v.numpy() for v in acc_per_class.values()]), axis=0)
        if return_accuracies_per_labels:
            return acc, mean_pair_acc, mean_acc_per_class
        return acc, mean_pair_acc

    def joint_coherence(self):
        """The share of latent codes, drawn from the fitted sampler when one was given and from the prior otherwise, whose
        generations get the same label from every modality's classifier: a 0-d tensor."""
        same = torch.zeros((), dtype=torch.int64, device=self.device)
        samples_to_generate = self.nb_samples_for_joint
        while samples_to_generate > 0:
            batch_samples = min(self.batch_size, samples_to_generate)
            if self.sampler is None:
                output_prior = self.model.generate_from_prior(batch_samples)
            else:
                output_prior = self.sampler.sample(batch_samples)
            # generate_from_prior(1) returns one code without a batch axis: the last, one-sample batch gets it back
            output_prior.z = output_prior.z.to(self.device).reshape(batch_samples, -1)
            if not output_prior.one_latent_space:
                for m in output_prior.modalities_z:
                    output_prior.modalities_z[m] = output_prior.modalities_z[m].to(self.device).reshape(batch_samples, -1)
            output_decode = self.model.decode(output_prior)
            with torch.no_grad():
                labels = []
                for m in output_decode.keys():
                    clf = self._fused(m, output_decode[m])
                    if clf is None:
                        labels.append(torch.argmax(self.clfs[m](output_decode[m]), dim=1))
                    else:
                        labels.append(clf.classify(output_decode[m]).long())
            same += torch.all(torch.stack([l == labels[0] for l in labels]), dim=0).sum()
            samples_to_generate -= batch_samples
        joint_coherence = same.float() / self.nb_samples_for_joint
        sampler_name = "prior" if self.sampler is None else self.sampler.name
        self.logger.info("Joint coherence with sampler %s: %s", sampler_name, joint_coherence)
        self.metrics.update({f"joint_coherence_{sampler_name}": joint_coherence})
        return joint_coherence

    def eval(self):
        """All cross-modal coherences and the joint coherence."""
        self.cross_coherences()
        self.joint_coherence()
        self.log_to_wandb()
        return ModelOutput(**self.metrics)
