"""`multivae/metrics/latent_clustering/clustering_class.py`: k-means accuracy of the joint latent representation.

The reference, `number_of_runs` times: embeds the training set, copies it to the host, fits scikit-learn's KMeans there, maps each
cluster to the majority label of its training rows, and classifies the test embeddings on the host batch by batch.  Here the
embeddings and labels stay on the GPU, all runs are fitted together by `DeviceKMeans` (csrc/kmeans.hip), the training
contingency table and the test-side correct counts are accumulated by the assignment launch, and the host reads one number."""
import torch
from torch.utils.data import DataLoader

from ... import _lib
from ... import kernels as K
from ..._output import ModelOutput
from ...data.utils import set_inputs_to_device
from ..base.evaluator_class import Evaluator
from .clustering_config import ClusteringConfig
from .kmeans import DeviceKMeans


class Clustering(Evaluator):
    """Fits k-means on the training embeddings, then classifies the test embeddings with the clusters' majority labels and
    returns the accuracy, averaged over `number_of_runs` fits.  Only the joint representation (`model.encode(...).z`) is used.

    model: the model to evaluate; test_dataset: the data the accuracy is computed on (needs labels); train_dataset: the data the
    clusters are fitted on; output: folder of `metrics.log`; eval_config: a ClusteringConfig."""

    def __init__(self, model, test_dataset, train_dataset, output: str = None, eval_config=ClusteringConfig()) -> None:
        super().__init__(model, test_dataset, output, eval_config)
        self.num_samples_for_fit = eval_config.num_samples_for_fit
        self.n_fits = eval_config.number_of_runs
        self.use_mean = eval_config.use_mean
        self.n_clusters = eval_config.n_clusters
        self.train_dataset = train_dataset
        self.generator = None  # a device torch.Generator for the k-means++ seeding (tests); None = torch's global one
        self.max_iter = 300    # the reference's KMeans(max_iter=300)

    def _embed_train(self, mods):
        """(z [n,L] fp32, labels [n] int32 or None), on the device, from a shuffled loader.  `num_samples_for_fit` has its
        documented meaning: no further batch is taken once more than that many rows are embedded (the reference's counter never
        advances, so there the field has no effect)."""
        loader = DataLoader(self.train_dataset, self.batch_size, shuffle=True)
        zs, labels, n_samples, labelled = [], [], 0, True
        for inputs in loader:
            if self.num_samples_for_fit is not None and n_samples > self.num_samples_for_fit:
                break
            inputs = set_inputs_to_device(inputs, self.device)
            with torch.no_grad():
                zs.append(self.model.encode(inputs, mods, return_mean=self.use_mean).z)
            lab = getattr(inputs, "labels", None)
            if lab is None:
                labelled = False
            else:
                labels.append(lab.reshape(-1))
            n_samples += len(zs[-1])
        z = torch.cat(zs).float().contiguous()
        return z, (torch.cat(labels).to(device=z.device, dtype=torch.int32).contiguous() if labelled and labels else None)

    def fit_clustering(self, mods="all"):
        """Fits all `number_of_runs` k-means runs and votes their clusters' labels; no host copy of the embeddings.

        With use_mean=True the embeddings are the same for every run, so the training set is embedded ONCE per call and all runs
        are fitted together on it (the reference re-embeds inside its loop over the runs, to the same values).  With
        use_mean=False an embedding is a sample, so every run gets a fresh embedding of the training set, as in the reference,
        and is fitted on its own.  Training data without labels leaves every cluster mapped to its own index."""
        R, C = self.n_fits, self.n_clusters
        centers, tables, empties, self.n_classes = [], [], [], 1
        self.kmeans = []
        for _ in range(1 if self.use_mean else R):
            z, y = self._embed_train(mods)
            km = DeviceKMeans(C, n_runs=R if self.use_mean else 1, max_iter=self.max_iter).fit(z, generator=self.generator)
            self.kmeans.append(km)
            centers.append(km.cluster_centers_)
            empties.append(km.n_empty_)
            if y is not None:
                # one past the largest label, read once per embedding: the table needs its width
                self.n_classes = max(self.n_classes, int(y.max()) + 1)
            tables.append((z, y, km.cluster_centers_))
        self.train_z_, self.train_y_ = z, y  # the (last) training embedding, in the shuffled order init_indices_ refers to
        self.cluster_centers_ = torch.cat(centers)
        dev = self.cluster_centers_.device
        self.table = torch.zeros(R, C, self.n_classes + 1, dtype=torch.int64, device=dev)
        self.majority = torch.arange(C, dtype=torch.int32, device=dev).repeat(R, 1).contiguous()
        r = 0
        for z, y, c in tables:
            if y is not None:
                for g0 in range(0, c.shape[0], _lib.KMEANS_MAX_RUNS):
                    g1 = min(c.shape[0], g0 + _lib.KMEANS_MAX_RUNS)
                    K.kmeans_assign(z, c[g0:g1], y=y, n_classes=self.n_classes, table=self.table[r + g0:r + g1])
                    K.kmeans_vote(self.table[r + g0:r + g1], self.majority[r + g0:r + g1])
            r += c.shape[0]
        if int(torch.cat(empties).sum()) > 0:
            self.logger.warning("k-means met an empty cluster in %d of %d runs: such a cluster keeps its centre "
                                "(scikit-learn would move it to the row farthest from its centre)",
                                int((torch.cat(empties) > 0).sum()), R)

    def cluster_accuracy(self, mods="all"):
        """One pass over the test loader: per batch one `encode` and one assignment launch per group of 32 runs that adds the rows
        whose cluster's majority label is the true label to correct[r]; the mean over the runs of correct[r] / n is read once."""
        self.fit_clustering(mods)
        R = self.n_fits
        correct = torch.zeros(R, dtype=torch.int64, device=self.cluster_centers_.device)
        n_samples = 0
        for inputs in self.test_loader:
            if getattr(inputs, "labels", None) is None:
                raise AttributeError("The cluster accuracy can not be computed on a test dataset without labels")
            inputs = set_inputs_to_device(inputs, self.device)
            with torch.no_grad():
                z = self.model.encode(inputs, mods, return_mean=self.use_mean).z.float().contiguous()
            y = inputs.labels.reshape(-1).to(device=z.device, dtype=torch.int32).contiguous()
            for g0 in range(0, R, _lib.KMEANS_MAX_RUNS):
                g1 = min(R, g0 + _lib.KMEANS_MAX_RUNS)
                K.kmeans_assign(z, self.cluster_centers_[g0:g1], y=y, majority=self.majority[g0:g1], correct=correct[g0:g1])
            n_samples += len(z)
        self.correct_ = correct
        accuracy = float((correct.double() / n_samples).mean())
        self.metrics["cluster_accuracy"] = accuracy
        self.logger.info(f"Cluster accuracy is {accuracy}")
        return ModelOutput(cluster_accuracy=accuracy)

    def eval(self):
        output = self.cluster_accuracy("all")
        self.log_to_wandb()
        return output
