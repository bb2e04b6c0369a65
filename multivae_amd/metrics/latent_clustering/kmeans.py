"""k-means on the device, several independent runs at once (csrc/kmeans.hip, kernels.kmeans_*).

The reference fits scikit-learn's `KMeans(n_clusters, max_iter=300)` on a host copy of the embeddings, once per run.  Here all runs
read the same device-resident rows and advance together: one Lloyd iteration of every run is two launches, convergence is
decided per run on the device, and the host reads the [R, 8] state block once every `check_every` iterations.

The iteration is scikit-learn's `_kmeans_single_lloyd` (labels from the centres, centres from the labels, stop on equal labels or
on a squared centre shift <= tol * mean of the column variances, then one more labelling).  Two stated deviations: the
k-means++ seeding draws ONE candidate per seed (scikit-learn tries 2 + log K and keeps the best), and a cluster without rows
keeps its centre (scikit-learn moves it to the row farthest from its own centre); `n_empty_` counts the latter."""
import torch

from ... import _lib
from ... import kernels as K


class DeviceKMeans:
    """`n_runs` k-means fits of `n_clusters` centres.  After `fit(x)`, each per run: cluster_centers_ [R,K,L] fp32, labels_ [R,N]
    int32, inertia_ [R] float64 (device tensors), n_iter_ [R], converged_ [R] (0 = stopped at max_iter, 1 = the labels repeated,
    2 = the centre shift fell to tol), n_empty_ [R] (clusters without rows, summed over the iterations) (host int64 tensors),
    init_indices_ [R,K] (the seed rows, None with init_centers)."""

    def __init__(self, n_clusters, n_runs=1, max_iter=300, tol=1e-4, check_every=8):
        self.n_clusters, self.n_runs, self.max_iter, self.tol = int(n_clusters), int(n_runs), int(max_iter), float(tol)
        self.check_every = max(1, int(check_every))
        if self.n_clusters < 1 or self.n_runs < 1:
            raise ValueError("n_clusters and n_runs must be at least 1")

    # ---- seeding --------------------------------------------------------------------------------------------------------
    def _seed(self, x, R, generator):
        """k-means++ for R runs at once: the first seed uniformly, every next one with probability proportional to the squared
        distance to the nearest seed so far.  One kmeans_assign (K = 1: the newest seed of every run) per added seed; the draw is
        an inverse CDF (fp64 cumsum, uniform * total, searchsorted, clamp), which needs no look at the values: an all-zero row of
        distances (fewer distinct rows than clusters) draws the last row instead of failing.  No host read."""
        N, dev = x.shape[0], x.device
        idx = torch.empty(R, self.n_clusters, dtype=torch.int64, device=dev)
        idx[:, 0] = torch.randint(N, (R,), generator=generator, device=dev)
        d2 = torch.full((R, N), float("inf"), dtype=torch.float32, device=dev)
        dnew = torch.empty(R, N, dtype=torch.float32, device=dev)
        for j in range(1, self.n_clusters):
            K.kmeans_assign(x, x[idx[:, j - 1]].unsqueeze(1).contiguous(), d2=dnew)
            torch.minimum(d2, dnew, out=d2)
            cdf = d2.double().cumsum(1)
            u = torch.rand(R, 1, generator=generator, device=dev, dtype=torch.float64) * cdf[:, -1:]
            idx[:, j] = torch.searchsorted(cdf, u, right=True).clamp_(max=N - 1)[:, 0]
        return idx

    # ---- fit ------------------------------------------------------------------------------------------------------------
    def fit(self, x, generator=None, init_indices=None, init_centers=None):
        """x [N,L] fp32 on the GPU.  init_indices [R,K]: rows of x as initial centres; init_centers [R,K,L]: the centres
        themselves; neither: k-means++ from `generator` (a device torch.Generator)."""
        _lib.require_gpu_tensor(x, "embeddings")
        x = x.detach().contiguous()
        N, L = x.shape
        R, C, dev = self.n_runs, self.n_clusters, x.device
        if N < 1:
            raise ValueError("k-means needs at least one row")
        if init_centers is not None:
            centers = torch.as_tensor(init_centers).to(device=dev, dtype=torch.float32).contiguous().clone()
            if tuple(centers.shape) != (R, C, L):
                raise ValueError(f"init_centers should have shape {(R, C, L)}, got {tuple(centers.shape)}")
            self.init_indices_ = None
        else:
            if init_indices is not None:
                idx = torch.as_tensor(init_indices).to(device=dev, dtype=torch.int64)
                if tuple(idx.shape) != (R, C):
                    raise ValueError(f"init_indices should have shape {(R, C)}, got {tuple(idx.shape)}")
            else:
                idx = torch.cat([self._seed(x, min(_lib.KMEANS_MAX_RUNS, R - r0), generator)
                                 for r0 in range(0, R, _lib.KMEANS_MAX_RUNS)])
            self.init_indices_ = idx
            centers = x[idx].contiguous()
        # scikit-learn's _tolerance: tol * mean of the column variances; fp64, on the device, never read back
        self.tol_ = x.double().var(dim=0, unbiased=False).mean() * self.tol
        labels = torch.full((R, N), -1, dtype=torch.int32, device=dev)
        inertia = torch.zeros(R, dtype=torch.float64, device=dev)
        S = _lib.KMEANS_STATE
        states = []
        for r0 in range(0, R, _lib.KMEANS_MAX_RUNS):  # more than 32 runs: groups of at most 32
            r1 = min(R, r0 + _lib.KMEANS_MAX_RUNS)
            c, lab = centers[r0:r1], labels[r0:r1]
            scratch, state = K.kmeans_scratch(L, C, r1 - r0, dev), K.kmeans_new_state(r1 - r0, dev)
            done, st = 0, None
            while done < self.max_iter:
                group = min(self.check_every, self.max_iter - done)
                for _ in range(group):
                    K.kmeans_step(x, self.tol_, c, lab, state, scratch)
                done += group
                st = state.cpu()  # the one host read per group
                if bool((st[:, S["converged"]] != 0).all()):
                    break
            # scikit-learn labels once more unless the labels repeated; for a run that did, this changes nothing
            K.kmeans_assign(x, c, scratch, labels=lab, inertia=inertia[r0:r1])
            states.append(state.cpu() if st is None else st)  # st is the last read: no step was enqueued after it
        st = torch.cat(states) if states else torch.zeros(0, _lib.KMEANS_STATE_DOUBLES, dtype=torch.float64)
        self.cluster_centers_, self.labels_, self.inertia_ = centers, labels, inertia
        self.n_iter_ = st[:, S["iter"]].long()
        self.converged_ = st[:, S["converged"]].long()
        self.n_empty_ = st[:, S["empty"]].long()
        return self

    def predict(self, x):
        """labels [R, n] int32 of the rows of x under every run's centres."""
        _lib.require_gpu_tensor(x, "embeddings")
        x = x.detach().contiguous()
        R = self.cluster_centers_.shape[0]
        labels = torch.empty(R, x.shape[0], dtype=torch.int32, device=x.device)
        for r0 in range(0, R, _lib.KMEANS_MAX_RUNS):
            r1 = min(R, r0 + _lib.KMEANS_MAX_RUNS)
            K.kmeans_assign(x, self.cluster_centers_[r0:r1], labels=labels[r0:r1])
        return labels
