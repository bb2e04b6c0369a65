"""Timing of the batched device k-means (csrc/kmeans.hip) against what the package offered before it: sequential
`DeviceGaussianMixture._kmeans` fits (two launches and one host read per Lloyd round, one fit at a time) on the SAME rows and seeds.

    python tools/kmeans_probe.py [--rows 60000] [--latent 20] [--clusters 10] [--runs 20] [--repeat 3] [--out FILE.json]

Timed, each after a warm-up of the same shape, host clock around work that ends in a device synchronise, the median of `--repeat`:
  * batched_fit_s: one `DeviceKMeans(K, n_runs=R).fit(x, init_indices=seeds)` (Lloyd from given seeds, tol 1e-4 as the evaluator runs
    it) and batched_strict_fit_s, the same with tol = 0 (stops like the baseline, on repeated labels only);
  * batched_seeded_fit_s: the same with the default k-means++ seeding of all runs;
  * sequential_fit_s: R times `DeviceGaussianMixture._kmeans` from the same seeds (it stops on repeated labels, at most 100 rounds);
  * step_s: one mvk_kmeans_step of R runs (device events, state never converging);
  * eval_s: `Clustering.eval()` on a stand-in model whose encoder is the identity on stored embeddings (the evaluator's own cost:
    the two loaders, the fit, the table, the vote, the test pass);
  * sklearn_fit_s (if scikit-learn is there, for orientation only): R host fits `KMeans(init=rows, n_init=1)`.
C-ABI calls are counted by wrapping `kernels.call`; host reads are counted from the loops' structure (one per `check_every` group
for the batched fit, one per round for the sequential one).  Needs a GPU; prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def blobs(N, L, K, seed):
    g = np.random.default_rng(seed)
    mu = 2.0 * g.standard_normal((K, L))
    blob = g.integers(0, K, N)
    return (mu[blob] + g.standard_normal((N, L))).astype(np.float32), blob


def timed(fn, repeat):
    fn()  # warm-up of the same shape
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), out


class IdentityModel(torch.nn.Module):
    """`encode` returns the stored embedding of the batch: the evaluator's time without a network's."""

    def encode(self, inputs, cond_mod="all", N=1, return_mean=False, **kwargs):
        from multivae_amd._output import ModelOutput

        return ModelOutput(z=inputs.data["z"], one_latent_space=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=60000)
    ap.add_argument("--latent", type=int, default=20)
    ap.add_argument("--clusters", type=int, default=10)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kmeans_probe needs a GPU: a CPU run measures nothing"
    from multivae_amd import kernels as K
    from multivae_amd.data.datasets.base import MultimodalBaseDataset
    from multivae_amd.metrics import Clustering, ClusteringConfig
    from multivae_amd.metrics.latent_clustering import DeviceKMeans
    from multivae_amd.samplers.gaussian_mixture import DeviceGaussianMixture

    dev = torch.device("cuda:0")
    N, L, C, R = a.rows, a.latent, a.clusters, a.runs
    X, blob = blobs(N + N // 6, L, C, 0)  # the evaluator's test rows come from the same blobs as the training rows
    X, blob, Xt, blob_t = X[:N], blob[:N], X[N:], blob[N:]
    x = torch.from_numpy(X).to(dev)
    seeds = np.stack([np.random.default_rng((0, r)).choice(N, C, replace=False) for r in range(R)])
    calls = [0]
    plain_call = K.call

    def counting_call(name, *args):
        calls[0] += 1
        return plain_call(name, *args)

    K.call = counting_call

    def counted(fn):
        calls[0] = 0
        out = fn()
        return calls[0], out

    # ---- the batched fit --------------------------------------------------------------------------------------------------
    fit = lambda tol: DeviceKMeans(C, n_runs=R, tol=tol).fit(x, init_indices=seeds)
    t_batched, km = timed(lambda: fit(1e-4), a.repeat)
    t_strict, km0 = timed(lambda: fit(0.0), a.repeat)
    n_calls, _ = counted(lambda: fit(1e-4))
    t_seeded, kms = timed(lambda: DeviceKMeans(C, n_runs=R).fit(x, generator=torch.Generator(device=dev).manual_seed(0)), a.repeat)
    steps = int(km.n_iter_.max())
    r = dict(N=N, L=L, K=C, R=R, batched_fit_s=t_batched, batched_n_iter=km.n_iter_.tolist(), batched_converged=km.converged_.tolist(),
             batched_abi_calls=n_calls, batched_host_reads=-(-steps // 8), batched_strict_fit_s=t_strict,
             batched_strict_n_iter=km0.n_iter_.tolist(), batched_seeded_fit_s=t_seeded, batched_seeded_n_iter=kms.n_iter_.tolist(),
             batched_n_empty=km.n_empty_.tolist())

    # ---- one step ---------------------------------------------------------------------------------------------------------
    centers, labels = x[torch.from_numpy(seeds).to(dev)].contiguous(), torch.full((R, N), -1, dtype=torch.int32, device=dev)
    state, scratch = K.kmeans_new_state(R, dev), K.kmeans_scratch(L, C, R, dev)
    tol = torch.full((), -1.0, dtype=torch.float64, device=dev)

    def step():
        state.zero_()  # never converged: every run takes every step
        K.kmeans_step(x, tol, centers, labels, state, scratch)

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(50):
        step()
    e1.record()
    torch.cuda.synchronize()
    r["step_s"] = e0.elapsed_time(e1) / 50 * 1e-3

    # ---- the baseline: one fit at a time ------------------------------------------------------------------------------------
    def sequential():
        rounds = []
        for s in seeds:
            g = DeviceGaussianMixture(C)
            p = K.gmm_new_params(L, C, dev)
            g._kmeans(x, p, torch.empty(N, C, device=dev), K.gmm_scratch(L, C, dev), None, s)
            rounds.append(g.kmeans_n_iter_)
        return rounds

    t_seq, rounds = timed(sequential, a.repeat)
    n_calls_seq, _ = counted(sequential)
    r.update(sequential_fit_s=t_seq, sequential_rounds=rounds, sequential_abi_calls=n_calls_seq,
             sequential_host_reads=sum(min(k + 1, 100) for k in rounds), speedup_vs_sequential=t_seq / t_strict)

    # ---- the evaluator ------------------------------------------------------------------------------------------------------
    train = MultimodalBaseDataset(data=dict(z=torch.from_numpy(X)), labels=torch.from_numpy(blob))
    test = MultimodalBaseDataset(data=dict(z=torch.from_numpy(Xt)), labels=torch.from_numpy(blob_t))

    def evaluate():
        ev = Clustering(IdentityModel(), test, train, eval_config=ClusteringConfig(n_clusters=C, number_of_runs=R))
        ev.generator = torch.Generator(device=dev).manual_seed(0)
        t0 = time.perf_counter()
        ev.fit_clustering()
        torch.cuda.synchronize()
        t_fit = time.perf_counter() - t0
        ev.finish()
        ev2 = Clustering(IdentityModel(), test, train, eval_config=ClusteringConfig(n_clusters=C, number_of_runs=R))
        ev2.generator = torch.Generator(device=dev).manual_seed(0)
        acc = ev2.eval().cluster_accuracy
        ev2.finish()
        return acc, t_fit

    evaluate()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    acc, t_fitc = evaluate()
    torch.cuda.synchronize()
    t_all = time.perf_counter() - t0
    r.update(eval_s=t_all - t_fitc, eval_fit_clustering_s=t_fitc, eval_cluster_accuracy=acc)
    t0 = time.perf_counter()
    for _ in torch.utils.data.DataLoader(train, 512, shuffle=True):
        pass
    r["train_loader_alone_s"] = time.perf_counter() - t0

    # ---- scikit-learn on the host, for orientation --------------------------------------------------------------------------
    if not a.no_sklearn:
        try:
            from sklearn.cluster import KMeans
        except ImportError:
            KMeans = None
        if KMeans is not None:
            t0 = time.perf_counter()
            its = [int(KMeans(C, init=X[s], n_init=1, max_iter=300).fit(X).n_iter_) for s in seeds]
            r.update(sklearn_fit_s=time.perf_counter() - t0, sklearn_n_iter=its, threads=os.environ.get("OMP_NUM_THREADS"))
    print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
