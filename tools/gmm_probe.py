"""Timing of the device Gaussian-mixture fit (csrc/gmm.hip) against scikit-learn's host fit from the SAME initial state.

    python tools/gmm_probe.py [--sizes 60000,1680000] [--latent 20] [--components 10] [--out FILE.json]

Per size: the time of one EM iteration (HIP events around `--iters` guarded steps that never converge, tol = 0), of the E-step and
the M-step alone, of a whole fit (host clock around fit + synchronise; tol 1e-3), the bytes one iteration has to move
(3 passes over rows and responsibilities) as a share of the HBM rate, and sklearn.mixture.GaussianMixture.fit on the fp32
embeddings from the same weights / means / precisions with the host's thread setting (and, up to --sklearn-default-upto rows,
scikit-learn's default fit with its own k-means initialisation, which is what the reference's sampler runs).  Needs a GPU; prints one JSON line per size.
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HBM_MEASURED = 6.29e12  # bytes / s, float4 copy on an MI355X (8.0e12 is the datasheet value)


def blobs(N, L, C, seed):
    g = np.random.default_rng(seed)
    centres = 6.0 * g.standard_normal((C, L))
    maps = np.eye(L) + 0.3 * g.standard_normal((C, L, L)) / np.sqrt(L)
    labels = g.integers(0, C, N)
    X = np.empty((N, L), np.float32)
    for c in range(C):
        m = labels == c
        X[m] = centres[c] + g.standard_normal((int(m.sum()), L)) @ maps[c].T
    return X, X[g.choice(N, C, replace=False)].astype(np.float64)


def events(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="60000,1680000")
    ap.add_argument("--latent", type=int, default=20)
    ap.add_argument("--components", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--sklearn-default-upto", type=int, default=100000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gmm_probe needs a GPU: a CPU run measures nothing"
    from multivae_amd import kernels as K
    from multivae_amd.samplers.gaussian_mixture import DeviceGaussianMixture

    dev = torch.device("cuda:0")
    L, C = a.latent, a.components
    results = []
    with warnings.catch_warnings():  # first use of the seeding path (torch.multinomial, randint, indexing) loads code: not timed
        warnings.simplefilter("ignore")
        DeviceGaussianMixture(C, max_iter=2).fit(torch.randn(4096, L, device=dev), generator=torch.Generator(device=dev).manual_seed(1))
    for N in [int(s) for s in a.sizes.split(",")]:
        X, means0 = blobs(N, L, C, seed=N % 1000)
        w0, prec0 = np.full(C, 1.0 / C), np.stack([np.eye(L)] * C)
        x = torch.from_numpy(X).to(dev)
        init = dict(weights_init=w0, means_init=means0, precisions_init=prec0)
        # whole fit (the second of two: the first loads code objects)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            DeviceGaussianMixture(C, max_iter=2).fit(x, **init)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g = DeviceGaussianMixture(C).fit(x, **init)
        torch.cuda.synchronize()
        t_fit = time.perf_counter() - t0
        # default initialisation (k-means++ and Lloyd on the device) + EM
        t0 = time.perf_counter()
        gk = DeviceGaussianMixture(C).fit(x, generator=torch.Generator(device=dev).manual_seed(0))
        torch.cuda.synchronize()
        t_fit_kmeans = time.perf_counter() - t0
        # one iteration: guarded steps that never converge, on a copy of the fitted parameters
        p = dict(weights=g.weights_.clone(), means=g.means_.clone(), covs=g.covariances_.clone(),
                 cov_chol=g.covariances_cholesky_.clone(), prec_chol=g.precisions_cholesky_.clone(),
                 logdet=torch.log(torch.diagonal(g.precisions_cholesky_, dim1=-2, dim2=-1)).sum(-1).contiguous())
        resp = torch.empty(N, C, device=dev)
        scratch, state = K.gmm_scratch(L, C, dev), K.gmm_new_state(dev)
        t_iter = events(lambda: K.gmm_em_step(x, p, resp, state, 1e-6, 0.0, scratch), a.iters)
        t_e = events(lambda: K.gmm_estep(x, p, resp, scratch), a.iters)
        q = {k: v.clone() for k, v in p.items()}
        t_m = events(lambda: K.gmm_mstep(x, resp, q, 1e-6, scratch), a.iters)
        need = 3 * N * (L + C) * 4  # E: rows in, responsibilities out; M: rows and responsibilities in, twice (two passes)
        r = dict(N=N, L=L, C=C, device_fit_s=t_fit, device_fit_n_iter=g.n_iter_, device_fit_converged=g.converged_,
                 device_fit_with_kmeans_s=t_fit_kmeans, device_kmeans_rounds=gk.kmeans_n_iter_, device_kmeans_fit_n_iter=gk.n_iter_,
                 em_iteration_s=t_iter, estep_s=t_e, mstep_s=t_m, bytes_needed_per_iteration=need,
                 hbm_share_of_measured_peak=need / t_iter / HBM_MEASURED, threads=os.environ.get("OMP_NUM_THREADS"))
        if not a.no_sklearn:
            from sklearn.mixture import GaussianMixture

            # init_params="random": scikit-learn runs its k-means even when all three *_init are given and then discards the
            # result; the cheap random responsibilities keep the timed region to the EM loop from the given state
            sk = GaussianMixture(n_components=C, covariance_type="full", tol=1e-3, max_iter=2000, init_params="random", **init)
            t0 = time.perf_counter()
            sk.fit(X)
            t_sk = time.perf_counter() - t0
            rel = lambda got, ref: float(np.max(np.abs(got.cpu().double().numpy() - ref)) / np.max(np.abs(ref)))
            r.update(sklearn_fit_s=t_sk, sklearn_n_iter=int(sk.n_iter_), sklearn_iteration_s=t_sk / sk.n_iter_,
                     speedup_fit=t_sk / t_fit, rel_weights=rel(g.weights_, sk.weights_), rel_means=rel(g.means_, sk.means_),
                     rel_covs=rel(g.covariances_, sk.covariances_), lower_bound_diff=abs(g.lower_bound_ - sk.lower_bound_))
            if N <= a.sklearn_default_upto:  # what the reference's sampler runs: k-means initialisation + EM
                t0 = time.perf_counter()
                skd = GaussianMixture(n_components=C, covariance_type="full", tol=1e-3, max_iter=2000, random_state=0).fit(X)
                r.update(sklearn_default_fit_s=time.perf_counter() - t0, sklearn_default_n_iter=int(skd.n_iter_))
        print(json.dumps(r), flush=True)
        results.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
