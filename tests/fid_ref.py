"""The Fréchet statistics and distance of the FIDEvaluator in float64, written from the definition.  Not a test.

For the activations of one stream, [N, D]: mean = the column mean, cov = np.cov(rowvar=False) (divisor N - 1).  The distance between
two streams is |mean0 - mean1|^2 + tr cov0 + tr cov1 - 2 tr sqrtm(cov0 cov1).

`stats64` / `fd64` are the reference (scipy's sqrtm, as the formula is written); `fd_eigh64` is the symmetric form that
multivae_amd.metrics.fids.frechet_distance uses, in numpy float64, for the cross-check of test_fid_host.py.
`emulate_shifted_fp32` restates the arithmetic of csrc/frechet.hip in numpy (a shift fixed by the first batch, fp32 differences,
fp32 products per chunk of rows, fp64 sums) and `unshifted_fp32` the same pipeline without the shift, so that the CPU suite can
say what the shift buys without a GPU.

Bars (relative to scale = |mean0 - mean1|^2 + tr cov0 + tr cov1, because the distance is a difference of these):
    BAR = 1e-4        the project's parity bar (README), distance against float64
    COV_BAR = 1e-5    |cov - float64| / max |cov|
    MEAN_BAR = 1e-6   |mean - float64| / max |mean|
"""
import os

import numpy as np
import scipy.linalg

BAR = 1e-4
COV_BAR = 1e-5
MEAN_BAR = 1e-6
EIGH_BAR = 1e-6   # fd_eigh64 against fd64, relative to scale
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fid_cases.npz")


def stats64(acts):
    a = np.asarray(acts, np.float64)
    return np.mean(a, axis=0), np.cov(a, rowvar=False)


def scale(mu0, s0, mu1, s1):
    d = np.atleast_1d(mu0).astype(np.float64) - np.atleast_1d(mu1)
    return float(d @ d + np.trace(np.atleast_2d(s0)) + np.trace(np.atleast_2d(s1)))


def fd64(mu0, s0, mu1, s1, eps=1e-6):
    """The distance with scipy.linalg.sqrtm of the product; a non-finite root is retried with eps on both diagonals, and the
    real part is taken."""
    mu0, mu1 = np.atleast_1d(np.asarray(mu0, np.float64)), np.atleast_1d(np.asarray(mu1, np.float64))
    s0, s1 = np.atleast_2d(np.asarray(s0, np.float64)), np.atleast_2d(np.asarray(s1, np.float64))
    root = scipy.linalg.sqrtm(s0 @ s1)
    if not np.isfinite(root).all():
        jitter = eps * np.eye(len(s0))
        root = scipy.linalg.sqrtm((s0 + jitter) @ (s1 + jitter))
    d = mu0 - mu1
    return float(d @ d + np.trace(s0) + np.trace(s1) - 2.0 * np.trace(root).real)


def fd_eigh64(mu0, s0, mu1, s1):
    """The symmetric form: the eigenvalues of cov0^(1/2) cov1 cov0^(1/2), with cov0^(1/2) from eigh, negatives clamped."""
    mu0, mu1 = np.atleast_1d(np.asarray(mu0, np.float64)), np.atleast_1d(np.asarray(mu1, np.float64))
    s0, s1 = np.atleast_2d(np.asarray(s0, np.float64)), np.atleast_2d(np.asarray(s1, np.float64))
    w, v = np.linalg.eigh(0.5 * (s0 + s0.T))
    root = (v * np.sqrt(np.maximum(w, 0.0))) @ v.T
    m = root @ s1 @ root
    lam = np.linalg.eigvalsh(0.5 * (m + m.T))
    d = mu0 - mu1
    return float(d @ d + np.trace(s0) + np.trace(s1) - 2.0 * np.sqrt(np.maximum(lam, 0.0)).sum())


def fd_of_acts(real, gen, fd=fd64):
    m0, s0 = stats64(real)
    m1, s1 = stats64(gen)
    return fd(m0, s0, m1, s1), scale(m0, s0, m1, s1)


# ---- float32 emulations (CPU statements about precision; the GPU tests compare the kernel itself) ---------------------------
def _stream_fp32(acts, batches, chunk, shifted):
    f = np.float32
    x = np.asarray(acts, f)
    N, D = x.shape
    assert sum(batches) == N
    c = (x[:batches[0]].astype(np.float64).sum(0) / batches[0]).astype(f) if shifted else np.zeros(D, f)
    S1, S2, at = np.zeros(D), np.zeros((D, D)), 0
    for b in batches:
        for r0 in range(at, at + b, chunk):
            d = x[r0:min(r0 + chunk, at + b)] - c
            assert d.dtype == f
            S2 += (d.T @ d).astype(np.float64)  # fp32 products and sums inside a chunk, every chunk added in fp64
            S1 += d.astype(np.float64).sum(0)
        at += b
    n = float(N)
    return c.astype(np.float64) + S1 / n, (S2 - np.outer(S1, S1) / n) / (n - 1.0)


def emulate_shifted_fp32(acts, batch, chunk=64):
    """(mean, cov) of one stream as csrc/frechet.hip forms them; batch = the sizes of the successive updates."""
    return _stream_fp32(acts, list(batch), chunk, True)


def unshifted_fp32(acts, batch, chunk=64):
    """The same pipeline with a zero shift: fp32 raw second moments."""
    return _stream_fp32(acts, list(batch), chunk, False)


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def make_pair(D, N, seed, offset=0.0, separation=1.0):
    """(real, generated) [N, D] float32 with different distributions: different mixing matrices, means `separation` apart per
    column (plus `offset` on both), seeded."""
    rng = np.random.default_rng([seed, D, N])
    mix0 = np.eye(D) + 0.3 * rng.standard_normal((D, D)) / np.sqrt(D)
    mix1 = 0.7 * np.eye(D) + 0.5 * rng.standard_normal((D, D)) / np.sqrt(D)
    real = rng.standard_normal((N, D)) @ mix0 + offset + 0.5 * rng.standard_normal(D)
    gen = rng.standard_normal((N, D)) @ mix1 + offset + separation + 0.5 * rng.standard_normal(D)
    return real.astype(np.float32), gen.astype(np.float32)


# golden cases: name -> (D, N, seed, offset); fid_cases.npz holds their inputs and the reference's values
GOLDEN_CASES = {
    "d1": (1, 50, 1, 0.0),
    "small": (5, 7, 2, 0.0),
    "rankdef": (40, 12, 3, 0.0),
    "offset": (16, 200, 4, 500.0),
    "wide": (48, 150, 5, 0.0),
}
OFFSET_CASE = "offset"
SEPARATED = ("d1", "small", "offset", "wide")  # the distance is a sizeable share of scale: also 1e-4 relative to the distance
GOLDEN_BATCHES = {"d1": (50,), "small": (3, 3, 1), "rankdef": (5, 7), "offset": (37, 37, 37, 37, 37, 15), "wide": (64, 65, 21)}


def load_golden():
    z = np.load(GOLDEN)
    return {k: dict(real=z[k + "/real"], gen=z[k + "/gen"], mu0=z[k + "/mu0"], mu1=z[k + "/mu1"], s0=z[k + "/s0"], s1=z[k + "/s1"],
                    fd=float(z[k + "/fd"])) for k in GOLDEN_CASES}


# kernel cases: D from the tile edge T, batch sequences from the row chunk
def kernel_dims(T):
    return [1, 5, T - 1, T, T + 1, 2 * T + 3]


def kernel_batches(chunk):
    return [(1,), (3, 3, 1), (37, 37, 5), (chunk + 1, 2)]
