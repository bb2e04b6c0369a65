"""Float64 restatement (NumPy / SciPy) of the Gaussian-mixture EM of csrc/gmm.hip, the case tables of test_gmm_host.py and
test_gpu_gmm.py, and the error model: the same formulas with the per-row arithmetic of the E-step in fp32, sums over rows in fp64 and every
parameter stored as fp32 between the steps.

The formulas are scikit-learn's (sklearn/mixture/_gaussian_mixture.py: _estimate_log_gaussian_prob, _estimate_gaussian_parameters,
_estimate_gaussian_covariances_full, _compute_precision_cholesky, and the loop of BaseMixture.fit); test_gmm_host.py holds the
restatement against sklearn.mixture.GaussianMixture itself.  One difference is a parameter: scikit-learn adds 10 * eps of the
DATA's dtype to n_c; the kernels add 10 * FLT_EPSILON (`nk_eps`), the float64 comparison with scikit-learn 10 * DBL_EPSILON.

Parity is defined FROM A GIVEN INITIAL STATE (weights, means, precisions): scikit-learn's k-means draws from NumPy's generator
and cannot be reproduced by another implementation.
"""
import numpy as np
from scipy import linalg

BAR = 1e-4  # the project's parity bar: max|got - ref| / max|ref| per tensor; absolute for the lower bound
TOL = 1e-3
REG = 1e-6
FLT_EPS = float(np.finfo(np.float32).eps)
DBL_EPS = float(np.finfo(np.float64).eps)


def rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref)) / max(np.max(np.abs(ref)), 1e-300))


# ---- float64 ---------------------------------------------------------------------------------------------------------------
def finish64(covs):
    """covs [C,L,L] -> (lower Cholesky factors, precision factors P = (factor^-1)^T, sum ln diag P); raises on a pivot <= 0."""
    C, L, _ = covs.shape
    chol, prec = np.empty_like(covs), np.empty_like(covs)
    for c in range(C):
        chol[c] = linalg.cholesky(covs[c], lower=True)
        prec[c] = linalg.solve_triangular(chol[c], np.eye(L), lower=True).T
    logdet = np.log(np.diagonal(prec, axis1=1, axis2=2)).sum(1)
    return chol, prec, logdet


def prec_chol_from_precisions(precisions):
    """scikit-learn's _compute_precision_cholesky_from_precisions: upper-triangular P with P P^T = precision."""
    flip = lambda a: np.flipud(np.fliplr(a))
    return np.array([flip(linalg.cholesky(flip(p), lower=True)) for p in precisions])


def estep64(X, weights, means, prec, drop_logw=False):
    """-> (resp [N,C], lse [N], lower bound).  drop_logw: the mutation `ln w_c left out`."""
    N, L = X.shape
    C = means.shape[0]
    lp = np.empty((N, C))
    for c in range(C):
        y = (X - means[c]) @ prec[c]
        lp[:, c] = -0.5 * (L * np.log(2 * np.pi) + (y * y).sum(1)) + np.log(np.diagonal(prec[c])).sum()
    if not drop_logw:
        lp = lp + np.log(weights)
    m = lp.max(1, keepdims=True)
    lse = (m + np.log(np.exp(lp - m).sum(1, keepdims=True)))[:, 0]
    return np.exp(lp - lse[:, None]), lse, float(lse.mean())


def mstep64(X, resp, reg=REG, nk_eps=FLT_EPS, no_recentre=False, no_reg=False):
    """-> dict(weights, means, covs).  Mutations: no_recentre (covariance as E[xx^T] about the origin, the mean never taken out),
    no_reg (reg_covar left out)."""
    N, L = X.shape
    C = resp.shape[1]
    nk = resp.sum(0) + 10 * nk_eps
    means = resp.T @ X / nk[:, None]
    covs = np.empty((C, L, L))
    for c in range(C):
        d = X if no_recentre else X - means[c]
        covs[c] = (resp[:, c] * d.T) @ d / nk[c]
        if not no_reg:
            covs[c].flat[:: L + 1] += reg
    return dict(weights=nk / nk.sum(), means=means, covs=covs)


def em64(X, weights, means, prec, tol=TOL, max_iter=2000, reg=REG, nk_eps=FLT_EPS, estep=estep64, mstep=mstep64, finish=finish64):
    """The loop of BaseMixture.fit from the given state -> dict(weights, means, covs, cov_chol, prec_chol, n_iter, converged,
    lower_bound, changes [n_iter], resp of the last E-step)."""
    lb, changes, converged, n_iter, p = -np.inf, [], False, 0, None
    for n_iter in range(1, max_iter + 1):
        prev = lb
        resp, _, lb = estep(X, weights, means, prec)
        p = mstep(X, resp, reg, nk_eps)
        chol, prec, _ = finish(p["covs"])
        weights, means = p["weights"], p["means"]
        changes.append(lb - prev)
        if abs(lb - prev) < tol:
            converged = True
            break
    return dict(weights=weights, means=means, covs=p["covs"], cov_chol=chol, prec_chol=prec, n_iter=n_iter, converged=converged,
                lower_bound=lb, changes=changes, resp=resp)


def hard64(X, means):
    """-> (labels = argmin_c |x - mu_c|^2 (first minimum), the minimum, the second smallest distance or inf)."""
    d2 = ((X[:, None, :] - means[None, :, :]) ** 2).sum(2)
    lab = d2.argmin(1)
    s = np.sort(d2, 1)
    return lab, s[:, 0], (s[:, 1] if d2.shape[1] > 1 else np.full(len(X), np.inf))


def lloyd64(X, idx, max_iter=100):
    """Lloyd from the rows idx until no label changes -> (labels, means, rounds with a mean update, smallest ratio second-nearest /
    nearest distance met in any round)."""
    means = X[np.asarray(idx)].copy()
    C = len(means)
    labels, rounds, gap = np.full(len(X), -1), 0, np.inf
    for _ in range(max_iter):
        lab, d1, d2 = hard64(X, means)
        gap = min(gap, float(np.min(d2 / np.maximum(d1, 1e-300))))
        if np.array_equal(lab, labels):
            break
        labels = lab
        onehot = np.eye(C)[labels]
        means = onehot.T @ X / (onehot.sum(0) + 10 * FLT_EPS)[:, None]
        rounds += 1
    return labels, means, rounds, gap


def sample64(means, cov_chol, comp, eps):
    return means[comp] + np.einsum("nab,nb->na", cov_chol[comp], eps)


# ---- the error model: rows in fp32, sums in fp64 ----------------------------------------------------------------------------
f32 = np.float32


def estep_emul(X, weights, means, prec):
    X, weights, means, prec = X.astype(f32), weights.astype(f32), means.astype(f32), prec.astype(f32)
    N, L = X.shape
    C = means.shape[0]
    logdet = np.log(np.diagonal(prec.astype(np.float64), axis1=1, axis2=2)).sum(1).astype(f32)  # stored by the fp64 finish
    lp = np.empty((N, C), f32)
    for c in range(C):
        y = (X - means[c]) @ prec[c]
        lp[:, c] = (f32(-0.5 * L * np.log(2 * np.pi)) - f32(0.5) * (y * y).sum(1, dtype=f32)) + logdet[c] + np.log(weights[c])
    m = lp.max(1, keepdims=True)
    lse = (m + np.log(np.exp(lp - m).sum(1, keepdims=True, dtype=f32)))[:, 0]
    return np.exp(lp - lse[:, None]), lse, float(lse.astype(np.float64).mean())


def mstep_emul(X, resp, reg=REG, nk_eps=FLT_EPS):
    """The M-step reads fp32 responsibilities and fp32 rows and is float64 from the first product on."""
    return mstep64(X.astype(f32).astype(np.float64), resp.astype(f32).astype(np.float64), reg, nk_eps)


def finish_emul(covs):
    chol, prec, logdet = finish64(covs)  # fp64 on the device too; what the next E-step reads was stored as fp32
    return chol, prec.astype(f32).astype(np.float64), logdet


def em_emul(X, weights, means, prec, **kw):
    def mstep(X, resp, reg, nk_eps):
        p = mstep_emul(X, resp, reg, nk_eps)
        p["weights"], p["means"] = p["weights"].astype(f32).astype(np.float64), p["means"].astype(f32).astype(np.float64)
        return p

    return em64(X, weights, means, prec, estep=estep_emul, mstep=mstep, finish=finish_emul, **kw)


# ---- data ------------------------------------------------------------------------------------------------------------------
def blobs(N, L, C, seed, spread=6.0):
    """C centres ~ spread N(0, I), a linear map I + 0.3 N(0, 1) / sqrt(L) per component, uniform labels.  fp32 values held as
    float64 (the kernels and the references read the same numbers)."""
    g = np.random.default_rng(seed)
    centres = spread * g.standard_normal((C, L))
    maps = np.eye(L) + 0.3 * g.standard_normal((C, L, L)) / np.sqrt(L)
    labels = g.integers(0, C, N)
    X = centres[labels] + np.einsum("nab,nb->na", maps[labels], g.standard_normal((N, L)))
    return X.astype(f32).astype(np.float64), labels, g


class FitCase:
    def __init__(self, N, L, C, seed, degenerate=False):
        self.N, self.L, self.C, self.seed, self.degenerate = N, L, C, seed, degenerate
        self.name = f"n{N}-l{L}-c{C}-s{seed}" + ("-degenerate" if degenerate else "")

    def make(self):
        """(X, weights_init, means_init, precisions_init): uniform weights, means drawn from the rows, identity precisions."""
        X, _, g = blobs(self.N, self.L, self.C, self.seed)
        rows = g.choice(self.N, self.C, replace=False)
        return X, np.full(self.C, 1.0 / self.C), X[rows].copy(), np.stack([np.eye(self.L)] * self.C)


# Seeds chosen so that condition (b) of test_gmm_host.py holds (the last |change| < tol / 2, the one before > 2 tol): the
# iteration count of a correct implementation cannot differ from the reference's by rounding.
FIT_TABLE = [(300, 5, 1, 0), (37, 1, 2, 2), (257, 2, 3, 2), (1003, 8, 3, 0), (600, 33, 4, 0), (900, 64, 5, 0), (4099, 20, 10, 8),
             # a component with no more than L points: its covariance is singular down to reg_covar, an all-fp32 EM meets a
             # non-positive pivot (smallest component of the float64 fit: 38 points at L = 64; 4 points at L = 20)
             (2500, 64, 10, 6, True), (1300, 20, 64, 0, True)]
FIT_CASES = [FitCase(*a) for a in FIT_TABLE]
_REF = {}


def fit_reference(case):
    """(inputs, float64 EM result) of a case: computed once per session, shared, left unchanged."""
    if case.name not in _REF:
        X, w, mu, pr = case.make()
        _REF[case.name] = ((X, w, mu, pr), em64(X, w, mu, prec_chol_from_precisions(pr)))
    return _REF[case.name]


class StepCase:
    """One E-step and one M-step.  The mixture is random and well conditioned; the responsibilities of the M-step are those of the
    float64 E-step with column `empty` (if any) zeroed and the rows renormalised.  Where fewer than 4 L rows per component are
    left, the covariances are rank deficient down to reg_covar and their factors are arbitrarily ill conditioned: those cases
    take reg_covar = 1 (condition number <= 1 + the data's variance), the others the default 1e-6."""

    def __init__(self, N, L, C, empty=None):
        self.N, self.L, self.C, self.empty = N, L, C, empty
        self.reg = REG if N >= 4 * L * C * 2 else 1.0
        self.name = f"n{N}-l{L}-c{C}" + (f"-empty{empty}" if empty is not None else "")

    def make(self):
        seed = 1000 + self.N * 7 + self.L * 131 + self.C * 17
        X, _, g = blobs(self.N, self.L, self.C, seed, spread=2.0)
        means = 2.0 * g.standard_normal((self.C, self.L))
        A = np.eye(self.L) + 0.3 * g.standard_normal((self.C, self.L, self.L)) / np.sqrt(self.L)
        covs = np.einsum("cab,cdb->cad", A, A)
        w = g.uniform(0.5, 1.5, self.C)
        w /= w.sum()
        to32 = lambda a: a.astype(f32).astype(np.float64)
        _, prec, _ = finish64(covs)
        return X, to32(w), to32(means), to32(prec)

    def resp(self, X, w, means, prec):
        r, _, _ = estep64(X, w, means, prec)
        if self.empty is not None and self.C > 1:
            r[:, self.empty] = 0.0
            r = r / np.maximum(r.sum(1, keepdims=True), 1e-30)
        return r.astype(f32).astype(np.float64)


# N in {1, 37, 257, 1003, 4099} x L in {1, 2, 20, 33, 64} x C in {1, 3, 10, 64}, pruned: every value of every axis at least
# three times, the four corners of (N, L C), C > N (n1-l64-c64, n37-l20-c64, n1-l20-c3), N never a multiple of a tile (64, 128)
STEP_CASES = [StepCase(*a) for a in [
    (1, 1, 1), (1, 64, 64), (1, 20, 3), (37, 1, 3), (37, 20, 64), (37, 33, 10, 2), (257, 2, 3, 0), (257, 64, 1), (257, 20, 10),
    (1003, 2, 64), (1003, 33, 10, 9), (1003, 64, 3), (4099, 1, 1), (4099, 20, 10, 4), (4099, 33, 64), (4099, 64, 64, 63),
    (4099, 2, 10), (1003, 1, 10)]]

MUTATION_CASE = StepCase(37, 33, 10, 2)  # reg_covar = 1 here: leaving it out moves the covariances by far more than the bar


def lloyd_case(N=1003, L=8, C=5, seed=11):
    """Well separated blobs and one seed row per blob: in every round every row's second-nearest centre is clearly farther than
    its nearest (asserted by test_gmm_host.py), so the labels do not depend on the precision of the distances."""
    X, labels, _ = blobs(N, L, C, seed, spread=10.0)
    return X, [int(np.flatnonzero(labels == c)[0]) for c in range(C)]
