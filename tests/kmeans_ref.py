"""Float64 restatement (NumPy) of the batched k-means of csrc/kmeans.hip and of the Clustering evaluator's vote and accuracy, the
case tables of test_kmeans_host.py and test_gpu_kmeans.py, and an fp32 emulation of the kernel's distance arithmetic.

The iteration is scikit-learn's _kmeans_single_lloyd (sklearn/cluster/_kmeans.py): labels from the centres (first minimum of the
squared distance), centres from the labels, replace, stop when the labels repeat (strict, `converged` 1) or when the squared
centre shift is <= tol * mean of the column variances (`converged` 2), then one more labelling.  test_kmeans_host.py holds the
restatement against sklearn.cluster.KMeans itself.  One stated difference: a cluster without rows keeps its centre and is
counted (scikit-learn moves it to the row farthest from its own centre); the parity cases meet no empty cluster.

Parity is defined FROM GIVEN INITIAL CENTRES: scikit-learn's k-means++ draws from NumPy's generator and cannot be reproduced by
another implementation.  The vote and the accuracy restate multivae/metrics/latent_clustering/clustering_class.py:79-107.
"""
import numpy as np

BAR = 1e-4  # the project's parity bar: max|got - ref| / max|ref| per tensor
TOL = 1e-4  # scikit-learn's default, scaled by the mean column variance
f32 = np.float32


def rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref)) / max(np.max(np.abs(ref)), 1e-300))


# ---- float64 ---------------------------------------------------------------------------------------------------------------
def dist64(X, centers):
    """[N,K] squared distances, taken directly (x - c)^2."""
    return ((X[:, None, :] - centers[None, :, :]) ** 2).sum(2)


def assign64(X, centers):
    """-> (labels = first minimum, that minimum, the second smallest distance or inf)."""
    d2 = dist64(X, centers)
    lab = d2.argmin(1)
    s = np.sort(d2, 1)
    return lab, s[:, 0], (s[:, 1] if d2.shape[1] > 1 else np.full(len(X), np.inf))


def scaled_tol(X, tol=TOL):
    return tol * float(np.mean(np.var(X, axis=0)))


def step64(X, centers, labels_prev, tol_abs, centres_from_previous_labels=False):
    """One iteration -> dict(labels, centers, changed, inertia, shift, empty, converged).  Mutation: centres averaged over the
    PREVIOUS labels (the labels of this iteration come one step too late)."""
    K = centers.shape[0]
    labels, d1, _ = assign64(X, centers)
    src = labels_prev if centres_from_previous_labels and labels_prev.min() >= 0 else labels
    new, empty = centers.copy(), 0
    for k in range(K):
        rows = X[src == k]
        if len(rows):
            new[k] = rows.sum(0) / len(rows)
        else:
            empty += 1
    changed = int(np.sum(labels != labels_prev))
    shift = float(((new - centers) ** 2).sum())
    converged = 1 if changed == 0 else (2 if shift <= tol_abs else 0)
    return dict(labels=labels, centers=new, changed=changed, inertia=float(d1.sum()), shift=shift, empty=empty, converged=converged)


def fit64(X, c0, tol=TOL, max_iter=300, unscaled_tol=False, no_final_relabel=False, centres_from_previous_labels=False):
    """The loop of _kmeans_single_lloyd from the centres c0 -> dict(labels, centers, inertia, n_iter, converged, n_empty, trace);
    trace[i] = (centres the labels of iteration i were taken from, labels, shift, tol).  Mutations: unscaled_tol (tol not
    multiplied by the variance), no_final_relabel, centres_from_previous_labels."""
    tol_abs = tol if unscaled_tol else scaled_tol(X, tol)
    centers, labels = np.array(c0, np.float64), np.full(len(X), -1)
    n_iter, converged, n_empty, trace = 0, 0, 0, []
    for n_iter in range(1, max_iter + 1):
        s = step64(X, centers, labels, tol_abs, centres_from_previous_labels)
        trace.append((centers, s["labels"], s["shift"], tol_abs))
        centers, labels, converged = s["centers"], s["labels"], s["converged"]
        n_empty += s["empty"]
        inertia = s["inertia"]
        if converged:
            break
    if not no_final_relabel:
        labels, d1, _ = assign64(X, centers)
        inertia = float(d1.sum())
    return dict(labels=labels, centers=centers, inertia=inertia, n_iter=n_iter, converged=converged, n_empty=n_empty, trace=trace)


def table64(cluster_labels, y, K, n_classes):
    """[K, n_classes + 1] contingency counts; a y outside [0, n_classes) goes to the extra last column."""
    t = np.zeros((K, n_classes + 1), np.int64)
    col = np.where((y >= 0) & (y < n_classes), y, n_classes)
    np.add.at(t, (cluster_labels, col), 1)
    return t


def vote64(table, last_max=False):
    """majority [K]: the first maximum over the real classes (np.bincount(...).argmax()); a cluster without a row in a real class
    maps to its own index.  Mutation: the LAST maximum."""
    real = table[:, :-1]
    K, C = real.shape
    arg = (C - 1 - real[:, ::-1].argmax(1)) if last_max else real.argmax(1)
    return np.where(real.max(1) > 0, arg, np.arange(K)).astype(np.int64)


def accuracy64(majority, cluster_labels, y):
    """rows whose cluster's majority label is the true label."""
    return int(np.sum(majority[cluster_labels] == y))


def reference_vote_and_accuracy(train_clusters, train_y, test_clusters, test_y):
    """clustering_class.py:79-107 on NumPy arrays, line for line: (labels_dict, correct rows)."""
    labels_dict = {str(m): m for m in np.unique(train_clusters)}
    if len(train_y) == len(train_clusters):
        for c in np.unique(train_clusters):
            labels_dict[str(c)] = np.bincount(train_y[train_clusters == c]).argmax()
    labels = np.array([labels_dict[str(c)] for c in test_clusters])
    return labels_dict, int(np.sum(labels == test_y))


# ---- the error model: the kernel's fp32 distance ---------------------------------------------------------------------------
def dist_emul(X, centers):
    """The kernel's distance: d = fl32(x - c), dist = fl32(fma(d, d, dist)) in index order, centres rounded to fp32 first (they are
    stored so).  d * d is exact in float64 (48 bits) and the sum with a 24-bit dist is rounded once more to fp32: the emulation
    differs from a true fma only by double rounding, far below the margins asserted on it."""
    Xf, Cf = X.astype(f32), centers.astype(f32)
    dist = np.zeros((len(X), len(Cf)), f32)
    for i in range(X.shape[1]):
        d = (Xf[:, None, i] - Cf[None, :, i]).astype(np.float64)
        dist = (d * d + dist.astype(np.float64)).astype(f32)
    return dist


def decidable(X, c0, tol=TOL, max_iter=300):
    """What test_kmeans_host.py asserts of a fit case: along the float64 fit, (the emulated fp32 labels equal the float64 labels in
    every iteration, the smallest relative gap between the nearest and the second-nearest squared distance, the largest relative
    error of the fp32 distance, the smallest |shift - tol| / tol)."""
    ref = fit64(X, c0, tol, max_iter)
    same, gap, err, margin = True, np.inf, 0.0, np.inf
    for centers, labels, shift, tol_abs in ref["trace"] + [(ref["centers"], ref["labels"], None, None)]:
        d64, d32 = dist64(X, centers), dist_emul(X, centers).astype(np.float64)
        same = same and np.array_equal(d32.argmin(1), labels)
        s = np.sort(d64, 1)
        if s.shape[1] > 1:
            gap = min(gap, float(np.min((s[:, 1] - s[:, 0]) / np.maximum(s[:, 1], 1e-300))))
        err = max(err, float(np.max(np.abs(d32 - d64) / np.maximum(d64, 1e-300))))
        if shift is not None:
            margin = min(margin, abs(shift - tol_abs) / tol_abs)
    return same, gap, err, margin, ref


# ---- data ------------------------------------------------------------------------------------------------------------------
def blobs(N, L, K, seed):
    """mu = 2 N(0,1) [K,L], X = mu[randint] + N(0,1), cast to fp32 and held as float64 (the kernels and the references read the same
    numbers); the true blob of every row; the generator, for the initial centres."""
    g = np.random.default_rng(seed)
    mu = 2.0 * g.standard_normal((K, L))
    blob = g.integers(0, K, N)
    X = mu[blob] + g.standard_normal((N, L))
    return X.astype(f32).astype(np.float64), blob, g


class FitCase:
    """A blob data set and R sets of initial centres, each K distinct rows of X."""

    def __init__(self, N, L, K, seed, R=3, tol=TOL, inits=None):
        self.N, self.L, self.K, self.seed, self.tol = N, L, K, seed, tol
        self.inits = tuple(range(R)) if inits is None else tuple(inits)
        self.R = len(self.inits)
        self.name = f"n{N}-l{L}-k{K}-s{seed}" + (f"-tol{tol:g}" if tol != TOL else "") + (f"-r{R}" if R != 3 else "")

    def make(self):
        """(X [N,L], init_indices [R,K]): initialisation r is drawn from its own generator (seed, inits[r])."""
        X, _, _ = blobs(self.N, self.L, self.K, self.seed)
        return X, np.stack([np.random.default_rng((self.seed, i)).choice(self.N, self.K, replace=False)
                            for i in self.inits])


# (N, L, K, seed): the shapes of the issue's list; test_kmeans_host.py asserts the conditions that make each decidable by fp32
# arithmetic, for every one of the R initialisations, and that scikit-learn's KMeans gives the same fit
# (initialisations 0 and 3 of the last one come within 16 fp32 errors of a tie between two centres and are not used)
FIT_TABLE = [(37, 2, 3, 0), (1003, 33, 10, 0), (1003, 64, 4, 1), (600, 8, 64, 0), (1003, 20, 10, 2), (4099, 16, 10, 0)]
FIT_CASES = [FitCase(*a) for a in FIT_TABLE[:-1]] + [FitCase(*FIT_TABLE[-1], inits=(1, 2, 4))]
TOL_CASE = FitCase(1003, 20, 10, 2, tol=1e-2)  # at least one run stops on the centre shift (converged 2), see the host test
BATCH_CASE = FitCase(1003, 20, 10, 2, R=20)     # independence of the batch: run r of 20 against the same centres alone
_REF = {}


def fit_reference(case):
    """(X, init_indices, [fit64 of every initialisation]): computed once per session, shared, left unchanged."""
    if case.name not in _REF:
        X, idx = case.make()
        _REF[case.name] = (X, idx, [fit64(X, X[i], case.tol) for i in idx])
    return _REF[case.name]


def empty_case():
    """(X, centres [K,L]) whose centre 3 is far from every row: that cluster is empty in the first step."""
    X, _, g = blobs(257, 20, 10, 0)
    c = X[g.choice(257, 10, replace=False)].copy()
    c[3] = 100.0
    return X, c


class AssignCase:
    """Rows, R sets of K centres (perturbed rows of X, or random where K > N), labels y in [0, n_classes) with a few outside."""

    def __init__(self, N, L, K, R, n_classes=5, salt=0):
        self.N, self.L, self.K, self.R, self.n_classes, self.salt = N, L, K, R, n_classes, salt
        self.name = f"n{N}-l{L}-k{K}-r{R}-c{n_classes}"

    def make(self):
        g = np.random.default_rng((7000 + self.N * 3 + self.L * 131 + self.K * 17 + self.R, self.salt))
        X = (2.0 * g.standard_normal((self.N, self.L))).astype(f32).astype(np.float64)
        centers = (2.0 * g.standard_normal((self.R, self.K, self.L))).astype(f32).astype(np.float64)
        y = g.integers(0, self.n_classes, self.N)
        y[:: 11] = self.n_classes + 2  # outside the classes
        if self.N > 5:
            y[5] = -1
        return X, centers, y.astype(np.int64)


# N in {1, 37, 257, 1003} x L in {1, 2, 20, 33, 64} x K in {1, 3, 10, 64} x R in {1, 3, 20, 32}, pruned: every value of every axis
# at least twice, K > N (n1-*, n37-l20-k64), N never a multiple of the tile (128), more than one workgroup per run (n257, n1003),
# a table of more than 2048 cells (k64 with 40 classes: the path without the LDS histogram).  The sixth entry is a salt of the
# generator: salt 0 of n1003-l20-k10-r20 puts a row within 16 fp32 errors of a tie between two centres (test_kmeans_host.py)
ASSIGN_CASES = [AssignCase(*a) for a in [
    (1, 1, 1, 1), (1, 64, 64, 3), (37, 2, 3, 20), (37, 20, 64, 32), (257, 33, 10, 3), (257, 1, 3, 32), (257, 64, 1, 20),
    (1003, 20, 10, 20, 5, 1), (1003, 2, 64, 1, 40), (1003, 33, 3, 1), (1003, 64, 10, 3), (37, 33, 1, 1)]]
