"""CPU checks behind test_gpu_kmeans.py: that tests/kmeans_ref.py IS scikit-learn's Lloyd iteration, that every fit case can be
decided by fp32 distance arithmetic (conditions on the INPUTS: a case that breaks one is replaced, not excused), that the vote and
the accuracy are the reference's own lines, that the configuration and the state-block mirror are what they claim, and that the
mutations test_gpu_kmeans.py rejects on the kernel's output are rejected on the restatement too."""
import json
import os
import re

import numpy as np
import pytest

import kmeans_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_FITS = R.FIT_CASES + [R.TOL_CASE]


@pytest.mark.parametrize("case", ALL_FITS, ids=lambda c: c.name)
def test_restatement_is_scikit_learn(case):
    cluster = pytest.importorskip("sklearn.cluster")
    X, idx, refs = R.fit_reference(case)
    for i, ref in zip(idx, refs):
        assert ref["n_empty"] == 0, "a parity case must not meet an empty cluster (scikit-learn relocates it)"
        km = cluster.KMeans(case.K, init=X[i], n_init=1, algorithm="lloyd", tol=case.tol, max_iter=300).fit(X)
        assert np.array_equal(km.labels_, ref["labels"]) and km.n_iter_ == ref["n_iter"]
        assert np.max(np.abs(km.cluster_centers_ - ref["centers"])) <= 1e-10
        assert abs(km.inertia_ - ref["inertia"]) <= 1e-10 * ref["inertia"]


@pytest.mark.parametrize("case", ALL_FITS, ids=lambda c: c.name)
def test_fit_cases_are_decidable_in_fp32(case):
    X, idx = case.make()
    iters = []
    for i in idx:
        same, gap, err, margin, ref = R.decidable(X, X[i], case.tol)
        print(case.name, "n_iter", ref["n_iter"], "converged", ref["converged"], f"gap {gap:.2e} fp32 error {err:.2e} margin {margin:.2e}")
        assert same, "the emulated fp32 labels differ from the float64 labels in some iteration"
        assert gap >= 16 * err, (gap, err)
        assert margin >= 1e-2, margin
        assert ref["converged"] in (1, 2) and ref["n_iter"] < 300
        iters.append(ref["n_iter"])
    assert len(set(iters)) > 1, "the runs of a case must stop at different iterations"


@pytest.mark.parametrize("case", R.ASSIGN_CASES, ids=lambda c: c.name)
def test_assign_cases_are_decidable_in_fp32(case):
    """test_gpu_kmeans.py asserts label EQUALITY on these: no row may lie within 16 fp32 errors of a tie."""
    X, centers, y = case.make()
    assert np.any((y < 0) | (y >= case.n_classes)) or case.N < 2
    for c in centers:
        d64, d32 = R.dist64(X, c), R.dist_emul(X, c).astype(np.float64)
        assert np.array_equal(d32.argmin(1), d64.argmin(1))
        err = float(np.max(np.abs(d32 - d64) / np.maximum(d64, 1e-300)))
        if case.K > 1:
            s = np.sort(d64, 1)
            assert float(np.min((s[:, 1] - s[:, 0]) / s[:, 1])) >= 16 * err


def test_a_case_stops_on_the_centre_shift():
    _, _, refs = R.fit_reference(R.TOL_CASE)
    assert 2 in [r["converged"] for r in refs] and 1 in [r["converged"] for r in refs]
    for case in R.FIT_CASES:
        assert all(r["converged"] == 1 for r in R.fit_reference(case)[2])


def test_empty_cluster_case():
    X, c = R.empty_case()
    s = R.step64(X, c, np.full(len(X), -1), R.scaled_tol(X))
    assert s["empty"] == 1 and np.array_equal(s["centers"][3], c[3]) and 3 not in s["labels"] and s["converged"] == 0


def test_vote_and_accuracy_are_the_reference_lines():
    g = np.random.default_rng(3)
    K, C = 6, 4
    train_c = g.integers(0, K - 1, 400)                    # cluster 5 has no training row
    train_y = g.integers(0, C, 400)
    rows2 = np.flatnonzero(train_c == 2)
    if len(rows2) % 2:
        train_c[rows2[-1]], rows2 = 0, rows2[:-1]
    train_y[rows2] = np.tile([3, 1], len(rows2) // 2)      # an exact tie between classes 1 and 3 in cluster 2
    test_c, test_y = g.integers(0, K - 1, 300), g.integers(0, C, 300)  # the reference has no entry for a cluster it never saw
    table = R.table64(train_c, train_y, K, C)
    assert table[2, 1] == table[2, 3] == table[2].max() and table[5].sum() == 0
    maj = R.vote64(table)
    d, correct = R.reference_vote_and_accuracy(train_c, train_y, test_c, test_y)
    assert maj[2] == 1 and maj[5] == 5                     # the tie goes to the smaller class; the empty cluster to itself
    assert all(maj[int(c)] == v for c, v in d.items())
    assert R.accuracy64(maj, test_c, test_y) == correct
    # labels outside the classes (never a cluster's majority): counted in the extra column, never correct
    train_y2, test_y2 = train_y.copy(), test_y.copy()
    train_y2[::17], test_y2[::13] = C + 3, C + 3
    t2 = R.table64(train_c, train_y2, K, C)
    assert t2[:, C].sum() == len(train_y2[::17]) and t2.sum() == 400
    d2, correct2 = R.reference_vote_and_accuracy(train_c, train_y2, test_c, test_y2)
    maj2 = R.vote64(t2)
    assert all(maj2[int(c)] == v for c, v in d2.items()) and R.accuracy64(maj2, test_c, test_y2) == correct2
    # unlabelled training data: the identity
    d3, correct3 = R.reference_vote_and_accuracy(train_c, np.zeros(0, np.int64), test_c, test_y)
    assert R.accuracy64(np.arange(K), test_c, test_y) == correct3 and all(int(c) == v for c, v in d3.items())


def test_config_and_state_mirror(tmp_path):
    from multivae_amd import _lib
    from multivae_amd.metrics import Clustering, ClusteringConfig, EvaluatorConfig
    from multivae_amd.metrics.latent_clustering import DeviceKMeans  # noqa: F401

    cfg = ClusteringConfig()
    want = dict(name="ClusteringConfig", batch_size=512, wandb_path=None, clustering_method="kmeans", n_clusters=10,
                number_of_runs=20, num_samples_for_fit=None, use_mean=True)
    assert issubclass(ClusteringConfig, EvaluatorConfig) and Clustering.__name__ == "Clustering"
    assert list(json.loads(cfg.to_json_string()).items()) == list(want.items())  # the reference's fields, order and defaults
    other = ClusteringConfig(n_clusters=3, number_of_runs=40, num_samples_for_fit=100, use_mean=False, batch_size=7)
    other.save_json(str(tmp_path), "c")
    assert ClusteringConfig.from_json_file(str(tmp_path / "c.json")) == other != cfg
    with pytest.raises(Exception):
        ClusteringConfig(clustering_method="dbscan")
    header = open(os.path.join(ROOT, "include", "mvk.h")).read()
    defs = {k.lower(): int(v) for k, v in re.findall(r"#define MVK_KMEANS_STATE_(\w+) (\d+)", header)}
    assert defs.pop("doubles") == _lib.KMEANS_STATE_DOUBLES == 8
    assert defs == _lib.KMEANS_STATE and len(set(defs.values())) == len(defs) and max(defs.values()) < 8
    assert set(defs) == {"iter", "converged", "shift", "changed", "inertia", "empty"}


def test_mutations_of_the_restatement_are_rejected():
    """Each mutation (test_gpu_kmeans.py asserts the same on the kernel's output) moves a fit used on the GPU further than the bar,
    or changes its labels or its iteration count."""
    X, idx, refs = R.fit_reference(R.TOL_CASE)

    def differs(ref, mut):
        return (mut["n_iter"] != ref["n_iter"] or not np.array_equal(mut["labels"], ref["labels"])
                or R.rel(mut["centers"], ref["centers"]) > R.BAR or abs(mut["inertia"] - ref["inertia"]) > R.BAR * ref["inertia"])

    r2 = [r for r in range(len(refs)) if refs[r]["converged"] == 2][0]
    c0 = X[idx[r2]]
    assert differs(refs[r2], R.fit64(X, c0, R.TOL_CASE.tol, centres_from_previous_labels=True))
    assert differs(refs[r2], R.fit64(X, c0, R.TOL_CASE.tol, unscaled_tol=True))
    assert differs(refs[r2], R.fit64(X, c0, R.TOL_CASE.tol, no_final_relabel=True))
    table = np.array([[3, 0, 3, 1], [0, 2, 2, 0], [1, 0, 0, 0]])
    assert not np.array_equal(R.vote64(table), R.vote64(table, last_max=True))
