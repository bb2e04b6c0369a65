"""The batched k-means of csrc/kmeans.hip on the GPU: the mvk_kmeans_* entry points through the C ABI against the float64 restatement
of tests/kmeans_ref.py, multivae_amd.metrics.latent_clustering.DeviceKMeans, and multivae_amd.metrics.Clustering end to end.

The bar (kmeans_ref.BAR) is the project's parity bar, 1e-4: max|got - ref| / max|ref| per tensor; labels, counts, iteration counts
and the convergence code are compared exactly.  test_kmeans_host.py shows that kmeans_ref IS scikit-learn's Lloyd iteration and
that no row of any case lies within 16 fp32 errors of a tie, so exact labels are a fair demand.

1. test_assign_cases: N in {1, 37, 257, 1003} x L in {1, 2, 20, 33, 64} x K in {1, 3, 10, 64} x R in {1, 3, 20, 32}, pruned (K > N and a
   y outside the classes included): labels, table, majority, correct exact; d2 and inertia within the bar; two calls accumulate
   to one call on the concatenation; a second launch is bit-identical.
2. test_step: one step from given centres, every state field; the empty cluster keeps its bits and EMPTY is 1.
3. test_fit_cases: R initialisations that stop at different iterations; test_freeze_check_every_and_max_iter: a stopped run keeps
   its bits while the others go on, check_every 1 and 8 give the same bits, later steps change nothing, max_iter cuts a fit short.
4. test_batch_independence: run r of an R = 20 fit against the same centres fitted alone.
5. test_seeding.  6. test_end_to_end.  7. test_errors_and_argument_checks.  8. test_mutated_reference_is_rejected.

Largest distance of the HIP kernels from float64 on an MI355X, per tensor, with the case that set it (test_zz_report prints
HIP_MEASURED; the bar is 1e-4):
    assign: d2 4.17e-07 (n257-l64-k1-r20-c5), inertia 1.08e-07 (n1-l64-k64-r3-c5)
    step: centers 4.08e-08 (n1003-l33-k10-s0 run 0 step 1), inertia 3.78e-09 (n1003-l33-k10-s0 run 2 step 1), shift 1.58e-08
        (n1003-l33-k10-s0 run 0 step 2)
    fit: centers 4.43e-08 (n1003-l20-k10-s2 run 0), inertia 1.04e-08 (n1003-l33-k10-s0 run 0)
Labels, tables, majorities, correct counts, n_iter_ and converged_ were equal to the float64 restatement on every case.
"""
import ctypes

import numpy as np
import pytest
import torch

import kmeans_ref as R

pytestmark = pytest.mark.gpu
D = torch.device("cuda:0")
MEASURED = {}


def _mods():
    from multivae_amd import _lib, kernels

    return _lib, kernels


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=D, dtype=dtype).contiguous()


def host(t):
    return t.detach().cpu().double().numpy()


def full(shape, value, dtype):
    return torch.full(shape, value, dtype=dtype, device=D)


def note(key, value, name):
    if value > MEASURED.get(key, (-1.0, ""))[0]:
        MEASURED[key] = (value, name)


def same_bits(a, b):
    if a.dtype == torch.float32:
        return torch.equal(a.view(torch.int32), b.view(torch.int32))
    if a.dtype == torch.float64:
        return torch.equal(a.view(torch.int64), b.view(torch.int64))
    return torch.equal(a, b)


# ---- 1. assign ------------------------------------------------------------------------------------------------------------
def assign_launch(case, x, c, y, majority=None):
    """Every output of one mvk_kmeans_assign of the case, from buffers pre-filled with NaN / -1 (the accumulated ones with 0)."""
    _, K = _mods()
    R_, N, C = case.R, case.N, case.n_classes
    scratch = K.kmeans_scratch(case.L, case.K, R_, D)
    scratch.fill_(float("nan"))
    out = dict(labels=full((R_, N), -1, torch.int32), d2=full((R_, N), float("nan"), torch.float32),
               inertia=full((R_,), float("nan"), torch.float64), table=full((R_, case.K, C + 1), 0, torch.int64),
               correct=full((R_,), 0, torch.int64))
    K.kmeans_assign(x, c, scratch, labels=out["labels"], d2=out["d2"], y=y, n_classes=C, table=out["table"], inertia=out["inertia"],
                    majority=majority, correct=out["correct"] if majority is not None else None)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", R.ASSIGN_CASES, ids=lambda c: c.name)
def test_assign_cases(case):
    _, K = _mods()
    X, centers, y = case.make()
    x, c, yy = dev(X), dev(centers), dev(y, torch.int32)
    got = assign_launch(case, x, c, yy)
    majority = full((case.R, case.K), -7, torch.int32)
    K.kmeans_vote(got["table"], majority)
    scored, again = assign_launch(case, x, c, yy, majority), assign_launch(case, x, c, yy, majority)
    for k in scored:
        assert same_bits(scored[k], again[k]), f"{k}: a second launch differs"
        assert k == "correct" or same_bits(scored[k], got[k]), k
    assert not bool(torch.isnan(got["d2"]).any()) and not bool(torch.isnan(got["inertia"]).any())
    d = dict(d2=0.0, inertia=0.0)
    for r in range(case.R):
        lab64, d1, _ = R.assign64(X, centers[r])
        assert np.array_equal(got["labels"][r].cpu().numpy(), lab64), f"run {r}: labels"
        t64 = R.table64(lab64, y, case.K, case.n_classes)
        assert np.array_equal(got["table"][r].cpu().numpy(), t64), f"run {r}: table"
        m64 = R.vote64(t64)
        assert np.array_equal(majority[r].cpu().numpy(), m64), f"run {r}: majority"
        assert int(scored["correct"][r]) == R.accuracy64(m64, lab64, y), f"run {r}: correct"
        d["d2"] = max(d["d2"], R.rel(host(got["d2"][r]), d1))
        d["inertia"] = max(d["inertia"], abs(float(got["inertia"][r]) - d1.sum()) / d1.sum())
    assert int(got["table"].sum()) == case.R * case.N and int(got["table"][:, :, -1].sum()) == case.R * int(np.sum((y < 0) | (y >= case.n_classes)))
    print(case.name, {k: f"{v:.2e}" for k, v in d.items()})
    for k, v in d.items():
        note("assign " + k, v, case.name)
        assert v <= R.BAR, f"{case.name}: {k} is {v:.3g} from float64"
    if case.N >= 2:  # two calls on the two parts of the rows accumulate to one call on all of them
        n0 = case.N // 3 + 1
        table, correct = torch.zeros_like(got["table"]), torch.zeros_like(scored["correct"])
        for a, b in ((0, n0), (n0, case.N)):
            K.kmeans_assign(x[a:b], c, y=yy[a:b], n_classes=case.n_classes, table=table, majority=majority, correct=correct)
        assert torch.equal(table, got["table"]) and torch.equal(correct, scored["correct"])


# ---- 2. step --------------------------------------------------------------------------------------------------------------
def run_steps(X, c0, tol_abs, n_steps):
    """n_steps mvk_kmeans_step from the centres c0 [R,K,L]; returns the (centres, labels, state) after every step."""
    _, K = _mods()
    x, c = dev(X), dev(c0)
    R_, Kc, L = c.shape
    labels, state = full((R_, len(X)), -1, torch.int32), K.kmeans_new_state(R_, D)
    scratch = K.kmeans_scratch(L, Kc, R_, D)
    scratch.fill_(float("nan"))
    tol = torch.tensor(tol_abs, dtype=torch.float64, device=D)
    snaps = []
    for _ in range(n_steps):
        K.kmeans_step(x, tol, c, labels, state, scratch)
        snaps.append((c.clone(), labels.clone(), state.clone()))
    torch.cuda.synchronize()
    return snaps


def test_step():
    L_, _ = _mods()
    S = L_.KMEANS_STATE
    case = R.FIT_CASES[1]
    X, idx = case.make()
    tol_abs = R.scaled_tol(X)
    snaps = run_steps(X, X[idx], tol_abs, 2)
    for r in range(case.R):
        cen, lab = X[idx[r]], np.full(case.N, -1)
        for i, (c, labels, state) in enumerate(snaps):
            s = R.step64(X, cen, lab, tol_abs)
            st = state[r].cpu().numpy()
            assert np.array_equal(labels[r].cpu().numpy(), s["labels"])
            assert st[S["iter"]] == i + 1 and st[S["converged"]] == s["converged"] == 0 and st[S["changed"]] == s["changed"]
            assert st[S["empty"]] == 0 and st[6] == 0 and st[7] == 0
            d = dict(centers=R.rel(host(c[r]), s["centers"]), inertia=abs(st[S["inertia"]] - s["inertia"]) / s["inertia"],
                     shift=abs(st[S["shift"]] - s["shift"]) / s["shift"])
            for k, v in d.items():
                note("step " + k, v, f"{case.name} run {r} step {i + 1}")
                assert v <= R.BAR, (k, v)
            cen, lab = s["centers"], s["labels"]
    # a cluster without rows keeps the bits of its centre and is counted
    X, c0 = R.empty_case()
    c, labels, state = run_steps(X, c0[None], R.scaled_tol(X), 1)[0]
    s = R.step64(X, c0, np.full(len(X), -1), R.scaled_tol(X))
    st = state[0].cpu().numpy()
    assert same_bits(c[0, 3], dev(c0[3])) and st[S["empty"]] == 1 and st[S["iter"]] == 1 and st[S["converged"]] == 0
    assert np.array_equal(labels[0].cpu().numpy(), s["labels"]) and R.rel(host(c[0]), s["centers"]) <= R.BAR
    assert abs(st[S["shift"]] - s["shift"]) <= R.BAR * s["shift"]


# ---- 3. fit ---------------------------------------------------------------------------------------------------------------
_FITS = {}


def device_fit(case, check_every=8, max_iter=300):
    """The fit of a case from its initial rows: run once per (case, check_every, max_iter), shared, left unchanged."""
    from multivae_amd.metrics.latent_clustering import DeviceKMeans

    key = (case.name, check_every, max_iter)
    if key not in _FITS:
        X, idx = case.make()
        _FITS[key] = DeviceKMeans(case.K, n_runs=case.R, tol=case.tol, check_every=check_every, max_iter=max_iter).fit(
            dev(X), init_indices=idx)
    return _FITS[key]


@pytest.mark.parametrize("case", R.FIT_CASES + [R.TOL_CASE], ids=lambda c: c.name)
def test_fit_cases(case):
    X, idx, refs = R.fit_reference(case)
    g = device_fit(case)
    assert g.cluster_centers_.shape == (case.R, case.K, case.L) and g.labels_.shape == (case.R, case.N) and g.inertia_.shape == (case.R,)
    assert np.array_equal(g.init_indices_.cpu().numpy(), idx)
    for r, ref in enumerate(refs):
        assert int(g.n_iter_[r]) == ref["n_iter"] and int(g.converged_[r]) == ref["converged"] and int(g.n_empty_[r]) == 0, (r, g.n_iter_, ref["n_iter"])
        assert np.array_equal(g.labels_[r].cpu().numpy(), ref["labels"])
        d = dict(centers=R.rel(host(g.cluster_centers_[r]), ref["centers"]), inertia=abs(float(g.inertia_[r]) - ref["inertia"]) / ref["inertia"])
        print(case.name, r, "n_iter", ref["n_iter"], "converged", ref["converged"], {k: f"{v:.2e}" for k, v in d.items()})
        for k, v in d.items():
            note("fit " + k, v, f"{case.name} run {r}")
            assert v <= R.BAR, f"{case.name} run {r}: {k} is {v:.3g} from float64"
        assert np.array_equal(g.predict(dev(X[:50]))[r].cpu().numpy(), R.assign64(X[:50], ref["centers"])[0])


def test_freeze_check_every_and_max_iter():
    L_, _ = _mods()
    S = L_.KMEANS_STATE
    case = R.TOL_CASE
    X, idx, refs = R.fit_reference(case)
    iters = [r["n_iter"] for r in refs]
    assert len(set(iters)) > 1
    snaps = run_steps(X, X[idx], R.scaled_tol(X, case.tol), max(iters) + 3)
    for r, ref in enumerate(refs):
        stop = ref["n_iter"]  # the run stops in this step: from then on every bit stays
        c0, l0, s0 = snaps[stop - 1]
        assert s0[r, S["converged"]] == ref["converged"] and s0[r, S["iter"]] == stop
        assert stop == 1 or snaps[stop - 2][2][r, S["converged"]] == 0
        for c, labels, state in snaps[stop:]:
            assert same_bits(c[r], c0[r]) and torch.equal(labels[r], l0[r]) and same_bits(state[r], s0[r]), f"run {r} moved after it stopped"
    # steps enqueued after every run has stopped change nothing at all
    last, before = snaps[-1], snaps[max(iters) - 1]
    assert all(same_bits(a, b) for a, b in zip(last, before))
    # check_every 1 and 8: the same bits, and the bits of the steps taken by hand
    a, b = device_fit(case, 8), device_fit(case, 1)
    for k in ("cluster_centers_", "labels_", "inertia_"):
        assert same_bits(getattr(a, k), getattr(b, k)), k
    assert torch.equal(a.n_iter_, b.n_iter_) and torch.equal(a.converged_, b.converged_)
    assert same_bits(a.cluster_centers_, last[0])
    # max_iter cuts a fit short
    cut = device_fit(case, 8, max_iter=2)
    assert all(int(v) == 2 for v in cut.n_iter_) and all(int(v) == 0 for v in cut.converged_)
    assert same_bits(cut.cluster_centers_, snaps[1][0])


# ---- 4. independence of the batch -----------------------------------------------------------------------------------------
def test_batch_independence():
    from multivae_amd.metrics.latent_clustering import DeviceKMeans

    case = R.BATCH_CASE
    X, idx = case.make()
    x = dev(X)
    whole = device_fit(case)
    assert len(set(int(v) for v in whole.n_iter_)) > 3
    for r in (0, 9, 19):
        alone = DeviceKMeans(case.K, n_runs=1).fit(x, init_indices=idx[r:r + 1])
        assert int(alone.n_iter_[0]) == int(whole.n_iter_[r]) and int(alone.converged_[0]) == int(whole.converged_[r])
        assert int(alone.n_empty_[0]) == int(whole.n_empty_[r])
        assert same_bits(alone.cluster_centers_[0], whole.cluster_centers_[r]), f"run {r}: centres"
        assert torch.equal(alone.labels_[0], whole.labels_[r]) and same_bits(alone.inertia_[0], whole.inertia_[r]), f"run {r}"


# ---- 5. seeding -----------------------------------------------------------------------------------------------------------
def test_seeding():
    from multivae_amd.metrics.latent_clustering import DeviceKMeans

    X, blob, _ = R.blobs(1003, 8, 5, 11)
    x = dev(X)
    fits = [DeviceKMeans(5, n_runs=3).fit(x, generator=torch.Generator(device=D).manual_seed(123)) for _ in range(2)]
    s = [f.init_indices_.cpu().numpy() for f in fits]
    assert np.array_equal(s[0], s[1]) and s[0].shape == (3, 5) and s[0].min() >= 0 and s[0].max() < 1003
    assert all(len(set(row.tolist())) == 5 for row in s[0]) and same_bits(fits[0].cluster_centers_, fits[1].cluster_centers_)
    assert all(int(v) in (1, 2) for v in fits[0].converged_)
    other = DeviceKMeans(5, n_runs=3).fit(x, generator=torch.Generator(device=D).manual_seed(124)).init_indices_.cpu().numpy()
    assert not np.array_equal(other, s[0])
    # fewer distinct rows than clusters: the draw meets an all-zero row of distances and the fit still finishes
    few = dev(np.repeat(X[:3], 7, axis=0))
    g = DeviceKMeans(5, n_runs=2).fit(few, generator=torch.Generator(device=D).manual_seed(5))
    assert bool(torch.isfinite(g.cluster_centers_).all()) and bool(((g.labels_ >= 0) & (g.labels_ < 5)).all())
    assert all(int(v) >= 1 for v in g.n_empty_) and float(g.inertia_.max()) == 0.0


# ---- 6. end to end --------------------------------------------------------------------------------------------------------
def _dataset(n, seed, labelled=True):
    from multivae_amd.data.datasets.base import MultimodalBaseDataset

    g = torch.Generator().manual_seed(seed)
    labels = torch.randint(0, 3, (n,), generator=g)
    a = torch.rand(n, 12, generator=g) * 0.3 + labels[:, None].float() * 0.35
    b = torch.rand(n, 2, 5, generator=g) * 0.3 + labels[:, None, None].float() * 0.35
    return MultimodalBaseDataset(data=dict(a=a, b=b), labels=labels if labelled else None)


def _restated_accuracy(ev, model, test, use_majority=True):
    """The evaluator's number from float64: the recorded training embedding and seed rows, fit64 per run, the vote, the test rows."""
    from multivae_amd.data.utils import set_inputs_to_device
    from torch.utils.data import DataLoader

    z, idx = host(ev.train_z_), ev.kmeans[0].init_indices_.cpu().numpy()
    y = ev.train_y_.cpu().numpy().astype(np.int64) if ev.train_y_ is not None else None
    zt, yt = [], []
    for inputs in DataLoader(test, batch_size=ev.batch_size):
        zt.append(host(model.encode(set_inputs_to_device(inputs, "cuda"), "all", return_mean=True).z))
        yt.append(inputs.labels.numpy())
    zt, yt = np.concatenate(zt), np.concatenate(yt)
    accs = []
    for i in idx:
        ref = R.fit64(z, z[i])
        maj = R.vote64(R.table64(ref["labels"], y, ev.n_clusters, ev.n_classes)) if y is not None else np.arange(ev.n_clusters)
        accs.append(R.accuracy64(maj, R.assign64(zt, ref["centers"])[0], yt) / len(yt))
    return float(np.mean(accs))


def test_end_to_end(tmp_path):
    from multivae_amd.metrics import Clustering, ClusteringConfig
    from multivae_amd.models import MoPoE, MoPoEConfig

    torch.manual_seed(0)
    model = MoPoE(MoPoEConfig(n_modalities=2, latent_dim=6, input_dims=dict(a=(12,), b=(2, 5))))
    train, test = _dataset(230, 0), _dataset(97, 1)
    ev = Clustering(model, test, train, output=str(tmp_path), eval_config=ClusteringConfig(batch_size=64, n_clusters=3, number_of_runs=3))
    ev.generator = torch.Generator(device=D).manual_seed(3)
    out = ev.eval()
    acc = out.cluster_accuracy
    assert isinstance(acc, float) and 0.0 <= acc <= 1.0 and ev.metrics["cluster_accuracy"] == acc
    assert ev.train_z_.shape == (230, 6) and ev.cluster_centers_.shape == (3, 3, 6) and ev.n_classes == 3
    assert int(ev.table.sum()) == 3 * 230 and int(ev.table[:, :, -1].sum()) == 0
    # the training embedding is the model's own, in the loader's shuffled order
    from multivae_amd.data.utils import set_inputs_to_device
    from torch.utils.data import DataLoader

    own = np.concatenate([host(model.encode(set_inputs_to_device(b, "cuda"), "all", return_mean=True).z) for b in DataLoader(train, batch_size=64)])
    assert np.allclose(np.sort(own, axis=0), np.sort(host(ev.train_z_), axis=0), rtol=0, atol=1e-5)
    want = _restated_accuracy(ev, model, test)
    print("cluster accuracy", acc, "restated", want)
    assert abs(acc - want) <= 1e-12
    ev.finish()
    log = (tmp_path / "metrics.log").read_text()
    assert "Cluster accuracy is" in log
    # unlabelled training data: every cluster maps to its own index
    ev2 = Clustering(model, test, _dataset(230, 0, labelled=False), eval_config=ClusteringConfig(batch_size=64, n_clusters=3, number_of_runs=2))
    ev2.generator = torch.Generator(device=D).manual_seed(4)
    acc2 = ev2.eval().cluster_accuracy
    assert ev2.train_y_ is None and torch.equal(ev2.majority.cpu(), torch.arange(3, dtype=torch.int32).repeat(2, 1))
    assert abs(acc2 - _restated_accuracy(ev2, model, test)) <= 1e-12
    ev2.finish()
    # sampled embeddings: a fresh embedding and a fit of its own per run
    ev3 = Clustering(model, test, train, eval_config=ClusteringConfig(batch_size=64, n_clusters=3, number_of_runs=2, use_mean=False))
    acc3 = ev3.eval().cluster_accuracy
    assert 0.0 <= acc3 <= 1.0 and len(ev3.kmeans) == 2 and ev3.cluster_centers_.shape == (2, 3, 6)
    ev3.finish()
    # 40 runs: two groups of at most 32
    ev4 = Clustering(model, test, train, eval_config=ClusteringConfig(batch_size=64, n_clusters=3, number_of_runs=40))
    ev4.generator = torch.Generator(device=D).manual_seed(6)
    acc4 = ev4.eval().cluster_accuracy
    assert ev4.cluster_centers_.shape == (40, 3, 6) and ev4.kmeans[0].init_indices_.shape == (40, 3)
    assert abs(acc4 - _restated_accuracy(ev4, model, test)) <= 1e-12
    ev4.finish()
    # num_samples_for_fit: no further batch once more than that many rows are embedded
    ev5 = Clustering(model, test, train, eval_config=ClusteringConfig(batch_size=64, n_clusters=3, number_of_runs=1, num_samples_for_fit=100))
    ev5.fit_clustering()
    assert ev5.train_z_.shape[0] == 128
    ev5.finish()
    # a test set without labels
    ev6 = Clustering(model, _dataset(20, 2, labelled=False), train, eval_config=ClusteringConfig(batch_size=64, n_clusters=3, number_of_runs=1))
    with pytest.raises(AttributeError, match="without labels"):
        ev6.eval()
    ev6.finish()


# ---- 7. errors ------------------------------------------------------------------------------------------------------------
def test_errors_and_argument_checks():
    L_, K = _mods()
    lib, sp, ptr = L_.load(), L_.stream_ptr, L_.ptr
    EINVAL = -1
    X, _, _ = R.blobs(300, 5, 3, 1)
    x, c = dev(X), dev(X[:6].reshape(2, 3, 5))
    labels, d2 = full((2, 300), -1, torch.int32), full((2, 300), float("nan"), torch.float32)
    y, table = torch.zeros(300, dtype=torch.int32, device=D), torch.zeros(2, 3, 5, dtype=torch.int64, device=D)
    majority, correct = torch.zeros(2, 3, dtype=torch.int32, device=D), torch.zeros(2, dtype=torch.int64, device=D)
    inertia, state = full((2,), float("nan"), torch.float64), K.kmeans_new_state(2, D)
    scratch, tol = K.kmeans_scratch(5, 3, 2, D), torch.zeros((), dtype=torch.float64, device=D)
    c_before = c.clone()

    def assign(N=300, L=5, Kc=3, R_=2, x=x, c=c, labels=labels, d2=d2, y=y, nc=4, table=table, maj=majority, cor=correct, ine=inertia, sc=scratch):
        return lib.mvk_kmeans_assign(ptr(x), N, L, Kc, R_, ptr(c), ptr(labels), ptr(d2), ptr(y), nc, ptr(table), ptr(maj), ptr(cor), ptr(ine),
                                     ptr(sc), sp())

    def step(N=300, L=5, Kc=3, R_=2, x=x, tol=tol, c=c, labels=labels, state=state, sc=scratch):
        return lib.mvk_kmeans_step(ptr(x), N, L, Kc, R_, ptr(tol), ptr(c), ptr(labels), ptr(state), ptr(sc), sp())

    def vote(table=table, R_=2, Kc=3, nc=4, maj=majority):
        return lib.mvk_kmeans_vote(ptr(table), R_, Kc, nc, ptr(maj), sp())

    n64 = ctypes.c_int64(-5)
    sb = lib.mvk_kmeans_scratch_bytes
    for bad in ((0, 3, 2), (65, 3, 2), (5, 0, 2), (5, 65, 2), (5, 3, 0), (5, 3, 33)):
        assert sb(*bad, ctypes.byref(n64)) == EINVAL, bad
    assert sb(5, 3, 2, None) == EINVAL and n64.value == -5
    assert sb(64, 64, 32, ctypes.byref(n64)) == 0 and 0 < n64.value < 64 << 20 and n64.value % 8 == 0
    for f in (assign, step):
        assert f(L=0) == EINVAL and f(L=65) == EINVAL and f(Kc=0) == EINVAL and f(Kc=65) == EINVAL, f.__name__
        assert f(R_=0) == EINVAL and f(R_=33) == EINVAL and f(N=-1) == EINVAL and f(x=None) == EINVAL and f(c=None) == EINVAL, f.__name__
    assert assign(y=None) == EINVAL and assign(nc=0) == EINVAL and assign(nc=(1 << 24) + 1) == EINVAL  # a table needs y and classes
    assert assign(table=None, y=None) == EINVAL                                                        # correct needs y
    assert assign(maj=None) == EINVAL and assign(sc=None) == EINVAL                                    # ... and majority; inertia needs scratch
    assert step(tol=None) == EINVAL and step(labels=None) == EINVAL and step(state=None) == EINVAL and step(sc=None) == EINVAL
    assert vote(table=None) == EINVAL and vote(maj=None) == EINVAL and vote(R_=0) == EINVAL and vote(R_=33) == EINVAL
    assert vote(Kc=0) == EINVAL and vote(Kc=65) == EINVAL and vote(nc=0) == EINVAL
    assert assign(N=0) == 0 and step(N=0) == 0
    torch.cuda.synchronize()
    assert bool((labels == -1).all()) and bool(torch.isnan(d2).all()) and bool(torch.isnan(inertia).all()) and int(table.sum()) == 0
    assert int(correct.sum()) == 0 and bool((state == 0).all()) and same_bits(c, c_before)
    # every output is optional, and the wrappers refuse what the ABI refuses
    assert assign(labels=None, d2=None, y=None, table=None, maj=None, cor=None, ine=None, sc=None) == 0
    with pytest.raises(L_.MvkError):
        K.kmeans_assign(x, c, table=table, n_classes=4)
    from multivae_amd.metrics.latent_clustering import DeviceKMeans

    with pytest.raises(ValueError):
        DeviceKMeans(3, n_runs=2).fit(x, init_indices=[[0, 1, 2]])
    with pytest.raises(ValueError):
        DeviceKMeans(3, n_runs=1).fit(x, init_centers=np.zeros((1, 3, 4)))
    with pytest.raises(L_.MvkError):
        DeviceKMeans(3).fit(x.cpu())


# ---- 8. mutations ---------------------------------------------------------------------------------------------------------
def test_mutated_reference_is_rejected():
    """The comparisons of test_fit_cases with one deliberate mistake in the REFERENCE must fail on the kernel's output."""
    _, K = _mods()
    case = R.TOL_CASE
    X, idx, refs = R.fit_reference(case)
    g = device_fit(case)
    r = [i for i in range(case.R) if refs[i]["converged"] == 2][0]

    def matches(ref):
        return (int(g.n_iter_[r]) == ref["n_iter"] and np.array_equal(g.labels_[r].cpu().numpy(), ref["labels"])
                and R.rel(host(g.cluster_centers_[r]), ref["centers"]) <= R.BAR
                and abs(float(g.inertia_[r]) - ref["inertia"]) <= R.BAR * ref["inertia"])

    assert matches(refs[r])
    for mutation in ("centres_from_previous_labels", "unscaled_tol", "no_final_relabel"):
        assert not matches(R.fit64(X, X[idx[r]], case.tol, **{mutation: True})), mutation
    table = np.array([[[3, 0, 3, 1], [0, 2, 2, 0], [1, 0, 0, 0]]])
    majority = full((1, 3), -7, torch.int32)
    K.kmeans_vote(dev(table, torch.int64), majority)
    assert np.array_equal(majority[0].cpu().numpy(), R.vote64(table[0]))
    assert not np.array_equal(majority[0].cpu().numpy(), R.vote64(table[0], last_max=True))


def test_zz_report():
    for k in sorted(MEASURED):
        print("HIP_MEASURED", k, f"{MEASURED[k][0]:.2e}", MEASURED[k][1])
