"""csrc/ssim.hip through the C ABI against the float64 definition of tests/ssim_ref.py, and the three evaluators of
multivae_amd.metrics end to end on tiny models.

Bars.  Per-image SSIM: |got - float64| <= 5e-6 in every regime (ssim_ref.BAR), the flat ones included -- about 15x the worst fp32
figure of well-conditioned inputs and 5x below what the un-centred E[x^2] - mu^2 form loses on the flat case.  sse_rows: relative
1e-6.  R: exactly the fp32 value of the definition.  Accumulate: 1e-12 relative against the float64 sum of the rows.  Evaluators:
the project's parity bar 1e-4 for Reconstruction, bit-identity for the likelihoods, exact counts for the coherences.

1. test_kernel_cases: ssim_ref.shapes x ssim_ref.REGIMES (7 shapes x 7 regimes; single window, H != W, the shipped 28 / 32 / 64, and [2,2,T+1,T+11]
   which crosses a tile boundary into a one-wide remainder tile), outputs pre-filled with NaN, a second run bit-identical, the
   by-value range path bit-identical to the device-range path.
2. R depends on the batch; R = 0 gives NaN rows and finite sse_rows; a NaN pixel gives R = NaN.
3. The squared-error-only path leaves ssim_rows untouched; every MVK_EINVAL branch; the accumulate entry on 3 + 3 + 1 rows.
4. Reconstruction (SSIM and MSE), LikelihoodsEvaluator, joint_nll_from_subset and CoherenceEvaluator on a 7-row dataset with
   input_dims a: (1,12,12), b: (3,11,13) and batch_size 3.

Largest distance of the HIP kernels from float64 on an MI355X per regime, with the case that set it (test_zz_report prints
HIP_MEASURED; first GPU run of the kernel):
    per-image SSIM (bar 5e-6): uniform 5.21e-08 (1x1x11x11), near 1.91e-07 (1x1x11x11), binary 3.38e-08 (2x1x11x13), square 5.65e-08
        (2x1x11x13), scaled255 6.67e-08 (2x1x12x11), flat 8.73e-08 (2x1x12x11), patch 8.16e-08 (2x1x11x13)
    sse_rows, relative (bar 1e-6): uniform 5.25e-08, near 5.04e-08, binary 5.58e-08, square 3.01e-08, scaled255 3.99e-08, flat 4.53e-08,
        patch 4.74e-08
    Reconstruction against the float64 aggregate of the recorded updates, relative (bar 1e-4): SSIM 1.91e-07, MSE 3.93e-08
"""
import ctypes

import numpy as np
import pytest
import torch

import ssim_ref as R

pytestmark = pytest.mark.gpu
D = torch.device("cuda:0")
MEASURED = {}
EINVAL = -1


def _mods():
    from multivae_amd import _lib, kernels

    return _lib, kernels


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=D, dtype=dtype).contiguous()


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=D)


def host(t):
    return t.detach().cpu().double().numpy()


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def note(key, value, name):
    if value > MEASURED.get(key, (-1.0, ""))[0]:
        MEASURED[key] = (value, name)


def _tile():
    return _mods()[1].ssim_tile()


def run_rows(p, t, data_range=None):
    """(R, ssim_rows, sse_rows) of one update from NaN-filled buffers and NaN-filled scratch."""
    _, K = _mods()
    B = p.shape[0]
    scratch = K.ssim_scratch(*p.shape, D)
    scratch.fill_(float("nan"))
    rng = K.ssim_range(p, t, scratch, out=nan(1))
    ssim, sse = K.ssim_rows(p, t, scratch, data_range=rng if data_range is None else data_range, ssim_out=nan(B), sse_out=nan(B))
    torch.cuda.synchronize()
    return rng, ssim, sse


@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("shape_index", range(7))
def test_kernel_cases(shape_index, regime):
    shape = R.shapes(_tile())[shape_index]  # [5] is [2,2,T+1,T+11] for the kernel's own tile edge T
    name = f"{regime}-{'x'.join(map(str, shape))}"
    p64, t64 = R.make(regime, shape)
    ref = R.ssim64(p64, t64)
    p, t = dev(p64), dev(t64)
    rng, ssim, sse = run_rows(p, t)
    rng2, ssim2, sse2 = run_rows(p, t)
    assert same_bits(rng, rng2) and same_bits(ssim, ssim2) and same_bits(sse, sse2), "a second run differs"
    _, ssim3, sse3 = run_rows(p, t, data_range=float(rng))
    assert same_bits(ssim, ssim3) and same_bits(sse, sse3), "the by-value range path differs from the device-range path"
    assert float(rng) == float(R.data_range(p64, t64)), "R is not the fp32 value of the definition"
    e_ssim = float(np.max(np.abs(host(ssim) - ref["rows"])))
    s64 = R.sse64(p64, t64)
    e_sse = float(np.max(np.abs(host(sse) - s64) / s64))
    print(name, f"ssim {e_ssim:.2e} sse {e_sse:.2e}")
    note("ssim " + regime, e_ssim, name)
    note("sse " + regime, e_sse, name)
    assert e_ssim <= R.BAR, f"{name}: per-image SSIM is {e_ssim:.3g} from float64"
    assert e_sse <= R.SSE_BAR, f"{name}: sse_rows is {e_sse:.3g} (relative) from float64"


def test_range_depends_on_the_batch():
    rng = np.random.default_rng(3)
    img = (0.25 + 0.5 * rng.random((1, 1, 28, 28))).astype(np.float32)
    rec = (img + 0.05 * rng.standard_normal(img.shape)).astype(np.float32)
    wide = (2.0 * rng.random((1, 1, 28, 28))).astype(np.float32)
    alone = R.ssim64(rec, img)
    p2, t2 = np.concatenate([rec, wide]), np.concatenate([img, wide[:, :, ::-1].copy()])
    both = R.ssim64(p2, t2)
    assert abs(alone["rows"][0] - both["rows"][0]) > 100 * R.BAR  # the two reference values differ
    r1, s1, _ = run_rows(dev(rec), dev(img))
    r2, s2, _ = run_rows(dev(p2), dev(t2))
    assert float(r1) == float(R.data_range(rec, img)) and float(r2) == float(R.data_range(p2, t2)) and float(r2) > float(r1)
    assert abs(float(s1[0]) - alone["rows"][0]) <= R.BAR and abs(float(s2[0]) - both["rows"][0]) <= R.BAR
    assert float(np.max(np.abs(host(s2) - both["rows"]))) <= R.BAR


def test_zero_range_and_nan():
    p, t = torch.full((2, 3, 12, 14), 0.25, device=D), torch.full((2, 3, 12, 14), 0.75, device=D)
    rng, ssim, sse = run_rows(p, t)
    assert float(rng) == 0.0 and bool(torch.isnan(ssim).all())
    assert np.allclose(host(sse), 0.25 * 3 * 12 * 14, rtol=1e-6)
    z = torch.zeros(1, 1, 11, 11, device=D)
    rng, ssim, sse = run_rows(z, z)
    assert float(rng) == 0.0 and bool(torch.isnan(ssim).all()) and float(sse[0]) == 0.0
    # NaN propagates: one NaN pixel makes R, and with it every row of the update, NaN
    q = torch.rand(2, 1, 16, 16, device=D)
    bad = q.clone()
    bad[1, 0, 3, 4] = float("nan")
    rng, ssim, _ = run_rows(bad, q)
    assert bool(torch.isnan(rng).all()) and bool(torch.isnan(ssim).all())


def test_mse_only_and_vectors():
    lib_, K = _mods()
    lib, ptr, sp = lib_.load(), lib_.ptr, lib_.stream_ptr
    p64, t64 = R.make("uniform", (5, 1, 28, 28))
    p, t = dev(p64), dev(t64)
    ssim, sse = nan(5), nan(5)
    assert lib.mvk_ssim_rows(ptr(p), ptr(t), 5, 1, 28, 28, None, 0.0, 1, ptr(ssim), ptr(sse), None, sp()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(ssim).all()), "the squared-error-only path wrote ssim_rows"
    s64 = R.sse64(p64, t64)
    assert float(np.max(np.abs(host(sse) - s64) / s64)) <= R.SSE_BAR
    _, _, full = run_rows(p, t)
    assert float(np.max(np.abs(host(full) - host(sse)) / s64)) <= 2 * R.SSE_BAR
    # rows that are no images: [B, D] with D below the window and D not a multiple of anything
    rng = np.random.default_rng(1)
    for shape in ((3, 7), (4, 1031), (2, 3, 5)):
        a, b = rng.random(shape).astype(np.float32), rng.random(shape).astype(np.float32)
        got = host(K.sse_rows(dev(a), dev(b), sse_out=nan(shape[0])))
        assert float(np.max(np.abs(got - R.sse64(a, b)) / R.sse64(a, b))) <= R.SSE_BAR, shape


def test_invalid_arguments():
    lib_, K = _mods()
    lib, ptr, sp = lib_.load(), lib_.ptr, lib_.stream_ptr
    p, t = torch.rand(2, 2, 12, 13, device=D), torch.rand(2, 2, 12, 13, device=D)
    scratch, rng, ssim, sse = K.ssim_scratch(2, 2, 12, 13, D), nan(1), nan(2), nan(2)
    acc = torch.zeros(3, dtype=torch.float64, device=D)
    n64 = ctypes.c_int64(-5)

    def sb(B=2, C=2, H=12, W=13, out=ctypes.byref(n64)):
        return lib.mvk_ssim_scratch_bytes(B, C, H, W, out)

    def rg(p=p, t=t, n=p.numel(), r=rng, sc=scratch):
        return lib.mvk_ssim_range(ptr(p), ptr(t), n, ptr(r), ptr(sc), sp())

    def rows(p=p, t=t, B=2, C=2, H=12, W=13, r=rng, only=0, ssim=ssim, sse=sse, sc=scratch):
        return lib.mvk_ssim_rows(ptr(p), ptr(t), B, C, H, W, ptr(r), 1.0, only, ptr(ssim), ptr(sse), ptr(sc), sp())

    def accum(ssim=ssim, sse=sse, B=2, acc=acc):
        return lib.mvk_ssim_accumulate(ptr(ssim), ptr(sse), B, ptr(acc), sp())

    assert sb(B=0) == EINVAL and sb(C=0) == EINVAL and sb(H=10) == EINVAL and sb(W=10) == EINVAL and sb(out=None) == EINVAL
    assert sb(B=1 << 30, C=1 << 10) == EINVAL and n64.value == -5  # more tiles than a grid holds
    assert sb() == 0 and n64.value > 0
    assert rg(p=None) == EINVAL and rg(t=None) == EINVAL and rg(r=None) == EINVAL and rg(sc=None) == EINVAL
    assert rg(n=0) == EINVAL and rg(n=-1) == EINVAL
    assert rows(p=None) == EINVAL and rows(t=None) == EINVAL and rows(sse=None) == EINVAL and rows(ssim=None) == EINVAL
    assert rows(sc=None) == EINVAL and rows(B=0) == EINVAL and rows(C=0) == EINVAL and rows(B=-1) == EINVAL
    assert rows(H=10) == EINVAL and rows(W=10) == EINVAL and rows(H=0, only=1) == EINVAL and rows(W=0, only=1) == EINVAL
    assert rows(only=1, sse=None) == EINVAL and rows(only=1, p=None) == EINVAL
    assert accum(sse=None) == EINVAL and accum(acc=None) == EINVAL and accum(B=0) == EINVAL and accum(B=-2) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(ssim).all()) and bool(torch.isnan(sse).all()) and bool(torch.isnan(rng).all()) and bool((acc == 0).all())
    # r = NULL is no error: the range is then taken by value
    assert rows(r=None) == 0 and accum() == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ssim).all()) and float(acc[2]) == 2.0


def test_accumulate():
    _, K = _mods()
    rng = np.random.default_rng(7)
    acc = K.ssim_new_acc(D)
    want = np.zeros(3)
    for n in (3, 3, 1):
        a, b = rng.random(n).astype(np.float32), (1e3 * rng.random(n)).astype(np.float32)
        K.ssim_accumulate(acc, dev(b), dev(a))
        for i in range(n):  # index order, float64
            want[0] += float(a[i])
            want[1] += float(b[i])
        want[2] += n
    got = acc.cpu().numpy()
    assert got[2] == 7.0 and np.all(np.abs(got[:2] - want[:2]) <= 1e-12 * np.abs(want[:2]))
    K.ssim_accumulate(acc, dev(np.ones(300, np.float32)))  # more rows than one pass of the workgroup; no SSIM rows
    got2 = acc.cpu().numpy()
    assert got2[0] == got[0] and got2[2] == 307.0 and abs(got2[1] - (want[1] + 300.0)) <= 1e-12 * got2[1]


# ---- the evaluators ------------------------------------------------------------------------------------------------------------
DIMS = dict(a=(1, 12, 12), b=(3, 11, 13))
N_ROWS, BATCH, CLASSES = 7, 3, 4


def _dataset(labels=True, n=N_ROWS):
    from multivae_amd.data.datasets.base import MultimodalBaseDataset

    g = torch.Generator().manual_seed(11)
    data = {m: torch.rand(n, *DIMS[m], generator=g) for m in DIMS}
    lab = torch.tensor([0, 1, 3, 3, 1, 0, 3]).repeat((n + 6) // 7)[:n]  # class 2 never occurs
    return MultimodalBaseDataset(data=data, labels=lab if labels else None)


_MODELS = {}


def _model(kind):
    """A tiny MLP-architecture model per kind, built once."""
    if kind not in _MODELS:
        from multivae_amd.models import MoPoE, MoPoEConfig, MVTCAE, MVTCAEConfig

        torch.manual_seed(5)
        cls, cfg = dict(mvtcae=(MVTCAE, MVTCAEConfig), mopoe=(MoPoE, MoPoEConfig))[kind]
        _MODELS[kind] = cls(cfg(n_modalities=2, latent_dim=5, input_dims=dict(DIMS))).to(D).eval()
    return _MODELS[kind]


def _record_predict(model, monkeypatch):
    """Wrap model.predict so that the test sees the inputs and what it returned."""
    calls, orig = [], model.predict

    def predict(inputs, *a, **k):
        out = orig(inputs, *a, **k)
        calls.append((inputs, out))
        return out

    monkeypatch.setattr(model, "predict", predict)
    return calls


@pytest.mark.parametrize("metric", ["SSIM", "MSE"])
def test_reconstruction(metric, monkeypatch, tmp_path):
    from multivae_amd._output import ModelOutput
    from multivae_amd.metrics import Reconstruction, ReconstructionConfig

    model = _model("mvtcae")
    ev = Reconstruction(model, _dataset(), str(tmp_path), ReconstructionConfig(batch_size=BATCH, metric=metric))
    calls = _record_predict(model, monkeypatch)
    torch.manual_seed(0)
    out = ev.eval()
    ev.finish()
    assert isinstance(out, ModelOutput) and (tmp_path / "metrics.log").exists()
    subsets = [["a", "b"], ["a"], ["b"]]
    assert list(out.keys()) == [f"{s} reconstruction error ({metric})" for s in subsets]
    assert len(calls) == 9
    at = 0
    for s in subsets:
        updates = []
        for inputs, rec in calls[at:at + 3]:
            updates += [(host(rec[m]), host(inputs.data[m])) for m in s]
        at += 3
        want = R.aggregate(updates, metric)
        got = out[f"{s} reconstruction error ({metric})"]
        assert torch.is_tensor(got) and got.dim() == 0
        gap = abs(float(got) - want) / abs(want)
        note("evaluator " + metric, gap, str(s))
        assert gap <= 1e-4, (s, float(got), want)


def test_reconstruction_ssim_rejects_vectors():
    from multivae_amd.data.datasets.base import MultimodalBaseDataset
    from multivae_amd.metrics import Reconstruction, ReconstructionConfig
    from multivae_amd.models import MVTCAE, MVTCAEConfig

    torch.manual_seed(1)
    model = MVTCAE(MVTCAEConfig(n_modalities=2, latent_dim=4, input_dims=dict(v=(9,), s=(1, 10, 12))))
    g = torch.Generator().manual_seed(2)
    ds = MultimodalBaseDataset(data=dict(v=torch.rand(4, 9, generator=g), s=torch.rand(4, 1, 10, 12, generator=g)))
    ev = Reconstruction(model, ds, None, ReconstructionConfig(batch_size=3))
    with pytest.raises(ValueError, match="modality v"):
        ev.reconstruction_from_subset(["v"])
    with pytest.raises(ValueError, match="modality s"):  # an image, but lower than the window
        ev.reconstruction_from_subset(["s"])
    ev.finish()
    mse = Reconstruction(model, ds, None, ReconstructionConfig(batch_size=3, metric="MSE"))
    assert bool(torch.isfinite(mse.reconstruction_from_subset(["v", "s"])))
    mse.finish()


def test_likelihoods():
    from multivae_amd.data.utils import set_inputs_to_device
    from multivae_amd.metrics import LikelihoodsEvaluator, LikelihoodsEvaluatorConfig

    cfg = LikelihoodsEvaluatorConfig(batch_size=BATCH, num_samples=7, batch_size_k=4)
    model, other = _model("mvtcae"), _model("mopoe")
    ev = LikelihoodsEvaluator(model, _dataset(), None, cfg)
    torch.manual_seed(123)
    got = ev.eval()["joint_likelihood"]
    torch.manual_seed(123)
    want = 0
    for batch in ev.test_loader:
        want += model.compute_joint_nll(set_inputs_to_device(batch, "cuda"), 7, 4)
    want = want / N_ROWS
    assert torch.is_tensor(got) and got.is_cuda and same_bits(got.reshape(1), want.reshape(1)) and bool(torch.isfinite(got))
    assert ev.joint_nll_from_subset(["a"]) is None
    ev.finish()
    # the MoPoE has the subset estimator and a paper estimator
    ev2 = LikelihoodsEvaluator(other, _dataset(), None, cfg)
    torch.manual_seed(9)
    sub = ev2.joint_nll_from_subset(["a"])
    torch.manual_seed(9)
    want = 0
    for batch in ev2.test_loader:
        want += other._compute_joint_nll_from_subset_encoding(["a"], set_inputs_to_device(batch, "cuda"), 7, 4)
    assert same_bits(sub.reshape(1), (want / N_ROWS).reshape(1)) and "Joint likelihood from subset ['a']" in ev2.metrics
    ev2.finish()
    paper = LikelihoodsEvaluator(other, _dataset(), None, LikelihoodsEvaluatorConfig(batch_size=BATCH, num_samples=7, unified_implementation=False))
    torch.manual_seed(4)
    a = paper.joint_nll()
    torch.manual_seed(4)
    want = 0
    for batch in paper.test_loader:
        want += other.compute_joint_nll_paper(set_inputs_to_device(batch, "cuda"), 7, 100)
    assert same_bits(a.reshape(1), (want / N_ROWS).reshape(1))
    paper.finish()


class Linear(torch.nn.Module):
    """A fixed linear classifier on the flattened input."""

    def __init__(self, d, seed):
        super().__init__()
        self.w = torch.nn.Parameter(torch.randn(d, CLASSES, generator=torch.Generator().manual_seed(seed)), requires_grad=False)

    def forward(self, x):
        return (x.reshape(len(x), -1) - 0.5) @ self.w


def _classifiers():
    return dict(a=Linear(144, 1), b=Linear(429, 2))


@pytest.mark.parametrize("n_cross,recon", [(1, False), (2, True)])
def test_coherences(n_cross, recon, monkeypatch):
    from multivae_amd.metrics import CoherenceEvaluator, CoherenceEvaluatorConfig

    model, ds = _model("mvtcae"), _dataset()
    clfs = _classifiers()
    cfg = CoherenceEvaluatorConfig(batch_size=BATCH, num_classes=CLASSES, nb_samples_for_cross=n_cross, include_recon=recon,
                                   nb_samples_for_joint=10, give_details_per_class=True)
    ev = CoherenceEvaluator(model, clfs, ds, None, cfg)
    calls = _record_predict(model, monkeypatch)
    torch.manual_seed(0)
    means, stds = ev.cross_coherences()
    assert len(calls) == 6  # subsets [a] and [b], three batches each
    at, pair_means, per_class_all = 0, [], {}
    for s in (["a"], ["b"]):
        gen = [m for m in DIMS if recon or m not in s]
        count = {m: np.zeros((CLASSES, 2)) for m in gen}
        for inputs, rec in calls[at:at + 3]:
            lab = np.tile(inputs.labels.cpu().numpy(), n_cross)
            for m in gen:
                assert rec[m].shape[0] == len(lab)
                pred = clfs[m](rec[m]).argmax(1).cpu().numpy()
                for y, q in zip(lab, pred):
                    count[m][y] += (int(y == q), 1)
        at += 3
        accs = []
        for m in gen:
            per_class = np.where(count[m][:, 1] > 0, count[m][:, 0] / np.maximum(count[m][:, 1], 1), 0.0).astype(np.float32)
            assert per_class[2] == 0.0  # class 2 never occurs
            accs.append(float(torch.from_numpy(per_class).mean()))
            assert float(ev.metrics[f"{'_'.join(s)}_to_{m}"]) == accs[-1]
            per_class_all.setdefault(tuple(s), []).append(per_class)
        pair_means.append(np.mean(accs))
    details = np.mean(np.stack([np.mean(np.stack(v), axis=0) for v in per_class_all.values()]), axis=0)
    for c in range(CLASSES):
        assert ev.metrics[f"mean_coherence_1_class_{c}"] == details[c]
    assert means == [np.mean(pair_means)] and stds == [np.std(pair_means)]
    assert ev.metrics["mean_coherence_1"] == means[0] and ev.metrics["std_coherence_1"] == stds[0]
    assert ev.metrics["mean_coherence_1_class_2"] == 0.0
    jc = ev.joint_coherence()
    assert torch.is_tensor(jc) and jc.dim() == 0 and 0.0 <= float(jc) <= 1.0 and "joint_coherence_prior" in ev.metrics
    ev.finish()


def test_joint_coherence_from_a_sampler_and_label_errors():
    from multivae_amd.data.datasets.base import DatasetOutput
    from multivae_amd.metrics import CoherenceEvaluator, CoherenceEvaluatorConfig
    from multivae_amd.samplers import GaussianMixtureSampler, GaussianMixtureSamplerConfig

    model = _model("mvtcae")
    cfg = CoherenceEvaluatorConfig(batch_size=4, num_classes=CLASSES, nb_samples_for_joint=10)
    sampler = GaussianMixtureSampler(model, GaussianMixtureSamplerConfig(n_components=2))
    with pytest.raises(AttributeError, match="not fitted"):
        CoherenceEvaluator(model, _classifiers(), _dataset(), None, cfg, sampler=sampler)
    sampler.fit(_dataset(n=64), generator=torch.Generator(device=D).manual_seed(3))
    ev = CoherenceEvaluator(model, _classifiers(), _dataset(), None, cfg, sampler=sampler)
    out = ev.eval()
    key = f"joint_coherence_{sampler.name}"
    assert key in out and 0.0 <= float(out[key]) <= 1.0 and "mean_coherence_1" in out
    ev.finish()
    no_labels = CoherenceEvaluator(model, _classifiers(), _dataset(labels=False), None, cfg)
    with pytest.raises(AttributeError, match="on a dataset without labels"):
        no_labels.coherence_from_subset(["a"])
    no_labels.test_loader = [DatasetOutput(data={m: torch.rand(2, *DIMS[m]) for m in DIMS}, labels=None)]
    with pytest.raises(AttributeError, match="None instead of tensor labels"):
        no_labels.coherence_from_subset(["a"])
    no_labels.finish()


def test_zz_report():
    for k in sorted(MEASURED):
        print("HIP_MEASURED", k, f"{MEASURED[k][0]:.2e}", MEASURED[k][1])
