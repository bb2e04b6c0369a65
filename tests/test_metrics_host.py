"""multivae_amd.metrics without a GPU: that tests/ssim_ref.py states the SSIM definition of DESIGN.md ("Metrics"), what the bar of
test_gpu_metrics.py separates, and the host logic of the evaluators on duck-typed models.

1. ssim_ref.ssim64 (window view + einsum) agrees to 1e-12 per image with ssim_ref.ssim64_loops (121 explicit shifted sums) on every
   case (per position too, except where float64's own E[xx] - mu^2 rounding is larger: 1e-11 in the flat regimes).
2. Deliberate mistakes in the reference (sigma 1.0, a 9-tap window, c2 from 0.01, the range per image, padded positions) move the
   per-image value by more than 100x the bar.  Clamped variances: no case with a genuinely negative float64 variance estimate
   exists (the weights are positive, so the variance is non-negative and an estimate below zero is rounding, > -1e-15 R^2); the
   test asserts that and that clamping then moves nothing.
3. The float32 emulation of the kernel's centred arithmetic stays below a tenth of the bar on every case; the textbook
   E[x^2] - mu^2 in float32 misses the bar on the flat cases.
4. The evaluator-level aggregate, the configs (fields, defaults, round trips), the package surface.
5. The per-class accuracy accumulation against a numpy count (a class that never occurs, nb_samples_for_cross = 2, include_recon
   both ways), and the evaluators' logic: metrics.log, the unfitted-sampler error, joint_nll_from_subset without the hook, the
   SSIM ValueError of a vector modality, the wandb error.
"""
import json
import sys

import numpy as np
import pytest
import torch

import ssim_ref as R

CASES = R.cases(32)
_REF = {}


def ref(name, regime, shape):
    """(preds, target, ssim64) of a case: computed once, shared, left unchanged."""
    if name not in _REF:
        p, t = R.make(regime, shape)
        _REF[name] = (p, t, R.ssim64(p, t))
    return _REF[name]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_reference_cross_check(case):
    p, t, a = ref(*case)
    b = R.ssim64_loops(p, t)
    assert a["R"] == b["R"] and a["maps"].shape == (case[2][0], case[2][1], case[2][2] - 10, case[2][3] - 10)
    assert float(np.max(np.abs(a["rows"] - b["rows"]))) <= 1e-12  # the per-image values, which every other test consumes
    # per position the two differ by float64's own rounding of E[xx] - mu^2: up to 121 roundings of 1.1e-16 * 0.49 in the flat
    # regime (6.5e-15 at worst) over c2 = 9e-4 R^2 there, 7e-12; 1e-12 everywhere else
    assert float(np.max(np.abs(a["maps"] - b["maps"]))) <= (1e-11 if case[1] in ("flat", "patch") else 1e-12)


def test_reference_by_hand():
    """One window: the weighted moments written out."""
    rng = np.random.default_rng(0)
    p, t = rng.random((1, 1, 11, 11)), rng.random((1, 1, 11, 11))
    g = np.exp(-0.5 * ((np.arange(11) - 5) / 1.5) ** 2)
    w = np.outer(g / g.sum(), g / g.sum())
    Rg = max(p.max() - p.min(), t.max() - t.min())
    mp, mt = (w * p[0, 0]).sum(), (w * t[0, 0]).sum()
    vp, vt, cv = (w * p[0, 0] ** 2).sum() - mp ** 2, (w * t[0, 0] ** 2).sum() - mt ** 2, (w * p[0, 0] * t[0, 0]).sum() - mp * mt
    c1, c2 = (0.01 * Rg) ** 2, (0.03 * Rg) ** 2
    want = (2 * mp * mt + c1) * (2 * cv + c2) / ((mp ** 2 + mt ** 2 + c1) * (vp + vt + c2))
    assert abs(R.ssim64(p, t)["rows"][0] - want) <= 1e-14 and abs(R.taps().sum() - 1.0) <= 1e-15
    # the per-image value is the mean over channels and positions
    q, u = rng.random((2, 3, 13, 12)), rng.random((2, 3, 13, 12))
    out = R.ssim64(q, u)
    assert out["maps"].shape == (2, 3, 3, 2) and np.allclose(out["rows"], out["maps"].reshape(2, -1).mean(1), rtol=0, atol=1e-15)


def test_mutations_move_the_result():
    far = 100 * R.BAR
    for regime in ("uniform", "binary", "patch"):
        p, t, good = ref(f"{regime}-5x1x28x28", regime, (5, 1, 28, 28))
        for name, kw in (("sigma 1.0", dict(sigma=1.0)), ("window 9", dict(win=9)), ("c2 from 0.01", dict(k2=0.01)),
                         ("padded positions", dict(padded=True))):
            moved = float(np.max(np.abs(R.ssim64(p, t, **kw)["rows"] - good["rows"])))
            print(regime, name, f"{moved / R.BAR:.3g}x the bar")
            assert moved > far, (regime, name, moved)
    # the range of each image instead of the update's: a batch whose images differ in range
    rng = np.random.default_rng(3)
    img = 0.25 + 0.5 * rng.random((1, 1, 28, 28))
    p = np.concatenate([img + 0.05 * rng.standard_normal(img.shape), 2.0 * rng.random(img.shape)])
    t = np.concatenate([img, 2.0 * rng.random(img.shape)])
    moved = float(np.max(np.abs(R.ssim64(p, t, per_image_range=True)["rows"] - R.ssim64(p, t)["rows"])))
    assert moved > far, moved


def test_no_case_has_a_negative_variance_to_clamp():
    """The weights are positive and sum to 1, so E[xx] - mu^2 >= 0 exactly; what float64 leaves below zero is rounding, and
    clamping it moves no result.  The kernel does not clamp either (its centred sums of squares cannot go negative)."""
    for case in CASES:
        p, t, good = ref(*case)
        floor = -1e-15 * max(good["R"], 1e-300) ** 2
        assert good["var_p"].min() >= floor and good["var_t"].min() >= floor, case[0]
        clamped = R.ssim64(p, t, clamp=True)["rows"]
        assert float(np.max(np.abs(clamped - good["rows"]))) <= 1e-3 * R.BAR, case[0]


def test_fp32_emulations():
    worst_centred, worst_flat_uncentred = 0.0, 0.0
    for case in CASES:
        p, t, good = ref(*case)
        e = float(np.max(np.abs(R.emulate_fp32(p, t) - good["rows"])))
        worst_centred = max(worst_centred, e)
        assert e <= R.BAR / 10, (case[0], e)
        if case[1] == "flat":
            worst_flat_uncentred = max(worst_flat_uncentred, float(np.max(np.abs(R.uncentred_fp32(p, t) - good["rows"]))))
    print(f"centred fp32 worst {worst_centred:.2e}; un-centred fp32 on the flat cases {worst_flat_uncentred:.2e}")
    assert worst_flat_uncentred > 5 * R.BAR
    # R = 0: the centred arithmetic gives 0 / 0 = NaN without a special case
    c = np.full((1, 2, 12, 12), 0.3, np.float32)
    assert np.isnan(R.emulate_fp32(c, c + np.float32(0.25))).all()


def test_aggregate():
    rng = np.random.default_rng(5)
    ups = [(rng.random((3, 1, 12, 12)), rng.random((3, 1, 12, 12))), (10 * rng.random((1, 3, 11, 13)), rng.random((1, 3, 11, 13)))]
    rows = [R.ssim64(p, t)["rows"] for p, t in ups]
    assert abs(R.aggregate(ups, "SSIM") - (rows[0].sum() + rows[1].sum()) / 4) <= 1e-15
    # the data range is per update: scoring the two updates as one batch of the same images is another number
    assert R.ssim64(*ups[1])["R"] > 5 * R.ssim64(*ups[0])["R"]
    sq = sum(((p - t) ** 2).sum() for p, t in ups)
    assert abs(R.aggregate(ups, "MSE") - sq / 4) <= 1e-12 * sq
    with pytest.raises(ValueError):
        R.aggregate(ups, "PSNR")


# ---- the package ---------------------------------------------------------------------------------------------------------------
def test_package_surface():
    import multivae_amd.metrics as M
    from multivae_amd.metrics.base import Evaluator, EvaluatorConfig
    from multivae_amd.metrics.coherences import CoherenceEvaluator, CoherenceEvaluatorConfig
    from multivae_amd.metrics.likelihoods import LikelihoodsEvaluator, LikelihoodsEvaluatorConfig
    from multivae_amd.metrics.reconstruction import Reconstruction, ReconstructionConfig

    names = {"Evaluator", "EvaluatorConfig", "LikelihoodsEvaluator", "LikelihoodsEvaluatorConfig", "Reconstruction",
             "ReconstructionConfig", "CoherenceEvaluator", "CoherenceEvaluatorConfig"}
    assert set(M.__all__) == names and all(hasattr(M, n) for n in names)
    assert M.Reconstruction is Reconstruction and M.CoherenceEvaluator is CoherenceEvaluator and M.Evaluator is Evaluator
    assert M.LikelihoodsEvaluator is LikelihoodsEvaluator and M.EvaluatorConfig is EvaluatorConfig
    assert issubclass(ReconstructionConfig, EvaluatorConfig) and issubclass(CoherenceEvaluatorConfig, EvaluatorConfig)
    assert issubclass(LikelihoodsEvaluatorConfig, EvaluatorConfig)
    for ev in (LikelihoodsEvaluator, Reconstruction, CoherenceEvaluator):
        assert issubclass(ev, Evaluator)


def test_configs(tmp_path):
    from multivae_amd.metrics import (CoherenceEvaluatorConfig, EvaluatorConfig, LikelihoodsEvaluatorConfig,
                                      ReconstructionConfig)
    from multivae_amd.models.base.base_config import BaseConfig

    base = dict(batch_size=512, wandb_path=None)
    want = {
        EvaluatorConfig: base,
        LikelihoodsEvaluatorConfig: dict(base, num_samples=1000, batch_size_k=100, unified_implementation=True),
        ReconstructionConfig: dict(base, metric="SSIM"),
        CoherenceEvaluatorConfig: dict(base, num_classes=10, include_recon=False, nb_samples_for_joint=10000, nb_samples_for_cross=1,
                                       give_details_per_class=False),
    }
    other = {
        EvaluatorConfig: dict(batch_size=3, wandb_path="e/p/r"),
        LikelihoodsEvaluatorConfig: dict(batch_size=7, num_samples=5, batch_size_k=2, unified_implementation=False),
        ReconstructionConfig: dict(metric="MSE", batch_size=9),
        CoherenceEvaluatorConfig: dict(num_classes=3, include_recon=True, nb_samples_for_joint=11, nb_samples_for_cross=2,
                                       give_details_per_class=True),
    }
    for cls, defaults in want.items():
        assert issubclass(cls, BaseConfig)
        assert cls().to_dict() == dict(defaults, name=cls.__name__)
        cfg = cls(**other[cls])
        for k, v in other[cls].items():
            assert getattr(cfg, k) == v
        assert cls.from_dict(cfg.to_dict()) == cfg and cls.from_dict(cls().to_dict()) == cls()
        cfg.save_json(str(tmp_path), cls.__name__)
        assert cls.from_json_file(str(tmp_path / f"{cls.__name__}.json")) == cfg
        assert json.loads(cfg.to_json_string())["name"] == cls.__name__
    with pytest.raises(Exception):
        ReconstructionConfig(metric="PSNR")
    with pytest.raises(ValueError):
        ReconstructionConfig.from_json_file(str(tmp_path / "EvaluatorConfig.json"))


# ---- evaluator logic on duck-typed models ----------------------------------------------------------------------------------------
CLASSES = 4


class FakeModel:
    """What the evaluators touch.  predict returns, for every generated modality, the conditioning data of that modality N times
    over (sample-major), the k-th copy rolled by k along the class axis: the data ARE the logits of the identity classifiers."""

    def __init__(self, mods):
        self.encoders = {m: None for m in mods}
        self.n_modalities = len(mods)
        self.calls = []

    def to(self, device):
        return self

    def eval(self):
        return self

    def predict(self, inputs, cond_mod, gen_mod, N=1, flatten=False, **kwargs):
        self.calls.append((list(cond_mod), list(gen_mod), N, flatten))
        return {m: torch.cat([torch.roll(inputs.data[m], k, dims=1) for k in range(N)]) for m in gen_mod}

    def compute_joint_nll(self, inputs, K, batch_size_K):
        self.calls.append(("nll", K, batch_size_K))
        return inputs.data["a"].sum() * K


def _labelled(n=7, seed=0, labels=True):
    from multivae_amd.data.datasets.base import MultimodalBaseDataset

    g = torch.Generator().manual_seed(seed)
    data = dict(a=torch.randn(n, CLASSES, generator=g), b=torch.randn(n, CLASSES, generator=g), c=torch.randn(n, CLASSES, generator=g))
    lab = torch.tensor([0, 1, 3, 3, 1, 0, 3, 1, 1, 0])[:n]  # class 2 never occurs
    return MultimodalBaseDataset(data=data, labels=lab if labels else None)


def _numpy_accuracy(logits, labels):
    count = np.zeros((CLASSES, 2))
    for row, y in zip(logits, labels):
        count[y] += (int(np.argmax(row) == y), 1)
    return np.where(count[:, 1] > 0, count[:, 0] / np.maximum(count[:, 1], 1), 0.0).astype(np.float32)


def test_class_counts():
    from multivae_amd.metrics.coherences.coherences import ClassCounts

    rng = np.random.default_rng(2)
    logits, labels = rng.standard_normal((40, CLASSES)).astype(np.float32), rng.choice([0, 1, 3], 40)
    cc = ClassCounts(CLASSES, "cpu")
    for a, b in ((0, 13), (13, 14), (14, 40)):  # accumulated over uneven updates
        cc.update(torch.from_numpy(logits[a:b]), torch.from_numpy(labels[a:b]))
    assert cc.counts.dtype == torch.int64 and int(cc.counts[:CLASSES, 1].sum()) == 40 and int(cc.counts[2].sum()) == 0
    got = cc.compute()
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), _numpy_accuracy(logits, labels)) and got[2] == 0
    # a label outside [0, num_classes) is counted for no class
    cc.update(torch.from_numpy(logits[:2]), torch.tensor([7, -1]))
    assert np.array_equal(cc.compute().numpy(), _numpy_accuracy(logits, labels))


@pytest.mark.parametrize("n_cross,recon", [(1, False), (2, False), (1, True), (2, True)])
def test_coherence_accumulation(n_cross, recon):
    from multivae_amd.metrics import CoherenceEvaluator, CoherenceEvaluatorConfig

    ds, model = _labelled(), FakeModel("abc")
    clfs = {m: torch.nn.Identity() for m in "abc"}
    cfg = CoherenceEvaluatorConfig(batch_size=3, num_classes=CLASSES, nb_samples_for_cross=n_cross, include_recon=recon)
    ev = CoherenceEvaluator(model, clfs, ds, None, cfg)
    subset = ["a", "c"]
    acc, mean_acc, per_class = ev.coherence_from_subset(subset, return_accuracies_per_labels=True)
    gen = ["a", "b", "c"] if recon else ["b"]
    assert list(acc) == [f"a_c_to_{m}" for m in gen]
    assert model.calls == [(subset, gen, n_cross, True)] * 3
    lab = ds.labels.numpy()
    want = {}
    for m in gen:  # what the fake model generated, batch by batch, sample-major inside a batch
        logits, labels = [], []
        for b0 in range(0, 7, 3):
            x = ds.data[m][b0:b0 + 3]
            for k in range(n_cross):
                logits.append(torch.roll(x, k, dims=1).numpy())
                labels.append(lab[b0:b0 + 3])
        want[m] = _numpy_accuracy(np.concatenate(logits), np.concatenate(labels))
        assert want[m][2] == 0.0
        assert float(acc[f"a_c_to_{m}"]) == float(torch.from_numpy(want[m]).mean())
    assert np.array_equal(per_class, np.mean(np.stack(list(want.values())), axis=0))
    assert mean_acc == np.mean([float(torch.from_numpy(v).mean()) for v in want.values()])
    assert len(ev.coherence_from_subset(subset)) == 2
    # all subsets of one and of two modalities
    means, stds = ev.cross_coherences()
    assert len(means) == 2 and len(stds) == 2
    assert {"mean_coherence_1", "std_coherence_1", "mean_coherence_2", "std_coherence_2", "a_b_to_c"} <= set(ev.metrics)
    assert ("a_to_a" in ev.metrics) == recon
    ev.finish()


def test_coherence_label_errors():
    from multivae_amd.data.datasets.base import DatasetOutput
    from multivae_amd.metrics import CoherenceEvaluator, CoherenceEvaluatorConfig

    ev = CoherenceEvaluator(FakeModel("ab"), {m: torch.nn.Identity() for m in "ab"}, _labelled(labels=False), None,
                            CoherenceEvaluatorConfig(batch_size=3, num_classes=CLASSES))
    with pytest.raises(AttributeError, match="on a dataset without labels"):
        ev.coherence_from_subset(["a"])
    ev.test_loader = [DatasetOutput(data=dict(a=torch.zeros(2, CLASSES), b=torch.zeros(2, CLASSES)), labels=None)]
    with pytest.raises(AttributeError, match="None instead of tensor labels"):
        ev.coherence_from_subset(["a"])
    ev.finish()


def test_evaluator_logic(tmp_path, monkeypatch):
    from multivae_amd._output import ModelOutput
    from multivae_amd.metrics import (Evaluator, EvaluatorConfig, LikelihoodsEvaluator, LikelihoodsEvaluatorConfig, Reconstruction,
                                      ReconstructionConfig)

    ds, model = _labelled(), FakeModel("ab")
    out_dir = tmp_path / "deep" / "metrics"
    ev = LikelihoodsEvaluator(model, ds, str(out_dir), LikelihoodsEvaluatorConfig(batch_size=3, num_samples=5, batch_size_k=2))
    assert (out_dir / "metrics.log").exists() and ev.n_data == 7 and ev.batch_size == 3 and ev.wandb_run is None
    out = ev.eval()
    assert isinstance(out, ModelOutput) and list(out.keys()) == ["joint_likelihood"] and torch.is_tensor(out.joint_likelihood)
    assert model.calls == [("nll", 5, 2)] * 3
    assert torch.allclose(out.joint_likelihood.cpu(), ds.data["a"].sum() * 5 / 7, rtol=1e-5)
    assert ev.joint_nll_from_subset(["a"]) is None and list(ev.metrics) == ["joint_likelihood"]
    ev.finish()
    assert "Mean Joint likelihood" in (out_dir / "metrics.log").read_text() and not ev.logger.handlers
    # the paper estimator is chosen only when asked for and present
    model.compute_joint_nll_paper = lambda inputs, K, bk: inputs.data["b"].sum()
    paper = LikelihoodsEvaluator(model, ds, None, LikelihoodsEvaluatorConfig(batch_size=4, unified_implementation=False))
    assert torch.allclose(paper.joint_nll().cpu(), ds.data["b"].sum() / 7, rtol=1e-5)
    paper.finish()
    unified = LikelihoodsEvaluator(model, ds, None, LikelihoodsEvaluatorConfig(batch_size=4, num_samples=2))
    assert torch.allclose(unified.joint_nll().cpu(), ds.data["a"].sum() * 2 / 7, rtol=1e-5)
    unified.finish()

    # a sampler that is not fitted
    class Sampler:
        is_fitted = False
        name = "S"

    with pytest.raises(AttributeError, match="not fitted"):
        Evaluator(model, ds, None, EvaluatorConfig(), sampler=Sampler())
    # SSIM of a vector modality: an error that names it, before anything is launched
    rec = Reconstruction(model, ds, None, ReconstructionConfig(batch_size=3))
    with pytest.raises(ValueError, match="modality a"):
        rec.reconstruction_from_subset(["a"])
    rec.finish()
    # wandb is imported only when a path is given, and its absence is reported
    monkeypatch.setitem(sys.modules, "wandb", None)
    with pytest.raises(ModuleNotFoundError, match="wandb"):
        Evaluator(model, ds, None, EvaluatorConfig(wandb_path="entity/project/run"))
