"""CPU tests of metrics.classifiers: the float64 reference of tests/clf_ref.py against the reference class's recorded logits, the
module's layout and CPU forward against the same fixture, dropout in train mode, the loader, a numpy model of the counts against
ClassCounts.update, and the origin of the GPU test's bar (the fp32-vs-float64 distance re-measured, the margin condition)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clf_ref as CR

from multivae_amd.metrics import ClassifierPolyMNIST, CoherenceEvaluator  # noqa: F401  (importable from the package)
from multivae_amd.metrics.classifiers import load_mmnist_classifiers
from multivae_amd.metrics.coherences.coherences import ClassCounts


@pytest.fixture(scope="module")
def golden():
    return np.load(CR.GOLDEN)


def _module(name="seeded"):
    clf = ClassifierPolyMNIST()
    clf.load_state_dict(CR.state_dict(CR.regime(name)[0], torch))
    return clf.eval()


def test_fixture_logits_match_float64(golden):
    ref = CR.logits64("seeded")[: CR.GOLDEN_ROWS]
    assert golden["logits"].shape == (CR.GOLDEN_ROWS, 10) and golden["logits"].dtype == np.float32
    d = CR.dist(golden["logits"], ref)
    print("reference class fp32 vs float64, 16 rows:", d)
    assert d <= CR.TORCH_FP32_WORST


def test_state_dict_layout_is_the_fixtures(golden):
    sd = ClassifierPolyMNIST().state_dict()
    assert list(sd.keys()) == [str(k) for k in golden["keys"]] == list(CR.KEYS)
    shapes = [tuple(int(v) for v in row[:r]) for row, r in zip(golden["shapes"], golden["rank"])]
    assert [tuple(v.shape) for v in sd.values()] == shapes == list(CR.SHAPES)
    assert isinstance(ClassifierPolyMNIST().encoder, torch.nn.Sequential)


def test_cpu_forward_reproduces_the_fixture(golden):
    clf = _module()
    x = torch.from_numpy(np.array(CR.seeded()[1][: CR.GOLDEN_ROWS]))
    with torch.no_grad():
        out = clf(x).numpy()
    # the same torch modules in the same order as the reference class: the same fp32 values up to the thread count's blocking
    assert CR.dist(out, golden["logits"].astype(np.float64)) <= 2 * CR.TORCH_FP32_WORST
    assert CR.dist(out, CR.logits64("seeded")[: CR.GOLDEN_ROWS]) <= CR.TORCH_FP32_WORST
    # gradients flow on the module path
    x.requires_grad_(True)
    clf(x).sum().backward()
    assert x.grad is not None and clf.encoder[0].weight.grad is not None


def test_train_mode_applies_dropout():
    clf = _module()
    x = torch.from_numpy(np.array(CR.seeded()[1][:8]))
    with torch.no_grad():
        e0, e1 = clf(x), clf(x)
        clf.train()
        torch.manual_seed(0)
        t0 = clf(x)
        t1 = clf(x)
    assert torch.equal(e0, e1)
    assert not torch.equal(t0, t1) and not torch.equal(t0, e0)


def test_load_mmnist_classifiers_round_trip(tmp_path):
    want = {}
    for i in range(5):
        clf = ClassifierPolyMNIST()
        with torch.no_grad():
            for p in clf.parameters():
                p.add_(i)
        want[f"m{i}"] = {k: v.clone() for k, v in clf.state_dict().items()}
        torch.save(clf.state_dict(), os.path.join(tmp_path, f"pretrained_img_to_digit_clf_m{i}"))
    clfs = load_mmnist_classifiers(data_path=str(tmp_path), device="cpu")
    assert list(clfs) == ["m0", "m1", "m2", "m3", "m4"]
    for m, clf in clfs.items():
        assert type(clf) is ClassifierPolyMNIST
        for k, v in clf.state_dict().items():
            assert torch.equal(v, want[m][k]), (m, k)
    with pytest.raises(FileNotFoundError):
        load_mmnist_classifiers(data_path=str(tmp_path / "missing"))


def test_counts_model_is_class_counts_update():
    """The numpy model the GPU test reads the kernel's counts against: stacked labels, labels outside [0, 10), accumulation."""
    rng = np.random.default_rng(1)
    logits = rng.standard_normal((24, 10)).astype(np.float32)
    labels = rng.integers(0, 10, 12)
    labels[3], labels[7] = -1, 10
    stacked = np.concatenate([labels, labels])  # sample-major stacking of two generations per row
    cc = ClassCounts(10, "cpu")
    model = None
    for _ in range(2):  # two accumulating updates
        cc.update(torch.from_numpy(logits), torch.from_numpy(stacked))
        model = CR.counts_model(logits.argmax(1), labels, label_rows=12, counts=model)
        assert np.array_equal(cc.counts.numpy(), model)
    assert model[10, 1] == 8 and model[10, 0] == 0 and model[:, 1].sum() == 48
    assert np.array_equal(CR.counts_model(logits.argmax(1), stacked), CR.counts_model(logits.argmax(1), labels, label_rows=12))


def test_bar_and_margins():
    """Where the GPU test's bar comes from: the fp32 CPU forward of the same modules against float64 on every regime's 256 rows,
    and every float64 top-2 margin more than MARGIN_FACTOR x BAR."""
    worst = 0.0
    for name in CR.REGIMES:
        w, x = CR.regime(name)
        ref = CR.logits64(name)
        with torch.no_grad():
            out = _module(name)(torch.from_numpy(np.array(x))).numpy()
        d = CR.dist(out, ref)
        m = float(CR.margins(ref).min())
        print(f"{name}: fp32 torch vs float64 {d:.3e}, smallest float64 top-2 margin {m:.3e}, classes {len(set(ref.argmax(1)))}")
        worst = max(worst, d)
        assert m > CR.MARGIN_FACTOR * CR.BAR, (name, m)
        assert np.array_equal(out.argmax(1), ref.argmax(1)), name
    # the recorded measurement is what this machine measures too (the blocking of a CPU GEMM differs between machines and thread
    # counts, so not to the digit), and the bar is 8 x the RECORDED figure
    assert 0.25 * CR.TORCH_FP32_WORST <= worst <= 2 * CR.TORCH_FP32_WORST, worst
    assert CR.BAR == 8 * CR.TORCH_FP32_WORST <= 1e-4
    pre = {name: CR.preacts64(name) for name in ("dead", "alive")}
    assert all(hi < 0 for _, hi in pre["dead"]), pre["dead"]      # every ReLU dead: the logits are the last bias
    assert all(lo > 0 for lo, _ in pre["alive"]), pre["alive"]    # every ReLU alive
    assert np.array_equal(CR.logits64("dead"), np.broadcast_to(CR.regime("dead")[0][CR.KEYS[7]].astype(np.float64), (CR.N_ROWS, 10)))
    assert len(set(CR.logits64("seeded").argmax(1))) == 9


def test_fused_path_is_not_taken_on_the_cpu():
    clf = _module()
    x = torch.from_numpy(np.array(CR.seeded()[1][:2]))
    assert not clf.fused_ok(x) and not clf.kernel_ok(x)
    with pytest.raises(ValueError):
        clf.classify(x)
