"""csrc/clf.hip through the C ABI against the float64 network of tests/clf_ref.py, ClassifierPolyMNIST's dispatch, and
CoherenceEvaluator's fused path against its general path end to end.

Bars.  Logits: distance from float64 (relative to the row's largest |logit|) <= clf_ref.BAR = 8 x the worst fp32-torch-vs-float64
distance of the host test = 1.06e-5, every regime, every row.  pred: exactly the argmax of the kernel's own logits, and exactly
the float64 argmax on all rows (every float64 margin is > 100 x BAR: test_classifier_host.py).  Counts, bit-identity, end-to-end
metrics: exact.

1. test_sizes: n in {1, T-1, T, T+1, 2T+3} (T = polyclf_tile()), outputs pre-filled with NaN / a sentinel and one row longer than
   n (the row past the end is untouched), a second run bit-identical.
2. test_regimes: the 256 rows of each of clf_ref.REGIMES (seeded, zeros, binary, every ReLU dead, every ReLU alive).
3. test_ties_and_nan; test_bit_identity (image i alone against image i inside n = 2T+3; the logits-only, pred-only and
   counts-only calls); test_counts (labels -1 and 10, label_rows = n / 2, two accumulating calls, n = 0) against
   ClassCounts.update fed the kernel's logits; test_invalid_arguments (every MVK_EINVAL branch).
4. test_module_dispatch; test_evaluator_end_to_end: three (3,28,28) modalities, 7 rows, batch 3, nb_samples_for_cross = 2.

Largest distance of the HIP kernel's logits from float64 on an MI355X per regime (test_zz_report prints HIP_MEASURED; first GPU
run of the kernel):
    seeded 8.98e-07 (n = 256; 6.42e-07 at n = 16 .. 35, 6.19e-07 at n = 1), zeros 1.35e-07, binary 9.93e-07, dead 0 (the logits are
    the last bias bit for bit), alive 7.21e-07: all below the fp32 CPU forward's own distance (clf_ref.TORCH_FP32_WORST = 1.32e-06)
"""
import ctypes

import numpy as np
import pytest
import torch

import clf_ref as CR

pytestmark = pytest.mark.gpu
D = torch.device("cuda:0")
MEASURED = {}
EINVAL = -1
_PARAMS = {}


def _mods():
    from multivae_amd import _lib, kernels

    return _lib, kernels


def T():
    return _mods()[1].polyclf_tile()


def params(name="seeded"):
    """The eight parameter tensors of a regime on the device: made once, never written to."""
    if name not in _PARAMS:
        w = CR.regime(name)[0]
        _PARAMS[name] = [torch.from_numpy(np.array(w[k])).to(D) for k in CR.KEYS]
    return _PARAMS[name]


def images(name, n):
    return torch.from_numpy(np.array(CR.regime(name)[1][:n])).to(D)


def nan_logits(n):
    return torch.full((n + 1, 10), float("nan"), dtype=torch.float32, device=D)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def run(x, p, logits=True, pred=True, labels=None, counts=None):
    """One launch on buffers one row longer than n; returns (logits [n,10] or None, pred [n] or None)."""
    _, K = _mods()
    n = x.shape[0]
    lg = nan_logits(n) if logits else None
    pr = torch.full((n + 1,), -7, dtype=torch.int32, device=D) if pred else None
    K.polyclf_forward(x, p, logits=None if lg is None else lg[:n], pred=None if pr is None else pr[:n], labels=labels, counts=counts)
    torch.cuda.synchronize()
    if lg is not None:
        assert torch.isnan(lg[n]).all() and torch.isfinite(lg[:n]).all()
    if pr is not None:
        assert int(pr[n]) == -7
    return (None if lg is None else lg[:n]), (None if pr is None else pr[:n])


def check(name, lg, pr, n):
    ref = CR.logits64(name)[:n]
    d = CR.dist(lg.cpu().numpy(), ref)
    if d > MEASURED.get(name, (-1.0, 0))[0]:
        MEASURED[name] = (d, n)
    print(f"{name} n={n}: HIP vs float64 {d:.3e} (bar {CR.BAR:.3e})")
    assert d <= CR.BAR, (name, n, d)
    assert torch.equal(pr.long(), torch.argmax(lg, dim=1))
    assert np.array_equal(pr.cpu().numpy(), ref.argmax(1))


def test_sizes():
    t = T()
    assert t >= 2
    for n in (1, t - 1, t, t + 1, 2 * t + 3):
        x = images("seeded", n)
        lg, pr = run(x, params())
        check("seeded", lg, pr, n)
        lg2, pr2 = run(x, params())
        assert same_bits(lg, lg2) and torch.equal(pr, pr2)


@pytest.mark.parametrize("name", CR.REGIMES)
def test_regimes(name):
    x = images(name, CR.N_ROWS)
    lg, pr = run(x, params(name))
    check(name, lg, pr, CR.N_ROWS)
    if name == "dead":  # the logits are the last bias, exactly
        assert same_bits(lg, params(name)[7].expand(CR.N_ROWS, 10))


def test_ties_and_nan():
    n = T() + 1
    x = images("alive", n)
    p = [q.clone() for q in params("alive")]
    p[6][3] = p[6][7] = 2 * p[6].abs().max(dim=0).values  # two equal rows of fc2, the largest by construction (fc1's output is > 0)
    p[7][3] = p[7][7] = p[7].abs().max()
    lg, pr = run(x, p)
    assert same_bits(lg[:, 3], lg[:, 7]) and bool((lg[:, 3:4] > lg[:, [0, 1, 2, 4, 5, 6, 8, 9]]).all())
    assert torch.equal(pr, torch.full_like(pr, 3)) and torch.equal(pr.long(), torch.argmax(lg, dim=1))
    _, K = _mods()
    lg = torch.empty(n, 10, dtype=torch.float32, device=D)
    pr = torch.empty(n, dtype=torch.int32, device=D)
    p[7][5] = float("nan")  # a NaN logit wins over the tie
    K.polyclf_forward(x, p, logits=lg, pred=pr)
    assert torch.isnan(lg[:, 5]).all() and torch.isfinite(lg[:, [0, 1, 2, 3, 4, 6, 7, 8, 9]]).all()
    assert torch.equal(pr, torch.full_like(pr, 5)) and torch.equal(pr.long(), torch.argmax(lg, dim=1))
    p[7][8] = p[7][2] = float("nan")  # of several NaNs the first
    K.polyclf_forward(x, p, logits=lg, pred=pr)
    assert torch.isnan(lg[:, [2, 5, 8]]).all() and torch.isfinite(lg[:, [0, 1, 3, 4, 6, 7, 9]]).all()
    assert torch.equal(pr, torch.full_like(pr, 2)) and torch.equal(pr.long(), torch.argmax(lg, dim=1))


def test_bit_identity():
    t = T()
    n = 2 * t + 3
    x = images("seeded", n)
    full, pred = run(x, params())
    for i in (0, 1, t - 1, t, t + 1, 2 * t + 2):  # alone (first place of a one-image tile) against its place inside n
        one, p1 = run(x[i:i + 1].contiguous(), params())
        assert same_bits(one[0], full[i]) and int(p1[0]) == int(pred[i]), i
    shifted, _ = run(x[3:].contiguous(), params())  # every image in another place of another tile
    assert same_bits(shifted, full[3:])
    # parameters that are views at an odd offset of a larger storage (fc1's rows are then read k by k, not four at a time)
    off = []
    for q in params():
        buf = torch.empty(q.numel() + 1, dtype=torch.float32, device=D)
        buf[1:].copy_(q.reshape(-1))
        off.append(buf[1:].view(q.shape))
        assert off[-1].data_ptr() % 16 != 0 and off[-1].is_contiguous()
    unaligned, _ = run(x, off)
    assert same_bits(unaligned, full)
    # the three single-output calls agree with the call that asks for everything
    lg_only, _ = run(x, params(), pred=False)
    _, pr_only = run(x, params(), logits=False)
    labels = torch.arange(n, device=D) % 10
    counts = torch.zeros(11, 2, dtype=torch.int64, device=D)
    run(x, params(), logits=False, pred=False, labels=labels, counts=counts)
    assert same_bits(lg_only, full) and torch.equal(pr_only, pred)
    assert np.array_equal(counts.cpu().numpy(), CR.counts_model(pred.cpu().numpy(), labels.cpu().numpy()))


def test_counts():
    from multivae_amd.metrics.coherences.coherences import ClassCounts

    _, K = _mods()
    t = T()
    n = 2 * t + 2
    rows = n // 2
    x = images("seeded", n)
    lg, pr = run(x, params())
    labels = torch.from_numpy(CR.logits64("seeded")[:rows].argmax(1)).to(D)  # mostly right, so both columns move
    labels[1], labels[t] = -1, 10
    labels[2] = (labels[2] + 1) % 10
    stacked = torch.cat([labels, labels])  # what coherence_from_subset builds for two generations per row
    want = ClassCounts(10, D)
    counts = torch.zeros(11, 2, dtype=torch.int64, device=D)
    for _ in range(2):  # two accumulating calls
        want.update(lg, stacked)
        K.polyclf_forward(x, params(), labels=labels, counts=counts)
        assert torch.equal(counts, want.counts)
    got = counts.cpu().numpy()
    assert got[10, 1] == 8 and got[10, 0] == 0 and got[:, 1].sum() == 2 * n and got[:10, 0].sum() > 0
    once = CR.counts_model(pr.cpu().numpy(), labels.cpu().numpy(), rows)
    assert np.array_equal(got, CR.counts_model(pr.cpu().numpy(), labels.cpu().numpy(), rows, once))
    # n = 0: nothing is written (the entry point itself at n = 0: test_invalid_arguments)
    before = counts.clone()
    K.polyclf_forward(x[:0], params(), labels=labels, counts=counts)
    assert K.polyclf_forward(x[:0], params()).shape == (0, 10)
    torch.cuda.synchronize()
    assert torch.equal(counts, before)


def test_invalid_arguments():
    L, _ = _mods()
    lib = L.load()
    n = 4
    x = images("seeded", n)
    lg, pr = nan_logits(n), torch.zeros(n, dtype=torch.int32, device=D)
    labels = torch.zeros(2, dtype=torch.int64, device=D)
    counts = torch.zeros(11, 2, dtype=torch.int64, device=D)
    w = [ctypes.c_void_p(q.data_ptr()) for q in params()]
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def call(x_=x, n_=n, w_=w, lg_=lg, pr_=pr, lab_=None, rows_=0, cnt_=None):
        return lib.mvk_polyclf_fwd(P(x_), n_, *w_, P(lg_), P(pr_), P(lab_), rows_, P(cnt_), L.stream_ptr())

    assert call() == 0
    assert call(lab_=labels, rows_=2, cnt_=counts) == 0
    assert call(x_=None) == EINVAL
    for i in range(8):
        assert call(w_=w[:i] + [None] + w[i + 1:]) == EINVAL, i
    assert call(n_=-1) == EINVAL
    assert call(lg_=None, pr_=None) == EINVAL                              # all three outputs NULL
    assert call(cnt_=counts, rows_=2) == EINVAL                            # counts without labels
    assert call(lab_=labels, rows_=0, cnt_=counts) == EINVAL               # label_rows <= 0
    assert call(lab_=labels, rows_=-2, cnt_=counts) == EINVAL
    assert call(lab_=labels, rows_=3, cnt_=counts) == EINVAL               # n % label_rows != 0
    assert call(n_=0, x_=None, w_=[None] * 8) == 0                         # n == 0: nothing is read
    assert call(n_=0, lg_=None, pr_=None, lab_=labels, rows_=2, cnt_=counts) == 0      # counts alone, n == 0: nothing is added
    assert call(n_=0, lg_=None, pr_=None) == EINVAL
    assert call(lab_=labels, rows_=3) == 0                                 # labels without counts are not looked at
    torch.cuda.synchronize()
    assert counts[:, 1].sum() == n  # only the one valid call with counts added anything


def _module(name="seeded"):
    from multivae_amd.metrics import ClassifierPolyMNIST

    clf = ClassifierPolyMNIST()
    clf.load_state_dict(CR.state_dict(CR.regime(name)[0], torch))
    return clf.to(D).eval()


def test_module_dispatch(monkeypatch):
    _, K = _mods()
    calls, orig = [], K.polyclf_forward
    monkeypatch.setattr(K, "polyclf_forward", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    clf = _module()
    n = T() + 1
    x = images("seeded", n)
    direct, pred = run(x, params())
    assert any(p.requires_grad for p in clf.parameters())
    with torch.no_grad():
        out = clf(x)
    assert len(calls) == 2 and same_bits(out, direct) and not out.requires_grad
    assert torch.equal(clf.classify(x), pred) and len(calls) == 3
    for p in clf.parameters():
        p.requires_grad_(False)
    assert same_bits(clf(x), direct) and len(calls) == 4  # grad mode on, nothing to record
    with torch.no_grad():  # in-place updates and load_state_dict need no invalidation: the parameters are read in place
        clf.encoder[10].bias.add_(1.0)
        assert torch.allclose(clf(x), direct + 1.0, rtol=0, atol=1e-5) and not same_bits(clf(x), direct)
        clf.load_state_dict(CR.state_dict(CR.regime("alive")[0], torch))
        assert CR.dist(clf(x).cpu().numpy(), CR.logits64("alive")[:n]) <= CR.BAR
    n_fused = len(calls)
    assert n_fused == 7
    # everything else is left to the torch modules: the CPU, other dtypes and shapes, something to record, train mode
    assert not clf.fused_ok(x.cpu()) and not clf.fused_ok(x.double()) and not clf.fused_ok(x[:, :, :27])
    xg = x.clone().requires_grad_(True)
    assert not clf.fused_ok(xg) and clf.kernel_ok(xg) and torch.equal(clf.classify(xg), clf.classify(x))
    n_fused += 2
    clf.train()
    assert not clf.fused_ok(x) and not clf.kernel_ok(x)
    with pytest.raises(ValueError):
        clf.classify(x)
    assert len(calls) == n_fused


# ---- the evaluator ----------------------------------------------------------------------------------------------------------------
MODS = ("m0", "m1", "m2")


class Plain(torch.nn.Module):
    """The same network from the same parameters, written with unfold and matmul in float64: not a ClassifierPolyMNIST, so the
    evaluator takes its general path (logits tensor, ClassCounts.update)."""

    def __init__(self, clf):
        super().__init__()
        self.p = torch.nn.ParameterList([torch.nn.Parameter(q.detach().clone(), requires_grad=False) for q in clf.kernel_params()])

    def forward(self, x):
        w1, b1, w2, b2, w3, b3, w4, b4 = [q.double() for q in self.p]
        h = x.double()
        for w, b in ((w1, b1), (w2, b2)):
            n, _, hh, _ = h.shape
            cols = torch.nn.functional.unfold(h, kernel_size=4, stride=2, padding=1)  # [n, C 16, positions]
            h = torch.relu(w.reshape(w.shape[0], -1) @ cols + b[:, None]).reshape(n, w.shape[0], hh // 2, hh // 2)
        h = torch.relu(h.reshape(len(h), -1) @ w3.T + b3)
        return h @ w4.T + b4


def test_evaluator_end_to_end(monkeypatch):
    from multivae_amd.data.datasets.base import MultimodalBaseDataset
    from multivae_amd.metrics import ClassifierPolyMNIST, CoherenceEvaluator, CoherenceEvaluatorConfig
    from multivae_amd.models import MVTCAE, MVTCAEConfig

    _, K = _mods()
    g = torch.Generator().manual_seed(11)
    ds = MultimodalBaseDataset(data={m: torch.rand(7, 3, 28, 28, generator=g) for m in MODS},
                               labels=torch.tensor([0, 1, 3, 9, 1, 0, 3]))
    torch.manual_seed(5)
    model = MVTCAE(MVTCAEConfig(n_modalities=3, latent_dim=5, input_dims={m: (3, 28, 28) for m in MODS})).to(D).eval()
    fused = {}
    for i, m in enumerate(MODS):
        torch.manual_seed(20)  # one set of weights for the three: codes can be classified alike
        fused[m] = ClassifierPolyMNIST()
    plain = {m: Plain(fused[m]) for m in MODS}
    cfg = CoherenceEvaluatorConfig(batch_size=3, num_classes=10, nb_samples_for_cross=2, nb_samples_for_joint=10,
                                   give_details_per_class=True)
    launches, orig = [], K.polyclf_forward
    monkeypatch.setattr(K, "polyclf_forward", lambda *a, **k: (launches.append(k.get("counts") is not None), orig(*a, **k))[1])
    tape = {"predict": [], "decode": []}
    real = {"predict": model.predict, "decode": model.decode}

    depth = [0]

    def recorder(name):
        def f(*a, **k):
            depth[0] += 1
            out = real[name](*a, **k)
            depth[0] -= 1
            if depth[0] == 0:  # predict decodes: only the evaluator's own calls are taped
                tape[name].append(out)
            return out
        return f

    for name in tape:
        monkeypatch.setattr(model, name, recorder(name))
    ev = CoherenceEvaluator(model, fused, ds, None, cfg)
    torch.manual_seed(0)
    got = ev.eval()
    ev.finish()
    # subsets of one and two modalities (6), three batches each, the modalities outside the subset: 3 x 3 x 2 + 3 x 3 x 1
    # launches that add into the counts; joint coherence: 10 codes in batches of 3 -> 4 batches x 3 modalities, pred only
    assert len(tape["predict"]) == 18 and len(tape["decode"]) == 4
    assert launches.count(True) == 27 and launches.count(False) == 12
    n_launches = len(launches)

    def replayer(name):
        it = iter(tape[name])
        return lambda *a, **k: next(it)

    for name in tape:
        monkeypatch.setattr(model, name, replayer(name))
    ev2 = CoherenceEvaluator(model, plain, ds, None, cfg)
    torch.manual_seed(0)
    want = ev2.eval()
    ev2.finish()
    assert len(launches) == n_launches  # the general path never reaches the kernel
    assert sorted(got.keys()) == sorted(want.keys()) and "joint_coherence_prior" in got and "m0_m1_to_m2" in got
    assert "mean_coherence_2_class_9" in got
    for k in want:
        a, b = got[k], want[k]
        a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
        assert a.dtype == b.dtype and np.array_equal(a, b), (k, a, b)


def test_zz_report():
    for k in sorted(MEASURED):
        print("HIP_MEASURED", k, f"{MEASURED[k][0]:.2e}", f"n={MEASURED[k][1]}")
