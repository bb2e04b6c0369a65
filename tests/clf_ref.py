"""The PolyMNIST classifier in float64, written from its definition, and the seeded inputs of its tests.  Not a test.

Network (eval mode, dropout = identity): x [n,3,28,28] -> conv 4x4 / stride 2 / padding 1 (10) + ReLU -> conv 4x4 / stride 2 /
padding 1 (20) + ReLU -> flatten (c, h, w) -> Linear(980, 128) + ReLU -> Linear(128, 10).

Seeded inputs: rng = np.random.default_rng(0); for every state-dict key in order a weight is standard_normal(shape) *
sqrt(2 / fan_in) and a bias 0.1 * standard_normal(shape); then x = rng.random((256, 3, 28, 28)).  Everything is rounded to float32
once (the module's dtype); the float64 reference computes on those float32 values.

Regimes (`regime(name)` -> (weights, x)).  "seeded": the above.  "zeros": x = 0, the bias path.  "binary": x = (x > 0.5), images in
{0, 1}.  "dead" / "alive": every ReLU dead / alive.  With weights of mixed sign no scaling of x alone does that, so the regime
scales the kernel's other inputs by signs: "dead" takes w1 -> -|w1| and b1, b2, b3 -> -|b| (conv1 is <= 0 on images >= 0, so conv2
sees zeros and is b2 < 0, fc1 is b3 < 0, and the logits are b4 exactly); "alive" takes |.| of w1, b1, w2, b2, w3, b3 (every
pre-activation > 0: nothing is clipped anywhere, the longest sums carry their full length).  `forward64` returns the smallest and
largest pre-activation of the three ReLUs so that the host test can assert both.

Distances are relative to the row's largest |float64 logit|: dist = max_j |logit_j - ref_j| / max_j |ref_j|, maximised over rows.

Bar.  TORCH_FP32_WORST is the largest distance of the reference class's fp32 CPU forward from float64 over the 256 rows of every
regime, measured by test_classifier_host.py (which re-measures it): seeded 9.2e-7 (median 3.7e-7), zeros 2.1e-7, binary 1.31e-6,
dead 0, alive 8.5e-7.  Two fp32 evaluations of the same network differ in the summation order over K <= 980 only, so the HIP
kernel is held to BAR = 8 x that, capped by the project's parity bar of 1e-4.  Every float64 top-2 margin of every regime is more
than MARGIN_FACTOR = 100 x BAR = 1.06e-3 on the same scale (asserted by the host test; the smallest are seeded 1.30e-3, binary
7.4e-3, alive 5.7e-2, dead 8.5e-2, zeros 0.66), which is what lets the GPU test compare the argmax with float64 on all rows."""
import os

import numpy as np

KEYS = ("encoder.0.weight", "encoder.0.bias", "encoder.3.weight", "encoder.3.bias", "encoder.7.weight", "encoder.7.bias",
        "encoder.10.weight", "encoder.10.bias")
SHAPES = ((10, 3, 4, 4), (10,), (20, 10, 4, 4), (20,), (128, 980), (128,), (10, 128), (10,))
N_ROWS = 256
GOLDEN_ROWS = 16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "classifier_polymnist.npz")
REGIMES = ("seeded", "zeros", "binary", "dead", "alive")

TORCH_FP32_WORST = 1.32e-6         # measured (the binary regime): see the docstring
BAR = min(1e-4, 8 * TORCH_FP32_WORST)
MARGIN_FACTOR = 100

_CACHE = {}


def seeded():
    """(weights {key: float32 array}, x [256,3,28,28] float32): computed once, shared, never written to."""
    if "seeded" not in _CACHE:
        rng = np.random.default_rng(0)
        w = {}
        for k, shape in zip(KEYS, SHAPES):
            if k.endswith("weight"):
                v = rng.standard_normal(shape) * np.sqrt(2.0 / np.prod(shape[1:]))
            else:
                v = 0.1 * rng.standard_normal(shape)
            w[k] = v.astype(np.float32)
            w[k].setflags(write=False)
        x = rng.random((N_ROWS, 3, 28, 28)).astype(np.float32)
        x.setflags(write=False)
        _CACHE["seeded"] = (w, x)
    return _CACHE["seeded"]


def regime(name):
    """(weights, x) of one of REGIMES; arrays are shared and read-only."""
    if name == "seeded":
        return seeded()
    if name not in _CACHE:
        w, x = seeded()
        w = dict(w)
        if name == "zeros":
            x = np.zeros_like(x)
        elif name == "binary":
            x = (x > 0.5).astype(np.float32)
        elif name == "dead":
            w[KEYS[0]] = -np.abs(w[KEYS[0]])
            for k in (KEYS[1], KEYS[3], KEYS[5]):
                w[k] = -np.abs(w[k])
        elif name == "alive":
            for k in KEYS[:6]:
                w[k] = np.abs(w[k])
        else:
            raise KeyError(name)
        for v in w.values():
            v.setflags(write=False)
        x.setflags(write=False)
        _CACHE[name] = (w, x)
    return _CACHE[name]


def _conv4s2(x, w, b):
    """conv 4x4, stride 2, padding 1 in float64: x [n,C,H,W] -> [n,O,H/2,W/2]."""
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    win = np.lib.stride_tricks.sliding_window_view(xp, (4, 4), axis=(2, 3))[:, :, ::2, ::2]  # [n,C,oh,ow,4,4]
    return np.einsum("nchwyx,ocyx->nohw", win, w, optimize=True) + b[None, :, None, None]


def forward64(weights, x):
    """-> (logits [n,10] float64, [(min, max) pre-activation of conv1, conv2, fc1])."""
    w = [np.asarray(weights[k], np.float64) for k in KEYS]
    h = np.asarray(x, np.float64)
    pre = []
    a = _conv4s2(h, w[0], w[1])
    pre.append((a.min(), a.max()))
    a = _conv4s2(np.maximum(a, 0), w[2], w[3])
    pre.append((a.min(), a.max()))
    a = np.maximum(a, 0).reshape(a.shape[0], -1) @ w[4].T + w[5]
    pre.append((a.min(), a.max()))
    return np.maximum(a, 0) @ w[6].T + w[7], pre


def logits64(name):
    """The float64 logits [256,10] of a regime: computed once, shared, read-only."""
    key = ("logits", name)
    if key not in _CACHE:
        out, pre = forward64(*regime(name))
        out.setflags(write=False)
        _CACHE[key] = out
        _CACHE[("pre", name)] = pre
    return _CACHE[key]


def preacts64(name):
    logits64(name)
    return _CACHE[("pre", name)]


def dist(logits, ref):
    """The largest row distance of logits from ref (float64), relative to each row's largest |ref|."""
    logits, ref = np.asarray(logits, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.max(np.abs(logits - ref), axis=1) / np.max(np.abs(ref), axis=1)))


def margins(ref):
    """The top-2 margin of every row of ref, relative to the row's largest |ref|."""
    s = np.sort(np.asarray(ref, np.float64), axis=1)
    return (s[:, -1] - s[:, -2]) / np.max(np.abs(ref), axis=1)


def counts_model(pred, labels, label_rows=None, counts=None):
    """The [11,2] counts after one update (ClassCounts.update / mvk_polyclf_fwd): row i has labels[i % label_rows]."""
    pred, labels = np.asarray(pred).reshape(-1), np.asarray(labels).reshape(-1)
    label_rows = len(labels) if label_rows is None else label_rows
    counts = np.zeros((11, 2), np.int64) if counts is None else counts.copy()
    for i, p in enumerate(pred):
        lab = labels[i % label_rows]
        r = lab if 0 <= lab < 10 else 10
        counts[r, 0] += int(p == lab)
        counts[r, 1] += 1
    return counts


def state_dict(weights, torch, device="cpu"):
    return {k: torch.from_numpy(np.array(weights[k])).to(device) for k in KEYS}
