"""The SSIM and squared-error definition of DESIGN.md ("Metrics") in float64, written from the definition.

For preds and target [B,C,H,W] of ONE update:
    R = max(preds.max() - preds.min(), target.max() - target.min()), c1 = (0.01 R)^2, c2 = (0.03 R)^2;
    g[i] ~ exp(-((i - 5) / 1.5)^2 / 2), 11 taps normalised to sum 1, the 2-D weight is the outer product, per channel;
    only the (H - 10) x (W - 10) positions whose window lies inside the image;
    ssim = (2 mu_p mu_t + c1) (2 s_pt + c2) / ((mu_p^2 + mu_t^2 + c1) (s_p^2 + s_t^2 + c2)) with s_p^2 = E[pp] - mu_p^2, not clamped;
    the SSIM of an image is the mean over its C (H - 10) (W - 10) positions.
An evaluation is a list of updates: SSIM = (sum of per-image SSIM) / (number of images), MSE = (sum of squared differences) /
(number of batch rows), both over every update.

`ssim64` is the reference (weighted moments through a strided window view); `ssim64_loops` is the same definition as 121 explicit
shifted sums, for the cross-check of test_metrics_host.py.  The keyword arguments of `ssim64` are deliberate MISTAKES, used to
show that the tests' bar separates them.  `emulate_fp32` restates the arithmetic of csrc/ssim.hip in numpy float32 and
`uncentred_fp32` the textbook E[x^2] - mu^2 in float32, so that the CPU suite can say what each costs without a GPU.
"""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

BAR = 5e-6        # |per-image SSIM - float64|, every regime
SSE_BAR = 1e-6    # relative, sse_rows against float64


def taps(sigma=1.5, win=11, dtype=np.float64):
    i = np.arange(win, dtype=np.float64) - (win - 1) / 2
    g = np.exp(-0.5 * (i / sigma) ** 2)
    return (g / g.sum()).astype(dtype)


def data_range(preds, target):
    """R of one update, in the dtype of the inputs (float32 inputs give the fp32 value of the definition)."""
    return max(preds.max() - preds.min(), target.max() - target.min())


def _moment(x, g):
    """Weighted window sums over the last two axes, valid positions only."""
    v = sliding_window_view(x, (len(g), len(g)), axis=(-2, -1))
    return np.einsum("...ij,i,j->...", v, g, g)


def ssim64(preds, target, R=None, *, sigma=1.5, win=11, k2=0.03, clamp=False, per_image_range=False, padded=False):
    p, t = np.asarray(preds, np.float64), np.asarray(target, np.float64)
    if R is None:
        R = float(data_range(p, t))
    Rb = np.full((p.shape[0], 1, 1, 1), float(R))
    if per_image_range:  # mistake: the range of each image instead of the update's
        ax = (1, 2, 3)
        Rb = np.maximum(p.max(ax) - p.min(ax), t.max(ax) - t.min(ax)).reshape(-1, 1, 1, 1)
    if padded:  # mistake: reflect-pad and keep every position
        pad = ((0, 0), (0, 0), (win // 2, win // 2), (win // 2, win // 2))
        p, t = np.pad(p, pad, mode="reflect"), np.pad(t, pad, mode="reflect")
    g = taps(sigma, win)
    c1, c2 = (0.01 * Rb) ** 2, (k2 * Rb) ** 2
    mp, mt = _moment(p, g), _moment(t, g)
    vp, vt, cv = _moment(p * p, g) - mp * mp, _moment(t * t, g) - mt * mt, _moment(p * t, g) - mp * mt
    if clamp:  # mistake: variances clamped at zero
        vp, vt = np.maximum(vp, 0.0), np.maximum(vt, 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        maps = ((2 * mp * mt + c1) * (2 * cv + c2)) / ((mp * mp + mt * mt + c1) * (vp + vt + c2))
    return dict(maps=maps, rows=maps.mean(axis=(1, 2, 3)), R=float(R), var_p=vp, var_t=vt)


def ssim64_loops(preds, target):
    """The same definition with explicit loops over the 11 x 11 taps (no window view, no einsum)."""
    p, t = np.asarray(preds, np.float64), np.asarray(target, np.float64)
    R = float(data_range(p, t))
    g = taps()
    H, W = p.shape[-2:]
    oh, ow = H - 10, W - 10

    def mom(x):
        out = np.zeros(x.shape[:-2] + (oh, ow))
        for i in range(11):
            for j in range(11):
                out += (g[i] * g[j]) * x[..., i:i + oh, j:j + ow]
        return out

    c1, c2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    mp, mt = mom(p), mom(t)
    vp, vt, cv = mom(p * p) - mp ** 2, mom(t * t) - mt ** 2, mom(p * t) - mp * mt
    with np.errstate(invalid="ignore", divide="ignore"):
        maps = ((2 * mp * mt + c1) * (2 * cv + c2)) / ((mp ** 2 + mt ** 2 + c1) * (vp + vt + c2))
    return dict(maps=maps, rows=maps.mean(axis=(1, 2, 3)), R=R)


def sse64(preds, target):
    """Per-row sum of squared differences, [B]."""
    d = np.asarray(preds, np.float64) - np.asarray(target, np.float64)
    return (d * d).reshape(len(d), -1).sum(1)


def aggregate(updates, metric):
    """The evaluator-level value of a list of (preds, target) updates; an update is one (batch, modality) pair."""
    rows = sum(len(p) for p, _ in updates)
    if metric == "SSIM":
        return sum(float(ssim64(p, t)["rows"].sum()) for p, t in updates) / rows
    if metric == "MSE":
        return sum(float(sse64(p, t).sum()) for p, t in updates) / rows
    raise ValueError(metric)


# ---- float32 emulations (CPU statements about precision; the GPU tests compare the kernel itself) ---------------------------
def emulate_fp32(preds, target, R=None):
    """csrc/ssim.hip's arithmetic in numpy float32: every mean is first tap + sum g (x - first tap), the row variance is centred on
    the row mean and the row means on the window mean (law of total variance).  Per-image rows, float64 mean of float32 positions."""
    f = np.float32
    p, t = np.asarray(preds, f), np.asarray(target, f)
    R = f(data_range(p, t) if R is None else R)
    g = taps(dtype=f)
    H, W = p.shape[-2:]
    oh, ow = H - 10, W - 10

    def centred(a, b, va=None, vb=None, vab=None, axis=-1, n=ow):
        sl = lambda x, k: x[..., k:k + n] if axis == -1 else x[..., k:k + n, :]
        a0, b0 = sl(a, 0), sl(b, 0)
        da, db = [sl(a, k) - a0 for k in range(11)], [sl(b, k) - b0 for k in range(11)]
        sa, sb = np.zeros_like(a0), np.zeros_like(b0)
        for k in range(11):
            sa, sb = sa + g[k] * da[k], sb + g[k] * db[k]
        qa, qb, qab = np.zeros_like(a0), np.zeros_like(a0), np.zeros_like(a0)
        for k in range(11):
            x, y = da[k] - sa, db[k] - sb
            qa = qa + g[k] * (x * x + (sl(va, k) if va is not None else f(0)))
            qb = qb + g[k] * (y * y + (sl(vb, k) if vb is not None else f(0)))
            qab = qab + g[k] * (x * y + (sl(vab, k) if vab is not None else f(0)))
        return a0 + sa, b0 + sb, qa, qb, qab

    mp, mt, vp, vt, cv = centred(p, t)
    mp, mt, vp, vt, cv = centred(mp, mt, vp, vt, cv, axis=-2, n=oh)
    c1, c2 = (f(0.01) * R) ** 2, (f(0.03) * R) ** 2
    with np.errstate(invalid="ignore", divide="ignore"):
        maps = ((f(2) * mp * mt + c1) * (f(2) * cv + c2)) / ((mp * mp + mt * mt + c1) * (vp + vt + c2))
    assert maps.dtype == f
    return maps.astype(np.float64).mean(axis=(1, 2, 3))


def uncentred_fp32(preds, target):
    """The textbook form in float32: E[x^2] - mu^2 from raw second moments."""
    f = np.float32
    p, t = np.asarray(preds, f), np.asarray(target, f)
    R = f(data_range(p, t))
    g = taps(dtype=f)
    mp, mt = _moment(p, g), _moment(t, g)
    vp, vt, cv = _moment(p * p, g) - mp * mp, _moment(t * t, g) - mt * mt, _moment(p * t, g) - mp * mt
    c1, c2 = (f(0.01) * R) ** 2, (f(0.03) * R) ** 2
    with np.errstate(invalid="ignore", divide="ignore"):
        maps = ((f(2) * mp * mt + c1) * (f(2) * cv + c2)) / ((mp * mp + mt * mt + c1) * (vp + vt + c2))
    return maps.astype(np.float64).mean(axis=(1, 2, 3))


# ---- the case table ---------------------------------------------------------------------------------------------------------
def shapes(tile):
    """The shapes of the kernel cases; `tile` is the kernel's tile edge in window positions (mvk_ssim_tile)."""
    return [(1, 1, 11, 11), (2, 1, 12, 11), (2, 1, 11, 13), (5, 1, 28, 28), (3, 3, 32, 32), (2, 2, tile + 1, tile + 11),
            (1, 3, 64, 64)]


REGIMES = ("uniform", "near", "binary", "square", "scaled255", "flat", "patch")


def make(regime, shape, seed=0):
    """(preds, target) of a regime as float32 arrays; seeded, so that host and GPU tests see the same inputs."""
    rng = np.random.default_rng([seed, REGIMES.index(regime), *shape])
    B, C, H, W = shape
    u = lambda: rng.random(shape)
    if regime == "uniform":
        p, t = u(), u()
    elif regime == "near":
        t = u()
        p = t + 1e-3 * rng.standard_normal(shape)
    elif regime == "binary":  # binary target, the prediction is its five-point average
        t = (u() > 0.5).astype(np.float64)
        p = (t + np.roll(t, 1, -1) + np.roll(t, -1, -1) + np.roll(t, 1, -2) + np.roll(t, -1, -2)) / 5
    elif regime == "square":  # a white square on black; the prediction is dimmer and one pixel off
        t = np.zeros(shape)
        t[..., H // 4:H - H // 4, W // 4:W - W // 4] = 1.0
        p = 0.9 * np.roll(t, 1, -1) + 0.05
    elif regime == "scaled255":
        p, t = 255 * u(), 255 * u()
    elif regime == "flat":  # constant 0.7 plus 1e-4 noise; two outlier pixels set R = 1
        p = 0.7 + 1e-4 * rng.standard_normal(shape)
        t = 0.7 + 1e-4 * rng.standard_normal(shape)
        t[0, 0, 0, 0], t[0, 0, H - 1, W - 1] = 0.0, 1.0
    elif regime == "patch":  # one flat bright patch inside a textured image
        p, t = u(), u()
        ys, xs = slice(H // 5, H - H // 5), slice(W // 5, W - W // 5)
        n = t[..., ys, xs].shape
        t[..., ys, xs] = 0.9 + 1e-4 * rng.standard_normal(n)
        p[..., ys, xs] = 0.9 + 1e-4 * rng.standard_normal(n)
    else:
        raise ValueError(regime)
    return p.astype(np.float32), t.astype(np.float32)


def cases(tile):
    return [(f"{r}-{'x'.join(map(str, s))}", r, s) for s in shapes(tile) for r in REGIMES]
