"""Float64 torch reference of the inverse autoregressive flow kernels (mvk_iaf_fwd/bwd/inverse, csrc/maf.hip), written from the
formulas, with the kernels' case table, seeded inputs and error model.  CPU only: no GPU, no libmvk.so; nothing here reads the
reference project or multivae_amd.  The MADE, its masks and the error model's building blocks are those of tests/jnf_ref.py.

Flow.  (m, s) = MADE(.).  Forward, block by block: from y = 0, y_i = (x_i - m_i(y)) exp(-s_i(y)), ladj -= s_i(y) for i = 0..D-1,
then x = flip(y).  Inverse, blocks in reverse: y = flip(y), x = y exp(s(y)) + m(y), ladj += sum_d s_d.  NLL row under N(0, I):
rows[b] = -(sum_d ln N(z0_d; 0, 1) + ladj).

Backward (`sweep_backward`), restated by the reverse sweep and NOT by autograd: a block defines y by x_j = y_j exp(s_j(y)) + m_j(y),
whose Jacobian in y is lower triangular with diagonal exp(s_j).  With gy = dL/dy and gl = dL/dladj, for i = D-1..0:
v_i = sum_{j>i} (cm_j dm_j/dy_i + cs_j ds_j/dy_i) (the MADE's input gradient at i for the cotangents known so far),
lam_i = exp(-s_i) (gy_i + v_i), cm_i = -lam_i, cs_i = -gl - lam_i y_i exp(s_i).  dx = lam; the parameter gradients are the MADE's
VJP at y with output cotangents (cm, cs).  tests/test_iaf_host.py checks the sweep against float64 autograd.

Error model: that of tests/jnf_ref.py (first-order running error analysis in float64, u = 2^-24), carried through the D steps of
the forward sweep and through the triangular solve of the backward.  A comparison passes when |got - ref| <= C_STAGE[stage] * base
for EVERY entry; C_STAGE = 4x the largest |err| / base that the same formulas in plain torch fp32 on the CPU (backward: fp32
autograd through the forward sweep) show over the case table, rounded up (tests/test_iaf_host.py::test_error_constants re-derives
it; the HIP kernels have no part in it).  `mut` names deliberate mistakes of the REFERENCE, used only to show that the bounds reject
them (TEETH)."""
import math
from dataclasses import dataclass

import torch

from jnf_ref import (F64, LOG_2PI, LV_MAX, TINY, U, _made_err, depth, layer_shapes, made, masks,  # noqa: F401
                     worst_ratio)

# one constant per output: 4x the value measured by tests/test_iaf_host.py::test_error_constants, rounded up
C_STAGE = {"z0": 3.0, "ladj": 0.5, "rows": 0.7, "dx": 10.0, "dW": 0.8, "db": 1.4, "x_inv": 2.6, "ladj_inv": 0.3}
STAGES = tuple(C_STAGE)

# ---- the kernels' case table --------------------------------------------------------------------------------------------------------
DS = (2, 3, 20, 65)        # all hidden degrees 0; odd (the flip has a fixed middle element); the default; past one wave and odd
HS = (3, 64, 130)
NHS = (1, 3)
NBS = (1, 2, 3)            # even and odd flip counts
BS = (1, 3, 70)            # partial row tiles
# the optional pointers, cycled over the grid: rows (and with it grows), dx, the weight gradients, the inverse's ladj
NULLS = ((), ("rows",), ("dx",), ("wgrad",), ("ladj_inv",), ("dx", "wgrad"))


@dataclass(frozen=True)
class Case:
    name: str
    D: int
    H: int
    nh: int
    nb: int
    B: int
    null: tuple
    seed: int
    backward: bool = True


def _cases():
    out, i = [], 0
    for D in DS:
        for H in HS:
            for nh in NHS:
                for nb in NBS:
                    for B in BS:
                        null = NULLS[(i + i // 6 + i // 36) % len(NULLS)]
                        out.append(Case(f"d{D}-h{H}-n{nh}-k{nb}-b{B}" + "".join("-null-" + n for n in null), D, H, nh, nb, B, null,
                                        8000 + i))
                        i += 1
    out.append(Case("d512-h128-n3-k2-b3-fwd-inv", 512, 128, 3, 2, 3, (), 8000 + i, backward=False))
    return out


CASES = _cases()
CASE_BY_NAME = {c.name: c for c in CASES}


def make_inputs(case):
    """Seeded fp32 inputs.  W[blk][l], b[blk][l]: U(-g, g) / sqrt(fan_in) with g graded over the blocks and small enough that every
    |s| stays below LV_MAX through the D-step sweep (asserted in `bases`); x, y [B,D]; the upstream gradients grows [B], dz0 [B,D],
    dladj [B] (None: not given — without rows both dz0 and dladj are given, with them grows always and the others in turn)."""
    g = torch.Generator().manual_seed(case.seed)
    D, H, nh, nb, B = case.D, case.H, case.nh, case.nb, case.B
    W, b = [], []
    for blk in range(nb):
        gain = 0.4 + 0.2 * (blk % 3)
        W.append([(2 * torch.rand(s, generator=g) - 1) * gain / math.sqrt(s[1]) for s in layer_shapes(D, H, nh)])
        b.append([(2 * torch.rand(s[0], generator=g) - 1) * 0.2 for s in layer_shapes(D, H, nh)])
    x = 1.5 * torch.randn(B, D, generator=g)
    y = 1.5 * torch.randn(B, D, generator=g)
    rows = "rows" not in case.null
    i = case.seed
    grows = torch.randn(B, generator=g) if rows else None
    dz0 = torch.randn(B, D, generator=g) if (not rows or i % 2 == 0) else None
    dladj = torch.randn(B, generator=g) if (not rows or i % 3 == 0) else None
    return dict(W=W, b=b, x=x, y=y, grows=grows, dz0=dz0, dladj=dladj)


# ---- formulas ------------------------------------------------------------------------------------------------------------------------
# flip_first: the flip in front of the block instead of behind it; ladj_sign: ladj += s in the forward; drop_gl: cs without its gl
# term; out_le: the output layer's degree threshold off by one (jnf_ref.masks)
MUTATIONS = ["flip_first", "ladj_sign", "drop_gl", "out_le"]
# (mutation, the stages where it must show, the cases named for it)
TEETH = [
    ("flip_first", ("z0",), ["d3-h64-n1-k1-b3-null-wgrad", "d20-h64-n3-k3-b3"]),
    ("ladj_sign", ("ladj", "rows"), ["d20-h64-n3-k3-b3", "d65-h130-n3-k2-b70"]),
    ("drop_gl", ("dx", "dW", "db"), ["d3-h64-n1-k2-b3", "d20-h64-n3-k3-b3", "d65-h130-n3-k2-b70"]),
    ("out_le", ("z0", "x_inv"), ["d2-h3-n1-k1-b1", "d20-h64-n3-k3-b3"]),
]


def _with_col(y, i, col):
    return torch.cat([y[:, :i], col.unsqueeze(1), y[:, i + 1:]], dim=1)


def iaf_forward(Wm, bm, x, mut=(), keep=None):
    """One flow: Wm[blk][l] -> z0 [B,D], ladj [B].  keep (a list): gets (y, s) of every block."""
    D, H, nh = x.shape[1], Wm[0][0].shape[0], len(Wm[0]) - 1
    mk = masks(D, H, nh, mut)
    ladj = torch.zeros(x.shape[0], dtype=x.dtype)
    for Wb, bb in zip(Wm, bm):
        if "flip_first" in mut:
            x = x.flip(1)
        y, s_all = torch.zeros_like(x), torch.zeros_like(x)
        for i in range(D):
            m, s = made(Wb, bb, mk, y)
            y = _with_col(y, i, (x[:, i] - m[:, i]) * torch.exp(-s[:, i]))
            s_all = _with_col(s_all, i, s[:, i])
            ladj = ladj + s[:, i] if "ladj_sign" in mut else ladj - s[:, i]
        if keep is not None:
            keep.append((y, s_all))
        x = y if "flip_first" in mut else y.flip(1)
    return x, ladj


def iaf_inverse(Wm, bm, y, mut=()):
    """One flow -> x [R,D] with forward(x) = y, ladj [R] (= -forward's)."""
    D, H, nh = y.shape[1], Wm[0][0].shape[0], len(Wm[0]) - 1
    mk = masks(D, H, nh, mut)
    ladj = torch.zeros(y.shape[0], dtype=y.dtype)
    for blk in range(len(Wm) - 1, -1, -1):
        if "flip_first" not in mut:
            y = y.flip(1)
        m, s = made(Wm[blk], bm[blk], mk, y)
        y = y * torch.exp(s) + m
        ladj = ladj + s.sum(-1)
        if "flip_first" in mut:
            y = y.flip(1)
    return y, ladj


def nll_rows(z0, ladj):
    return -((-0.5 * (LOG_2PI + z0 ** 2)).sum(-1) + ladj)


def made_acts(Wb, bb, mk, y):
    """The inputs of the MADE's layers at y: [y, h_0, .., h_{nh-1}]."""
    acts, h = [], y
    for l, (w, bias, m) in enumerate(zip(Wb, bb, mk)):
        acts.append(h)
        if l < len(Wb) - 1:
            h = torch.relu(h @ (w * m.to(w.dtype)).T + bias)
    return acts


def made_vjp(Wb, mk, acts, cout):
    """cout [B,2D]: the cotangents of (m, s) -> the input gradient [B,D], the pre-activation deltas of every layer."""
    delta, deltas = cout, [None] * len(Wb)
    for l in range(len(Wb) - 1, -1, -1):
        deltas[l] = delta
        back = delta @ (Wb[l] * mk[l].to(Wb[l].dtype))
        delta = back * (acts[l] > 0).to(back.dtype) if l > 0 else back
    return delta, deltas


def upstream(I, z0, dtype):
    """-> gz0 [B,D], gl [B]: dL/dz0 and dL/dladj of L = grows . rows + dz0 . z0 + dladj . ladj."""
    gz0 = torch.zeros_like(z0)
    gl = torch.zeros(z0.shape[0], dtype=dtype)
    if I["grows"] is not None:
        gz0 = I["grows"].to(dtype).unsqueeze(1) * z0
        gl = -I["grows"].to(dtype)
    if I["dz0"] is not None:
        gz0 = gz0 + I["dz0"].to(dtype)
    if I["dladj"] is not None:
        gl = gl + I["dladj"].to(dtype)
    return gz0, gl


def sweep_backward(Wm, bm, saved, gz0, gl, mut=()):
    """saved: [(y, s)] of every block -> dx [B,D], dW, db (lists over (block, layer))."""
    D, H, nh = gz0.shape[1], Wm[0][0].shape[0], len(Wm[0]) - 1
    mk = masks(D, H, nh, mut)
    g = gz0
    dW, db = [None] * len(Wm), [None] * len(Wm)
    for blk in range(len(Wm) - 1, -1, -1):
        y, s = saved[blk]
        gy = g.flip(1)
        acts = made_acts(Wm[blk], bm[blk], mk, y)
        lam = torch.zeros_like(y)
        cout = torch.zeros(y.shape[0], 2 * D, dtype=y.dtype)
        for i in range(D - 1, -1, -1):
            v, _ = made_vjp(Wm[blk], mk, acts, cout)  # cout holds the cotangents of j > i only
            lam_i = torch.exp(-s[:, i]) * (gy[:, i] + v[:, i])
            lam[:, i] = lam_i
            cout[:, i] = -lam_i
            cout[:, D + i] = (0 if "drop_gl" in mut else -gl) - lam_i * (y[:, i] * torch.exp(s[:, i]))
        _, deltas = made_vjp(Wm[blk], mk, acts, cout)
        dW[blk] = [(d.T @ a) * m.to(d.dtype) for d, a, m in zip(deltas, acts, mk)]
        db[blk] = [d.sum(0) for d in deltas]
        g = lam
    return g, [w for Wb in dW for w in Wb], [v for bb in db for v in bb]


def _cast(I, dtype, grad):
    W = [[w.to(dtype, copy=True).requires_grad_(grad) for w in Wb] for Wb in I["W"]]
    b = [[v.to(dtype, copy=True).requires_grad_(grad) for v in bb] for bb in I["b"]]
    return W, b


def evaluate(case, I, dtype, mut=(), autograd=False, inverse=True):
    """Forward, backward (the reverse sweep, or autograd through the forward sweep) and inverse in `dtype` on the fp32 inputs ->
    dict of STAGES (None: not produced).  dW, db: lists over (block, layer)."""
    grad = case.backward and autograd
    W, b = _cast(I, dtype, grad)
    x = I["x"].to(dtype, copy=True).requires_grad_(grad)
    saved = []
    with torch.set_grad_enabled(grad):
        z0, ladj = iaf_forward(W, b, x, mut, keep=saved)
        rows = nll_rows(z0, ladj)
    out = dict(z0=z0.detach(), ladj=ladj.detach(), rows=rows.detach() if "rows" not in case.null else None, dx=None, dW=None, db=None,
               x_inv=None, ladj_inv=None)
    if case.backward and autograd:
        total = z0.sum() * 0
        if I["grows"] is not None:
            total = total + (rows * I["grows"].to(dtype)).sum()
        if I["dz0"] is not None:
            total = total + (z0 * I["dz0"].to(dtype)).sum()
        if I["dladj"] is not None:
            total = total + (ladj * I["dladj"].to(dtype)).sum()
        flatW, flatb = [w for Wb in W for w in Wb], [v for bb in b for v in bb]
        gs = torch.autograd.grad(total, [x] + flatW + flatb, allow_unused=True)
        gs = [torch.zeros_like(t) if g is None else g for g, t in zip(gs, [x] + flatW + flatb)]
        out["dx"], out["dW"], out["db"] = gs[0], list(gs[1:1 + len(flatW)]), list(gs[1 + len(flatW):])
    elif case.backward:
        with torch.no_grad():
            gz0, gl = upstream(I, z0, dtype)
            out["dx"], out["dW"], out["db"] = sweep_backward(W, b, saved, gz0, gl, mut)
    if inverse:
        with torch.no_grad():
            Wd, bd = _cast(I, dtype, False)
            out["x_inv"], out["ladj_inv"] = iaf_inverse(Wd, bd, I["y"].to(dtype), mut)
    return out


def reference(case, I, mut=()):
    return evaluate(case, I, F64, mut)


def run_torch32(case, I):
    return evaluate(case, I, torch.float32, autograd=True)


# ---- the running error analysis ---------------------------------------------------------------------------------------------------------
def _vjp_err(Wb, mk, acts, cout, ecout):
    """made_vjp with the bound of every value: -> v, ev, deltas, edeltas.  A sum over n outputs is a lane's run plus the wave tree."""
    delta, edelta = cout, ecout
    deltas, edeltas = [None] * len(Wb), [None] * len(Wb)
    for l in range(len(Wb) - 1, -1, -1):
        deltas[l], edeltas[l] = delta, edelta
        wm = Wb[l] * mk[l].to(F64)
        A = wm.abs()
        back = delta @ wm
        eback = edelta @ A + (depth(Wb[l].shape[0]) + 1) * U * (delta.abs() @ A)
        if l > 0:
            on = (acts[l] > 0).to(F64)
            delta, edelta = back * on, eback * on
        else:
            delta, edelta = back, eback
    return delta, edelta, deltas, edeltas


def bases(case, I, ref=None):
    """The error model's base of every output (float64, the shapes of `reference`), and the largest |s| met."""
    ref = reference(case, I) if ref is None else ref
    D, H, nh, nb, B = case.D, case.H, case.nh, case.nb, case.B
    mk = masks(D, H, nh)
    out = {k: None for k in STAGES}
    with torch.no_grad():
        W, b = _cast(I, F64, False)
        x, ex = I["x"].to(F64), torch.zeros(B, D, dtype=F64)
        ladj, eladj = torch.zeros(B, dtype=F64), torch.zeros(B, dtype=F64)
        lv_max = 0.0
        saved = []
        for blk in range(nb):
            y, ey = torch.zeros_like(x), torch.zeros_like(x)
            s_all, es_all = torch.zeros_like(x), torch.zeros_like(x)
            for i in range(D):
                o, eo, _, _ = _made_err(W[blk], b[blk], mk, y, ey)
                m, s, em, es = o[:, i], o[:, D + i], eo[:, i], eo[:, D + i]
                lv_max = max(lv_max, float(s.abs().max()))
                d = x[:, i] - m
                ed = ex[:, i] + em + U * d.abs()
                E = torch.exp(-s)
                eE = E * (es + U * (1 + s.abs()))
                y[:, i] = d * E
                ey[:, i] = ed * E + d.abs() * eE + U * y[:, i].abs()
                s_all[:, i], es_all[:, i] = s, es
                ladj = ladj - s
                eladj = eladj + es + U * ladj.abs()
            _, _, acts, errs = _made_err(W[blk], b[blk], mk, y, ey)
            saved.append((y, ey, s_all, es_all, acts, errs))
            x, ex = y.flip(1), ey.flip(1)
        out["z0"], out["ladj"] = ex + TINY, eladj + TINY
        term = 0.5 * (LOG_2PI + x ** 2)
        out["rows"] = (x.abs() * ex + 2 * U * term).sum(-1) + depth(D) * U * term.sum(-1) + eladj + U * nll_rows(x, ladj).abs() + TINY
        if case.backward:
            gz0, gl = upstream(I, x, F64)
            egz0 = U * gz0.abs()
            if I["grows"] is not None:
                gr = I["grows"].to(F64).abs().unsqueeze(1)
                egz0 = egz0 + gr * ex + U * gr * x.abs()
            egl = U * gl.abs()
            g, eg = gz0, egz0
            e_dW, e_db = [None] * nb, [None] * nb
            for blk in range(nb - 1, -1, -1):
                y, ey, s, es, acts, errs = saved[blk]
                gy, egy = g.flip(1), eg.flip(1)
                lam, elam = torch.zeros_like(y), torch.zeros_like(y)
                cout, ecout = torch.zeros(B, 2 * D, dtype=F64), torch.zeros(B, 2 * D, dtype=F64)
                for i in range(D - 1, -1, -1):
                    v, ev, _, _ = _vjp_err(W[blk], mk, acts, cout, ecout)
                    E = torch.exp(-s[:, i])
                    eE = E * (es[:, i] + U * (1 + s[:, i].abs()))
                    a = gy[:, i] + v[:, i]
                    ea = egy[:, i] + ev[:, i] + U * a.abs()
                    lam[:, i] = E * a
                    elam[:, i] = E * ea + a.abs() * eE + U * lam[:, i].abs()
                    Ep = torch.exp(s[:, i])
                    t = y[:, i] * Ep
                    et = ey[:, i] * Ep + y[:, i].abs() * Ep * (es[:, i] + U * (1 + s[:, i].abs())) + U * t.abs()
                    cout[:, i], ecout[:, i] = -lam[:, i], elam[:, i]
                    cout[:, D + i] = -gl - lam[:, i] * t
                    ecout[:, D + i] = egl + elam[:, i] * t.abs() + lam[:, i].abs() * et + U * (lam[:, i] * t).abs() \
                        + U * cout[:, D + i].abs()
                _, _, deltas, edeltas = _vjp_err(W[blk], mk, acts, cout, ecout)
                e_dW[blk] = [(ed.T @ a.abs() + d.abs().T @ ea + (depth(4 * B) + 1) * U * (d.abs().T @ a.abs()) + TINY) * m.to(F64) + TINY
                             for d, ed, a, ea, m in zip(deltas, edeltas, acts, errs, mk)]
                e_db[blk] = [ed.sum(0) + (depth(4 * B) + 1) * U * d.abs().sum(0) + TINY for d, ed in zip(deltas, edeltas)]
                g, eg = lam, elam
            out["dx"] = eg + TINY
            out["dW"], out["db"] = [w for e in e_dW for w in e], [v for e in e_db for v in e]
        # inverse
        y, ey = I["y"].to(F64), torch.zeros(B, D, dtype=F64)
        ladj, eladj = torch.zeros(B, dtype=F64), torch.zeros(B, dtype=F64)
        for blk in range(nb - 1, -1, -1):
            y, ey = y.flip(1), ey.flip(1)
            o, eo, _, _ = _made_err(W[blk], b[blk], mk, y, ey)
            m, s, em, es = o[:, :D], o[:, D:], eo[:, :D], eo[:, D:]
            lv_max = max(lv_max, float(s.abs().max()))
            E = torch.exp(s)
            xn = y * E + m
            ey = ey * E + y.abs() * E * (es + U * (1 + s.abs())) + em + U * ((y * E).abs() + xn.abs())
            y = xn
            ladj = ladj + s.sum(-1)
            eladj = eladj + es.sum(-1) + depth(D) * U * s.abs().sum(-1) + U * ladj.abs()
        out["x_inv"], out["ladj_inv"] = ey + TINY, eladj + TINY
    out["lv_max"] = lv_max
    assert lv_max < LV_MAX, f"{case.name}: |s| reaches {lv_max}: the inputs, not the flow, would overflow exp"
    return out


def ratios(case, I, got, mut=(), ref=None, base=None):
    """max |got - ref| / base per stage over EVERY entry (`got[k]` None: not written) -> {stage: ratio}."""
    ref = reference(case, I, mut) if ref is None else ref
    base = bases(case, I) if base is None else base
    out = {}
    for k in STAGES:
        if got.get(k) is None or ref.get(k) is None:
            continue
        if isinstance(ref[k], list):
            assert len(got[k]) == len(ref[k]) == len(base[k]), (k, len(got[k]), len(ref[k]), len(base[k]))
            worst = 0.0
            for g, r, bs in zip(got[k], ref[k], base[k]):
                if g is None:
                    continue
                assert g.shape == r.shape == bs.shape, (k, g.shape, r.shape, bs.shape)
                worst = max(worst, worst_ratio(g, r, bs))
            out[k] = worst
        else:
            assert got[k].shape == ref[k].shape == base[k].shape, (k, got[k].shape, ref[k].shape, base[k].shape)
            out[k] = worst_ratio(got[k], ref[k], base[k])
    return out
