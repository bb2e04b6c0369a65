"""Float64 torch reference of the masked autoregressive flow kernels (mvk_maf_fwd/bwd/inverse, csrc/maf.hip), of both stages of the
JNF training loss, of the product-of-experts log-density of JNF's sampler and of that sampler (Hamiltonian Monte Carlo fed with given
draws), written from the formulas; plus the kernels' case table, seeded inputs and error model, and the procedural inputs of the JNF
golden cases (tests/golden/jnf_*.npz).  CPU only: no GPU, no libmvk.so; nothing here reads the reference project or
multivae_amd.

Flow.  D inputs, hidden width H, nh hidden layers, nb blocks.  Degrees: inputs arange(D), hidden unit k: k % (D - 1).  Layer 0
[H,D]: W[o,k] counts when deg(o) >= k; hidden layers [H,H]: when deg(o) >= deg(k); output layer [2D,H]: rows d and D + d when
deg(k) < d.  MADE(x) = (mu, lv) = the two halves of the output.  Forward, block by block: u = (x - mu(x)) exp(-lv(x)),
ladj -= sum_d lv_d, x = flip(u).  Inverse, blocks in reverse: y = flip(y), x_i = y_i exp(lv_i(x)) + mu_i(x) for i = 0..D-1 from
x = 0, ladj += lv_i.  Row term of JNF's stage two: rows[m,b] = -(sum_l ln N(z0; mu0, exp(lv0 / 2)) + ladj).

Error model (the form of tests/telbo_ref.py): a first-order running error analysis in float64.  u = 2^-24.  Every value of the
chain carries a bound of its absolute error, handed on through every operation: a masked linear layer y = W x + b with n addends
hands on |W| e_x + (depth(n) + 1) u (|W| |x| + |b|) (depth: the longest chain of additions of the kernels' sums, a lane's
sequential run plus the wave tree), exp(a) hands on exp(a) (e_a + u (1 + |a|)), a product or a sum its operands' bounds plus u
times its own magnitude.  The backward chain is analysed the same way with the forward's bounds in its coefficients.  An output
entry's `base` is that bound (plus the smallest normal).  A comparison passes when |got - ref| <= C_STAGE[stage] * base for EVERY
entry; C_STAGE = 4x the largest |err| / base that the same formulas in plain torch fp32 on the CPU (backward: fp32 autograd) show
over the case table, rounded up (tests/test_jnf_host.py::test_error_constants re-derives it; the HIP kernels have no part in it).
`mut` names deliberate mistakes of the REFERENCE, used only to show that the bounds reject them (MUTATIONS)."""
import math
import os
import sys
from collections import OrderedDict
from dataclasses import dataclass

import numpy as np
import torch

from cvae_ref import LOG_2PI, joint_encoder
from mmvae_ref import TINY, U, worst_ratio  # noqa: F401  (re-exported to the tests)
from telbo_ref import mlp_decoder, mlp_encoder, nll_rows

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import procedural as P  # noqa: E402

F64 = torch.float64
LV_MAX = 6.0  # every |lv| of the case table stays below: exp(+-lv) over several blocks must not overflow (asserted in `reference`)

# one constant per output: 4x the value measured by tests/test_jnf_host.py::test_error_constants, rounded up
C_STAGE = {"z0": 3.0, "ladj": 0.4, "rows": 1.0, "dmu0": 2.5, "dlv0": 2.5, "dz": 2.0, "dW": 1.0, "db": 1.0, "x_inv": 3.0,
           "ladj_inv": 0.4}
STAGES = tuple(C_STAGE)

# ---- the kernels' case table --------------------------------------------------------------------------------------------------------
DS = (2, 3, 20, 65)        # all hidden degrees 0; odd (the flip has a fixed middle element); the default; past one wave and odd
HS = (3, 64, 130)
NHS = (1, 3)
NBS = (1, 2, 3)            # even and odd flip counts
BS = (1, 3, 70)            # partial row tiles
MS = (1, 2, 3)
# the optional pointers, cycled over the grid: the posteriors (mu0 / lv0, with them rows and grows), dz, the weight gradients, the
# inverse's ladj
NULLS = ((), ("post",), ("dz",), ("wgrad",), ("ladj_inv",), ("dz", "wgrad"))


@dataclass(frozen=True)
class Case:
    name: str
    D: int
    H: int
    nh: int
    nb: int
    B: int
    M: int
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
                        for M in MS:
                            null = NULLS[(i + i // 6 + i // 36) % len(NULLS)]
                            out.append(Case(f"d{D}-h{H}-n{nh}-k{nb}-b{B}-m{M}" + "".join("-null-" + n for n in null), D, H, nh, nb,
                                            B, M, null, 7000 + i))
                            i += 1
    out.append(Case("d512-h128-n3-k2-b3-m1-fwd-inv", 512, 128, 3, 2, 3, 1, (), 7000 + i, backward=False))
    return out


CASES = _cases()
CASE_BY_NAME = {c.name: c for c in CASES}


def layer_shapes(D, H, nh):
    return [(H, D)] + [(H, H)] * (nh - 1) + [(2 * D, H)]


def make_inputs(case):
    """Seeded fp32 inputs.  W[m][blk][l], b[m][blk][l]: U(-g, g) / sqrt(fan_in) with g graded over the flows and blocks; z, y [B,D];
    the posteriors mu0, lv0 [M,B,D]; the upstream gradients grows [M,B], dz0 [M,B,D], dladj [M,B] (None: not given — without the
    posteriors both dz0 and dladj are given, with them grows always and the others in turn)."""
    g = torch.Generator().manual_seed(case.seed)
    D, H, nh, nb, B, M = case.D, case.H, case.nh, case.nb, case.B, case.M
    W, b = [], []
    for m in range(M):
        Wm, bm = [], []
        for blk in range(nb):
            gain = 0.5 + 0.3 * ((m + blk) % 3)
            Wm.append([(2 * torch.rand(s, generator=g) - 1) * gain / math.sqrt(s[1]) for s in layer_shapes(D, H, nh)])
            bm.append([(2 * torch.rand(s[0], generator=g) - 1) * 0.2 for s in layer_shapes(D, H, nh)])
        W.append(Wm)
        b.append(bm)
    z = 1.5 * torch.randn(B, D, generator=g)
    y = 1.5 * torch.randn(B, D, generator=g)
    post = "post" not in case.null
    mu0 = torch.randn(M, B, D, generator=g) if post else None
    lv0 = (-3.0 + 5.0 * torch.rand(M, B, D, generator=g)) if post else None
    i = case.seed
    grows = torch.randn(M, B, generator=g) if post else None
    dz0 = torch.randn(M, B, D, generator=g) if (not post or i % 2 == 0) else None
    dladj = torch.randn(M, B, generator=g) if (not post or i % 3 == 0) else None
    return dict(W=W, b=b, z=z, y=y, mu0=mu0, lv0=lv0, grows=grows, dz0=dz0, dladj=dladj)


# ---- formulas ------------------------------------------------------------------------------------------------------------------------
MUTATIONS = ["no_flip", "flip_first", "exp_plus", "hidden_gt", "out_le", "drop_ladj", "inv_order"]
# (mutation, the stages where it must show, the cases named for it)
TEETH = [
    ("no_flip", ("z0",), ["d3-h64-n1-k1-b3-m2", "d20-h64-n3-k2-b3-m2"]),
    ("flip_first", ("z0", "ladj"), ["d3-h64-n1-k1-b3-m2", "d20-h64-n3-k2-b3-m2"]),
    ("exp_plus", ("z0", "ladj"), ["d20-h64-n3-k2-b3-m2", "d65-h130-n1-k3-b70-m3"]),
    ("hidden_gt", ("z0", "ladj"), ["d2-h3-n1-k1-b3-m2", "d20-h64-n3-k2-b3-m2"]),
    ("out_le", ("z0", "x_inv"), ["d2-h3-n1-k1-b3-m2", "d20-h64-n3-k2-b3-m2"]),
    ("drop_ladj", ("ladj", "rows"), ["d20-h64-n3-k2-b3-m2", "d65-h130-n1-k3-b70-m3"]),
    ("inv_order", ("x_inv",), ["d20-h64-n3-k2-b3-m2", "d65-h130-n1-k3-b70-m3"]),
]


def degrees(D, H):
    return torch.arange(D), torch.arange(H) % (D - 1)


def masks(D, H, nh, mut=()):
    """The nh + 1 masks [out, in] (bool) from the degree formulas."""
    din, dh = degrees(D, H)
    ge = (lambda a, c: a > c) if "hidden_gt" in mut else (lambda a, c: a >= c)
    out = [ge(dh[:, None], din[None, :])] + [ge(dh[:, None], dh[None, :]) for _ in range(nh - 1)]
    last = (dh[None, :] <= din[:, None]) if "out_le" in mut else (dh[None, :] < din[:, None])
    out.append(torch.cat([last, last]))
    return out


def made(Wb, bb, mk, x):
    """One MADE: Wb, bb the nh + 1 weights / biases of the block, mk its masks -> mu, lv."""
    h = x
    for l, (w, bias, m) in enumerate(zip(Wb, bb, mk)):
        h = h @ (w * m.to(w.dtype)).T + bias
        if l < len(Wb) - 1:
            h = torch.relu(h)
    D = x.shape[1]
    return h[:, :D], h[:, D:]


def maf_forward(Wm, bm, x, mut=()):
    """One flow: Wm[blk][l] -> z0 [B,D], ladj [B]."""
    D, H, nh = x.shape[1], Wm[0][0].shape[0], len(Wm[0]) - 1
    mk = masks(D, H, nh, mut)
    ladj = torch.zeros(x.shape[0], dtype=x.dtype)
    for blk, (Wb, bb) in enumerate(zip(Wm, bm)):
        if "flip_first" in mut:
            x = x.flip(1)
        mu, lv = made(Wb, bb, mk, x)
        x = (x - mu) * torch.exp(lv if "exp_plus" in mut else -lv)
        if not ("drop_ladj" in mut and blk == len(Wm) - 1):
            ladj = ladj - lv.sum(-1)
        if "no_flip" not in mut and "flip_first" not in mut:
            x = x.flip(1)
    return x, ladj


def maf_inverse(Wm, bm, y, mut=()):
    """One flow -> x [R,D] with forward(x) = y, ladj [R] (= -forward's)."""
    D, H, nh = y.shape[1], Wm[0][0].shape[0], len(Wm[0]) - 1
    mk = masks(D, H, nh, mut)
    ladj = torch.zeros(y.shape[0], dtype=y.dtype)
    order = range(len(Wm)) if "inv_order" in mut else range(len(Wm) - 1, -1, -1)
    for blk in order:
        y = y.flip(1)
        x = torch.zeros_like(y)
        for i in range(D):
            mu, lv = made(Wm[blk], bm[blk], mk, x)
            x = torch.cat([x[:, :i], (y[:, i] * torch.exp(lv[:, i]) + mu[:, i]).unsqueeze(1), x[:, i + 1:]], dim=1)
            ladj = ladj + lv[:, i]
        y = x
    return y, ladj


def row_term(z0, ladj, mu0, lv0):
    return -((-0.5 * (lv0 + LOG_2PI + (z0 - mu0) ** 2 * torch.exp(-lv0))).sum(-1) + ladj)


def _cast(I, dtype, grad):
    W = [[[w.to(dtype).requires_grad_(grad) for w in Wb] for Wb in Wm] for Wm in I["W"]]
    b = [[[v.to(dtype).requires_grad_(grad) for v in bb] for bb in bm] for bm in I["b"]]
    return W, b


def evaluate(case, I, dtype, mut=(), inverse=True):
    """Forward, autograd backward and inverse (flow 0) in `dtype` on the fp32 inputs -> dict of STAGES (None: not produced).
    dW, db: lists over (flow, block, layer)."""
    grad = case.backward
    W, b = _cast(I, dtype, grad)
    z = I["z"].to(dtype).requires_grad_(grad)
    post = I["mu0"] is not None
    mu0 = I["mu0"].to(dtype).requires_grad_(grad) if post else None
    lv0 = I["lv0"].to(dtype).requires_grad_(grad) if post else None
    z0s, ladjs, rows = [], [], []
    for m in range(case.M):
        z0, ladj = maf_forward(W[m], b[m], z, mut)
        z0s.append(z0)
        ladjs.append(ladj)
        if post:
            rows.append(row_term(z0, ladj, mu0[m], lv0[m]))
    z0, ladj = torch.stack(z0s), torch.stack(ladjs)
    out = dict(z0=z0.detach(), ladj=ladj.detach(), rows=torch.stack(rows).detach() if post else None, dmu0=None, dlv0=None, dz=None,
               dW=None, db=None, x_inv=None, ladj_inv=None, lv_max=0.0)
    if grad:
        total = z0.sum() * 0
        if post:
            total = total + (torch.stack(rows) * I["grows"].to(dtype)).sum()
        if I["dz0"] is not None:
            total = total + (z0 * I["dz0"].to(dtype)).sum()
        if I["dladj"] is not None:
            total = total + (ladj * I["dladj"].to(dtype)).sum()
        flatW = [w for Wm in W for Wb in Wm for w in Wb]
        flatb = [v for bm in b for bb in bm for v in bb]
        gs = torch.autograd.grad(total, [z] + ([mu0, lv0] if post else []) + flatW + flatb, allow_unused=True)
        gs = [torch.zeros_like(t) if g is None else g for g, t in zip(gs, [z] + ([mu0, lv0] if post else []) + flatW + flatb)]
        out["dz"] = gs[0]
        k = 1
        if post:
            out["dmu0"], out["dlv0"] = gs[1], gs[2]
            k = 3
        out["dW"], out["db"] = list(gs[k:k + len(flatW)]), list(gs[k + len(flatW):])
    if inverse:
        with torch.no_grad():
            Wd, bd = _cast(I, dtype, False)
            out["x_inv"], out["ladj_inv"] = maf_inverse(Wd[0], bd[0], I["y"].to(dtype), mut)
    return out


def reference(case, I, mut=()):
    return evaluate(case, I, F64, mut)


def run_torch32(case, I):
    return evaluate(case, I, torch.float32)


# ---- the running error analysis ---------------------------------------------------------------------------------------------------------
def depth(n):
    """The longest chain of additions in a sum of n addends as the kernels take it: a lane's sequential run, the six steps of the
    wave's tree, the bias."""
    return math.ceil(n / 64) + 7


def _made_err(Wb, bb, mk, x, ex):
    """-> out, e_out, [inputs of every layer], [their bounds]."""
    h, eh = x, ex
    acts, errs = [], []
    for l, (w, bias, m) in enumerate(zip(Wb, bb, mk)):
        wm = w * m.to(w.dtype)
        A = wm.abs()
        acts.append(h)
        errs.append(eh)
        pre = h @ wm.T + bias
        epre = eh @ A.T + (depth(w.shape[1]) + 1) * U * (h.abs() @ A.T + bias.abs())
        if l < len(Wb) - 1:
            h, eh = torch.relu(pre), epre
        else:
            h, eh = pre, epre
    return h, eh, acts, errs


def bases(case, I, ref=None):
    """The error model's base of every output (float64, the shapes of `reference`), and the largest |lv| met."""
    ref = reference(case, I) if ref is None else ref
    D, H, nh, nb, B, M = case.D, case.H, case.nh, case.nb, case.B, case.M
    mk = masks(D, H, nh)
    out = {k: None for k in STAGES}
    with torch.no_grad():
        W, b = _cast(I, F64, False)
        z = I["z"].to(F64)
        post = I["mu0"] is not None
        e_z0, e_ladj, e_rows, e_dmu0, e_dlv0, e_dW, e_db = [], [], [], [], [], [], []
        e_dz = torch.zeros(B, D, dtype=F64)
        sum_abs_gx = torch.zeros(B, D, dtype=F64)
        lv_max = 0.0
        for m in range(M):
            x, ex = z, torch.zeros_like(z)
            ladj, eladj = torch.zeros(B, dtype=F64), torch.zeros(B, dtype=F64)
            saved = []
            for blk in range(nb):
                o, eo, acts, errs = _made_err(W[m][blk], b[m][blk], mk, x, ex)
                mu, lv, emu, elv = o[:, :D], o[:, D:], eo[:, :D], eo[:, D:]
                lv_max = max(lv_max, float(lv.abs().max()))
                d = x - mu
                ed = ex + emu + U * d.abs()
                E = torch.exp(-lv)
                eE = E * (elv + U * (1 + lv.abs()))
                u = d * E
                eu = ed * E + d.abs() * eE + U * u.abs()
                ladj = ladj - lv.sum(-1)
                eladj = eladj + elv.sum(-1) + depth(D) * U * lv.abs().sum(-1) + U * ladj.abs()
                saved.append((acts, errs, E, eE, u, eu))
                x, ex = u.flip(1), eu.flip(1)
            e_z0.append(ex)
            e_ladj.append(eladj)
            if post:
                mu0, lv0 = I["mu0"][m].to(F64), I["lv0"][m].to(F64)
                dlt = x - mu0
                edlt = ex + U * dlt.abs()
                e0 = torch.exp(-lv0)
                ee0 = e0 * U * (1 + lv0.abs())
                t2 = dlt * dlt * e0
                et2 = 2 * dlt.abs() * edlt * e0 + dlt * dlt * ee0 + 2 * U * t2
                term = -0.5 * (lv0 + LOG_2PI + t2)
                eterm = 0.5 * (et2 + 2 * U * (lv0.abs() + LOG_2PI + t2))
                e_rows.append(eterm.sum(-1) + depth(D) * U * term.abs().sum(-1) + eladj + U * ref["rows"][m].abs())
            if not case.backward:
                continue
            # backward
            gr = I["grows"][m].to(F64).unsqueeze(1) if post else torch.zeros(B, 1, dtype=F64)
            gx = torch.zeros(B, D, dtype=F64)
            egx = torch.zeros(B, D, dtype=F64)
            if post:
                t1 = dlt * e0
                et1 = edlt * e0 + dlt.abs() * ee0 + U * t1.abs()
                gx = gr * t1
                egx = gr.abs() * et1 + U * gx.abs()
                e_dmu0.append(egx.clone())
                dlv0 = gr * 0.5 * (1 - dlt * t1)
                e_dlv0.append(gr.abs() * 0.5 * (edlt * t1.abs() + dlt.abs() * et1 + U * (1 + (dlt * t1).abs())) + U * dlv0.abs())
            if I["dz0"] is not None:
                gx = gx + I["dz0"][m].to(F64)
                egx = egx + U * gx.abs()
            gl = -gr.squeeze(1) + (I["dladj"][m].to(F64) if I["dladj"] is not None else 0)
            egl = U * gl.abs()
            eWm, ebm = [], []
            for blk in range(nb - 1, -1, -1):
                acts, errs, E, eE, u, eu = saved[blk]
                gu, egu = gx.flip(1), egx.flip(1)
                dx = gu * E
                edx = egu * E + gu.abs() * eE + U * dx.abs()
                dlv = -gu * u - gl.unsqueeze(1)
                edlv = egu * u.abs() + gu.abs() * eu + U * (gu * u).abs() + egl.unsqueeze(1) + U * dlv.abs()
                delta, edelta = torch.cat([-dx, dlv], 1), torch.cat([edx, edlv], 1)
                eWb, ebb = [None] * (nh + 1), [None] * (nh + 1)
                for l in range(nh, -1, -1):
                    w = W[m][blk][l]
                    wm = w * mk[l].to(F64)
                    A = wm.abs()
                    inp, einp = acts[l], errs[l]
                    eWb[l] = (edelta.T @ inp.abs() + delta.abs().T @ einp + (depth(4 * B) + 1) * U * (delta.abs().T @ inp.abs())
                              + TINY) * mk[l].to(F64) + TINY
                    ebb[l] = edelta.sum(0) + (depth(4 * B) + 1) * U * delta.abs().sum(0) + TINY
                    back = delta @ wm
                    eback = edelta @ A + (w.shape[0] + 1) * U * (delta.abs() @ A)  # one thread's sequential run over the outputs
                    if l > 0:
                        on = (inp > 0).to(F64)
                        delta, edelta = back * on, eback * on
                    else:
                        gx = dx + back
                        egx = edx + eback + U * gx.abs()
                eWm.append(eWb)
                ebm.append(ebb)
            e_dW.extend(w for eWb in reversed(eWm) for w in eWb)
            e_db.extend(v for ebb in reversed(ebm) for v in ebb)
            e_dz = e_dz + egx
            sum_abs_gx = sum_abs_gx + gx.abs()
        out["z0"] = torch.stack(e_z0) + TINY
        out["ladj"] = torch.stack(e_ladj) + TINY
        if post:
            out["rows"] = torch.stack(e_rows) + TINY
        if case.backward:
            if post:
                out["dmu0"], out["dlv0"] = torch.stack(e_dmu0) + TINY, torch.stack(e_dlv0) + TINY
            out["dz"] = e_dz + M * U * sum_abs_gx + TINY
            out["dW"], out["db"] = e_dW, e_db
        # inverse of flow 0
        y, ey = I["y"].to(F64), torch.zeros(B, D, dtype=F64)
        ladj, eladj = torch.zeros(B, dtype=F64), torch.zeros(B, dtype=F64)
        for blk in range(nb - 1, -1, -1):
            y, ey = y.flip(1), ey.flip(1)
            x, ex = torch.zeros_like(y), torch.zeros_like(y)
            for i in range(D):
                o, eo, _, _ = _made_err(W[0][blk], b[0][blk], mk, x, ex)
                mu, lv, emu, elv = o[:, i], o[:, D + i], eo[:, i], eo[:, D + i]
                lv_max = max(lv_max, float(lv.abs().max()))
                E = torch.exp(lv)
                xi = y[:, i] * E + mu
                x[:, i] = xi
                ex[:, i] = ey[:, i] * E + y[:, i].abs() * E * (elv + U * (1 + lv.abs())) + emu + U * ((y[:, i] * E).abs() + xi.abs())
                ladj = ladj + lv
                eladj = eladj + elv + U * ladj.abs()
            y, ey = x, ex
        out["x_inv"], out["ladj_inv"] = ey + TINY, eladj + TINY
    out["lv_max"] = lv_max
    assert lv_max <= LV_MAX, f"{case.name}: |lv| reaches {lv_max}: the inputs, not the flow, would overflow exp"
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


# ---- the JNF golden cases: procedural inputs, float64 loss -----------------------------------------------------------------------------
TINY_DIMS = [["m1", [2]], ["m2", [3]], ["m3", [4]]]
JNF_CASES = ["jnf_tiny_stage1", "jnf_tiny_stage2", "jnf_tiny_stage2_beta_rescale", "jnf_mnistsvhn_mlp_stage2"]
CASE_CONFIGS = {
    "jnf_tiny_stage1": dict(dims=TINY_DIMS, L=5, B=6, seed=3401, warmup=2, epoch=2, beta=1.0, dists=None, rescaling=False,
                            scale=None),
    "jnf_tiny_stage2": dict(dims=TINY_DIMS, L=5, B=6, seed=3402, warmup=2, epoch=3, beta=1.0, dists=None, rescaling=False,
                            scale=None),
    "jnf_tiny_stage2_beta_rescale": dict(dims=TINY_DIMS, L=5, B=5, seed=3403, warmup=2, epoch=3, beta=2.5,
                                         dists=dict(m1="normal", m2="laplace", m3="bernoulli"), rescaling=True, scale=0.75),
    "jnf_mnistsvhn_mlp_stage2": dict(dims=[["mnist", [1, 28, 28]], ["svhn", [3, 32, 32]]], L=20, B=8, seed=3404, warmup=2,
                                     epoch=3, beta=1.0, dists=None, rescaling=False, scale=None),
}
FOLDER = "jnf_reference_folder"
FOLDER_CONFIG = dict(dims=TINY_DIMS, L=3, warmup=4, beta=0.5)
FLOW_GAIN = 1.0  # the flows' procedural weights: U(-1, 1) / sqrt(fan_in)


def case_dims(cfg):
    return OrderedDict((m, tuple(d)) for m, d in cfg["dims"])


def case_dists(cfg):
    return {m: (cfg["dists"] or {}).get(m, "normal") for m, _ in cfg["dims"]}


def config_kwargs(cfg):
    """Keyword arguments of JNFConfig (this package's and the reference's) for a golden case."""
    dims = case_dims(cfg)
    kw = dict(n_modalities=len(dims), latent_dim=cfg["L"], input_dims=dict(dims), warmup=cfg["warmup"], beta=cfg["beta"],
              uses_likelihood_rescaling=cfg["rescaling"])
    if cfg["dists"]:
        kw["decoders_dist"] = dict(cfg["dists"])
    if cfg["scale"] is not None:
        kw["decoder_dist_params"] = {m: {"scale": cfg["scale"]} for m, d in case_dists(cfg).items() if d in ("normal", "laplace")}
    return kw


def case_inputs(cfg):
    """-> dims, data {m: np [B, *dim]} (procedural, bit-exact)."""
    dims = case_dims(cfg)
    dists = case_dists(cfg)
    data = {m: P.uniform((cfg["B"],) + d, cfg["seed"] + i) for i, (m, d) in enumerate(dims.items())}
    for m in dims:
        if dists[m] == "bernoulli":
            data[m] = (data[m] > 0.5).astype(np.float32)
    return dims, data


def flow_shapes(names, L, n_blocks=2, n_hidden=3, H=128):
    """The default MAF of every modality, parameters only, in state-dict order (the `mask` buffers are not parameters)."""
    s = OrderedDict()
    for m in names:
        for blk in range(n_blocks):
            for l, shape in enumerate(layer_shapes(L, H, n_hidden)):
                s[f"flows.{m}.net.{blk}.net.{2 * l}.weight"] = shape
                s[f"flows.{m}.net.{blk}.net.{2 * l}.bias"] = (shape[0],)
    return s


def case_state_dict(cfg):
    """The procedural parameters: default MLP encoders / decoders, MultipleHeadJointEncoder (the layout of JMVAE), default flows."""
    dims = case_dims(cfg)
    sd = P.make_state_dict(P.jmvae_mlp_shapes(dims, cfg["L"]), cfg["seed"])
    sd.update(P.make_state_dict(flow_shapes(list(dims), cfg["L"]), cfg["seed"] + 500, gain=FLOW_GAIN))
    return sd


def rescale_factors(cfg):
    dims = case_dims(cfg)
    if not cfg["rescaling"]:
        return {m: 1.0 for m in dims}
    mx = max(int(np.prod(d)) for d in dims.values())
    return {m: mx / int(np.prod(d)) for m, d in dims.items()}


def flow_params(sd, m):
    """-> W[blk][l], b[blk][l] of modality m's flow from a state dict."""
    W, b, blk = [], [], 0
    while f"flows.{m}.net.{blk}.net.0.weight" in sd:
        Wb, bb, l = [], [], 0
        while f"flows.{m}.net.{blk}.net.{2 * l}.weight" in sd:
            Wb.append(sd[f"flows.{m}.net.{blk}.net.{2 * l}.weight"])
            bb.append(sd[f"flows.{m}.net.{blk}.net.{2 * l}.bias"])
            l += 1
        W.append(Wb)
        b.append(bb)
        blk += 1
    return W, b


def jnf_loss(cfg, sd, data, eps):
    """sd: name -> tensor; data {m: tensor}; eps [B,L]: the joint posterior's draw -> the ModelOutput's entries as a dict."""
    names = [m for m, _ in cfg["dims"]]
    dists = case_dists(cfg)
    scale = 1.0 if cfg["scale"] is None else cfg["scale"]
    resc = rescale_factors(cfg)
    jmu, jlv = joint_encoder(sd, "joint_encoder.", data, names)
    B = jmu.shape[0]
    z = jmu + torch.exp(0.5 * jlv) * eps
    recon = sum(resc[m] * nll_rows(dists[m], mlp_decoder(sd, f"decoders.{m}.", z), data[m], scale).sum() for m in names)
    kld = -0.5 * torch.sum(1 + jlv - jmu.pow(2) - jlv.exp()) * cfg["beta"]
    if cfg["epoch"] <= cfg["warmup"]:
        return dict(loss=(recon + kld) / B, loss_sum=recon + kld, metrics=dict(kld_prior=kld, recon_loss=recon / B, ljm=0))
    z = z.detach()
    ljm = 0
    for m in names:
        mu0, lv0 = mlp_encoder(sd, f"encoders.{m}.", data[m])
        W, b = flow_params(sd, m)
        z0, ladj = maf_forward(W, b, z)
        ljm = ljm + row_term(z0, ladj, mu0, lv0).sum()
    return dict(loss=ljm / B, loss_sum=ljm, metrics=dict(kld_prior=kld.detach(), recon_loss=recon.detach() / B, ljm=ljm / B))


def case_tensors(cfg, arrays, dtype=F64):
    _, data = case_inputs(cfg)
    return {m: torch.from_numpy(v).to(dtype) for m, v in data.items()}, torch.from_numpy(arrays["eps"]).to(dtype)


def reference_grads(cfg, arrays):
    """-> (result dict, {name: float64 gradient or None}) of the float64 loss at the golden case's recorded draw.  In stage one the
    unimodal encoders and the flows take no part; in stage two the joint encoder and the decoders are frozen."""
    sd = {k: torch.from_numpy(v).double() for k, v in case_state_dict(cfg).items()}
    stage2 = cfg["epoch"] > cfg["warmup"]
    for k, v in sd.items():
        v.requires_grad_(k.startswith(("encoders.", "flows.")) if stage2 else True)
    data, eps = case_tensors(cfg, arrays)
    out = jnf_loss(cfg, sd, data, eps)
    out["loss"].backward()
    return out, {k: v.grad for k, v in sd.items()}


# ---- the sampler of a subset's product of experts ------------------------------------------------------------------------------------------
def poe_logdensity(flows, post, z, divide_prior=True, grad=True):
    """flows: [(W, b)] of the subset, post: [(mu0, lv0)] -> ln q [n] (and its gradient [n,L]) at z, in z's dtype."""
    with torch.enable_grad():
        zz = z.detach().clone().requires_grad_(True)
        ln = 0
        if divide_prior:
            ln = ln + (0.5 * (zz ** 2 + LOG_2PI)).sum(1)
        for (W, b), (mu0, lv0) in zip(flows, post):
            z0, ladj = maf_forward(W, b, zz)
            ln = ln - row_term(z0, ladj, mu0, lv0)
        if not grad:
            return ln.detach()
        return ln.detach(), torch.autograd.grad(ln.sum(), zz)[0]


def hmc(flows, post, start_mod, start_noise, gamma, acc, n_lf, eps_lf, divide_prior=True):
    """The reference's sampler on given draws: start_mod [n] (index of the expert a chain starts from), start_noise [n,L], gamma
    [steps,n,L], acc [steps,n] -> z [n,L], min |acc - alpha| over every decision (the margin no decision may fall below), the number of accepted moves."""
    dtype = start_noise.dtype
    z0 = torch.zeros_like(start_noise)
    for i, (mu0, lv0) in enumerate(post):
        z0 = torch.where((start_mod == i).unsqueeze(1), mu0 + torch.exp(0.5 * lv0) * start_noise, z0)
    z = z0
    margin, accepted = math.inf, 0
    for s in range(gamma.shape[0]):
        rho = gamma[s].to(dtype)
        ln, g = poe_logdensity(flows, post, z, divide_prior)
        H0 = -ln + 0.5 * (rho ** 2).sum(1)
        for _ in range(n_lf):
            rho_ = rho + (eps_lf / 2) * g
            z = z + eps_lf * rho_
            ln, g = poe_logdensity(flows, post, z, divide_prior)
            rho = rho_ + (eps_lf / 2) * g
        H = -ln + 0.5 * (rho ** 2).sum(1)
        alpha = torch.exp(H0 - H)
        u = acc[s].to(dtype)
        margin = min(margin, float((u - alpha).abs().min()))
        accepted += int((u < alpha).sum())
        z = torch.where((u < alpha).unsqueeze(1), z, z0)
        z0 = z
    return z, margin, accepted


# the sampler's test: the tiny stage-two model, a two-modality subset, two chains per data point, given draws.  eps_lf is large (the
# default 0.01 accepts everything): with this seed the float64 sampler both accepts and rejects, and every |u - alpha| exceeds
# HMC_MARGIN, far more than three steps of fp32 drift — no decision can flip (tests/test_jnf_host.py::test_hmc_oracle_condition).
HMC = dict(case="jnf_tiny_stage2", subset=["m1", "m3"], n_data=4, K=2, mcmc_steps=3, n_lf=2, eps_lf=0.5, seed=1)
HMC_MARGIN = 1e-3
C_HMC = 1.0  # 4x what the sampler in torch fp32 shows against float64 in units of hmc_base, rounded up (test_hmc_oracle_condition)


def hmc_draws():
    """-> data {m: fp32 [n_data, *dim]}, start_mod [n] int64, start_noise [n,L], gamma [steps,n,L], acc [steps,n] (fp32, seeded)."""
    cfg = CASE_CONFIGS[HMC["case"]]
    dims = case_dims(cfg)
    data = {m: torch.from_numpy(P.uniform((HMC["n_data"],) + d, 9100 + i)) for i, (m, d) in enumerate(dims.items())}
    g = torch.Generator().manual_seed(HMC["seed"])
    n, L, S = HMC["n_data"] * HMC["K"], cfg["L"], HMC["mcmc_steps"]
    return (data, torch.randint(0, len(HMC["subset"]), (n,), generator=g), torch.randn(n, L, generator=g),
            torch.randn(S, n, L, generator=g), torch.rand(S, n, generator=g))


def hmc_setup(dtype):
    """-> flows [(W, b)], post [(mu0, lv0)] (rows K-major: the data repeated K times), draws, in `dtype`."""
    cfg = CASE_CONFIGS[HMC["case"]]
    sd = {k: torch.from_numpy(v).to(dtype) for k, v in case_state_dict(cfg).items()}
    data, start_mod, start_noise, gamma, acc = hmc_draws()
    flows = [flow_params(sd, m) for m in HMC["subset"]]
    post = [tuple(torch.cat([t] * HMC["K"]) for t in mlp_encoder(sd, f"encoders.{m}.", data[m].to(dtype))) for m in HMC["subset"]]
    return flows, post, (start_mod, start_noise.to(dtype), gamma.to(dtype), acc.to(dtype))


def hmc_run(dtype):
    """-> z [n,L], the smallest |u - alpha| over every decision, the number of accepted moves."""
    flows, post, (start_mod, start_noise, gamma, acc) = hmc_setup(dtype)
    with torch.no_grad():
        return hmc(flows, post, start_mod, start_noise, gamma, acc, HMC["n_lf"], HMC["eps_lf"])


def hmc_base(z_ref):
    """u times the number of density evaluations times (1 + |z|): the scale fp32 drift is measured in."""
    return U * HMC["mcmc_steps"] * (HMC["n_lf"] + 1) * (1 + z_ref.abs().to(F64))
