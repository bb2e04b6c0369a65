"""float64 references of the small-channel 4x4 / stride-2 / pad-1 layers (csrc/smallconv.hip, csrc/smallcin.hip).

For every operation: the float64 reference (F.conv2d / F.conv_transpose2d, float64 autograd for the backward), the bound of the
same formula on absolute values (bound = sum |a b| + |bias|, what C_ENTRY multiplies) and two DEGRADED emulations in float64 that
a per-entry check must reject:

  two_piece   both operands rounded to hi + mid of a bf16 split (16 of 24 significant bits: the split engine without its third
              piece; `two_piece` of tests/test_gpu_gemm_dispatch.py);
  f16_drop    both operands as scaled fp16 pairs (csrc/bf3.hpp: x s = hi + lo / 2048) and the product with one cross term
              dropped: hi hi' + hi lo' / 2048 only.  Defined for the products (every operation here is bilinear in its two
              operands), not for the plain sums (db, which has one operand).

Every operation is written as a bilinear map op(a, b) of two tensors, so the bound and both emulations come from ONE statement
of the formula: bound = op(|a|, |b|), two_piece = op(tp(a), tp(b)), f16_drop = (op(hi, hi') + op(hi, lo') / 2048) / (s s').

Operations: the up layer's pre-activation (ConvTranspose2d(Cv, Cu, 4, 2, 1)), the NLL rows and dpre of its fused Normal tail
(models/base/base_utils.py:62-87), its backward (dV with the fused activation mask of V, dW, db, the channel sums of dV), the down
layer (Conv2d(Cu, Cv, 4, 2, 1)) and its weight gradient (smallcin, also slab by slab).
"""
import math

import torch
import torch.nn.functional as F

NONE, RELU, SIGMOID, LEAKY = 0, 1, 2, 3
F02 = float(torch.tensor(0.2, dtype=torch.float32))  # the kernels' 0.2f
C_ENTRY = 5e-7  # tests/test_gpu_gemm_dispatch.py: per-entry constant of a <= 1024-term fp32 chain


def g(seed):
    return torch.Generator().manual_seed(seed)


# ---- degraded operands ---------------------------------------------------------------------------------------------------
def two_piece(x):
    hi = x.float().bfloat16()
    mid = (x.float() - hi.float()).bfloat16()
    return hi.double() + mid.double()


def f16_pair(x):
    """(hi, lo, s) of bf3.hpp's scaled pair in float64: s = the power of two with max|x| s in [2^13, 2^14), hi = fp16(x s),
    lo = fp16((x s - hi) 2048)."""
    amax = float(x.abs().max())
    s = 2.0 ** (14 - math.frexp(amax)[1]) if amax > 0 else 1.0
    xs = x.float() * s  # exact: a power of two
    hi = xs.half()
    lo = ((xs - hi.float()) * 2048.0).half()
    return hi.double(), lo.double(), s


def degraded(op, a, b, want_h=True):
    """(two_piece, f16_drop) of the bilinear op(a, b); want_h = False leaves f16_drop out (None)."""
    if not want_h:
        return op(two_piece(a), two_piece(b)), None
    ha, _, sa = f16_pair(a)
    hb, lb, sb = f16_pair(b)
    return op(two_piece(a), two_piece(b)), (op(ha, hb) + op(ha, lb) / 2048.0) / (sa * sb)


# ---- activations -----------------------------------------------------------------------------------------------------------
def act64(v, act):
    if act == RELU:
        return v.clamp_min(0)
    if act == SIGMOID:
        return torch.sigmoid(v)
    if act == LEAKY:
        return torch.where(v > 0, v, F02 * v)
    return v


def actgrad64(y, act):
    """act'(pre) from the stored fp32 output y (mvk_act_grad_from_out; the sigmoid's y (1 - y) is an fp32 product)."""
    if act == RELU:
        return (y > 0).double()
    if act == LEAKY:
        return torch.where(y > 0, torch.ones_like(y, dtype=torch.float64), torch.full_like(y, F02, dtype=torch.float64))
    if act == SIGMOID:
        return (y.float() * (1 - y.float())).double()
    return torch.ones_like(y, dtype=torch.float64)


def stored(pre, act):
    """A stored fp32 activation output with the sign pattern / range of act(pre)."""
    return act64(pre.double(), act).float()


# ---- the bilinear maps -----------------------------------------------------------------------------------------------------
def op_up(V, W):
    """ConvTranspose2d(Cv, Cu, 4, 2, 1) without bias: V [n][Cv][h][w], W [Cv][Cu][4][4] -> [n][Cu][2h][2w]."""
    return F.conv_transpose2d(V, W, None, stride=2, padding=1)


def op_down(U, W):
    """Conv2d(Cu, Cv, 4, 2, 1) without bias: U [n][Cu][2h][2w], W [Cv][Cu][4][4] -> [n][Cv][h][w]."""
    return F.conv2d(U, W, None, stride=2, padding=1)


def op_wgrad(U, dV):
    """d/dW of sum(op_down(U, W) * dV): [Cv][Cu][4][4]."""
    return torch.nn.grad.conv2d_weight(U, (dV.shape[1], U.shape[1], 4, 4), dV, stride=2, padding=1)


class Ref:
    """One output: float64 reference, bound and the degraded emulations (deg_h is None where f16_drop is not defined)."""

    def __init__(self, ref, bound, deg2, degh=None):
        self.ref, self.bound, self.deg2, self.degh = ref, bound, deg2, degh

    def map(self, f):
        return Ref(f(self.ref), f(self.bound), f(self.deg2), None if self.degh is None else f(self.degh))

    def ratios(self, tol=None):
        """Worst |deg - ref| / tol of each emulation (tol: C_ENTRY * bound by default)."""
        tol = C_ENTRY * self.bound + 1e-30 if tol is None else tol
        r2 = float(((self.deg2 - self.ref).abs() / tol).max())
        rh = None if self.degh is None else float(((self.degh - self.ref).abs() / tol).max())
        return r2, rh


def bilinear(op, a, b, bias=None, bias_dim=1, want_h=True):
    """Ref of op(a, b) + bias (bias broadcast along bias_dim)."""
    a64, b64 = a.double(), b.double()
    ref, bound = op(a64, b64), op(a64.abs(), b64.abs())
    d2, dh = degraded(op, a, b, want_h)
    if bias is not None:
        shape = [1] * ref.dim()
        shape[bias_dim] = -1
        bb = bias.double().view(shape)
        ref, bound, d2, dh = ref + bb, bound + bb.abs(), d2 + bb, None if dh is None else dh + bb
    return Ref(ref, bound, d2, dh)


# ---- operands ----------------------------------------------------------------------------------------------------------------
def up_operands(seed, n, h, w, Cu, Cv, bias=True):
    """V with every image on its own scale (0.25 .. 4.25), W with every output channel on its own scale."""
    gn = g(seed)
    V = torch.randn(n, Cv, h, w, generator=gn) * (torch.rand(n, 1, 1, 1, generator=gn) * 4 + 0.25)
    W = torch.randn(Cv, Cu, 4, 4, generator=gn) * (torch.rand(1, Cu, 1, 1, generator=gn) + 0.5) / math.sqrt(4 * Cv)
    b = torch.randn(Cu, generator=gn) if bias else None
    return V, W, b


def down_operands(seed, n, h, w, Cu, Cv, bias=True):
    gn = g(seed)
    U = torch.randn(n, Cu, 2 * h, 2 * w, generator=gn) * (torch.rand(n, 1, 1, 1, generator=gn) * 4 + 0.25)
    W = torch.randn(Cv, Cu, 4, 4, generator=gn) * (torch.rand(Cv, 1, 1, 1, generator=gn) + 0.5) / math.sqrt(16 * Cu)
    b = torch.randn(Cv, generator=gn) if bias else None
    return U, W, b


def bwd_operands(seed, n, h, w, Cu, Cv, u_act, v_act):
    """dU (per-image scales), the stored outputs Uout = u_act(.) and V = v_act(.), W, and the initial content of dW, db, db_v."""
    gn = g(seed)
    dU = torch.randn(n, Cu, 2 * h, 2 * w, generator=gn) * (torch.rand(n, 1, 1, 1, generator=gn) * 4 + 0.25)
    Uout = stored(torch.randn(n, Cu, 2 * h, 2 * w, generator=gn), u_act)
    V = stored(torch.randn(n, Cv, h, w, generator=gn) * (torch.rand(1, Cv, 1, 1, generator=gn) + 0.5), v_act)
    W = torch.randn(Cv, Cu, 4, 4, generator=gn) * (torch.rand(1, Cu, 1, 1, generator=gn) + 0.5) / math.sqrt(4 * Cv)
    init = (torch.randn(Cv, Cu, 4, 4, generator=gn), torch.randn(Cu, generator=gn), torch.randn(Cv, generator=gn))
    return dU, Uout, V, W, init


def wgrad_operands(seed, n, h, w, Cu, Cv):
    gn = g(seed)
    U = torch.randn(n, Cu, 2 * h, 2 * w, generator=gn) * (torch.rand(n, 1, 1, 1, generator=gn) * 4 + 0.25)
    dV = torch.randn(n, Cv, h, w, generator=gn) * (torch.rand(1, Cv, 1, 1, generator=gn) + 0.5) / math.sqrt(n * h * w)
    init = torch.randn(Cv, Cu, 4, 4, generator=gn)
    return U, dV, init


# ---- the operations ------------------------------------------------------------------------------------------------------------
def up_pre(V, W, b):
    """Pre-activation of the up layer, NCHW."""
    return bilinear(op_up, V, W, b)


def down_pre(U, W, b):
    """Pre-activation of the down layer, NCHW [n][Cv][h][w]."""
    return bilinear(op_down, U, W, b)


def up_bwd(dU, Uout, u_act, V, v_act, W):
    """dict(dV, dW, db, dbv) of the up layer's backward: dpre = dU u_act'(Uout); dV = op_down(dpre, W) v_act'(V) (NCHW),
    dW = op_wgrad(dpre, V), db = sums of dpre, dbv = channel sums of dV.  dpre is exact here (float64); the kernels' one fp32
    rounding of it is part of the error they are held to."""
    dpre = dU.double() * actgrad64(Uout, u_act)
    vm = actgrad64(V, v_act)
    dV = bilinear(op_down, dpre, W).map(lambda t: t * vm)
    dW = bilinear(op_wgrad, dpre, V)
    s = lambda t: t.sum((0, 2, 3))  # noqa: E731
    db = Ref(s(dpre), s(dpre.abs()), s(two_piece(dpre)))
    return dict(dV=dV, dW=dW, db=db, dbv=dV.map(s))


def up_bwd_autograd(dU, Uout, u_act, V, v_act, W):
    """The same four tensors from float64 autograd of conv_transpose2d (dpre as the output gradient; the mask of V applied
    afterwards, as the consumer of dV would)."""
    dpre = dU.double() * actgrad64(Uout, u_act)
    Vr, Wr = V.double().requires_grad_(), W.double().requires_grad_()
    br = torch.zeros(W.shape[1], dtype=torch.float64, requires_grad=True)
    F.conv_transpose2d(Vr, Wr, br, stride=2, padding=1).backward(dpre)
    dV = Vr.grad * actgrad64(V, v_act)
    return dict(dV=dV, dW=Wr.grad, db=br.grad, dbv=dV.sum((0, 2, 3)))


def down_wgrad(U, dV):
    """dW [Cv][Cu][4][4] of the down layer (the smallcin weight gradient)."""
    return bilinear(op_wgrad, U, dV)


def down_wgrad_autograd(U, dV):
    Wr = torch.zeros(dV.shape[1], U.shape[1], 4, 4, dtype=torch.float64, requires_grad=True)
    (F.conv2d(U.double(), Wr, None, stride=2, padding=1) * dV.double()).sum().backward()
    return Wr.grad


def wgrad_blocks(U, dV, ppb, want_h=True):
    """The per-workgroup slabs of smallcin_wgrad_kernel: slab[b][(tap Cu + cu)][cv] = the weight gradient summed over the positions
    [b ppb, (b + 1) ppb) of the flat (image, row, column) order only.  Ref of shape [blocks][16 Cu][Cv]."""
    n, Cu = U.shape[:2]
    Cv, npos = dV.shape[1], dV.shape[0] * dV.shape[2] * dV.shape[3]
    nb = -(-npos // ppb)

    def op(a, b):
        cols = F.unfold(a, 4, padding=1, stride=2).transpose(1, 2).reshape(npos, Cu, 16).transpose(1, 2).reshape(npos, 16 * Cu)
        rows = b.permute(0, 2, 3, 1).reshape(npos, Cv)
        pad = nb * ppb - npos
        if pad:
            cols, rows = F.pad(cols, (0, 0, 0, pad)), F.pad(rows, (0, 0, 0, pad))
        return torch.bmm(cols.view(nb, ppb, 16 * Cu).transpose(1, 2), rows.view(nb, ppb, Cv))

    return bilinear(op, U, dV, want_h=want_h)


def slabs_to_ref_layout(s, Cu, Cv):
    """sum over blocks of [blocks][(tap Cu + cu)][cv] -> [Cv][Cu][4][4]."""
    return s.sum(0).view(16, Cu, Cv).permute(2, 1, 0).reshape(Cv, Cu, 4, 4)


# ---- the fused Normal-NLL tail of the 16x16x32 -> 3 layer (models/base/base_utils.py:62-87) -------------------------------------
def ulp32(x):
    """fp32 spacing at |x| (x in float64)."""
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126))) - 23)


def nll_tail(pre, X, xrows, scale, gw, sig_ulps):
    """From a Ref of the pre-activation [n][Cu][H][W]: Refs of rows[n] = sum_d (r - x)^2 / (2 s^2) + D (log s + 1/2 log 2 pi) and
    dpre = gw (r - x) / s^2 r (1 - r), r = sigmoid(pre), image i scored against X[i % xrows].

    rows bound: sum of |terms| (C_ENTRY of it is the tolerance the check uses).
    dpre tolerance (returned as bound = tolerance / C_ENTRY): the pre-activation's C_ENTRY * bound carried to first order through
    the float64 derivative d dpre / d pre, + the sigmoid allowance (sig_ulps ulps of r) through d dpre / d r, + 8 x 2^-24 |dpre|
    for the eight fp32 roundings between the arguments and the stored value, each a relative 2^-24 of the product: on the host
    s s, 1 / (s s), (1 / s^2) gw (launch_fwd), in the kernel r - x, 1 - r, r (1 - r), (r - x) g and the final product.  Where
    d dpre / d r = 0 (r (1 - r) = (x - r)(1 - 2 r)) the first two terms vanish and this one is the whole tolerance.  gw and scale
    are the fp32 values the entry point receives."""
    n = pre.ref.shape[0]
    x = X.double()[torch.arange(n) % xrows]
    D_ = pre.ref[0].numel()
    const = D_ * (math.log(scale) + 0.5 * math.log(2 * math.pi))
    k = gw / (scale * scale)

    def rows_of(p):
        r = torch.sigmoid(p)
        return ((r - x) ** 2).flatten(1).sum(1) / (2 * scale * scale) + const

    def dpre_of(p):
        r = torch.sigmoid(p)
        return k * (r - x) * r * (1 - r)

    r = torch.sigmoid(pre.ref)
    s1 = r * (1 - r)
    dfdr = k * (s1 + (r - x) * (1 - 2 * r))        # d dpre / d r
    dfdp = dfdr * s1                               # d dpre / d pre
    rows = Ref(rows_of(pre.ref), rows_of(pre.ref) - const + abs(const), rows_of(pre.deg2),
               None if pre.degh is None else rows_of(pre.degh))
    tol = dfdp.abs() * C_ENTRY * pre.bound + dfdr.abs() * sig_ulps * ulp32(r) + 8 * 2.0 ** -24 * dpre_of(pre.ref).abs()
    dpre = Ref(dpre_of(pre.ref), tol / C_ENTRY, dpre_of(pre.deg2), None if pre.degh is None else dpre_of(pre.degh))
    dpre.derived = True  # its bound is a propagated tolerance, not a sum of |terms|
    return rows, dpre


def sigmoid_ulps(pre32, ref=None):
    """Largest error of torch.sigmoid in fp32 on `pre32` (on its device) in ulps of the float64 sigmoid."""
    ref = torch.sigmoid(pre32.double()) if ref is None else ref
    return float(((torch.sigmoid(pre32).double() - ref).abs() / ulp32(ref)).max())
