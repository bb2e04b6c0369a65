"""float64 references of the 3x3 / stride-1 / pad-1 layers (csrc/conv3small.hip, csrc/conv3rs.hip, the tw = 3 routes of
csrc/igemm.hip), and the host arithmetic of the register-stationary kernels' position stream restated in Python.

Every operation is ONE bilinear map op(a, b), so the float64 reference op(a, b), the bound op(|a|, |b|) that C_ENTRY multiplies and
both degraded emulations (tests/conv_small_ref.py: two_piece = both operands on two bf16 pieces, f16_drop = scaled fp16 pairs with
one cross term dropped) come from one statement of the formula:

  op_conv3(x, w)   = F.conv2d(x, w, None, 1, 1)                       x [n][Cin][H][W], w [Cout][Cin][3][3]
  op_wgrad3(x, dy) = torch.nn.grad.conv2d_weight(x, w.shape, dy)      d/dw of sum(op_conv3(x, w) dy)
  the bias gradient: a plain sum of dy over (image, row, column).

The epilogues are derived from these, none has a constant of its own (forward / c3wg):

  input activation  x > 0 ? x : x * 0.2f (0.f for ReLU) in fp32, exactly what the kernels stage: the operand of op is the fp32 result
  pre_scale         multiplies the convolution sum: reference and bound scale with it
  bias              + b, bound + |b|
  res_pre           act(v + res): checked at act = none: reference + res, bound + |res|
  mask              x act'(stored fp32 source) (conv_small_ref.actgrad64)
  column sums       the sum over positions of the reference; tolerance C_ENTRY (sum_p bound + sum_p |ref|): the rounding of every
                    stored entry plus the fp32 sum of the stored entries
  residual          res + alpha v: tolerance C_ENTRY (|res| + |alpha| bound)
  scaled fp16       + the floor of csrc/bf3.hpp: 2^-39 of the two operand BOUNDS per product, times the products of an entry
  dy_scale, x_act   of the weight gradient: the same statements on op_wgrad3.
"""
import math

import torch
import torch.nn.functional as F

from conv_small_ref import C_ENTRY, F02, LEAKY, NONE, RELU, SIGMOID, Ref, actgrad64, bilinear, g, two_piece  # noqa: F401

FLOOR = 2.0 ** -39  # csrc/bf3.hpp: absolute error of a scaled fp16 pair below 2^-28 of its tensor's bound, per unit of that bound


# ---- the bilinear maps ---------------------------------------------------------------------------------------------------
def op_conv3(x, w):
    return F.conv2d(x, w, None, 1, 1)


def op_wgrad3(x, dy):
    return torch.nn.grad.conv2d_weight(x, (dy.shape[1], x.shape[1], 3, 3), dy, stride=1, padding=1)


def pack_fwd(w):
    """The forward GEMM operand of mvk_conv3x3: Wp[(kh 3 + kw) Cin + ci][co] = w[co][ci][kh][kw] (a permutation: exact)."""
    return w.permute(2, 3, 1, 0).reshape(9 * w.shape[1], w.shape[0]).contiguous()


def in_act32(x, act):
    """The activation of the layer that produced x as the kernels apply it while staging: fp32, x > 0 ? x : x * slope."""
    if act == NONE:
        return x.float()
    slope = torch.tensor(0.2 if act == LEAKY else 0.0, dtype=torch.float32)
    assert act in (LEAKY, RELU)
    return torch.where(x.float() > 0, x.float(), x.float() * slope)


# ---- operands --------------------------------------------------------------------------------------------------------------
def fwd_operands(seed, n, H, W, Cin, Cout, spread=0.0, tiny=False, chan=0.0):
    """x with every image on its own scale (0.25 .. 4.25), w with every output channel on its own scale, bias, mask source,
    residual, the initial content of a column-sum accumulator.  spread: images and weight rows over e^(+- spread sigma).
    tiny: one image and one weight row 2^-30 of the others (below the fp16 pair's full-precision range).  chan: the input channels
    over e^(+- chan sigma): a few channels carry most of every sum.  (The rounding of 16-bit operands averages out over a 2304-term
    sum of equal-sized terms: on unit data the two-piece emulation stays at 0.7x the tolerance there.  The chain the kernel adds
    up is as long as before.)"""
    gn = g(seed)
    x = torch.randn(n, Cin, H, W, generator=gn) * (torch.rand(n, 1, 1, 1, generator=gn) * 4 + 0.25)
    w = torch.randn(Cout, Cin, 3, 3, generator=gn) * (torch.rand(Cout, 1, 1, 1, generator=gn) + 0.5) / math.sqrt(9 * Cin)
    if spread:
        x = x * torch.exp(spread * torch.randn(n, 1, 1, 1, generator=gn))
        w = w * torch.exp(spread * torch.randn(Cout, 1, 1, 1, generator=gn))
    if chan:
        x = x * torch.exp(chan * torch.randn(1, Cin, 1, 1, generator=gn))
    if tiny:
        x[0, :, :, W // 2:] *= 2.0 ** -30
        w[Cout // 2] *= 2.0 ** -30
    b = torch.randn(Cout, generator=gn)
    src = torch.randn(n, Cout, H, W, generator=gn)
    res = torch.randn(n, Cout, H, W, generator=gn) * (torch.rand(n, 1, 1, 1, generator=gn) * 4 + 0.25)
    cinit = torch.randn(Cout, generator=gn)
    return x, w, b, src, res, cinit


def wgrad_operands(seed, n, H, W, Cin, Cout, spread=0.0):
    gn = g(seed)
    x = torch.randn(n, Cin, H, W, generator=gn) * (torch.rand(n, 1, 1, 1, generator=gn) * 4 + 0.25)
    dy = torch.randn(n, Cout, H, W, generator=gn) * (torch.rand(1, Cout, 1, 1, generator=gn) + 0.5) / math.sqrt(n * H * W)
    if spread:
        x = x * torch.exp(spread * torch.randn(n, 1, 1, 1, generator=gn))
        dy = dy * torch.exp(spread * torch.randn(n, 1, 1, 1, generator=gn))
    init = torch.randn(Cout, Cin, 3, 3, generator=gn)
    binit = torch.randn(Cout, generator=gn)
    return x, dy, init, binit


# ---- the operations ----------------------------------------------------------------------------------------------------------
def _affine(r, mul=None, add=None):
    """Ref of mul * r + add (mul, add: float64 tensors or numbers; the bound takes their absolute values)."""
    ref, bound, d2, dh = r.ref, r.bound, r.deg2, r.degh
    if mul is not None:
        am = mul.abs() if isinstance(mul, torch.Tensor) else abs(mul)
        ref, bound, d2, dh = ref * mul, bound * am, d2 * mul, None if dh is None else dh * mul
    if add is not None:
        ref, bound, d2, dh = ref + add, bound + add.abs(), d2 + add, None if dh is None else dh + add
    return Ref(ref, bound, d2, dh)


def conv3_fwd(x, w, bias=None, x_act=NONE, pre_scale=1.0, mask_src=None, mask_act=NONE, res=None, res_alpha=1.0, res_pre=False,
              colsum=False, floor_bounds=None, want_h=True):
    """dict(y=Ref [n][Cout][H][W], a=Ref of the value before the residual sum, colsum=Ref [Cout] or None) of

        a = (pre_scale conv3(x_act(x), w) + bias [+ res if res_pre]) * mask_act'(mask_src);   y = a, or res + res_alpha a.

    floor_bounds = (bound of |x|, bound of |w|) of a scaled-fp16 launch: the tolerance gains 2^-39 xb wb |pre_scale| 9 Cin."""
    xa = in_act32(x, x_act)
    r = bilinear(op_conv3, xa, w, want_h=want_h)
    ps = float(torch.tensor(pre_scale, dtype=torch.float32))
    if ps != 1.0:
        r = _affine(r, mul=ps)
    if floor_bounds is not None:
        fl = FLOOR * floor_bounds[0] * floor_bounds[1] * abs(ps) * 9 * x.shape[1]
        r = Ref(r.ref, r.bound + fl / C_ENTRY, r.deg2, r.degh)
    if bias is not None:
        r = _affine(r, add=bias.double().view(1, -1, 1, 1))
    if res is not None and res_pre:
        r = _affine(r, add=res.double())
    if mask_src is not None:
        r = _affine(r, mul=actgrad64(mask_src, mask_act))
    cs = None
    if colsum:
        s = lambda t: t.sum((0, 2, 3))  # noqa: E731
        cs = Ref(s(r.ref), s(r.bound) + s(r.ref.abs()), s(r.deg2), None if r.degh is None else s(r.degh))
    y = r
    if res is not None and not res_pre:
        y = _affine(r, mul=float(torch.tensor(res_alpha, dtype=torch.float32)), add=res.double())
    return dict(y=y, a=r, colsum=cs)


def conv3_wgrad(x, dy, x_act=NONE, dy_scale=1.0, floor_bounds=None, want_h=True):
    """dict(dw=Ref [Cout][Cin][3][3], db=Ref [Cout]) of dy_scale * (op_wgrad3(x_act(x), dy), sum dy)."""
    xa = in_act32(x, x_act)
    ds = float(torch.tensor(dy_scale, dtype=torch.float32))
    r = bilinear(op_wgrad3, xa, dy, want_h=want_h)
    if floor_bounds is not None:
        fl = FLOOR * floor_bounds[0] * floor_bounds[1] * x.shape[0] * x.shape[2] * x.shape[3]
        r = Ref(r.ref, r.bound + fl / C_ENTRY, r.deg2, r.degh)
    s = lambda t: t.sum((0, 2, 3))  # noqa: E731
    db = Ref(s(dy.double()), s(dy.double().abs()), s(two_piece(dy)))
    if ds != 1.0:
        r, db = _affine(r, mul=ds), _affine(db, mul=ds)
    return dict(dw=r, db=db)


def conv3_autograd(x, w, bias, dy):
    """(y, dx, dw, db) of float64 autograd."""
    xr, wr, br = x.double().requires_grad_(), w.double().requires_grad_(), bias.double().requires_grad_()
    y = F.conv2d(xr, wr, br, 1, 1)
    y.backward(dy.double())
    return y.detach(), xr.grad, wr.grad, br.grad


def conv3_loops(x, w):
    """The same convolution as a direct loop over (output channel, input channel, tap) in numpy float64."""
    import numpy as np

    xn, wn = x.double().numpy(), w.double().numpy()
    n, Cin, H, W = xn.shape
    xp = np.zeros((n, Cin, H + 2, W + 2))
    xp[:, :, 1:-1, 1:-1] = xn
    y = np.zeros((n, wn.shape[0], H, W))
    for co in range(wn.shape[0]):
        for ci in range(Cin):
            for tap in range(9):
                y[:, co] += wn[co, ci, tap // 3, tap % 3] * xp[:, ci, tap // 3:tap // 3 + H, tap % 3:tap % 3 + W]
    return torch.from_numpy(y)


# ---- host arithmetic of csrc/conv3rs.hip ---------------------------------------------------------------------------------------
RS_PAIRS = [(64, 64), (64, 128), (128, 64), (128, 128), (128, 256)]  # the instantiated (Cin, Cout) of c3rs_kernel


def tiles(n, H, W):
    """32-position tiles of the stream: every image with one zero column per row and one zero row below it."""
    return -(-(n * (H + 1) * (W + 1)) // 32)


def reach(W):
    """D: the reach of the window in 32-position chunks."""
    return (W + 2 + 31) // 32


def ring(W):
    """LDS ring length in positions (c3_ring)."""
    D = reach(W)
    r = 32 * (2 * D + 2)
    while r <= 32 * D + 63 + W + 2:
        r += 32
    return r


def fwd_types(Cin, Cout):
    """C3Cfg::WG_TYPES: (Cout / 32 column tiles) x (Cin / 32 waves per tile) / 4 waves."""
    return (Cout // 32) * (Cin // 32) // 4


def fwd_workers(Cin, Cout):
    return 256 // fwd_types(Cin, Cout)


def wgrad_types(Cin, Cout):
    return (Cin // 64) * (Cout // 64)


def wgrad_workers(Cin, Cout):
    return 256 // wgrad_types(Cin, Cout)


def split(ntiles, workers):
    """[T0, T1) of every worker."""
    return [(ntiles * w // workers, ntiles * (w + 1) // workers) for w in range(workers)]


def fwd_lds(Cin, Cout, rng, np_):
    S = 2 * np_ * Cin + 16
    ksplit = Cin // 32
    own = 16 // ksplit
    xbuf = 4 * (ksplit - 1) * own * 64 * 4
    return rng * S + 2 * xbuf + 16 * 32 * 4 + 4 * 32 * 4


def wgrad_lds(rng):
    return (rng + 64) * (6 * 64 + 16) + 16 * 32 * 4


def _stream_ok(n, H, W, Cin, Cout):
    if n <= 0 or H < 4 or W < 4 or W > 96:
        return False
    if n * (H + 1) * (W + 1) >= (1 << 31) - 64 or n * H * W * max(Cin, Cout) * 4 >= (1 << 32) - 8192:
        return False
    D = reach(W)
    return (H + 1) * (W + 1) >= 32 * D and 32 // (W + 1) + 1 <= H + 1


def fwd_shape_ok(n, H, W, Cin, Cout, np_=3):
    """c3rs_shape_ok: what mvk_conv3x3_scaled_ok (np = 2) answers with every problem size admitted."""
    if not _stream_ok(n, H, W, Cin, Cout) or (Cin, Cout) not in RS_PAIRS:
        return False
    if reach(W) > (3 if Cin == 64 else (2 if np_ == 2 else 1)):
        return False
    return fwd_lds(Cin, Cout, ring(W), np_) <= 160 * 1024


def wgrad_shape_ok(n, H, W, Cin, Cout):
    """c3rs_wgrad_ok (mvk_conv3x3_wgrad_scaled_ok)."""
    if Cin % 64 or Cout % 64 or Cin > 256 or Cout > 256 or Cin <= 0 or Cout <= 0 or wgrad_types(Cin, Cout) > 16:
        return False
    return _stream_ok(n, H, W, Cin, Cout) and reach(W) <= 3 and wgrad_lds(ring(W)) <= 160 * 1024


def fused_ok(n, H, W, Cin, Cout):
    """mvk_conv3x3_fused_ok."""
    return fwd_shape_ok(n, H, W, Cin, Cout, 3) and wgrad_shape_ok(n, H, W, Cin, Cout)


def tiles_per_worker(n, H, W, workers):
    return tiles(n, H, W) / workers


# ---- host arithmetic of conv3_small_wgrad (csrc/conv3small.hip) ----------------------------------------------------------------
def small_wgrad_plan(n, H, W, Cin, Cout, scratch_floats=1 << 40):
    """None when the kernel declines; else dict(CS, CB, PG, loop = 'single' | 'row', grid, items, lds)."""
    in_small, out_small = Cin <= 4, Cout <= 4
    if n < 1 or not (in_small or out_small) or W > 256:
        return None
    CS, CB = (Cin, Cout) if in_small else (Cout, Cin)
    CG = CB // 4
    if CB % 4 or CG < 1 or CG > 64 or 64 % CG:
        return None
    total = 9 * Cin * Cout
    items = n * (-(-H // 8))
    grid = min(items, 1024, scratch_floats // total)
    if grid < 1:
        return None
    PG = 64 // CG
    lds = (((10 * (W + 2) * CS + 3) & ~3) + PG * total) * 4
    if lds > 64 * 1024:
        return None
    return dict(CS=CS, CB=CB, PG=PG, loop="single" if W >= PG else "row", grid=grid, items=items, lds=lds)


def splitk_slabs(M, N, K, target=768):
    """z of launch_splitk (csrc/igemm.hip): slices of an even number of 16-wide k-tiles."""
    tl = -(-M // 128) * (1 if N <= 32 else -(-N // 64))
    kt = -(-K // 16)
    sp = max(1, min(kt, target // tl))
    ks = -(-kt // sp)
    ks += ks & 1
    return -(-kt // ks)
