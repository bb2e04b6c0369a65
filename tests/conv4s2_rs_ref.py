"""float64 references of the register-stationary 4x4 / stride-2 / pad-1 kernels (csrc/imgconv.hip: imgconv_kernel, imgwgrad_kernel)
and the host arithmetic their control flow depends on, restated in Python.

Every operation is ONE bilinear map op(a, b) (tests/conv_small_ref.py), so the float64 reference op(a, b), the bound op(|a|, |b|)
that C_ENTRY multiplies and both degraded emulations (two_piece = both operands on two bf16 pieces: the bf16-piece form without its
third piece; f16_drop = scaled fp16 pairs with one cross term dropped: the scaled form without hi lo') come from one statement:

  op_down(U, W)   = F.conv2d(U, W, None, 2, 1)              U [n][Cu][2h][2w], W [Cv][Cu][4][4] -> [n][Cv][h][w]
  op_up(V, W)     = F.conv_transpose2d(V, W, None, 2, 1)    V [n][Cv][h][w]                      -> [n][Cu][2h][2w]
  op_wgrad(U, dV) = torch.nn.grad.conv2d_weight(U, ., dV)   d/dW of sum(op_down(U, W) dV)        -> [Cv][Cu][4][4]

The epilogue is that of imgconv.hip's epilogue_row, in its order:

  bias          + b, bound + |b|
  act           max(., 0) for ReLU (1-Lipschitz: the bound stays)
  mask          x [src > 0] for a ReLU mask source, x 1 for a `none` mask source (which still selects the HAS_SRC instantiation)
  column sums   the sum of the reference over (image, row, column); tolerance C_ENTRY (sum of bounds + sum |ref|): the rounding of
                every stored entry plus the fp32 sum of the stored entries
  scaled fp16   + the floor of csrc/bf3.hpp: 2^-39 of the two operand BOUNDS per product, times the products of an entry
                (16 Cu down, 4 Cv up, n h w for the weight gradient).
"""
import math

import torch

from conv3_ref import FLOOR
from conv_small_ref import (C_ENTRY, LEAKY, NONE, RELU, SIGMOID, Ref, act64, actgrad64, bilinear, degraded, f16_pair, g,  # noqa: F401
                            op_down, op_up, op_wgrad, two_piece)

PAIRS = ((8, 32, 64), (4, 64, 128))  # (h = w, Cu, Cv): the two inner layer pairs of the SVHN networks
GRID = 256                           # workgroups of every launch (imgconv_launch, imgwgrad_launch_np)
OPS = dict(down=op_down, up=op_up)


# ---- host arithmetic of csrc/imgconv.hip ---------------------------------------------------------------------------------------
def icfg(kind, h, Cu, Cv):
    """ICfg<KIND, HS, CIN, COUT> of the forward / backward-data kernel (kind 'down' | 'up')."""
    up = kind == "up"
    cin, cout = (Cv, Cu) if up else (Cu, Cv)
    pix = h * h
    chunks = cin // 16
    ntaps = 16 // chunks
    taps_all = 4 if up else 16
    ksplit = taps_all // ntaps
    nct = cout // 32
    roles = (4 if up else 1) * nct * ksplit
    return dict(kind=int(not up), cin=cin, cout=cout, pix=pix, ksplit=ksplit, nct=nct, roles=roles, types=roles // 4,
                su=1 if pix >= 32 else 32 // pix, tpu=pix // 32 if pix >= 32 else 1, products=(4 if up else 16) * cin)


def wcfg(h, Cu, Cv):
    """WCfg<HS, CU, CV> of the weight-gradient kernel."""
    pix = h * h
    split_kh = Cu * Cv > 32 * 64
    su = 1 if pix >= 32 else 2
    return dict(pix=pix, types=4 if split_kh else 1, su=su, ks=su * pix // 16)


def cfg(kind, pair):
    h, Cu, Cv = pair
    return wcfg(h, Cu, Cv) if kind == "wgrad" else icfg(kind, h, Cu, Cv)


def workers(kind, pair):
    """Workers (groups of workgroup types that walk the same images): 256 at 8x8, 64 at 4x4, for all three kernels."""
    return GRID // cfg(kind, pair)["types"]


def units(n, kind, pair):
    """Stage units of a launch: n // SU (an odd image at 4x4 is never reached: the host declines odd n)."""
    return n // cfg(kind, pair)["su"]


def unit_ranges(n, kind, pair):
    """[u0, u1) of every worker: units * worker / workers."""
    u, w = units(n, kind, pair), workers(kind, pair)
    return [(u * i // w, u * (i + 1) // w) for i in range(w)]


def tiles_per_worker(n, kind, pair):
    """32-row tiles every worker of imgconv_kernel owns: TPU * (u1 - u0)."""
    tpu = cfg(kind, pair)["tpu"]
    return [tpu * (u1 - u0) for u0, u1 in unit_ranges(n, kind, pair)]


def regime(n, kind, pair):
    """The set of tiles-per-worker counts present in a launch: what the main loop, its placeholder rows, its tail and its clamped
    read-ahead depend on (0: nothing; 1: drain only; 2: one placeholder tile; >= 3: the steady two-tile-latency loop)."""
    return set(tiles_per_worker(n, kind, pair))


def block_role(b, types, grid=GRID):
    """(worker, wgtype) of block b: plain division, or the XCD remap when the grid is a multiple of 8 * types."""
    wgtype, worker = b % types, b // types
    if types > 1 and grid % (8 * types) == 0:
        xcd, slot = b & 7, b >> 3
        wgtype = slot % types
        worker = xcd * (grid // (8 * types)) + slot // types
    return worker, wgtype


def wgrad_chains(n, pair):
    """Per worker of imgwgrad_kernel: (first image, images, terms of each of its accumulator chains = images * h * h)."""
    c = wcfg(*pair)
    return [(u0 * c["su"], (u1 - u0) * c["su"], (u1 - u0) * c["su"] * c["pix"]) for u0, u1 in unit_ranges(n, "wgrad", pair)]


def wgrad_chain(n, pair):
    """The longest accumulator chain of a weight-gradient launch, in products."""
    return max(t for _, _, t in wgrad_chains(n, pair))


def frag_bytes(kind, pair):
    """Bytes of the bf16-piece fragment pack the kernel reads: roles x 16 k-steps x 3 pieces x 64 lanes x 16 bytes."""
    return cfg(kind, pair)["roles"] * 16 * 3 * 64 * 16


def min_wgrad_scratch(pair):
    """Floats of slab scratch imgconv_wgrad asks for: one [16 Cu][Cv] slab per worker."""
    h, Cu, Cv = pair
    return workers("wgrad", pair) * 16 * Cu * Cv


def kernel_name(kind, pair, has_src, np_):
    """imgconv_kernel<KIND, HS, CIN, COUT, HAS_SRC, PIPE = true, NP> as torch.profiler reports it, spaces removed."""
    c = cfg(kind, pair)
    return f"imgconv_kernel<{c['kind']},{pair[0]},{c['cin']},{c['cout']},{str(bool(has_src)).lower()},true,{np_}>"


def wgrad_kernel_name(pair, np_):
    return f"imgwgrad_kernel<{pair[0]},{pair[1]},{pair[2]},{np_}>"


# ---- operands ---------------------------------------------------------------------------------------------------------------------
def fwd_operands(seed, kind, n, h, w, Cu, Cv, data="unit"):
    """(x, W, bias, mask source, initial column sums): x with every image on its own scale (0.25 .. 4.25), W [Cv][Cu][4][4] with
    every OUTPUT channel of the direction on its own scale.  data: 'spread' = images and weight rows over e^(+-3 sigma); 'tiny' =
    one image and one weight row 2^-30 of the others (below the full-precision range of a scaled fp16 pair)."""
    gn = g(seed)
    up = kind == "up"
    cin, cout = (Cv, Cu) if up else (Cu, Cv)
    ih, iw, oh, ow = (h, w, 2 * h, 2 * w) if up else (2 * h, 2 * w, h, w)
    oshape = (1, Cu, 1, 1) if up else (Cv, 1, 1, 1)
    x = torch.randn(n, cin, ih, iw, generator=gn) * (torch.rand(n, 1, 1, 1, generator=gn) * 4 + 0.25)
    W = torch.randn(Cv, Cu, 4, 4, generator=gn) * (torch.rand(oshape, generator=gn) + 0.5) / math.sqrt((4 if up else 16) * cin)
    if data == "spread":
        x = x * torch.exp(3.0 * torch.randn(n, 1, 1, 1, generator=gn))
        W = W * torch.exp(3.0 * torch.randn(oshape, generator=gn))
    if data == "tiny":
        x[n // 2] *= 2.0 ** -30
        if up:
            W[:, Cu // 2] *= 2.0 ** -30
        else:
            W[Cv // 2] *= 2.0 ** -30
    b = torch.randn(cout, generator=gn)
    src = torch.randn(n, cout, oh, ow, generator=gn)
    cinit = torch.randn(cout, generator=gn)
    return x, W, b, src, cinit


def wgrad_operands(seed, n, h, w, Cu, Cv, data="unit"):
    """(U, dV, initial dW).  data: 'spread' = the images of U over e^(+-3 sigma), those of dV (independently) over e^(+-1 sigma):
    with both over 3 sigma the largest |U| and the largest |dV| sit in different images, every product is far below the product
    of the operand bounds and the floor of the scaled form is the whole tolerance.  'imgs' = the images of U over e^(+-2.5 sigma):
    a few images carry most of every sum.  (The rounding of 16-bit operands averages out over an n h w-term sum of equal-sized
    terms: on unit data the two-piece emulation stays inside the tolerance from a few thousand terms on.  The chains the kernel
    adds up are as long as before.)"""
    gn = g(seed)
    U = torch.randn(n, Cu, 2 * h, 2 * w, generator=gn) * (torch.rand(n, 1, 1, 1, generator=gn) * 4 + 0.25)
    dV = torch.randn(n, Cv, h, w, generator=gn) * (torch.rand(1, Cv, 1, 1, generator=gn) + 0.5) / math.sqrt(n * h * w)
    if data == "spread":
        U = U * torch.exp(3.0 * torch.randn(n, 1, 1, 1, generator=gn))
        dV = dV * torch.exp(1.0 * torch.randn(n, 1, 1, 1, generator=gn))
    if data == "imgs":
        U = U * torch.exp(2.5 * torch.randn(n, 1, 1, 1, generator=gn))
    init = torch.randn(Cv, Cu, 4, 4, generator=gn)
    return U, dV, init


# ---- the operations ---------------------------------------------------------------------------------------------------------------
def _with_floor(r, fl):
    return Ref(r.ref, r.bound + fl / C_ENTRY, r.deg2, r.degh)


def conv_fwd(kind, x, W, bias=None, act=NONE, mask_src=None, mask_act=NONE, colsum=False, floor_bounds=None, want_h=True):
    """dict(y=Ref [n][cout][oh][ow], colsum=Ref [cout] or None) of  y = act(op(x, W) + bias) * mask_act'(mask_src).
    floor_bounds = (bound of |x|, bound of |W|) of a scaled-fp16 launch."""
    r = bilinear(OPS[kind], x, W, want_h=want_h)
    if floor_bounds is not None:
        products = (4 if kind == "up" else 16) * x.shape[1]
        r = _with_floor(r, FLOOR * floor_bounds[0] * floor_bounds[1] * products)
    if bias is not None:
        bb = bias.double().view(1, -1, 1, 1)
        r = Ref(r.ref + bb, r.bound + bb.abs(), r.deg2 + bb, None if r.degh is None else r.degh + bb)
    if act != NONE:
        bound = 0.25 * r.bound if act == SIGMOID else r.bound
        r = Ref(act64(r.ref, act), bound, act64(r.deg2, act), None if r.degh is None else act64(r.degh, act))
    if mask_src is not None:
        m = actgrad64(mask_src, mask_act)
        r = r.map(lambda t: t * m)
    cs = None
    if colsum:
        s = lambda t: t.sum((0, 2, 3))  # noqa: E731
        cs = Ref(s(r.ref), s(r.bound) + s(r.ref.abs()), s(r.deg2), None if r.degh is None else s(r.degh))
    return dict(y=r, colsum=cs)


def conv_wgrad(U, dV, floor_bounds=None, want_h=True):
    """Ref [Cv][Cu][4][4] of op_wgrad(U, dV)."""
    r = bilinear(op_wgrad, U, dV, want_h=want_h)
    if floor_bounds is not None:
        r = _with_floor(r, FLOOR * floor_bounds[0] * floor_bounds[1] * dV.shape[0] * dV.shape[2] * dV.shape[3])
    return r


def cpu_fp32(kind, x, W, bias=None, act=NONE, mask_src=None, mask_act=NONE):
    """The same layer by torch's float32 convolution on the CPU: a correct fp32 implementation, which the tolerance must admit."""
    import torch.nn.functional as F

    if kind == "down":
        y = F.conv2d(x, W, bias, stride=2, padding=1)
    else:
        y = F.conv_transpose2d(x, W, bias, stride=2, padding=1)
    y = act64(y, act) if act != SIGMOID else torch.sigmoid(y)
    if mask_src is not None:
        y = y * actgrad64(mask_src, mask_act).float()
    return y


def cpu_fp32_wgrad(U, dV, pair):
    """torch's float32 conv2d_weight on the CPU over the images of each accumulator chain of imgwgrad_kernel (wgrad_chains), then
    the ordered float32 sum of the slabs: a correct fp32 implementation whose chains stay inside the 1024 terms C_ENTRY was set
    for.  (One conv2d_weight call over the whole batch runs chains of n h w / threads products: up to 8192 here.)"""
    out = None
    for i0, k, _ in wgrad_chains(U.shape[0], pair):
        if k:
            s = op_wgrad(U[i0:i0 + k], dV[i0:i0 + k])
            out = s if out is None else out + s
    last = U.shape[0] - U.shape[0] % wcfg(*pair)["su"]
    if last < U.shape[0]:  # the odd image of a declined 4x4 batch
        out = out + op_wgrad(U[last:], dV[last:])
    return out
