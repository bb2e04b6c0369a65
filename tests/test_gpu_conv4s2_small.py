"""The small-channel 4x4 / stride-2 kernels (csrc/smallconv.hip, csrc/smallcin.hip), leaf by leaf, against float64.

The machinery is that of tests/test_gpu_gemm_dispatch.py (imported as D: launched_kernels, Prep, Out, execute, check_case,
C_ENTRY); the references, bounds and degraded emulations are tests/conv_small_ref.py, and tests/test_conv_small_ref_host.py
shows on the CPU that both emulations leave the tolerance of every case of CASES.  Each case

1. names its entry point and the exact set of device kernels it must launch (torch.profiler);
2. compares EVERY output entry with float64: |got - ref| <= C_ENTRY * (sum |a b| + |bias| + |initial|), C_ENTRY = 5e-7;
3. carries the two-piece bf16 emulation of the same formula, which must FAIL that check;
4. runs twice from the same buffers and must be bit-identical (ordered slabs everywhere; the one exception is the weight gradient
   that falls to the implicit GEMM's fp32-atomic split K when its scratch is too small).

Activations carry no unmeasured constant: the table checks pre-activations (act = 0) per entry; ReLU / LeakyReLU outputs must equal
act(pre-activation output) BIT FOR BIT (same sums, then a select); the sigmoid output is compared with the float64 sigmoid of the
kernel's OWN fp32 pre-activation, allowance = 2x the largest ulp error of torch.sigmoid (fp32, GPU) on that same tensor, never
less than 1 ulp.  Measured on an MI355X (largest ulp error, kernel / torch): 2.04 / 2.04 over test_activations for the kernels that
evaluate 1 / (1 + expf(-v)) (the same bits as torch), 2.11 / 1.80 for mvk_fast_sigmoid in small_up_fwd_h_kernel there and 2.68 / 2.12
over 1.5 M entries (n = 513); small_up_fwd_bf_kernel 2.20 / 2.20.

Chain lengths (basis of C_ENTRY, <= 1024 terms per fp32 accumulator chain): the forward kernels reduce over 4 Cv <= 256 (up) or
16 Cu <= 64 (down) terms.  small_up_bwd_kernel: dV over 16 Cu <= 64 terms; dW per wave over 64 positions per image and the images
of its workgroup (n <= 5 on <= 5 workgroups here, 2 images at n = 513 on 512), then 4 waves, then small_up_bwd_reduce_kernel (8
strided partial sums of <= 64 slabs, a tree of 8).  smallcin_wgrad_kernel: pos_per_block / 4 <= 80 terms per wave, 4 waves, the
ordered slab sum.  The large cases (n = 513 backward: test_up_bwd_large_batch, n = 1030 smallcin weight gradient:
test_cin_wgrad_block_cap) are held to criterion (b) of the GEMM table: max and rms error no worse than 2x torch's fp32 GEMM of the
same operands on the GPU; the second one, where (b) has no teeth, also slab by slab.

Worst measured |got - ref| / tolerance over the table on an MI355X (per-kernel list: profiles/NOTES_conv_small.md):
small_up_fwd_kernel 0.26, small_down_fwd_kernel 0.61, small_up_bwd_kernel 0.56 (dV) / 0.50 (dW) / 0.02 (db) / 0.04 (db_v),
smallcin_fwd_kernel 0.59, smallcin_wgrad_kernel 0.20 (slabs of the block-cap case 0.45), small_up_fwd_bf_kernel 0.16 (image) /
0.39 (dpre) / 0.12 (rows), small_up_fwd_h_kernel 0.21 / 0.46 / 0.14, small_up_bwd_bf_kernel 0.38 / 0.12 / 0.02 / 0.03,
small_up_bwd_h_kernel 0.29 / 0.18 / 0.01 / 0.01.  The two-piece emulation sits at 2 - 9x the tolerance on the products (dV, dW,
images, dpre); the plain sums (db, db_v) and the NLL rows (tolerance C_ENTRY * sum |terms|, dominated by the constant
D (log s + 1/2 log 2 pi)) do not reject it on their own: a case is rejected through its other outputs.

The shape gate: supported() admits h, w <= 16 only (the halo staging of small_down_fwd_kernel and small_up_bwd_kernel is sized for
34 x 34 elements per channel; 4 x 64 or 2 x 128 maps with the same position count left the tail of the tile unstaged).  Elongated
maps are refused by the small entry points and computed by smallcin / the tiled engine: test_shape_gate and the `gate-` cases.

Leaves of this family NOT covered here:
- small_up_fwd_kernel<3,32,...> at 16x16: shipped builds send that shape to small_up_fwd_bf_kernel; only MVK_SMALL_FWD_BF=0,
  read once per process, reaches it.  Likewise the half-image units (MVK_SMALL_BWD_UNITS), MVK_SMALL_BWD_OCC, _BWD_DENSE=0 and
  MVK_SMALL_NLL_NT=1024 instantiations.
- small_up_fwd_bf_kernel<3,512,false> (MVK_SMALL_FWD_BF=512), read once per process as well.
mvk_conv4s2_wgrad_pair (igemm_bf_pair_kernel) is in the GEMM table of tests/test_gpu_gemm_dispatch.py.
"""
import math
import os
import zlib

import pytest
import torch
import torch.nn.functional as F

import conv_small_ref as R
import test_gpu_gemm_dispatch as D

pytestmark = pytest.mark.gpu

NONE, RELU, SIGMOID, LEAKY = R.NONE, R.RELU, R.SIGMOID, R.LEAKY
PAIRS = [(cu, cv) for cu in (1, 2, 3, 4) for cv in (16, 32, 64)]  # MVK_SMALL_DISPATCH
OTHER = [(8, 8), (16, 8), (8, 16), (12, 16), (4, 16)]             # P = 64, 128, 128, 192, 64
REDUCE = "small_up_bwd_reduce_kernel"


def k_up_fwd(cu, cv, dense):
    return f"small_up_fwd_kernel<{cu},{cv},1024,{str(dense).lower()}>"


def k_up_bwd(cu, cv, spec, dense):
    return f"small_up_bwd_kernel<{cu},{cv},256,256,2,{'2,1' if spec else '-1,-1'},{str(dense).lower()}>"


def k_down(cu, cv):
    return f"small_down_fwd_kernel<{cu},{cv},512>"


def k_cin_wgrad(cu, cv):
    return f"smallcin_wgrad_kernel<{cu},{cv // 16}>"


def _out(r, lay=lambda t: t, init=None, shape=None, rows=None):
    """D.Out of a conv_small_ref.Ref (the two-piece emulation is the one the GPU check carries)."""
    bound = lay(r.bound) if init is None else lay(r.bound) + init.double().abs()
    o = D.Out(lay(r.ref), bound, lay(r.deg2), init=init, shape=shape, rows=rows)
    o.degh = None if r.degh is None else lay(r.degh)
    o.derived = getattr(r, "derived", False)
    return o


_NHWC = lambda t: t.permute(0, 2, 3, 1)  # noqa: E731


# ---- entry points -----------------------------------------------------------------------------------------------------------
def p_up_fwd(seed, n, h, w, Cu, Cv, bias=True, act=NONE, host=False, cap=48):
    """mvk_conv4s2_small_up_fwd: U [n][Cu][2h][2w] = act(convT4x4s2p1(V [n][h][w][Cv], Wref [Cv][Cu][4][4]) + b)."""
    V, W, b = R.up_operands(seed, n, h, w, Cu, Cv, bias)
    imgs = D._imgs(n, cap)
    r = R.up_pre(V if imgs is None else V[imgs], W, b)
    assert act == NONE
    outs = [_out(r, shape=(n, Cu, 2 * h, 2 * w), rows=imgs)]
    if host:
        return D.Prep(None, outs)
    from multivae_amd._lib import call, ptr, stream_ptr

    d = D.dev()
    Vd, Wd, bd = D._nhwc(V).to(d), W.to(d), None if b is None else b.to(d)

    def run(bufs):
        call("mvk_conv4s2_small_up_fwd", ptr(Vd), ptr(Wd), ptr(bd), ptr(bufs[0]), n, h, w, Cu, Cv, act, stream_ptr())

    return D.Prep(run, outs, keep=[Vd, Wd, bd])


def p_down_fwd(seed, n, h, w, Cu, Cv, bias=True, entry="fwd", host=False, cap=48):
    """The down layer V [n][h][w][Cv] = conv4x4s2p1(U [n][Cu][2h][2w]) + b through mvk_conv4s2_small_down_fwd (packed weight),
    _fwd_wref (reference weight layout) or mvk_conv4s2_down(u_nchw = 1) (the routing of the network-input layer; also the way
    into smallcin_fwd_kernel for the shapes supported() refuses)."""
    U, W, b = R.down_operands(seed, n, h, w, Cu, Cv, bias)
    imgs = D._imgs(n, cap)
    r = R.down_pre(U if imgs is None else U[imgs], W, b)
    outs = [_out(r, _NHWC, shape=(n, h, w, Cv), rows=imgs)]
    if host:
        return D.Prep(None, outs)
    from multivae_amd import kernels as KK
    from multivae_amd._lib import call, ptr, stream_ptr

    d = D.dev()
    Ud, Wd, bd = U.to(d), W.to(d), None if b is None else b.to(d)
    wdown, _ = KK.pack_conv(Wd, want_up=False)
    wsp, wsn = D.WS("ws")

    def run(bufs):
        if entry == "route":
            call("mvk_conv4s2_down", ptr(Ud), ptr(wdown), ptr(bd), ptr(bufs[0]), n, h, w, Cu, Cv, NONE, 1, None, NONE, None, NONE,
                 None, wsp, wsn, 0, None, stream_ptr())
        elif entry == "wref":
            call("mvk_conv4s2_small_down_fwd_wref", ptr(Ud), ptr(Wd), ptr(bd), ptr(bufs[0]), n, h, w, Cu, Cv, NONE, stream_ptr())
        else:
            call("mvk_conv4s2_small_down_fwd", ptr(Ud), ptr(wdown), ptr(bd), ptr(bufs[0]), n, h, w, Cu, Cv, NONE, stream_ptr())

    return D.Prep(run, outs, keep=[Ud, Wd, wdown, bd])


def p_up_tiled(seed, n, h, w, Cu, Cv, bias=True, host=False):
    """mvk_conv4s2_up(u_nchw = 1) from the packed up weight: where an up layer with Cu <= 4 goes when supported() refuses its map."""
    V, W, b = R.up_operands(seed, n, h, w, Cu, Cv, bias)
    outs = [_out(R.up_pre(V, W, b))]
    if host:
        return D.Prep(None, outs)
    from multivae_amd import kernels as KK
    from multivae_amd._lib import call, ptr, stream_ptr

    d = D.dev()
    _, wup = KK.pack_conv(W.to(d), want_down=False)
    Vd, bd = D._nhwc(V).to(d), None if b is None else b.to(d)
    wsp, wsn = D.WS("ws")

    def run(bufs):
        call("mvk_conv4s2_up", ptr(Vd), ptr(wup), ptr(bd), ptr(bufs[0]), n, h, w, Cu, Cv, NONE, 1, None, NONE, None, wsp, wsn, 0, None,
             stream_ptr())

    return D.Prep(run, outs, keep=[Vd, wup, bd])


def bwd_slab(Cu, Cv):
    return Cv * 16 * Cu + Cu + Cv  # floats per workgroup: dW, db, db_v partials (launch_bwd)


def p_up_bwd(seed, n, h, w, Cu, Cv, u_act=SIGMOID, v_act=RELU, du_off=False, ws_grid=None, deferred=False, exact=False,
             host=False, cap=48):
    """mvk_conv4s2_small_up_bwd: dV [n][h][w][Cv] = conv4x4s2p1(dU u_act'(Uout), W) v_act'(V); dW, db, db_v += (ordered slabs).
    du_off: dU at storage offset 1 (no 16-byte loads: the non-DENSE form at 16x16).  ws_grid: scratch for that many workgroups
    only.  exact: MVK_SMALL_BWD_BF=0 for the call (the exact-fp32 kernel at the split-bf16 kernel's shape)."""
    dU, Uout, V, W, init = R.bwd_operands(seed, n, h, w, Cu, Cv, u_act, v_act)
    imgs = D._imgs(n, cap)
    r = R.up_bwd(dU, Uout, u_act, V, v_act, W)
    dV = r["dV"] if imgs is None else r["dV"].map(lambda t: t[imgs])
    outs = [_out(dV, _NHWC, shape=(n, h, w, Cv), rows=imgs), _out(r["dW"], init=init[0]), _out(r["db"], init=init[1]),
            _out(r["dbv"], init=init[2])]
    if host:
        return D.Prep(None, outs, deferred=deferred)
    from multivae_amd._lib import call, ptr, stream_ptr

    d = D.dev()
    dUd = D.unaligned(dU.to(d)) if du_off else dU.to(d)
    Uod, Vd, Wd = Uout.to(d), D._nhwc(V).to(d), W.to(d)
    wsp, wsn = D.WS("ws")
    if ws_grid is not None:
        wsn = ws_grid * bwd_slab(Cu, Cv)

    def run(bufs):
        old = os.environ.get("MVK_SMALL_BWD_BF")
        if exact:
            os.environ["MVK_SMALL_BWD_BF"] = "0"
        try:
            call("mvk_conv4s2_small_up_bwd", ptr(dUd), ptr(Uod), u_act, ptr(Vd), v_act, ptr(Wd), ptr(bufs[0]), ptr(bufs[1]),
                 ptr(bufs[2]), ptr(bufs[3]), wsp, wsn, n, h, w, Cu, Cv, stream_ptr())
        finally:
            if exact and old is None:
                del os.environ["MVK_SMALL_BWD_BF"]
            elif exact:
                os.environ["MVK_SMALL_BWD_BF"] = old

    p = D.Prep(run, outs, deferred=deferred, keep=[dUd, Uod, Vd, Wd])
    p.torch32 = lambda: _bwd_torch32(dUd, Uod, u_act, Vd, v_act, Wd, n, h, w, Cu, Cv)
    return p


def _bwd_torch32(dUd, Uod, u_act, Vd, v_act, Wd, n, h, w, Cu, Cv):
    """(dW, db, db_v) by torch's fp32 ops on the GPU from the same operands (im2col + matmul, sums): the yardstick of (b)."""
    d = D.dev()
    dpre = dUd * R.actgrad64(Uod.cpu(), u_act).float().to(d)
    cols = F.unfold(dpre, 4, padding=1, stride=2).transpose(1, 2).reshape(n * h * w, Cu * 16)
    Vm = Vd.reshape(n * h * w, Cv)
    dW = (Vm.t() @ cols).view(Cv, Cu, 4, 4)
    dV = (cols @ Wd.view(Cv, Cu * 16).t()) * R.actgrad64(Vm.cpu(), v_act).float().to(d)
    return [dW.double().cpu(), dpre.sum((0, 2, 3)).double().cpu(), dV.sum(0).double().cpu()]


def p_cin_wgrad(seed, n, h, w, Cu, Cv, ws="ws", deferred=False, agg=False, host=False):
    """mvk_conv4s2_wgrad(u_nchw = 1) on an NCHW image with Cu <= 4 channels: dWref [Cv][Cu][4][4] += the weight gradient of
    Conv2d(Cu, Cv, 4, 2, 1) (smallcin_wgrad_kernel + the ordered slab sum); ws = 'short': one float below smallcin's need, the
    launch falls to the implicit GEMM."""
    U, dV, init = R.wgrad_operands(seed, n, h, w, Cu, Cv)
    r = R.bilinear(R.op_wgrad, U, dV, want_h=host)
    outs = [_out(r, init=init)]
    if host:
        return D.Prep(None, outs, deferred=deferred, det=ws == "ws")
    from multivae_amd._lib import call, ptr, stream_ptr

    d = D.dev()
    Ud, dVd = U.to(d), D._nhwc(dV).to(d)
    npos = n * h * w
    need = min((npos + 255) // 256, 1024) * 16 * Cu * Cv
    wsp, wsn = D.WS(ws, need)

    def run(bufs):
        call("mvk_conv4s2_wgrad", ptr(Ud), ptr(dVd), ptr(bufs[0]), n, h, w, Cu, Cv, 1, None, NONE, wsp, wsn, stream_ptr())

    def agg_():  # torch's fp32 GEMM of the same operands (im2col + matmul)
        cols = F.unfold(Ud, 4, padding=1, stride=2).transpose(1, 2).reshape(npos, Cu * 16)
        return (dVd.reshape(npos, Cv).t() @ cols).view(Cv, Cu, 4, 4).double()

    return D.Prep(run, outs, agg=agg_ if agg else None, det=ws == "ws", deferred=deferred, keep=[Ud, dVd])


# ---- the split-bf16 and scaled-fp16 kernels of the SVHN decoder's image layer (16x16 x 32 -> 3 x 32x32) -----------------------------
SV = dict(h=16, w=16, Cu=3, Cv=32)
SIGMOID_ULP_GPU = 2.04  # largest ulp error of torch.sigmoid (fp32) on an MI355X over these tensors: the host stand-in's floor
FLOOR = 2.0 ** -39      # bf3.hpp: absolute error of a scaled fp16 pair below 2^-28 of the tensor's bound, per unit of that bound


def _sv_operands(seed, n, data):
    """V = ReLU output (with a tiny positive entry: its leading fp16 piece is zero), W, b; data = 'spread': images 10^+-3 apart."""
    gn = R.g(seed)
    V = torch.relu(torch.randn(n, 32, 16, 16, generator=gn)) * (torch.rand(1, 32, 1, 1, generator=gn) + 0.5)
    if data == "spread":
        V = V * (10.0 ** ((torch.rand(n, 1, 1, 1, generator=gn) * 2 - 1) * 3.0))
    V[0, 0, 0, 0] = 1e-12 * float(V.max())
    W = torch.randn(32, 3, 4, 4, generator=gn) * (torch.rand(1, 3, 1, 1, generator=gn) + 0.5) / math.sqrt(128)
    b = torch.randn(3, generator=gn)
    return gn, V, W, b


def _floor(r, floor):
    """The Ref with an absolute allowance `floor` added to its tolerance (bound = tolerance / C_ENTRY)."""
    return R.Ref(r.ref, r.bound + floor / R.C_ENTRY, r.deg2, r.degh)


def p_sv_fwd(seed, n, form="bf", data="unit", bias=True, host=False, cap=24):
    """The pre-activation of the image layer on three bf16 pieces (mvk_conv4s2_small_up_fwd at this shape: small_up_fwd_bf_kernel)
    or on scaled fp16 pairs (mvk_conv4s2_small_up_fwd_s: small_up_fwd_h_kernel; V under the bound max |V|, x 1000 for
    data = 'loose').  The scaled form's tolerance adds bf3.hpp's floor 2^-39 bound_V max |W| 4 Cv."""
    _, V, W, b = _sv_operands(seed, n, data)
    b = b if bias else None
    imgs = D._imgs(n, cap)
    r = R.up_pre(V if imgs is None else V[imgs], W, b)
    vb = float(V.abs().max()) * (1000.0 if data == "loose" else 1.0)
    if form == "h":
        r = _floor(r, FLOOR * vb * float(W.abs().max()) * 128)
    outs = [_out(r, shape=(n, 3, 32, 32), rows=imgs)]
    if host:
        return D.Prep(None, outs)
    from multivae_amd._lib import call, ptr, stream_ptr

    d = D.dev()
    Vd, Wd, bd = D._nhwc(V).to(d), W.to(d), None if b is None else b.to(d)
    amax = torch.full((1,), vb, device=d)

    def run(bufs):
        if form == "h":
            call("mvk_conv4s2_small_up_fwd_s", ptr(Vd), ptr(Wd), ptr(bd), ptr(bufs[0]), n, 16, 16, 3, 32, NONE, ptr(amax), stream_ptr())
        else:
            call("mvk_conv4s2_small_up_fwd", ptr(Vd), ptr(Wd), ptr(bd), ptr(bufs[0]), n, 16, 16, 3, 32, NONE, stream_ptr())

    return D.Prep(run, outs, keep=[Vd, Wd, bd, amax])


NLL_SCALE, NLL_GW = 0.75, float(torch.tensor(0.3, dtype=torch.float32))  # the fp32 values the entry point receives


def p_sv_nll(seed, n, xrows, form="w", data="unit", host=False, cap=24):
    """The fused tail: rows[n] (Normal NLL of the sigmoid image against X[i % xrows]) and dpre = d rows / d pre-activation x gw,
    by mvk_conv4s2_small_up_fwd_nll_w (bf16 pieces) or _nll_s (scaled fp16 pairs)."""
    gn, V, W, b = _sv_operands(seed, n, data)
    X = torch.rand(xrows, 3, 32, 32, generator=gn)
    imgs = D._imgs(n, cap)
    sel = torch.arange(n) if imgs is None else imgs
    pre = R.up_pre(V[sel], W, b)
    vb = float(V.abs().max())
    if form == "s":
        pre = _floor(pre, FLOOR * vb * float(W.abs().max()) * 128)
    d = None if host else D.dev()
    yard = R.sigmoid_ulps(pre.ref.float() if host else pre.ref.float().to(d), None if host else torch.sigmoid(pre.ref).to(d))
    allow = max(2 * max(yard, SIGMOID_ULP_GPU if host else 0.0), 1.0)
    # image sel[i] is scored against X[sel[i] % xrows]
    rows, dpre = R.nll_tail(pre, X[sel % xrows], len(sel), NLL_SCALE, NLL_GW, allow)
    outs = [_out(dpre, shape=(n, 3, 32, 32), rows=imgs), _out(rows, shape=(n,), rows=imgs)]
    if host:
        return D.Prep(None, outs)
    from multivae_amd._lib import call, ptr, stream_ptr

    Vd, Wd, bd, Xd = D._nhwc(V).to(d), W.to(d), b.to(d), X.to(d)
    amax = torch.full((1,), vb, device=d)

    def run(bufs):
        if form == "s":
            call("mvk_conv4s2_small_up_fwd_nll_s", ptr(Vd), ptr(Wd), ptr(bd), ptr(Xd), xrows, NLL_SCALE, NLL_GW, ptr(bufs[0]), ptr(bufs[1]),
                 n, 16, 16, 3, 32, SIGMOID, ptr(amax), stream_ptr())
        else:
            call("mvk_conv4s2_small_up_fwd_nll_w", ptr(Vd), ptr(Wd), ptr(bd), ptr(Xd), xrows, NLL_SCALE, NLL_GW, ptr(bufs[0]), ptr(bufs[1]),
                 n, 16, 16, 3, 32, SIGMOID, stream_ptr())

    p = D.Prep(run, outs, keep=[Vd, Wd, bd, Xd, amax])
    p.sigmoid_yard = yard
    return p


def p_sv_bwd(seed, n, entry="bwd", rowscale=False, deferred=False, data="unit", host=False, cap=24):
    """The image layer's backward at the SVHN decoder's shape: mvk_conv4s2_small_up_bwd (sigmoid image, ReLU input map:
    small_up_bwd_bf_kernel<3,false>), _bwd_pre / _bwd_pre_y (dU is the pre-activation gradient per unit of its image's score, times
    rowscale[n]: <3,true>; _y publishes max |dV|) and _bwd_pre_s (scaled fp16 pairs: small_up_bwd_h_kernel<3>)."""
    gn, V, W, _ = _sv_operands(seed, n, data)
    dU = torch.randn(n, 3, 32, 32, generator=gn) * 0.05 * (torch.rand(n, 1, 1, 1, generator=gn) * 4 + 0.25)
    if data == "spread":
        dU = dU * (10.0 ** ((torch.rand(n, 1, 1, 1, generator=gn) * 2 - 1) * 3.0))
    Uout = R.stored(torch.randn(n, 3, 32, 32, generator=gn), SIGMOID)
    rs = None
    if rowscale:
        rs = torch.randn(n, generator=gn)
        if n >= 3:
            rs[n // 2] = 0.0  # a row that does not enter the loss
    init = (torch.randn(32, 3, 4, 4, generator=gn), torch.randn(3, generator=gn), torch.randn(32, generator=gn))
    pre_form = entry != "bwd"
    eff = dU.double() * (rs.double().view(n, 1, 1, 1) if rs is not None else 1.0)  # what enters the layer, exact
    r = R.up_bwd(eff, Uout, NONE if pre_form else SIGMOID, V, RELU, W)
    db_, vb = float(dU.abs().max()) * (float(rs.abs().max()) if rs is not None else 1.0), float(V.abs().max())
    if entry == "pre_s":  # bf3.hpp's floor per product x the number of products of an entry
        f = FLOOR * db_
        r = dict(dV=_floor(r["dV"], f * float(W.abs().max()) * 48), dW=_floor(r["dW"], f * vb * 256 * n), db=_floor(r["db"], f * 1024 * n),
                 dbv=_floor(r["dbv"], f * float(W.abs().max()) * 48 * 256 * n))
    imgs = D._imgs(n, cap)
    dV = r["dV"] if imgs is None else r["dV"].map(lambda t: t[imgs])
    outs = [_out(dV, _NHWC, shape=(n, 16, 16, 32), rows=imgs), _out(r["dW"], init=init[0]), _out(r["db"], init=init[1]),
            _out(r["dbv"], init=init[2])]
    if host:
        return D.Prep(None, outs, deferred=deferred)
    from multivae_amd._lib import call, ptr, stream_ptr

    d = D.dev()
    dUd, Uod, Vd, Wd = dU.to(d), Uout.to(d), D._nhwc(V).to(d), W.to(d)
    rsd = None if rs is None else rs.to(d)
    du_amax, v_amax = torch.full((1,), float(dU.abs().max()), device=d), torch.full((1,), vb, device=d)
    pub = torch.zeros(1, device=d)
    wsp, wsn = D.WS("ws")

    def run(bufs):  # (pub holds 0 at the first launch; a repeat of the same launch leaves its maximum where it is)
        tail = (wsp, wsn, n, 16, 16, 3, 32)
        if entry == "bwd":
            call("mvk_conv4s2_small_up_bwd", ptr(dUd), ptr(Uod), SIGMOID, ptr(Vd), RELU, ptr(Wd), ptr(bufs[0]), ptr(bufs[1]), ptr(bufs[2]),
                 ptr(bufs[3]), *tail, stream_ptr())
            return
        head = (ptr(dUd), ptr(rsd), ptr(Vd), RELU, ptr(Wd), ptr(bufs[0]), ptr(bufs[1]), ptr(bufs[2]), ptr(bufs[3]))
        if entry == "pre":
            call("mvk_conv4s2_small_up_bwd_pre", *head, *tail, stream_ptr())
        elif entry == "pre_y":
            call("mvk_conv4s2_small_up_bwd_pre_y", *head, *tail, ptr(pub), stream_ptr())
        else:
            call("mvk_conv4s2_small_up_bwd_pre_s", *head, *tail, ptr(du_amax), ptr(v_amax), ptr(pub), stream_ptr())

    p = D.Prep(run, outs, deferred=deferred, keep=[dUd, Uod, Vd, Wd, rsd, du_amax, v_amax])
    p.pub, p.V = pub, V
    effd = dUd if rsd is None else dUd * rsd.view(n, 1, 1, 1)
    p.torch32 = lambda: _bwd_torch32(effd, Uod, NONE if pre_form else SIGMOID, Vd, RELU, Wd, n, 16, 16, 3, 32)
    return p


K_FWD_BF, K_FWD_BF_NLL = "small_up_fwd_bf_kernel<3,1024,false>", "small_up_fwd_bf_kernel<3,512,true>"
K_FWD_H, K_FWD_H_NLL = "small_up_fwd_h_kernel<3,512,false>", "small_up_fwd_h_kernel<3,512,true>"
K_BWD_BF, K_BWD_BF_PRE, K_BWD_H = "small_up_bwd_bf_kernel<3,false>", "small_up_bwd_bf_kernel<3,true>", "small_up_bwd_h_kernel<3>"


# ---- the table ---------------------------------------------------------------------------------------------------------------
def case(id_, fn, kw, expect, note=""):
    seed = zlib.crc32(id_.encode()) % 100003
    c = D.Case(id_, lambda: fn(seed, **kw), tuple(sorted(expect)), None, note)
    c.host = lambda: fn(seed, host=True, **kw)
    return c


CASES = []
for _i, (_cu, _cv) in enumerate(PAIRS):
    _g = OTHER[_i % 5]
    _n1, _n2 = (1, 3) if _i % 2 else (3, 1)
    # --- small_up_fwd_kernel (exact fp32): every pair at 16x16 (DENSE) and one other geometry; (3,32) at 16x16 is the bf kernel's
    CASES.append(case(f"upfwd-{_cu}x{_cv}-{_g[0]}x{_g[1]}-n{_n1}", p_up_fwd, dict(n=_n1, h=_g[0], w=_g[1], Cu=_cu, Cv=_cv, bias=_i % 2 == 0),
                      [k_up_fwd(_cu, _cv, False)], "not 16x16: the guarded instantiation"))
    if (_cu, _cv) != (3, 32):
        CASES.append(case(f"upfwd-{_cu}x{_cv}-16x16-n{_n2}-dense", p_up_fwd, dict(n=_n2, h=16, w=16, Cu=_cu, Cv=_cv, bias=_i % 2 == 1),
                          [k_up_fwd(_cu, _cv, True)], "16x16, 256 Cv / 4 and 1024 Cu divide 1024 threads: DENSE (smallconv.hip launch_fwd)"))
    else:
        _g2 = OTHER[(_i + 2) % 5]
        CASES.append(case(f"upfwd-3x32-{_g2[0]}x{_g2[1]}-n{_n2}", p_up_fwd, dict(n=_n2, h=_g2[0], w=_g2[1], Cu=3, Cv=32, bias=False),
                          [k_up_fwd(3, 32, False)], "a second geometry instead of 16x16 (the split-bf16 kernel's)"))
    # --- small_down_fwd_kernel: the same spread; the three entries in turn
    _e = ("fwd", "wref", "route")
    CASES.append(case(f"down-{_cu}x{_cv}-{_g[0]}x{_g[1]}-n{_n1}-{_e[_i % 3]}", p_down_fwd,
                      dict(n=_n1, h=_g[0], w=_g[1], Cu=_cu, Cv=_cv, bias=_i % 2 == 0, entry=_e[_i % 3]), [k_down(_cu, _cv)]))
    CASES.append(case(f"down-{_cu}x{_cv}-16x16-n{_n2}-{_e[(_i + 1) % 3]}", p_down_fwd,
                      dict(n=_n2, h=16, w=16, Cu=_cu, Cv=_cv, bias=_i % 2 == 1, entry=_e[(_i + 1) % 3]), [k_down(_cu, _cv)]))
    # --- small_up_bwd_kernel: DENSE at 16x16 and guarded elsewhere, sigmoid/ReLU (compile-time) and generic activations in turn
    _acts = [(SIGMOID, RELU), (NONE, NONE), (NONE, RELU), (SIGMOID, LEAKY)]
    _a, _b = _acts[_i % 4], _acts[(_i + 1) % 4]
    CASES.append(case(f"upbwd-{_cu}x{_cv}-16x16-n{_n2}-u{_a[0]}v{_a[1]}-dense", p_up_bwd,
                      dict(n=_n2, h=16, w=16, Cu=_cu, Cv=_cv, u_act=_a[0], v_act=_a[1]),
                      [k_up_bwd(_cu, _cv, _a == (SIGMOID, RELU), True), REDUCE], "16x16, dU and Uout 16-byte aligned: DENSE"))
    CASES.append(case(f"upbwd-{_cu}x{_cv}-{_g[0]}x{_g[1]}-n{_n1}-u{_b[0]}v{_b[1]}", p_up_bwd,
                      dict(n=_n1, h=_g[0], w=_g[1], Cu=_cu, Cv=_cv, u_act=_b[0], v_act=_b[1]),
                      [k_up_bwd(_cu, _cv, _b == (SIGMOID, RELU), False), REDUCE]))
    # --- smallcin_fwd_kernel / smallcin_wgrad_kernel: shapes supported() refuses
    _c = [(6, 8), (20, 20), (32, 32)][_i % 3]
    _nc = 3 if _c[0] < 32 and _i % 2 else 1
    CASES.append(case(f"cinfwd-{_cu}x{_cv}-{_c[0]}x{_c[1]}-n{_nc}", p_down_fwd,
                      dict(n=_nc, h=_c[0], w=_c[1], Cu=_cu, Cv=_cv, bias=_i % 2 == 0, entry="route"), [f"smallcin_fwd_kernel<{_cu}>"],
                      "supported() refuses (P % 64 or P > 256): smallcin (igemm.hip conv4s2_down_impl)"))
    CASES.append(case(f"cinwgrad-{_cu}x{_cv}-{_c[0]}x{_c[1]}-n{_nc}", p_cin_wgrad, dict(n=_nc, h=_c[0], w=_c[1], Cu=_cu, Cv=_cv),
                      [k_cin_wgrad(_cu, _cv), D.RED]))

CASES += [
    case("upfwd-1x16-8x8-n513-second-image", p_up_fwd, dict(n=513, h=8, w=8, Cu=1, Cv=16), [k_up_fwd(1, 16, False)],
         "513 > 512 workgroups: workgroup 0 takes a second image (prefetch loop)"),
    case("down-1x16-8x8-n1025-second-image", p_down_fwd, dict(n=1025, h=8, w=8, Cu=1, Cv=16), [k_down(1, 16)],
         "1025 > 1024 workgroups"),
    case("upbwd-3x32-16x16-n2-u2v1-dense-exact", p_up_bwd, dict(n=2, h=16, w=16, Cu=3, Cv=32, exact=True),
         [k_up_bwd(3, 32, True, True), REDUCE], "MVK_SMALL_BWD_BF=0 (read per call): the exact kernel at the SVHN decoder's shape"),
    case("upbwd-3x32-16x16-n3-u2v1-duoff", p_up_bwd, dict(n=3, h=16, w=16, Cu=3, Cv=32, du_off=True),
         [k_up_bwd(3, 32, True, False), REDUCE], "dU not 16-byte aligned: neither the split-bf16 kernel nor DENSE"),
    case("upbwd-2x16-16x16-n1-u0v1-duoff", p_up_bwd, dict(n=1, h=16, w=16, Cu=2, Cv=16, u_act=NONE, v_act=RELU, du_off=True),
         [k_up_bwd(2, 16, False, False), REDUCE], "generic activations, 16x16, guarded form"),
    case("upbwd-2x32-8x16-n5-grid2", p_up_bwd, dict(n=5, h=8, w=16, Cu=2, Cv=32, ws_grid=2),
         [k_up_bwd(2, 32, True, False), REDUCE], "scratch for 2 slabs: grid = ws_floats / slab = 2, 3 and 2 images per workgroup"),
    case("upbwd-4x16-16x16-n3-u0v1-deferred", p_up_bwd, dict(n=3, h=16, w=16, Cu=4, Cv=16, u_act=NONE, v_act=RELU, deferred=True),
         [k_up_bwd(4, 16, False, True), D.BATCH], "dW, db, db_v in the flat gradient buffer: slabs from the deferred arena (dslab)"),
    # npos around the 256-position blocks / 64-position tiles of smallcin
    case("cinfwd-3x32-15x17-n1-npos255", p_down_fwd, dict(n=1, h=15, w=17, Cu=3, Cv=32, entry="route"), ["smallcin_fwd_kernel<3>"]),
    case("cinfwd-2x16-8x32-n1-npos256", p_down_fwd, dict(n=1, h=8, w=32, Cu=2, Cv=16, entry="route"), ["smallcin_fwd_kernel<2>"],
         "P = 256 but w > 16: refused by the shape gate"),
    case("cinfwd-4x64-1x257-n1-npos257", p_down_fwd, dict(n=1, h=1, w=257, Cu=4, Cv=64, entry="route"), ["smallcin_fwd_kernel<4>"]),
    case("cinwgrad-3x32-15x17-n1-npos255", p_cin_wgrad, dict(n=1, h=15, w=17, Cu=3, Cv=32), [k_cin_wgrad(3, 32), D.RED]),
    case("cinwgrad-2x16-8x32-n1-npos256", p_cin_wgrad, dict(n=1, h=8, w=32, Cu=2, Cv=16), [k_cin_wgrad(2, 16), D.RED]),
    case("cinwgrad-4x64-1x257-n1-npos257", p_cin_wgrad, dict(n=1, h=1, w=257, Cu=4, Cv=64), [k_cin_wgrad(4, 64), D.RED],
         "2 blocks of 192 positions, the second one 65"),
    case("cinwgrad-3x32-20x20-n1-shortscratch-igemm", p_cin_wgrad, dict(n=1, h=20, w=20, Cu=3, Cv=32, ws="short"),
         [D.gen(128, 32)], "smallcin_wgrad returns 1 -> implicit GEMM, NCHW gather: generic kernel, fp32-atomic split K"),
    case("cinwgrad-3x32-20x20-n4-deferred", p_cin_wgrad, dict(n=4, h=20, w=20, Cu=3, Cv=32, deferred=True),
         [k_cin_wgrad(3, 32), D.BATCH]),
    # the shape gate: elongated maps with P % 64 == 0, P <= 256 through the fallbacks
    case("gate-down-3x32-4x64-n3-smallcin", p_down_fwd, dict(n=3, h=4, w=64, Cu=3, Cv=32, entry="route"), ["smallcin_fwd_kernel<3>"],
         "10 x 130 halo tile per channel > 34 x 34"),
    case("gate-down-4x64-32x8-n1-smallcin", p_down_fwd, dict(n=1, h=32, w=8, Cu=4, Cv=64, entry="route"), ["smallcin_fwd_kernel<4>"]),
    case("gate-up-3x32-4x64-n3-tiled", p_up_tiled, dict(n=3, h=4, w=64, Cu=3, Cv=32), [D.gen(128, 32)],
         "mvk_conv4s2_up: the packed up weight [4][4 Cv][3] has no 16-byte rows -> generic kernel"),
    case("gate-up-4x64-32x8-n1-tiled", p_up_tiled, dict(n=1, h=32, w=8, Cu=4, Cv=64, bias=False), [D.bf(128, 32, "ROW", "N")]),
]
# --- the split-bf16 / scaled-fp16 kernels at 16x16 x 32 -> 3
for _n in (1, 3, 513):
    _x = {1: (1,), 3: (3, 1), 513: (513, 1, 27)}[_n]  # xrows: n, 1, a divisor of n
    CASES += [
        case(f"sv-fwd-bf-n{_n}", p_sv_fwd, dict(n=_n, bias=_n != 3), [K_FWD_BF], "16x16, (3, 32): three bf16 pieces, 1024 threads"),
        case(f"sv-fwd-h-n{_n}-unit", p_sv_fwd, dict(n=_n, form="h"), [K_FWD_H], "v_amax given: scaled fp16 pairs"),
        case(f"sv-fwd-h-n{_n}-spread", p_sv_fwd, dict(n=_n, form="h", data="spread", bias=False), [K_FWD_H], "images 10^+-3 apart"),
    ]
    for _xr in _x:
        CASES += [
            case(f"sv-nll-w-n{_n}-x{_xr}", p_sv_nll, dict(n=_n, xrows=_xr), [K_FWD_BF_NLL], "fused tail: 512 threads"),
            case(f"sv-nll-s-n{_n}-x{_xr}", p_sv_nll, dict(n=_n, xrows=_xr, form="s"), [K_FWD_H_NLL]),
        ]
CASES += [
    case("sv-fwd-h-n3-loose", p_sv_fwd, dict(n=3, form="h", data="loose"), [K_FWD_H], "a bound 1000x above max |V|: range, not precision"),
    case("sv-nll-s-n3-x3-spread", p_sv_nll, dict(n=3, xrows=3, form="s", data="spread"), [K_FWD_H_NLL]),
    case("sv-bwd-bf-n1", p_sv_bwd, dict(n=1), [K_BWD_BF, REDUCE], "sigmoid / ReLU, everything 16-byte aligned: the split-bf16 kernel"),
    case("sv-bwd-bf-n3", p_sv_bwd, dict(n=3), [K_BWD_BF, REDUCE]),
    case("sv-bwd-bf-n3-deferred", p_sv_bwd, dict(n=3, deferred=True), [K_BWD_BF, D.BATCH]),
    case("sv-bwd-pre-n1", p_sv_bwd, dict(n=1, entry="pre"), [K_BWD_BF_PRE, REDUCE]),
    case("sv-bwd-pre-n3-rowscale", p_sv_bwd, dict(n=3, entry="pre", rowscale=True), [K_BWD_BF_PRE, REDUCE], "a zero row"),
    case("sv-bwd-pre_y-n3-rowscale", p_sv_bwd, dict(n=3, entry="pre_y", rowscale=True), [K_BWD_BF_PRE, REDUCE]),
    case("sv-bwd-pre_y-n1", p_sv_bwd, dict(n=1, entry="pre_y"), [K_BWD_BF_PRE, REDUCE]),
    case("sv-bwd-pre_s-n1", p_sv_bwd, dict(n=1, entry="pre_s"), [K_BWD_H, REDUCE]),
    case("sv-bwd-pre_s-n3-rowscale", p_sv_bwd, dict(n=3, entry="pre_s", rowscale=True), [K_BWD_H, REDUCE]),
    case("sv-bwd-pre_s-n3-spread", p_sv_bwd, dict(n=3, entry="pre_s", data="spread"), [K_BWD_H, REDUCE]),
    case("sv-bwd-pre_s-n3-rowscale-deferred", p_sv_bwd, dict(n=3, entry="pre_s", rowscale=True, deferred=True), [K_BWD_H, D.BATCH]),
]
IDS = [c.id for c in CASES]


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_small_leaf(c):
    D.check_case(c, engine_f32=False)


def test_case_ids_are_unique():
    assert len(IDS) == len(set(IDS))


LARGE = {  # (Prep, kernels, the outputs held to criterion (b))
    "exact-1x16-8x8": (lambda: p_up_bwd(4711, 513, 8, 8, 1, 16), [k_up_bwd(1, 16, True, False), REDUCE], ("dW", "db", "db_v")),
    "sv-bwd-bf": (lambda: p_sv_bwd(4712, 513), [K_BWD_BF, REDUCE], ("dW",)),
    "sv-bwd-pre-rowscale": (lambda: p_sv_bwd(4713, 513, entry="pre", rowscale=True), [K_BWD_BF_PRE, REDUCE], ("dW",)),
    "sv-bwd-pre_s-rowscale": (lambda: p_sv_bwd(4714, 513, entry="pre_s", rowscale=True), [K_BWD_H, REDUCE], ("dW",)),
}


@pytest.mark.parametrize("which", list(LARGE))
def test_up_bwd_large_batch(which):
    """n = 513: more images than the 512 persistent workgroups (one takes a second image).  dV per entry.  The exact-fp32 kernel's
    dW, db, db_v (sums over 513 images) by criterion (b) of the GEMM table: max and rms error no worse than 2x torch's fp32 ops on
    the GPU against the same float64 reference.  The split-bf16 / scaled-fp16 kernels: dW by (b) (a GEMM against torch's GEMM); their
    db and db_v per entry at C_ENTRY * sum |terms| (every chain <= 1024 terms: 32 + 8 in the workgroup, 64 + 8 in
    small_up_bwd_reduce_kernel).  Held to (b) against torch.sum's tree reduction these two sums MISS it (measured on an MI355X:
    db_v max / rms error 3.8x / 6.5x torch's with bf16 pieces, 5.8x / 8.3x with rowscale, db 2.4x / 2.5x on fp16 pairs): ordered
    fp32 chains, recorded as a finding in profiles/NOTES_conv_small.md, not asserted.  The two-piece emulation must fail at least
    one check; the launch is bit-reproducible."""
    make, want, held_b = LARGE[which]
    torch.backends.cuda.matmul.allow_tf32 = False
    p = make()
    bufs, run = D.execute(p)
    assert D.launched_kernels(run) == sorted(want)
    got = [b.detach().cpu().double() for b in bufs]
    o = p.outs[0]
    tol = D.C_ENTRY * o.bound + 1e-30
    err = (got[0][o.rows] - o.ref).abs() / tol
    print(f"{which}: dV worst {float(err.max()):.3f}x the bound")
    assert float(err.max()) <= 1.0
    rejected = [float(((o.deg - o.ref).abs() / tol).max()) > 1.0]
    for name, o, t, y in zip(("dW", "db", "db_v"), p.outs[1:], got[1:], p.torch32()):
        e = [(x - o.ref).abs() for x in (t - o.init.double(), y, o.deg)]
        mx, rms = [float(x.max()) for x in e], [float(x.pow(2).mean().sqrt()) for x in e]
        worst = float((e[0] / (D.C_ENTRY * o.bound)).max())
        print(f"{which}: {name}: {worst:.4f}x C_ENTRY * bound; max {mx}, rms {rms} (kernel, torch fp32, two-piece)")
        if name in held_b:
            assert mx[0] <= 2 * mx[1] + 1e-30 and rms[0] <= 2 * rms[1] + 1e-30, (name, mx, rms)
            rejected.append(mx[2] > 2 * mx[1] or rms[2] > 2 * rms[1])
        else:
            assert worst <= 1.0, (name, worst)
    assert any(rejected), "no teeth: the two-piece operands pass every check"
    bufs2, run2 = D.execute(p)
    run2()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(bufs, bufs2))


@pytest.mark.parametrize("entry", ["pre_y", "pre_s"])
def test_sv_bwd_published_max_and_mask(entry):
    """The published max |dV| is exact (the maximum of what the launch stored), the ReLU mask of V is applied exactly, a tiny positive V
    (leading fp16 piece zero) keeps its gradient, and the image of a zero row gets a zero gradient."""
    p = p_sv_bwd(77, 3, entry=entry, rowscale=True)
    bufs, run = D.execute(p)
    run()
    torch.cuda.synchronize()
    dV = bufs[0].cpu().permute(0, 3, 1, 2)
    assert float(p.pub) == float(dV.abs().max()) and float(p.pub) > 0
    assert bool((dV[p.V <= 0] == 0).all()), "the ReLU mask of V"
    assert float(p.V[0, 0, 0, 0]) > 0 and float(dV[0, 0, 0, 0]) != 0.0, "a tiny positive V lost its gradient"
    assert float(dV[1].abs().max()) == 0.0, "rowscale[1] = 0"


@pytest.mark.parametrize("n,xrows", [(3, 1), (513, 27)])
def test_sv_nll_published_bound(n, xrows):
    """mvk_conv4s2_small_up_fwd_nll_sy = _nll_s bit for bit, plus an upper bound of max |dpre| (from the largest row sum: at most
    sqrt(3072) = 55x above, so <= 64x) in a slot that held 0."""
    from multivae_amd._lib import call, ptr, stream_ptr

    p = p_sv_nll(31, n, xrows, form="s")
    bufs, run = D.execute(p)
    run()
    Vd, Wd, bd, Xd, amax = p.keep
    d = D.dev()
    dpre, rows, pub = torch.empty_like(bufs[0]), torch.empty_like(bufs[1]), torch.zeros(1, device=d)
    names = D.launched_kernels(lambda: call("mvk_conv4s2_small_up_fwd_nll_sy", ptr(Vd), ptr(Wd), ptr(bd), ptr(Xd), xrows, NLL_SCALE, NLL_GW,
                                            ptr(dpre), ptr(rows), n, 16, 16, 3, 32, SIGMOID, ptr(amax), ptr(pub), stream_ptr()))
    assert names == [K_FWD_H_NLL]
    assert torch.equal(dpre, bufs[0]) and torch.equal(rows, bufs[1])
    assert float(dpre.abs().max()) <= float(pub) <= 64.0 * float(dpre.abs().max())


def cin_blocks(npos):
    """(blocks, pos_per_block) of smallcin_wgrad (smallcin.hip): at most 1024 blocks, 64-position tiles."""
    blocks = min((npos + 255) // 256, 1024)
    ppb = (-(-npos // blocks) + 63) // 64 * 64
    return -(-npos // ppb), ppb


BLOCKCAP = dict(n=1030, h=16, w=16, Cu=3, Cv=32)  # 263680 positions > 1024 blocks of 256: 824 blocks of 320 positions


def blockcap_refs(want_h=False):
    """Operands, initial dW and the float64 slab references of the block-cap case (shared with the host test)."""
    c = BLOCKCAP
    U, dV, init = R.wgrad_operands(1030, c["n"], c["h"], c["w"], c["Cu"], c["Cv"])
    nb, ppb = cin_blocks(c["n"] * c["h"] * c["w"])
    return U, dV, init, nb, ppb, R.wgrad_blocks(U, dV, ppb, want_h=want_h)


def test_cin_wgrad_block_cap():
    """smallcin_wgrad above its 1024-block cap (pos_per_block = 320 > 256).  A 263680-term sum leaves a per-entry bound without teeth
    (the roundings of 16-bit operands average out to 0.08x C_ENTRY * bound) and torch's fp32 GEMM of that length is no yardstick
    either (measured: max error 1.1e-4 against the kernel's 2.9e-6 and the two-piece emulation's 3.7e-5).  So the launch is checked
    at the two levels it computes, each a chain of <= 1024 terms:
      1. every entry of every workgroup's slab (read back from the scratch) against the float64 sum over that workgroup's 320
         positions, at C_ENTRY * sum |u dv|: the two-piece emulation must leave this bound;
      2. dW - initial against the float64 sum of the kernel's OWN fp32 slabs, at C_ENTRY * (sum |slab| + |initial|) (a plain
         825-term sum: no products, so no operand emulation applies);
    plus the end-to-end result at C_ENTRY * bound and criterion (b) of the GEMM table, the exact kernel set, and bit-identity."""
    from multivae_amd._lib import call, ptr, stream_ptr

    c = BLOCKCAP
    n, h, w, Cu, Cv = c["n"], c["h"], c["w"], c["Cu"], c["Cv"]
    U, dV, init, nb, ppb, blk = blockcap_refs()
    assert (nb, ppb) == (824, 320)
    d = D.dev()
    Ud, dVd = U.to(d), D._nhwc(dV).to(d)
    ws = D._ws()
    nout = 16 * Cu * Cv

    def launch():
        dW = init.to(d)
        ws[:nb * nout].fill_(float("nan"))
        names = D.launched_kernels(lambda: call("mvk_conv4s2_wgrad", ptr(Ud), ptr(dVd), ptr(dW), n, h, w, Cu, Cv, 1, None, NONE, ptr(ws),
                                                ws.numel(), stream_ptr()))
        return names, dW, ws[:nb * nout].view(nb, 16 * Cu, Cv).clone()

    names, dW, slabs = launch()
    assert names == sorted([k_cin_wgrad(Cu, Cv), D.RED])
    s64 = slabs.double().cpu()
    assert bool(torch.isfinite(s64).all())
    tol = D.C_ENTRY * blk.bound + 1e-30
    worst, deg = float(((s64 - blk.ref).abs() / tol).max()), float(((blk.deg2 - blk.ref).abs() / tol).max())
    print(f"slabs: worst {worst:.3f}x the bound, two-piece {deg:.2f}x")
    assert worst <= 1.0 and deg > 1.0
    got = dW.double().cpu() - init.double()
    own = R.slabs_to_ref_layout(s64, Cu, Cv)
    tol2 = D.C_ENTRY * (R.slabs_to_ref_layout(s64.abs(), Cu, Cv) + init.double().abs())
    r2 = float(((got - own).abs() / tol2).max())
    ref, bound = R.slabs_to_ref_layout(blk.ref, Cu, Cv), R.slabs_to_ref_layout(blk.bound, Cu, Cv) + init.double().abs()
    r3 = float(((got - ref).abs() / (D.C_ENTRY * bound)).max())
    print(f"slab sum: worst {r2:.3f}x its bound; end to end {r3:.4f}x C_ENTRY * bound")
    assert r2 <= 1.0 and r3 <= 1.0
    torch.backends.cuda.matmul.allow_tf32 = False
    cols = F.unfold(Ud, 4, padding=1, stride=2).transpose(1, 2).reshape(n * h * w, Cu * 16)
    yard = (dVd.reshape(n * h * w, Cv).t() @ cols).view(Cv, Cu, 4, 4).double().cpu()
    e = [(x - ref).abs() for x in (got, yard)]
    mx, rms = [float(x.max()) for x in e], [float(x.pow(2).mean().sqrt()) for x in e]
    print(f"(b): max {mx}, rms {rms} (kernel, torch fp32)")
    assert mx[0] <= 2 * mx[1] and rms[0] <= 2 * rms[1]
    names2, dW2, slabs2 = launch()
    assert torch.equal(dW, dW2) and torch.equal(slabs, slabs2)


# ---- activations ---------------------------------------------------------------------------------------------------------------
def _launch_act(kind, Cu, Cv, h, w, n, act, seed=5):
    """The layer's output with activation `act` from fixed operands (kind: 'up', 'down', 'cin')."""
    from multivae_amd import kernels as KK
    from multivae_amd._lib import call, ptr, stream_ptr

    d = D.dev()
    if kind in ("up", "ups"):
        V, W, b = R.up_operands(seed, n, h, w, Cu, Cv)
        Vd, Wd, bd = D._nhwc(V).to(d), W.to(d), b.to(d)
        out = torch.full((n, Cu, 2 * h, 2 * w), float("nan"), device=d)
        if kind == "ups":  # scaled fp16 pairs (small_up_fwd_h_kernel)
            amax = Vd.abs().max().reshape(1)
            call("mvk_conv4s2_small_up_fwd_s", ptr(Vd), ptr(Wd), ptr(bd), ptr(out), n, h, w, Cu, Cv, act, ptr(amax), stream_ptr())
        else:
            call("mvk_conv4s2_small_up_fwd", ptr(Vd), ptr(Wd), ptr(bd), ptr(out), n, h, w, Cu, Cv, act, stream_ptr())
    else:
        U, W, b = R.down_operands(seed, n, h, w, Cu, Cv)
        Ud, bd = U.to(d), b.to(d)
        wdown, _ = KK.pack_conv(W.to(d), want_up=False)
        out = torch.full((n, h, w, Cv), float("nan"), device=d)
        wsp, wsn = D.WS("ws")
        call("mvk_conv4s2_down", ptr(Ud), ptr(wdown), ptr(bd), ptr(out), n, h, w, Cu, Cv, act, 1, None, NONE, None, NONE, None, wsp,
             wsn, 0, None, stream_ptr())
    torch.cuda.synchronize()
    return out


def _ulps(got, ref64):
    """|got - ref| in units of the fp32 spacing at |ref| (ref in float64)."""
    ulp = torch.exp2(torch.floor(torch.log2(ref64.abs().clamp_min(2.0 ** -126))) - 23)
    return float(((got.double() - ref64).abs() / ulp).max())


ACT_SHAPES = [("up", 1, 16, 8, 8, 3), ("up", 4, 64, 16, 16, 1), ("up", 2, 32, 12, 16, 2), ("down", 3, 32, 16, 16, 2),
              ("down", 2, 64, 4, 16, 3), ("cin", 3, 32, 20, 20, 1), ("cin", 1, 16, 6, 8, 3), ("up", 3, 32, 16, 16, 2),
              ("ups", 3, 32, 16, 16, 2)]  # the last two: small_up_fwd_bf_kernel, small_up_fwd_h_kernel (mvk_fast_sigmoid)


@pytest.mark.parametrize("kind,Cu,Cv,h,w,n", ACT_SHAPES)
def test_activations(kind, Cu, Cv, h, w, n):
    """ReLU / LeakyReLU: bit-identical to act(output with act = 0).  Sigmoid: against the float64 sigmoid of the kernel's own fp32
    pre-activation, within 2x the largest ulp error of torch.sigmoid (fp32, GPU) on the same tensor, at least 1 ulp.
    Measured on an MI355X: 1.74 - 2.04 ulp for both where the kernel evaluates 1 / (1 + expf(-v)) (bit-identical to torch),
    2.11 against 1.80 for mvk_fast_sigmoid (small_up_fwd_h_kernel)."""
    pre = _launch_act(kind, Cu, Cv, h, w, n, NONE)
    assert bool(torch.isfinite(pre).all())
    assert torch.equal(_launch_act(kind, Cu, Cv, h, w, n, RELU), pre.clamp_min(0))
    assert torch.equal(_launch_act(kind, Cu, Cv, h, w, n, LEAKY), torch.where(pre > 0, pre, R.F02 * pre))
    ref = torch.sigmoid(pre.double())
    mine, yard = _ulps(_launch_act(kind, Cu, Cv, h, w, n, SIGMOID), ref), _ulps(torch.sigmoid(pre), ref)
    print(f"sigmoid ulp: kernel {mine:.3f}, torch fp32 {yard:.3f}")
    assert mine <= max(2 * yard, 1.0), (mine, yard)


# ---- bit identities of the down layer's entries --------------------------------------------------------------------------------
@pytest.mark.parametrize("Cu,Cv", PAIRS)
def test_down_entries_bit_identical(Cu, Cv):
    """mvk_conv4s2_small_down_fwd (packed weight), _fwd_wref (reference layout, transposed while staged) and the routing through
    mvk_conv4s2_down(u_nchw = 1) give the same bits: the same kernel on the same LDS image of the weight."""
    h, w = OTHER[(Cu + Cv // 16) % 5]
    outs = []
    for entry in ("fwd", "wref", "route"):
        p = p_down_fwd(99 + Cu, 3, h, w, Cu, Cv, entry=entry)
        bufs, run = D.execute(p)
        assert D.launched_kernels(run) == [k_down(Cu, Cv)]
        outs.append(bufs[0])
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


# ---- the shape gate ------------------------------------------------------------------------------------------------------------
def test_shape_gate():
    """supported() takes h, w <= 16 only, and the small entry points refuse what it refuses."""
    from multivae_amd import _lib
    from multivae_amd._lib import MvkError, call, ptr, stream_ptr

    sup = _lib.load().mvk_conv4s2_small_up_supported
    for h, w in [(4, 64), (2, 128), (32, 8), (64, 4), (8, 32), (1, 256), (1, 64)]:
        assert sup(h, w, 3, 32) == 0, (h, w)
    for h, w in OTHER + [(16, 16), (16, 4), (16, 12)]:
        assert sup(h, w, 3, 32) == 1, (h, w)
    d = D.dev()
    n, h, w, Cu, Cv = 1, 4, 64, 3, 32
    V, U, W = torch.zeros(n, h, w, Cv, device=d), torch.zeros(n, Cu, 2 * h, 2 * w, device=d), torch.zeros(Cv, Cu, 4, 4, device=d)
    wsp, wsn = D.WS("ws")
    with pytest.raises(MvkError):
        call("mvk_conv4s2_small_up_fwd", ptr(V), ptr(W), None, ptr(U), n, h, w, Cu, Cv, NONE, stream_ptr())
    with pytest.raises(MvkError):
        call("mvk_conv4s2_small_down_fwd", ptr(U), ptr(W), None, ptr(V), n, h, w, Cu, Cv, NONE, stream_ptr())
    with pytest.raises(MvkError):
        call("mvk_conv4s2_small_down_fwd_wref", ptr(U), ptr(W), None, ptr(V), n, h, w, Cu, Cv, NONE, stream_ptr())
    with pytest.raises(MvkError):
        call("mvk_conv4s2_small_up_bwd", ptr(U), ptr(U), SIGMOID, ptr(V), RELU, ptr(W), ptr(torch.zeros_like(V)), ptr(torch.zeros_like(W)),
             None, None, wsp, wsn, n, h, w, Cu, Cv, stream_ptr())
