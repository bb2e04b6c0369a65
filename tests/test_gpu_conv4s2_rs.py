"""The register-stationary 4x4 / stride-2 kernels (csrc/imgconv.hip: imgconv_kernel, imgwgrad_kernel), leaf by leaf, against float64.

The machinery is that of tests/test_gpu_gemm_dispatch.py (imported as D: launched_kernels, Prep, Out, execute, check_case, Case,
C_ENTRY); the references, bounds, degraded emulations and the restated host arithmetic are tests/conv4s2_rs_ref.py, and
tests/test_conv4s2_rs_ref_host.py shows on the CPU, for every case of CASES, that the case's degraded emulation leaves its
tolerance, that a float32 CPU convolution stays inside it and that the case's named regime is the one its batch produces.  Each case

1. names its entry point and the exact set of device kernels it must launch (torch.profiler);
2. compares EVERY entry of every output of every image with float64: |got - ref| <= C_ENTRY * (sum |a b| + |bias| + |initial|),
   C_ENTRY = 5e-7, plus 2^-39 of the operand bounds per product in the scaled-fp16 form;
3. carries the degraded emulation of its form (bf16 pieces: two pieces per operand; scaled fp16: hi lo' dropped), which must FAIL
   that check;
4. runs twice from the same buffers and must be bit-identical (column sums and weight-gradient slabs are summed in a fixed order);
   deferred cases leave mvk_defer_pending() = 0 behind the flush; scaled cases publish max |stored output| bit for bit.

Cases run under mvk_debug_set_flags(0x200) (the kernels take every batch), the threshold cases under flags 0.  A regime is the set
of 32-row tiles per worker present in the launch (conv4s2_rs_ref.regime): 0 = an idle worker, 1 = drain only, 2 = one placeholder
tile, >= 3 = the steady two-tile-latency loop.  8x8: 256 workers, two tiles per image; 4x4: 64 workers of 4 workgroup types under
the XCD remap of blockIdx, one tile per two images.

Chain lengths (basis of C_ENTRY: <= 1024 terms per fp32 accumulator chain):
  imgconv_kernel   16 k-steps of 16 per wave, alternating between two MFMA accumulators (bf16 pieces: 6 piece products per
                   product; scaled fp16: a main and a cross accumulator), then the ordered sum over the KSPLIT <= 4 waves of a tile;
                   column sums: one fma chain per lane over the worker's tiles, then an ordered sum over <= 256 partial rows
  imgwgrad_kernel  one accumulator per entry over the worker's images x h x h pixels: 64 (n = 4 at 8x8) .. 256 (n = 1024 at 8x8),
                   32 (n = 4 at 4x4) .. 512 (n = 2048 at 4x4; stated per case), then the ordered sum of 256 / 64 slabs.  The workload's
                   batch (5120 images) gives chains of 1280 at 8x8 and 1280 at 4x4: longer than this table reaches.
  tiled engine     the declined cases: K = 16 Cu or 4 Cv in one chain, weight gradients in split-K slices.

Worst measured |got - ref| / tolerance over the table on an MI355X (per case, with the commit: profiles/NOTES_imgconv.md; in
brackets the ratio of the case's degraded emulation at that case): imgconv_kernel on bf16 pieces 0.33 (5.7), on scaled fp16 0.30
(374.0); imgwgrad_kernel<.., 3> 0.41 (8.4), <.., 2> 0.41 (555.6); the tiled engine's declined launches 0.70 (2.8).  Column sums stay
below 0.03 and do not reject 16-bit operands on their own: a case is rejected through its products (weakest rejection of the table:
1.31x, wgrad-8x8-bf-imgs-n1024-chain256).  With the down layer's batch gate of csrc/igemm.hip inverted by hand, both
gate-down-8x8 cases fail on the kernel set alone (their results stay right).

Leaves of this file NOT reachable here: MVK_IMGCONV (the batch threshold), MVK_IMGCONV_PIPE=0 (the one-tile-latency loop, PIPE =
false), MVK_IMGWGRAD_GRID (a smaller weight-gradient grid, which also leaves the XCD remap) and MVK_IMGWGRAD_MIN are read once per
process under MVK_TUNE; MVK_IC_DEPTH2 and MVK_ICPROF are compile-time.  The tests use the debug flags 0x100 / 0x200 instead.
"""
import zlib

import pytest
import torch

import conv4s2_rs_ref as R
import test_gpu_gemm_dispatch as D

pytestmark = pytest.mark.gpu

NONE, RELU, SIGMOID, LEAKY = R.NONE, R.RELU, R.SIGMOID, R.LEAKY
TAKE = 0x200  # mvk_debug_set_flags: the register-stationary 4x4/stride-2 kernels take every batch size
P8, P4 = R.PAIRS
FROW, FCOL = D.fast(64, 64, 32, "ROW", "N"), D.fast(64, 64, 32, "COL", "N")
FORMS = dict(plain=dict(bias=True, act=RELU, mask=None, colsum=False),      # the forward layer
             nobias=dict(bias=False, act=NONE, mask=None, colsum=False),
             maskcs=dict(bias=False, act=NONE, mask=RELU, colsum=True),     # backward data: x ReLU'(saved output), bias gradient
             nonemask=dict(bias=True, act=RELU, mask=NONE, colsum=False))   # a source with act none: HAS_SRC = true, x 1
LOOSE = (3.7, 5.3)  # operand bounds this many times the true maxima (no powers of two)


def _out(r, scaled, lay=lambda t: t, init=None, shape=None):
    """D.Out of a Ref; deg = the emulation of the case's form (deg2 / degh keep both for the host test)."""
    bound = lay(r.bound) if init is None else lay(r.bound) + init.double().abs()
    o = D.Out(lay(r.ref), bound, lay(r.degh if scaled else r.deg2), init=init, shape=shape)
    o.deg2, o.degh = lay(r.deg2), None if r.degh is None else lay(r.degh)
    return o


def _scratch(ws):
    """(pointer, floats): 'ws' ample, 'none' NULL, or a number of floats of the ample buffer."""
    if isinstance(ws, int):
        return D.WS("ws")[0], ws
    return D.WS(ws)


def p_fwd(seed, kind, n, pair, w=None, form="plain", scaled=False, data="unit", loose=None, yam_only=False, deferred=False,
          flags=TAKE, act=None, mask=None, off=False, u_nchw=False, ws="ws", frag=True, host=False):
    """mvk_conv4s2_down / _up (scaled or yam_only: _down_s / _up_s): out = act(conv(x) + bias) * mask'(source) in NHWC, column sums
    into an accumulator that starts non-zero.  act / mask override the form's; off: x at storage offset 1; u_nchw: NCHW destination
    of up; loose = (x, w) factors on the operand bounds; frag = False passes wfrag = NULL."""
    h, Cu, Cv = pair
    w = h if w is None else w
    f = dict(FORMS[form])
    if act is not None:
        f["act"] = act
    if mask is not None:
        f["mask"] = mask
    up = kind == "up"
    cout = Cu if up else Cv
    x, W, b, src, cinit = R.fwd_operands(seed, kind, n, h, w, Cu, Cv, data=data)
    b = b if f["bias"] else None
    has_src = f["mask"] is not None
    xb, wb = float(x.abs().max()) * (loose or (1, 1))[0], float(W.abs().max()) * (loose or (1, 1))[1]
    r = R.conv_fwd(kind, x, W, b, act=f["act"], mask_src=src if has_src else None, mask_act=f["mask"] or NONE, colsum=f["colsum"],
                   floor_bounds=(xb, wb) if scaled else None, want_h=scaled or host)
    lay = (lambda t: t) if u_nchw else (lambda t: t.permute(0, 2, 3, 1))
    oh, ow = (2 * h, 2 * w) if up else (h, w)
    outs = [_out(r["y"], scaled, lay, shape=(n, cout, oh, ow) if u_nchw else (n, oh, ow, cout))]
    if f["colsum"]:
        outs.append(_out(r["colsum"], scaled, init=cinit))
    if host:
        y32 = R.cpu_fp32(kind, x, W, b, f["act"], src if has_src else None, f["mask"] or NONE)
        outs[0].cpu = lay(y32.double())
        if f["colsum"]:
            outs[1].cpu = y32.sum((0, 2, 3)).double()
        return D.Prep(None, outs, deferred=deferred, flags=flags)
    from multivae_amd import kernels as KK
    from multivae_amd._lib import call, ptr, stream_ptr

    d = D.dev()
    wd, wu = KK.pack_conv(W.to(d))
    Wp = wu if up else wd
    fr = KK.wfrag(Wp) if frag else None
    Xd = D.unaligned(D._nhwc(x).to(d)) if off else D._nhwc(x).to(d)
    bd = None if b is None else b.to(d)
    sd = None if not has_src else (src.to(d) if u_nchw else D._nhwc(src).to(d))
    xam, wam, yam = torch.full((1,), xb, device=d), torch.full((1,), wb, device=d), torch.zeros(1, device=d)
    wsp, wsn = _scratch(ws)

    def run(bufs):
        cs = ptr(bufs[1]) if f["colsum"] else None
        dims = (n, h, w, Cu, Cv)
        amax = (ptr(xam), ptr(wam), ptr(yam)) if scaled else (None, None, ptr(yam))
        if up and (scaled or yam_only):
            call("mvk_conv4s2_up_s", ptr(Xd), ptr(Wp), ptr(bd), ptr(bufs[0]), *dims, f["act"], ptr(sd), f["mask"] or NONE, cs, *amax,
                 wsp, wsn, ptr(fr), stream_ptr())
        elif up:
            call("mvk_conv4s2_up", ptr(Xd), ptr(Wp), ptr(bd), ptr(bufs[0]), *dims, f["act"], int(u_nchw), ptr(sd), f["mask"] or NONE,
                 cs, wsp, wsn, 0, ptr(fr), stream_ptr())
        elif scaled or yam_only:
            call("mvk_conv4s2_down_s", ptr(Xd), ptr(Wp), ptr(bd), ptr(bufs[0]), *dims, f["act"], ptr(sd), f["mask"] or NONE, cs,
                 *amax, wsp, wsn, ptr(fr), stream_ptr())
        else:
            call("mvk_conv4s2_down", ptr(Xd), ptr(Wp), ptr(bd), ptr(bufs[0]), *dims, f["act"], 0, None, NONE, ptr(sd),
                 f["mask"] or NONE, cs, wsp, wsn, 0, ptr(fr), stream_ptr())

    p = D.Prep(run, outs, deferred=deferred, flags=flags, keep=[Xd, wd, wu, fr, bd, sd, xam, wam, yam])
    p.yam = yam if (scaled or yam_only) else None
    return p


def p_wgrad(seed, n, pair, w=None, scaled=False, data="unit", loose=None, deferred=False, flags=TAKE, ws="ws", host=False):
    """mvk_conv4s2_wgrad (scaled: _wgrad_s): dW [Cv][Cu][4][4] += d/dW sum(conv(U, W) dV), into a gradient that starts non-zero.
    Products per accumulator chain (conv4s2_rs_ref.wgrad_chain, in every case id): 8x8 n = 4: 64, 300: 128, 1024: 256; 4x4 n = 4:
    32, 130: 64, 2048: 512; then 256 / 64 slabs in order.  The workload's batch of 5120 images gives chains of 1280: longer than
    the table reaches."""
    h, Cu, Cv = pair
    w = h if w is None else w
    U, dV, init = R.wgrad_operands(seed, n, h, w, Cu, Cv, data=data)
    ub, vb = float(U.abs().max()) * (loose or (1, 1))[0], float(dV.abs().max()) * (loose or (1, 1))[1]
    r = R.conv_wgrad(U, dV, floor_bounds=(ub, vb) if scaled else None, want_h=scaled or host)
    outs = [_out(r, scaled, init=init)]
    if host:
        outs[0].cpu = R.cpu_fp32_wgrad(U, dV, pair).double()
        return D.Prep(None, outs, deferred=deferred, flags=flags)
    from multivae_amd._lib import call, ptr, stream_ptr

    d = D.dev()
    Ud, Vd = D._nhwc(U).to(d), D._nhwc(dV).to(d)
    uam, vam = torch.full((1,), ub, device=d), torch.full((1,), vb, device=d)
    wsp, wsn = _scratch(ws)

    def run(bufs):
        if scaled:
            call("mvk_conv4s2_wgrad_s", ptr(Ud), ptr(Vd), ptr(bufs[0]), n, h, w, Cu, Cv, ptr(uam), ptr(vam), wsp, wsn, stream_ptr())
        else:
            call("mvk_conv4s2_wgrad", ptr(Ud), ptr(Vd), ptr(bufs[0]), n, h, w, Cu, Cv, 0, None, NONE, wsp, wsn, stream_ptr())

    p = D.Prep(run, outs, deferred=deferred, flags=flags, keep=[Ud, Vd, uam, vam])
    p.yam = None
    return p


def case(id_, fn, kw, expect, note="", regime=None):
    seed = zlib.crc32(id_.encode()) % 100003

    def make():
        p = fn(seed, **kw)
        if p.deferred:  # the arena grows between scopes to what the last one asked for: a first step sizes it
            _, prime = D.execute(p)
            prime()
            torch.cuda.synchronize()
        c.last = p
        return p

    c = D.Case(id_, make, tuple(sorted(expect)), None, note)
    c.host = lambda: fn(seed, host=True, **kw)
    c.kw, c.regime, c.fn, c.last = kw, regime, fn, None
    return c


def _pname(pair):
    return f"{pair[0]}x{pair[0]}"


CASES = []

# ---- forward and backward data on bf16 pieces (NP = 3): every regime of every (pair, direction), the forms in rotation ----------------------
FWD_BF = {
    (P8, "down"): [(1, "maskcs"), (256, "plain"), (300, "nonemask"), (768, "nobias")],
    (P8, "up"): [(1, "nobias"), (256, "nonemask"), (300, "maskcs-deferred"), (768, "plain")],
    (P4, "down"): [(2, "plain"), (128, "nobias"), (130, "maskcs-deferred"), (256, "nonemask"), (384, "plain"), (700, "maskcs")],
    (P4, "up"): [(2, "maskcs"), (128, "nonemask"), (130, "nobias"), (256, "plain"), (384, "maskcs-deferred"), (700, "nobias")],
}
# ---- the scaled form (NP = 2): (n, form, operands) -----------------------------------------------------------------------------------------
FWD_FP = {
    (P8, "down"): [(1, "plain", "unit"), (256, "nobias", "tiny"), (300, "maskcs", "spread"), (768, "nonemask", "loose")],
    (P8, "up"): [(1, "maskcs-deferred", "unit"), (256, "nonemask", "loose"), (300, "nobias", "tiny"), (768, "plain", "spread")],
    (P4, "down"): [(2, "nobias", "tiny"), (130, "maskcs-deferred", "unit"), (384, "plain", "loose"), (700, "nonemask", "spread")],
    (P4, "up"): [(2, "maskcs", "loose"), (256, "nonemask", "spread"), (384, "plain", "tiny"), (700, "nobias", "unit")],
}


def _fwd_case(pair, kind, n, form, np_, data="unit", **extra):
    deferred = form.endswith("-deferred")
    form = form.split("-")[0]
    f = FORMS[form]
    kw = dict(kind=kind, n=n, pair=pair, form=form, scaled=np_ == 2, deferred=deferred, **extra)
    if data == "loose":
        kw.update(loose=LOOSE)
    elif data != "unit":
        kw.update(data=data)
    exp = [R.kernel_name(kind, pair, f["mask"] is not None, 2 if kw["scaled"] else 3)]
    if f["colsum"]:
        exp.append(D.BATCH if deferred else D.FIN)
    tag = "fp" if np_ == 2 else "bf"
    tag += "" if data == "unit" else f"-{data}"
    tag += "-yamonly" if extra.get("yam_only") else ""
    tag += "-nofrag" if extra.get("frag") is False else ""
    reg = R.regime(n, kind, pair)
    name = f"{kind}-{_pname(pair)}-{tag}-{form}{'-deferred' if deferred else ''}-n{n}-tpw{'_'.join(map(str, sorted(reg)))}"
    return case(name, p_fwd, kw, exp, regime=reg)


for (_pair, _kind), _rows in FWD_BF.items():
    CASES += [_fwd_case(_pair, _kind, _n, _form, 3) for _n, _form in _rows]
for (_pair, _kind), _rows in FWD_FP.items():
    CASES += [_fwd_case(_pair, _kind, _n, _form, 2, _data) for _n, _form, _data in _rows]
# y_amax alone: the bf16-piece kernel runs and publishes
CASES.append(_fwd_case(P8, "down", 256, "plain", 3, yam_only=True))
CASES.append(_fwd_case(P4, "up", 130, "maskcs", 3, yam_only=True))
# wfrag = NULL: the in-kernel split of the fp32 pack, per entry (test_weight_routes holds it to the fragment route bit for bit)
CASES.append(_fwd_case(P8, "up", 300, "plain", 3, frag=False))
CASES.append(_fwd_case(P4, "down", 130, "nonemask", 3, frag=False))

# ---- weight gradient: (pair, n, scaled, deferred, operands) ---------------------------------------------------------------------------------
WG = [
    (P8, 4, False, False, "unit"), (P8, 300, False, True, "imgs"), (P8, 1024, False, False, "imgs"),
    (P8, 4, True, True, "spread"), (P8, 300, True, False, "spread"), (P8, 1024, True, True, "spread"),
    (P4, 4, False, True, "unit"), (P4, 130, False, False, "unit"), (P4, 2048, False, True, "imgs"),
    (P4, 4, True, False, "spread"), (P4, 130, True, True, "spread"), (P4, 2048, True, False, "spread"),
]
for _pair, _n, _sc, _df, _data in WG:
    _kw = dict(n=_n, pair=_pair, scaled=_sc, deferred=_df)
    if _data != "unit":
        _kw.update(data=_data)
    if _sc:
        _kw.update(loose=LOOSE)
    CASES.append(case(f"wgrad-{_pname(_pair)}-{'fp-loose' if _sc else 'bf'}-{_data}-n{_n}{'-deferred' if _df else ''}"
                      f"-chain{R.wgrad_chain(_n, _pair)}", p_wgrad, _kw,
                      [R.wgrad_kernel_name(_pair, 2 if _sc else 3), D.BATCH if _df else D.RED],
                      f"{R.wgrad_chain(_n, _pair)} products per accumulator chain, {R.workers('wgrad', _pair)} slabs",
                      regime=dict(chain=R.wgrad_chain(_n, _pair))))

# ---- gates: the batch thresholds under flags 0 -----------------------------------------------------------------------------------------------
CASES += [
    case("gate-down-8x8-n256-taken", p_fwd, dict(kind="down", n=256, pair=P8, flags=0), [R.kernel_name("down", P8, False, 3)],
         "n >= imgconv_min_images() = 256", regime={2}),
    case("gate-down-8x8-n255-tiled", p_fwd, dict(kind="down", n=255, pair=P8, flags=0), [FROW], "n = 255: tiled engine, 128 blocks"),
    case("gate-up-4x4-n256-taken", p_fwd, dict(kind="up", n=256, pair=P4, flags=0), [R.kernel_name("up", P4, False, 3)], regime={2}),
    case("gate-up-4x4-n254-tiled", p_fwd, dict(kind="up", n=254, pair=P4, flags=0), [FROW], "even, below the threshold"),
    case("gate-wgrad-8x8-n1024-taken", p_wgrad, dict(n=1024, pair=P8, flags=0, data="imgs"), [R.wgrad_kernel_name(P8, 3), D.RED],
         "n / 4 >= 256", regime=dict(chain=256)),
    case("gate-wgrad-8x8-n1023-tiled", p_wgrad, dict(n=1023, pair=P8, flags=0, data="imgs"), [D.bf(128, 64, "COL", "N"), D.RED],
         "n / 4 = 255: split K on the tiled engine, 4 tiles x 64 slices"),
    # ---- declines under 0x200: the tiled engine, with a right result ----------------------------------------------------------------------------
    case("decline-down-4x4-n129-odd", p_fwd, dict(kind="down", n=129, pair=P4), [FROW], "4x4 stages two images per unit: odd n"),
    case("decline-up-4x4-n129-odd", p_fwd, dict(kind="up", n=129, pair=P4, form="nobias"), [FROW]),
    case("decline-down-8x4-n6", p_fwd, dict(kind="down", n=6, pair=P8, w=4), [FROW], "h != w"),
    case("decline-up-8x4-n6", p_fwd, dict(kind="up", n=6, pair=P8, w=4), [D.bf(128, 32, "ROW", "N")], "h != w"),
    case("decline-down-8x8-n6-unaligned", p_fwd, dict(kind="down", n=6, pair=P8, off=True), [D.gen(128, 64)],
         "input at storage offset 1: no 16-byte loads -> generic kernel"),
    case("decline-up-8x8-n6-unaligned", p_fwd, dict(kind="up", n=6, pair=P8, off=True), [D.gen(128, 32)]),
    case("decline-down-8x8-n6-leaky", p_fwd, dict(kind="down", n=6, pair=P8, act=LEAKY), [FROW], "act = LeakyReLU"),
    case("decline-up-4x4-n6-leakymask", p_fwd, dict(kind="up", n=6, pair=P4, form="maskcs", mask=LEAKY), [FROW, D.FIN],
         "mask of a LeakyReLU layer"),
    case("decline-up-4x4-n6-nchw", p_fwd, dict(kind="up", n=6, pair=P4, u_nchw=True), [FROW], "NCHW destination"),
    case("decline-wgrad-8x8-n64-shortscratch", p_wgrad, dict(n=64, pair=P8, ws=R.min_wgrad_scratch(P8) - 1, data="imgs"),
         [D.bf(128, 64, "COL", "N"), D.RED], "one float below 256 slabs, no arena"),
    case("decline-wgrad-4x4-n64-shortscratch", p_wgrad, dict(n=64, pair=P4, ws=R.min_wgrad_scratch(P4) - 1),
         [D.bf(128, 64, "COL", "N"), D.RED], "one float below 64 slabs, no arena"),
    case("decline-down-8x8-n6-colsum-shortscratch", p_fwd, dict(kind="down", n=6, pair=P8, form="maskcs", ws=256 * 64 - 1),
         [FROW, D.FIN], "one float below 256 partial rows"),
    case("decline-up-8x8-n6-colsum-shortscratch", p_fwd, dict(kind="up", n=6, pair=P8, form="maskcs", ws=256 * 32 - 1),
         [D.bf(128, 32, "ROW", "N"), D.FIN]),
    # ---- a decline AFTER the arena reservation: the tiled engine asks the arena again for the same output ----------------------------------------
    case("reserved-down-4x4-n5-colsum-deferred", p_fwd, dict(kind="down", n=5, pair=P4, form="maskcs", deferred=True), [FROW, D.BATCH]),
    case("reserved-up-4x4-n5-colsum-deferred", p_fwd, dict(kind="up", n=5, pair=P4, form="maskcs", deferred=True), [FROW, D.BATCH]),
    case("reserved-wgrad-4x4-n5-deferred", p_wgrad, dict(n=5, pair=P4, deferred=True), [FCOL, D.BATCH]),
    case("reserved-wgrad-8x4-n8-deferred", p_wgrad, dict(n=8, pair=P8, w=4, deferred=True), [FCOL, D.BATCH], "h != w"),
]
IDS = [c.id for c in CASES]


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_conv4s2_rs_leaf(c):
    from multivae_amd import _lib

    report = D.check_case(c, engine_f32=False)
    print(c.id, {k: v for k, v in report.items() if k != "kernels"})
    p = c.last
    if p.deferred:
        assert int(_lib.load().mvk_defer_pending()) == 0
    if p.yam is not None:  # the published maximum: bit for bit max |stored output|
        p.yam.zero_()
        bufs, run = D.execute(p)
        run()
        torch.cuda.synchronize()
        assert float(p.yam) == float(bufs[0].abs().max()) > 0


def test_case_ids_are_unique():
    assert len(IDS) == len(set(IDS))


# ---- the weight routes ----------------------------------------------------------------------------------------------------------------------
ROUTES = [(P8, "down", 300), (P8, "up", 300), (P4, "down", 130), (P4, "up", 130)]


@pytest.mark.parametrize("pair,kind,n", ROUTES, ids=[f"{k}-{_pname(p)}" for p, k, _ in ROUTES])
def test_weight_routes(pair, kind, n):
    """bf16 form: wfrag = NULL (the in-kernel split of the fp32 pack) is bit-identical to the fragment pack of the same weights; and a
    launch given the fp32 pack of weights A with the fragment pack of weights B computes B's layer (inside B's tolerance on every
    entry, outside A's): the fragment route is the one that ran."""
    from multivae_amd import kernels as KK
    from multivae_amd._lib import call, ptr, stream_ptr

    h, Cu, Cv = pair
    up = kind == "up"
    xA, WA, b, _, _ = R.fwd_operands(31, kind, n, h, h, Cu, Cv)
    _, WB, _, _, _ = R.fwd_operands(32, kind, n, h, h, Cu, Cv)
    d = D.dev()
    packs = {k: KK.pack_conv(W.to(d))[1 if up else 0] for k, W in (("A", WA), ("B", WB))}
    Xd, bd = D._nhwc(xA).to(d), b.to(d)
    wsp, wsn = D.WS("ws")
    oshape = (n, 2 * h, 2 * h, Cu) if up else (n, h, h, Cv)
    name = R.kernel_name(kind, pair, False, 3)

    def launch(Wp, fr):
        out = torch.full(oshape, float("nan"), device=d)

        def go():
            if up:
                call("mvk_conv4s2_up", ptr(Xd), ptr(Wp), ptr(bd), ptr(out), n, h, h, Cu, Cv, NONE, 0, None, NONE, None, wsp, wsn, 0,
                     ptr(fr), stream_ptr())
            else:
                call("mvk_conv4s2_down", ptr(Xd), ptr(Wp), ptr(bd), ptr(out), n, h, h, Cu, Cv, NONE, 0, None, NONE, None, NONE, None,
                     wsp, wsn, 0, ptr(fr), stream_ptr())

        D._flags(TAKE)
        try:
            assert D.launched_kernels(go) == [name]
        finally:
            D._flags(0)
        return out

    with_frag = launch(packs["A"], KK.wfrag(packs["A"]))
    assert KK.wfrag(packs["A"]).numel() == R.frag_bytes(kind, pair)
    assert torch.equal(launch(packs["A"], None), with_frag), "wfrag = NULL differs from the fragment pack of the same weights"
    mixed = launch(packs["A"], KK.wfrag(packs["B"])).cpu().double().permute(0, 3, 1, 2)
    rA, rB = (R.conv_fwd(kind, xA, W, b, want_h=False)["y"] for W in (WA, WB))
    toB = float(((mixed - rB.ref).abs() / (D.C_ENTRY * rB.bound)).max())
    toA = float(((mixed - rA.ref).abs() / (D.C_ENTRY * rA.bound)).max())
    print(f"fp32 pack A + fragments B: {toB:.3f}x B's tolerance, {toA:.3g}x A's")
    assert toB <= 1.0 < toA


def test_frag_bytes():
    """mvk_imgconv_frag_bytes: non-zero for exactly the two covered channel pairs, where it is what the kernel reads (roles x 16
    k-steps x 3 pieces x 64 lanes x 16 bytes, the same for both directions)."""
    from multivae_amd import _lib

    lib = _lib.load()
    covered = {(Cu, Cv) for _, Cu, Cv in R.PAIRS}
    for Cu in (3, 16, 32, 64, 128):
        for Cv in (3, 32, 64, 128, 256):
            nb = int(lib.mvk_imgconv_frag_bytes(Cu, Cv))
            assert (nb != 0) == ((Cu, Cv) in covered), (Cu, Cv, nb)
    for pair in R.PAIRS:
        nb = int(lib.mvk_imgconv_frag_bytes(pair[1], pair[2]))
        assert nb == R.frag_bytes("down", pair) == R.frag_bytes("up", pair)


# ---- what the scaled entries refuse, and empty batches ----------------------------------------------------------------------------------------
def _raw_args(kind, n, pair, scaled_ptrs):
    """(entry name, argument tuple, output) of a _down_s / _up_s / _wgrad_s call with an all-NaN output."""
    from multivae_amd._lib import ptr, stream_ptr

    h, Cu, Cv = pair
    d = D.dev()
    m = max(n, 1)
    U, V = torch.randn(m, 2 * h, 2 * h, Cu, device=d), torch.randn(m, h, h, Cv, device=d)
    W = torch.randn(16 * Cu * Cv, device=d)
    one = torch.ones(1, device=d)
    wsp, wsn = D.WS("ws")
    am = [ptr(one) if s else None for s in scaled_ptrs]
    if kind == "wgrad":
        out = torch.full((Cv, Cu, 4, 4), float("nan"), device=d)
        return "mvk_conv4s2_wgrad_s", (ptr(U), ptr(V), ptr(out), n, h, h, Cu, Cv, am[0], am[1], wsp, wsn, stream_ptr()), out, (U, V, one)
    x, oshape = (V, (m, 2 * h, 2 * h, Cu)) if kind == "up" else (U, (m, h, h, Cv))
    out = torch.full(oshape, float("nan"), device=d)
    return (f"mvk_conv4s2_{kind}_s", (ptr(x), ptr(W), None, ptr(out), n, h, h, Cu, Cv, NONE, None, NONE, None, am[0], am[1], am[2], wsp,
                                      wsn, None, stream_ptr()), out, (x, W, one))


REFUSED = [  # (id, kind, n, pair, which amax pointers are given, flags)
    ("down-4x4-odd", "down", 129, P4, (1, 1, 1), TAKE), ("up-4x4-odd", "up", 129, P4, (1, 1, 1), TAKE),
    ("down-8x8-below-threshold", "down", 255, P8, (1, 1, 1), 0), ("up-4x4-below-threshold", "up", 254, P4, (1, 1, 1), 0),
    ("down-foreign-pair", "down", 256, (8, 64, 64), (1, 1, 1), TAKE), ("up-foreign-pair", "up", 256, (4, 32, 64), (1, 1, 1), TAKE),
    ("down-x-bound-alone", "down", 256, P8, (1, 0, 1), TAKE), ("up-w-bound-alone", "up", 256, P4, (0, 1, 1), TAKE),
    ("down-no-amax", "down", 256, P8, (0, 0, 0), TAKE), ("up-no-amax", "up", 256, P4, (0, 0, 0), TAKE),
    ("wgrad-4x4-odd", "wgrad", 129, P4, (1, 1), TAKE), ("wgrad-8x8-below-threshold", "wgrad", 1023, P8, (1, 1), 0),
    ("wgrad-foreign-pair", "wgrad", 1024, (8, 64, 64), (1, 1), TAKE), ("wgrad-u-bound-alone", "wgrad", 1024, P8, (1, 0), TAKE),
    ("wgrad-v-bound-alone", "wgrad", 1024, P8, (0, 1), TAKE),
]


@pytest.mark.parametrize("id_,kind,n,pair,given,flags", REFUSED, ids=[r[0] for r in REFUSED])
def test_scaled_entries_refuse(id_, kind, n, pair, given, flags):
    """MVK_EINVAL (-1), no launch, and the all-NaN output stays all NaN: no silent fall-back from the scaled entry points."""
    from multivae_amd import _lib

    lib = _lib.load()
    name, args, out, keep = _raw_args(kind, n, pair, given)
    rc = []
    D._flags(flags)
    try:
        if all(given) and len(given) == 3:
            ok = lib.mvk_conv4s2_scaled_ok(n, pair[0], pair[0], pair[1], pair[2])
            assert ok == 0, "the gate the caller asks first"
        if kind == "wgrad" and all(given):
            assert lib.mvk_conv4s2_wgrad_scaled_ok(n, pair[0], pair[0], pair[1], pair[2]) == 0
        names = D.launched_kernels(lambda: rc.append(getattr(lib, name)(*args)))
    finally:
        D._flags(0)
    assert rc == [-1] and names == []
    assert bool(torch.isnan(out).all())


@pytest.mark.parametrize("flags", [0, TAKE])
def test_empty_batch_launches_nothing(flags):
    """n = 0: every entry returns MVK_OK and launches nothing."""
    from multivae_amd import _lib
    from multivae_amd._lib import ptr, stream_ptr

    lib = _lib.load()
    calls, keep, rc = [], [], []
    for pair in R.PAIRS:  # (the buffers are made here: no torch kernel inside the profiled region)
        h, Cu, Cv = pair
        for kind in ("down", "up", "wgrad"):
            name, args, out, k = _raw_args(kind, 0, pair, (1, 1, 1)[:2 if kind == "wgrad" else 3])
            calls.append((name, args))
            keep.append((out, k))
        _, _, out, (x, W, one) = _raw_args("down", 0, pair, (0, 0, 0))
        keep.append((out, x, W))
        wsp, wsn = D.WS("ws")
        calls += [("mvk_conv4s2_down", (ptr(x), ptr(W), None, ptr(out), 0, h, h, Cu, Cv, NONE, 0, None, NONE, None, NONE, None, wsp, wsn, 0,
                                        None, stream_ptr())),
                  ("mvk_conv4s2_up", (ptr(x), ptr(W), None, ptr(out), 0, h, h, Cu, Cv, NONE, 0, None, NONE, None, wsp, wsn, 0, None,
                                      stream_ptr())),
                  ("mvk_conv4s2_wgrad", (ptr(x), ptr(x), ptr(out), 0, h, h, Cu, Cv, 0, None, NONE, wsp, wsn, stream_ptr()))]
    D._flags(flags)
    try:
        names = D.launched_kernels(lambda: rc.extend(getattr(lib, name)(*args) for name, args in calls))
    finally:
        D._flags(0)
    assert names == [] and rc == [0] * 12, (names, rc)
