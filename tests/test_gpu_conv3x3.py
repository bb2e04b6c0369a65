"""The 3x3 / stride-1 / pad-1 kernels (csrc/conv3small.hip, csrc/conv3rs.hip), leaf by leaf, against float64.

The machinery is that of tests/test_gpu_gemm_dispatch.py (imported as D: launched_kernels, Prep, Out, execute, check_case, C_ENTRY,
and the entry-point wrappers p_conv3 / p_conv3_wgrad); the references, bounds and degraded emulations are tests/conv3_ref.py, and
tests/test_conv3_ref_host.py shows on the CPU that both emulations leave the tolerance of every case of CASES and that every case
that names a regime of the position stream produces it.  Each case

1. names its entry point and the exact set of device kernels it must launch (torch.profiler);
2. compares EVERY entry of every output with float64: |got - ref| <= C_ENTRY * (sum |a b| + |bias| + |initial| ...), C_ENTRY = 5e-7;
3. carries the two-piece bf16 emulation of the same formula, which must FAIL that check;
4. runs twice from the same buffers and must be bit-identical (the one exception: the weight gradient that falls to the tiled
   engine's fp32-atomic split K when it has no scratch, held to the tolerance alone).

The table checks pre-activations (act = 0); test_activations holds ReLU / LeakyReLU outputs to act(pre-activation launch) BIT FOR
BIT and the sigmoid to the protocol of tests/test_gpu_conv4s2_small.py (float64 sigmoid of the kernel's own pre-activation, 2x the
largest ulp error of torch.sigmoid on the same tensor, at least 1 ulp).

Chain lengths (basis of C_ENTRY: <= 1024 terms per fp32 accumulator chain):
  conv3_smallcin_kernel     9 Cin <= 36 fma in one register
  conv3_smallcout_v_kernel  9 Cin fma in one register: 144 .. 2304 (Cin = 256: beyond the 1024 terms C_ENTRY was derived for)
  conv3_small_wgrad_kernel  per thread the positions of its position group (<= 8 W / PG per band, times the bands a workgroup takes),
                            then PG partial sums, then the ordered sum of <= 1024 slabs
  c3rs_kernel               18 k-steps of 16 per wave in two MFMA accumulators (288 terms each), then the Cin / 32 waves of a tile
  c3wg_kernel               32 positions per tile and MFMA accumulator over the worker's tiles, then the ordered sum of the workers
  tiled engine              K = 9 Cin in one chain (2304 at Cin = 256: tests/test_gpu_gemm_dispatch.py c3fwd-bf128x32-row-K2304)

Worst measured |got - ref| / tolerance over the table on an MI355X (per output and with the case: profiles/NOTES_conv3.md; in
brackets the two-piece ratio at that case): conv3_smallcin_kernel 0.54 (8.0), conv3_smallcout_v_kernel 0.75 (3.1; the 2304-term
chain of cout-256x2-3x70-n1), conv3_small_wgrad_kernel 0.23 (7.7; slabs of the grid-cap test 0.28 (14.8)), c3rs_kernel on bf16
pieces 0.27 (3.6), on scaled fp16 0.27 (4.2), its channel slices 0.20 (1.4), c3wg_kernel<3> 0.48 (12.7) / db 0.06, c3wg_kernel<2>
0.17 (4.4) / db 0.07, the tiled engine's fallbacks 0.67 (2.2).  Column sums and bias gradients stay below 0.16 and do not reject
16-bit operands on their own: a case is rejected through its products (weakest rejection of the table: 1.15x).

Leaves of this family NOT reachable here: MVK_CONV3SMALL=0 (the image-side shapes on the tiled engine) and MVK_C3RS=<tiles> (the
size threshold of the register-stationary kernels) are read once per process under MVK_TUNE; the tests use the debug flags 0x400 /
0x800 of mvk_debug_set_flags instead, and shapes the image-side kernels decline.
"""
import zlib

import pytest
import torch

import conv3_ref as R3
import test_gpu_gemm_dispatch as D

pytestmark = pytest.mark.gpu

NONE, RELU, SIGMOID, LEAKY = R3.NONE, R3.RELU, R3.SIGMOID, R3.LEAKY
RS, TILED = D.RS_ALL, D.TILED_ONLY
G32, FROW, FCOL = D.gen(128, 32), D.fast(64, 64, 32, "ROW", "N"), D.fast(64, 64, 32, "COL", "N")


def k_cin(cs):
    return f"conv3_smallcin_kernel<{cs}>"


def k_cout(cs):
    return f"conv3_smallcout_v_kernel<{cs}>"


def k_swg(cs):
    return f"conv3_small_wgrad_kernel<{cs}>"


def k_rs(cin, cout, src, res, np_, dual=False):
    return f"c3rs_kernel<{cin},{cout},{str(src).lower()},{str(res).lower()},{np_},{str(dual).lower()}>"


def k_wg(np_):
    return f"c3wg_kernel<{np_}>"


def case(id_, fn, kw, expect, note="", regime=None):
    seed = zlib.crc32(id_.encode()) % 100003
    c = D.Case(id_, lambda: fn(seed, **kw), tuple(sorted(expect)), None, note)
    c.host = lambda: fn(seed, host=True, **kw)
    c.kw, c.regime, c.fn = kw, regime, fn
    return c


def F_(n, H, W, Cin, Cout, **kw):
    return dict(n=n, H=H, W=W, Cin=Cin, Cout=Cout, **kw)


CASES = [
    # ---- conv3_smallcin_kernel<1..4>: a band of 8 rows per workgroup, thread = (4 output channels) x (position lane) ---------------
    case("cin-1x4-1x1-n3", D.p_conv3, F_(3, 1, 1, 1, 4), [k_cin(1)], "1x1 map: the tile is all halo but one element; Cout = 4"),
    case("cin-2x12-8x5-n2-leakymask", D.p_conv3, F_(2, 8, 5, 2, 12, mask=LEAKY), [k_cin(2)],
         "one full band; Cout / 4 = 3 does not divide 256: lane 255 is idle"),
    case("cin-3x32-9x13-n2-relumask-colsum", D.p_conv3, F_(2, 9, 13, 3, 32, mask=RELU, colsum=True), [k_cin(3), D.CS4, D.FIN],
         "second band of one row; the column sums are a pass over Y"),
    case("cin-4x64-3x2-n1-nobias", D.p_conv3, F_(1, 3, 2, 4, 64, bias=False), [k_cin(4)], "6 positions for 16 position lanes"),
    case("cin-3x1024-9x3-n1-sigmoidmask", D.p_conv3, F_(1, 9, 3, 3, 1024, mask=SIGMOID), [k_cin(3)], "Cout = 1024: one position lane"),
    case("cin-1x32-2x256-n1", D.p_conv3, F_(1, 2, 256, 1, 32), [k_cin(1)], "W = 256: the widest map taken"),
    case("cin-4x12-17x7-n2-y", D.p_conv3, F_(2, 17, 7, 4, 12, entry="y", mask=RELU), [k_cin(4)], "mvk_conv3x3_y; three bands"),
    case("cin-3x64-8x8-n2-colsum-deferred", D.p_conv3, F_(2, 8, 8, 3, 64, bias=False, colsum=True, deferred=True),
         [k_cin(3), D.CS4, D.BATCH], "column-sum partials in the deferred arena"),
    case("cin-3x8-1x257-n1-tiled", D.p_conv3, F_(1, 1, 257, 3, 8), [G32], "W = 257: declined -> tiled engine, generic kernel (K = 27)"),
    case("cin-3x6-5x5-n2-tiled", D.p_conv3, F_(2, 5, 5, 3, 6), [G32], "Cout % 4 != 0: declined"),
    case("cin-3x32-5x5-n2-biasoff-tiled", D.p_conv3, F_(2, 5, 5, 3, 32, off="bias"), [G32], "bias not 16-byte aligned: declined"),
    case("cin-3x32-5x5-n2-yoff-tiled", D.p_conv3, F_(2, 5, 5, 3, 32, off="y"), [G32], "Y not 16-byte aligned: declined"),
    case("cin-3x32-5x5-n2-maskoff-tiled", D.p_conv3, F_(2, 5, 5, 3, 32, off="mask", mask=LEAKY), [G32], "mask source not aligned: declined"),
    # ---- conv3_smallcout_v_kernel<1..4>: 8 x 32 position tiles, 16 input channels per stage ----------------------------------------
    case("cout-16x1-8x32-n2", D.p_conv3, F_(2, 8, 32, 16, 1), [k_cout(1)], "exactly one tile per image; Cin = 16: one stage"),
    case("cout-48x3-9x33-n1-leakymask-colsum", D.p_conv3, F_(1, 9, 33, 48, 3, mask=LEAKY, colsum=True), [k_cout(3), D.CS1, D.FINS],
         "2 x 2 tiles, the second ones one row / one column; three stages"),
    case("cout-256x2-3x70-n1", D.p_conv3, F_(1, 3, 70, 256, 2, data="chan"), [k_cout(2)], "three column tiles; 2304 terms in one fp32 chain"),
    case("cout-16x4-1x1-n3-sigmoidmask", D.p_conv3, F_(3, 1, 1, 16, 4, mask=SIGMOID), [k_cout(4)], "1x1 map"),
    case("cout-32x4-5x40-n2-relumask-colsum", D.p_conv3, F_(2, 5, 40, 32, 4, bias=False, mask=RELU, colsum=True),
         [k_cout(4), D.CS4, D.FIN]),
    case("cout-24x3-5x5-n2-tiled", D.p_conv3, F_(2, 5, 5, 24, 3), [G32], "Cin % 16 != 0: declined; N = 3 -> generic"),
    case("cout-272x2-4x4-n1-tiled", D.p_conv3, F_(1, 4, 4, 272, 2, data="chan"), [G32], "Cin > 256: declined"),
    case("cout-16x3-5x5-n2-xoff-tiled", D.p_conv3, F_(2, 5, 5, 16, 3, off="x"), [G32], "X not 16-byte aligned: declined"),
    # ---- conv3_small_wgrad_kernel<1..4>: CB = the many-channel side, PG = 64 / (CB / 4) position groups ---------------------------
    case("swg-in-3x64-9x13-n2", D.p_conv3_wgrad, F_(2, 9, 13, 3, 64), [k_swg(3), D.FIN],
         "image = input; CB = 64: PG = 4 <= W: the single loop, W no multiple of PG", dict(loop="single", grid=4)),
    case("swg-in-1x4-8x64-n1", D.p_conv3_wgrad, F_(1, 8, 64, 1, 4), [k_swg(1), D.FIN], "CB = 4: PG = 64 = W", dict(loop="single", grid=1)),
    case("swg-in-1x4-3x5-n2-rowloop", D.p_conv3_wgrad, F_(2, 3, 5, 1, 4), [k_swg(1), D.FIN], "CB = 4, W = 5 < PG = 64", dict(loop="row", grid=2)),
    case("swg-out-16x2-9x13-n2-rowloop", D.p_conv3_wgrad, F_(2, 9, 13, 16, 2), [k_swg(2), D.FIN],
         "image = output (sgn = -1); CB = 16: PG = 16 > W = 13", dict(loop="row", grid=4)),
    case("swg-out-256x4-4x4-n2", D.p_conv3_wgrad, F_(2, 4, 4, 256, 4), [k_swg(4), D.FIN], "CB = 256: PG = 1", dict(loop="single", grid=2)),
    case("swg-in-2x8-8x32-n3", D.p_conv3_wgrad, F_(3, 8, 32, 2, 8), [k_swg(2), D.FIN], "CB = 8: PG = 32 = W", dict(loop="single", grid=3)),
    case("swg-out-8x3-11x7-n2-rowloop", D.p_conv3_wgrad, F_(2, 11, 7, 8, 3), [k_swg(3), D.FIN], "CB = 8, W = 7 < 32", dict(loop="row", grid=4)),
    case("swg-in-3x16-9x13-n2-grid2", D.p_conv3_wgrad, F_(2, 9, 13, 3, 16, ws=2 * 432 + 5), [k_swg(3), D.FIN],
         "scratch for two slabs: a grid of 2, two items each", dict(loop="row", grid=2, items=4, scratch=2 * 432 + 5)),
    case("swg-in-3x16-9x13-n2-shortscratch-atomic", D.p_conv3_wgrad, F_(2, 9, 13, 3, 16, ws=431, det=False), [G32],
         "scratch below one slab: declined -> tiled engine, generic kernel, 8 slices on fp32 atomics", dict(declined=True, scratch=431)),
    case("swg-in-3x16-9x13-n2-noscratch-atomic", D.p_conv3_wgrad, F_(2, 9, 13, 3, 16, ws="none", det=False), [G32], "NULL scratch"),
    case("swg-in-4x8-1x177-n1", D.p_conv3_wgrad, F_(1, 1, 177, 4, 8), [k_swg(4), D.FIN], "CS = 4: the widest map whose tile fits 64 KB of LDS",
         dict(loop="single", grid=1)),
    case("swg-in-4x8-1x178-n1-lds-declined", D.p_conv3_wgrad, F_(1, 1, 178, 4, 8), [D.bf(128, 32, "COL", "N"), D.RED],
         "65600 bytes of LDS: declined -> tiled engine (Cin = 4: AM_COL), 6 ordered slabs", dict(declined=True)),
    case("swg-in-3x12-5x5-n1-declined", D.p_conv3_wgrad, F_(1, 5, 5, 3, 12), [G32], "CB = 12: 64 % 3 != 0", dict(declined=True)),
    case("swg-out-512x3-4x8-n1-declined", D.p_conv3_wgrad, F_(1, 4, 8, 512, 3), [G32], "CB = 512", dict(declined=True)),
    case("swg-in-3x64-9x13-n2-deferred", D.p_conv3_wgrad, F_(2, 9, 13, 3, 64, deferred=True), [k_swg(3), D.BATCH], "slabs in the arena"),
]

# ---- c3rs_kernel (debug flag 0x800: taken at every size it covers) -----------------------------------------------------------------
# geometries per channel pair: (n, H, W, stated reach D, stated tiles per worker: 'lt1' < 1, '1to2', '2to3', 'ge3')
RS_GEO = {
    (64, 64): dict(bf=[(1, 6, 4, 1, "lt1"), (1, 4, 94, 3, "lt1"), (150, 7, 7, 1, "1to2"), (400, 7, 7, 1, "ge3")],
                   fp=[(1, 4, 63, 3, "lt1"), (2, 9, 31, 2, "lt1"), (300, 7, 7, 1, "2to3"), (3, 8, 30, 1, "lt1"), (1, 5, 62, 2, "lt1")]),
    (64, 128): dict(bf=[(1, 4, 6, 1, "lt1"), (1, 4, 63, 3, "lt1"), (80, 7, 7, 1, "1to2"), (3, 9, 13, 1, "lt1")],
                    fp=[(1, 4, 94, 3, "lt1"), (200, 7, 7, 1, "ge3"), (1, 6, 4, 1, "lt1"), (150, 7, 7, 1, "2to3"), (2, 5, 31, 2, "lt1")]),
    (128, 64): dict(bf=[(1, 5, 5, 1, "lt1"), (1, 6, 30, 1, "lt1"), (150, 7, 7, 1, "2to3"), (3, 9, 13, 1, "lt1")],
                    fp=[(1, 4, 62, 2, "lt1"), (1, 5, 31, 2, "lt1"), (80, 7, 7, 1, "1to2"), (1, 4, 6, 1, "lt1"), (200, 7, 7, 1, "ge3")]),
    (128, 128): dict(bf=[(1, 4, 30, 1, "lt1"), (2, 7, 7, 1, "lt1"), (40, 7, 7, 1, "1to2"), (3, 9, 13, 1, "lt1")],
                     fp=[(1, 4, 31, 2, "lt1"), (1, 4, 62, 2, "lt1"), (100, 7, 7, 1, "ge3"), (1, 5, 5, 1, "lt1"), (70, 7, 7, 1, "2to3")]),
    (128, 256): dict(bf=[(2, 7, 7, 1, "lt1"), (20, 7, 7, 1, "1to2"), (40, 7, 7, 1, "2to3"), (50, 7, 7, 1, "ge3")],
                     fp=[(1, 6, 62, 2, "lt1"), (1, 5, 5, 1, "lt1"), (20, 7, 7, 1, "1to2"), (1, 6, 30, 1, "lt1"), (50, 7, 7, 1, "ge3")]),
}
_XACT = {NONE: "", LEAKY: "-xleaky", RELU: "-xrelu"}
for _pi, ((_ci, _co), _geo) in enumerate(RS_GEO.items()):
    for _np, _key in ((3, "bf"), (2, "fp")):
        _forms = ["plain", "maskcs", "res", "maskres"] + (["dual"] if _np == 2 else [])
        for _fi, (_form, (_n, _H, _W, _D, _tpw)) in enumerate(zip(_forms, _geo[_key])):
            _k = _pi + _fi
            _xa = (NONE, LEAKY, RELU)[_k % 3]
            _kw = F_(_n, _H, _W, _ci, _co, flags=RS, bias=_k % 2 == 0)
            _opt = ""
            if _form == "dual":
                _kw.update(entry="s2", res=True, res_alpha=0.1, bias=True)
            else:
                # bf16 pieces: the plain entries where no fused option is set (mvk_conv3x3 / _res), mvk_conv3x3_f otherwise
                _fused = _np == 2 or _xa != NONE or (_form == "maskcs" and _k % 2 == 1)
                _kw.update(entry="s" if _np == 2 else ("f" if _fused else ("res" if "res" in _form else "plain")))
                if _fused:
                    _kw.update(x_act=_xa)
                    _opt += _XACT[_xa]
                if _form == "maskcs":
                    _kw.update(mask=(LEAKY, RELU)[_k % 2], colsum=True, deferred=_k % 3 == 0, bias=False)
                    if _fused and _k % 2 == 1:
                        _kw.update(pre_scale=0.1)
                        _opt += "-pre0.1"
                    _opt += "-deferred" if _kw["deferred"] else ""
                if _form == "res":
                    _kw.update(res=True, res_alpha=(0.1, -1.5)[_k % 2])
                if _form == "maskres":
                    _kw.update(res=True, res_alpha=1.0, mask=(RELU, LEAKY)[_k % 2])
            _src, _res = _form in ("maskcs", "maskres"), _form in ("res", "maskres", "dual")
            _exp = [k_rs(_ci, _co, _src, _res, _np, _form == "dual")]
            if _form == "maskcs":
                _exp.append(D.BATCH if _kw["deferred"] else D.FIN)
            CASES.append(case(f"rs-{_ci}x{_co}-{_key}-{_form}-{_H}x{_W}-n{_n}-D{_D}-tpw{_tpw}-{_kw['entry']}{_opt}", D.p_conv3, _kw, _exp,
                              regime=dict(kind="fwd", D=_D, tpw=_tpw)))

CASES += [
    # a 256-channel layer as two 128-channel launches, and a 64-channel slice of a 192-channel tensor
    case("rs-part-256to128-off0-7x7-n20", D.p_conv3, F_(20, 7, 7, 128, 128, entry="s_part", part=(256, 0), bias=False, flags=RS),
         [k_rs(128, 128, False, False, 2)], "first slice: act = none, no bias", dict(kind="fwd", D=1, tpw="lt1")),
    case("rs-part-256to128-off128-7x7-n20-respre-xleaky", D.p_conv3,
         F_(20, 7, 7, 128, 128, entry="s_part", part=(256, 128), res=True, res_pre=True, x_act=LEAKY, flags=RS),
         [k_rs(128, 128, False, True, 2)], "second slice: the other slice's partial sum enters before the activation",
         dict(kind="fwd", D=1, tpw="lt1")),
    case("rs-part-192to64-off64-9x13-n3-mask-respre", D.p_conv3,
         F_(3, 9, 13, 64, 64, entry="s_part", part=(192, 64), res=True, res_pre=True, mask=LEAKY, pre_scale=0.1, flags=RS),
         [k_rs(64, 64, True, True, 2)], "pixels 192 channels apart, weight taps 192 rows apart", dict(kind="fwd", D=1, tpw="lt1")),
    # the scaled form's range
    case("rs-64x64-fp-spread-9x13-n6", D.p_conv3, F_(6, 9, 13, 64, 64, entry="s", data="spread", flags=RS),
         [k_rs(64, 64, False, False, 2)], "images and weight rows over e^(+-3 sigma)"),
    case("rs-128x128-fp-loose-7x7-n4", D.p_conv3, F_(4, 7, 7, 128, 128, entry="s", data="loose", bias=False, flags=RS),
         [k_rs(128, 128, False, False, 2)], "an operand bound 1000x above max |X|: range, not precision"),
    case("rs-64x128-fp-tiny-8x8-n2", D.p_conv3, F_(2, 8, 8, 64, 128, entry="s", data="tiny", bias=False, flags=RS),
         [k_rs(64, 128, False, False, 2)], "half an image and a weight row 2^-30 of the rest: held to the floor"),
    # past the reach: the plain entry lands on the tiled engine with the same per-entry result
    case("rs-128x128-bf-4x31-n1-reach-tiled", D.p_conv3, F_(1, 4, 31, 128, 128, flags=RS), [FROW], "D = 2 > 1 for 128 channels on bf16 pieces"),
    case("rs-64x64-bf-4x95-n1-reach-tiled", D.p_conv3, F_(1, 4, 95, 64, 64, flags=RS), [FROW], "D = 4"),
]

# ---- c3wg_kernel<3> / <2>: every value of types = (Cin / 64) (Cout / 64) once ---------------------------------------------------------
# (a weight-gradient entry sums n H W products: the large tile counts sit on the pairs with few workers, so that the sums stay near
# 1024 terms and the per-entry bound keeps its teeth)
WG = [  # (Cin, Cout, entry, n, H, W, D, tpw, options)
    (64, 64, "plain", 1, 6, 4, 1, "lt1", {}),
    (128, 64, "f", 3, 9, 13, 1, "lt1", dict(x_act=LEAKY, dy_scale=0.1, db=True)),
    (192, 64, "s", 2, 5, 62, 2, "lt1", dict(db=True)),  # (no forward kernel has 192 channels: mvk_conv3x3_wgrad_f refuses them)
    (128, 128, "s", 1, 4, 31, 2, "lt1", dict(db=True, dy_scale=0.1)),
    (192, 128, "plain", 1, 4, 30, 1, "lt1", {}),
    (256, 128, "s", 20, 7, 7, 1, "1to2", dict(x_act=RELU)),
    (192, 192, "s", 1, 4, 63, 3, "lt1", dict(db=True, deferred=True)),
    (256, 192, "plain", 25, 7, 7, 1, "2to3", {}),
    (256, 256, "s", 25, 7, 7, 1, "ge3", dict(db=True, x_act=LEAKY)),
    (64, 128, "s", 3, 9, 13, 1, "lt1", dict(db=True, deferred=True, data="spread")),
    (64, 64, "f", 1, 4, 94, 3, "lt1", dict(db=True, x_act=RELU)),
    (64, 192, "plain", 1, 4, 6, 1, "lt1", {}),
    (128, 64, "plain", 1, 5, 5, 1, "lt1", {}),
]
for _ci, _co, _e, _n, _H, _W, _D, _tpw, _o in WG:
    _exp = [k_wg(2 if _e == "s" else 3)] + ([D.BATCH] if _o.get("deferred") else [D.RED] + ([D.FIN] if _o.get("db") else []))
    _tag = "".join(f"-{k}{'' if v is True else v}" for k, v in _o.items())
    CASES.append(case(f"wg-{_ci}x{_co}-{_e}-{_H}x{_W}-n{_n}-D{_D}-tpw{_tpw}{_tag}", D.p_conv3_wgrad,
                      F_(_n, _H, _W, _ci, _co, entry=_e, flags=RS, **_o), _exp,
                      f"types = {R3.wgrad_types(_ci, _co)}: {R3.wgrad_workers(_ci, _co)} workers", dict(kind="wgrad", D=_D, tpw=_tpw)))
CASES += [
    case("wg-64x64-plain-4x95-n1-reach-tiled", D.p_conv3_wgrad, F_(1, 4, 95, 64, 64, flags=RS), [FCOL, D.RED], "D = 4: tiled engine"),
    case("wg-64x64-plain-7x7-n2-shortscratch-tiled", D.p_conv3_wgrad, F_(2, 7, 7, 64, 64, ws=256 * 9 * 64 * 64 - 1, flags=RS),
         [FCOL, D.RED], "one float below 256 slabs: the plain form falls to the tiled engine (4 ordered slabs fit)"),
    case("wg-64x64-plain-7x7-n2-unalignedscratch-tiled", D.p_conv3_wgrad, F_(2, 7, 7, 64, 64, ws="unaligned", flags=RS),
         [FCOL, D.RED], "scratch not 16-byte aligned: tiled engine"),
]
IDS = [c.id for c in CASES]


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_conv3_leaf(c):
    report = D.check_case(c, engine_f32=False)
    print(c.id, {k: v for k, v in report.items() if k != "kernels"})


def test_case_ids_are_unique():
    assert len(IDS) == len(set(IDS))


# ---- activations ---------------------------------------------------------------------------------------------------------------------
ACTS = [  # (id, prep keywords, the sigmoid is the kernel's own: True / the launch goes to the tiled engine: False)
    ("cin", F_(2, 9, 13, 3, 32), True),
    ("cout", F_(2, 9, 33, 48, 3), True),
    ("rs-bf", F_(3, 9, 13, 64, 128, flags=RS), False),
    ("rs-fp", F_(3, 9, 13, 128, 64, flags=RS, entry="s"), None),  # the scaled entry refuses the sigmoid
    ("rs-fp-respre", F_(3, 9, 13, 64, 64, flags=RS, entry="s_part", part=(64, 0), res=True, res_pre=True), None),
    ("tiled", F_(3, 7, 7, 32, 32, flags=TILED), False),
]


def _launch_act(kw, act):
    """The layer's output with activation `act` from fixed operands."""
    bufs, go = D.execute(D.p_conv3(5, act=act, **kw))
    go()
    torch.cuda.synchronize()
    return bufs[0]


@pytest.mark.parametrize("name,kw,own_sigmoid", ACTS, ids=[a[0] for a in ACTS])
def test_activations(name, kw, own_sigmoid):
    """ReLU / LeakyReLU: bit-identical to act(output with act = 0) (the same sums, then a select; with res_pre the residual enters
    before the activation).  Sigmoid: against the float64 sigmoid of the launch's own fp32 pre-activation, within 2x the largest ulp
    error of torch.sigmoid (fp32, GPU) on the same tensor, at least 1 ulp; the register-stationary kernels decline it (the plain entry
    then runs the tiled engine, the scaled entries refuse)."""
    from multivae_amd._lib import MvkError

    pre = _launch_act(kw, NONE)
    assert bool(torch.isfinite(pre).all())
    assert torch.equal(_launch_act(kw, RELU), pre.clamp_min(0))
    assert torch.equal(_launch_act(kw, LEAKY), torch.where(pre > 0, pre, R3.F02 * pre))
    if own_sigmoid is None:
        with pytest.raises(MvkError):
            _launch_act(kw, SIGMOID)
        return
    if not own_sigmoid:  # the pre-activation of the kernel that evaluates the sigmoid
        pre = _launch_act(dict(kw, flags=TILED), NONE)
    ref = torch.sigmoid(pre.double())
    ulp = torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126))) - 23)
    mine = float(((_launch_act(kw, SIGMOID).double() - ref).abs() / ulp).max())
    yard = float(((torch.sigmoid(pre).double() - ref).abs() / ulp).max())
    print(f"{name}: sigmoid ulp: kernel {mine:.3f}, torch fp32 {yard:.3f}")
    assert mine <= max(2 * yard, 1.0), (mine, yard)


# ---- published maxima -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [F_(2, 9, 13, 3, 32, mask=RELU), F_(3, 1, 1, 1, 4), F_(1, 9, 3, 2, 1024, bias=False), F_(2, 8, 5, 2, 12)],
                         ids=["3x32-9x13", "1x4-1x1", "2x1024-9x3", "2x12-idle-lanes"])
def test_image_side_amax(kw):
    """mvk_conv3x3_y = mvk_conv3x3 bit for bit, and the slot (0 before the launch) holds max |Y| exactly: idle position lanes, ragged
    bands and 1x1 maps included."""
    plain, run = D.execute(D.p_conv3(11, **kw))
    run()
    py = D.p_conv3(11, entry="y", **kw)
    bufs, run = D.execute(py)
    assert D.launched_kernels(run) == [k_cin(kw["Cin"])]
    assert torch.equal(bufs[0], plain[0])
    assert float(py.yam) == float(bufs[0].abs().max()) and float(py.yam) > 0


# ---- the smallest admitted maps: two tiles, every other worker idle -------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(6, 4), (4, 6), (5, 5)])
def test_smallest_maps_idle_workers(H, W):
    """n = 1 on the smallest maps the position stream admits: 2 tiles for 256 workers.  The column-sum partial rows of the workers
    without a tile are zero (the scratch held NaN), the two others add up to the column sums, and the published max |Y| is exact."""
    from multivae_amd._lib import call, ptr, stream_ptr

    Cin = Cout = 64
    assert R3.tiles(1, H, W) == 2 and R3.fwd_workers(Cin, Cout) == 256
    busy = [w for w, (t0, t1) in enumerate(R3.split(2, 256)) if t1 > t0]
    assert busy == [127, 255]
    x, w, b, src, _, _ = R3.fwd_operands(3, 1, H, W, Cin, Cout)
    d = D.dev()
    Xd, Wd, sd = D._nhwc(x).to(d), R3.pack_fwd(w).to(d), D._nhwc(src).to(d)
    xam, wam, yam = x.abs().max().reshape(1).to(d), w.abs().max().reshape(1).to(d), torch.zeros(1, device=d)
    Y, cs = torch.full((1, H, W, Cout), float("nan"), device=d), torch.zeros(Cout, device=d)
    ws = D._ws()
    ws[:256 * Cout].fill_(float("nan"))
    D._flags(RS)
    try:
        names = D.launched_kernels(lambda: call("mvk_conv3x3_s", ptr(Xd), ptr(Wd), None, ptr(Y), 1, H, W, Cin, Cout, NONE, ptr(sd), LEAKY,
                                                None, 1.0, ptr(cs), NONE, 1.0, ptr(xam), ptr(wam), ptr(yam), ptr(ws), ws.numel(),
                                                stream_ptr()))
    finally:
        D._flags(0)
    assert names == sorted([k_rs(64, 64, True, False, 2), D.FIN])
    part = ws[:256 * Cout].view(256, Cout).cpu()
    idle = torch.ones(256, dtype=torch.bool)
    idle[busy] = False
    assert bool((part[idle] == 0).all()), "partial rows of idle workers"
    assert bool(torch.isfinite(part).all()) and bool(torch.isfinite(Y).all())
    assert float(yam) == float(Y.abs().max()) > 0
    assert torch.allclose(cs.cpu(), part.sum(0), rtol=1e-6, atol=0)


# ---- gates, without a launch ---------------------------------------------------------------------------------------------------------------
def test_shape_gates_match_the_restatement():
    """mvk_conv3x3_scaled_ok, _fused_ok and _wgrad_scaled_ok over H, W in 1..100 (the three reach limits W = 30 | 31, 62 | 63, 94 | 95
    included) against tests/conv3_ref.py, with the size threshold off (0x800); the 32-bit offset gate; 0x400 refuses everything."""
    from multivae_amd import _lib

    lib = _lib.load()
    D._flags(RS)
    try:
        for Cin, Cout in R3.RS_PAIRS + [(192, 64), (192, 192), (256, 256), (64, 192), (32, 64), (64, 96), (320, 64)]:
            for H in range(1, 101):
                for W in range(1, 101):
                    a = (1, H, W, Cin, Cout)
                    assert lib.mvk_conv3x3_scaled_ok(*a) == int(R3.fwd_shape_ok(*a, 2)), ("scaled_ok", a)
                    assert lib.mvk_conv3x3_fused_ok(*a) == int(R3.fused_ok(*a)), ("fused_ok", a)
                    assert lib.mvk_conv3x3_wgrad_scaled_ok(*a) == int(R3.wgrad_shape_ok(*a)), ("wgrad_scaled_ok", a)
        for W, bf128, fp128, c64 in [(30, 1, 1, 1), (31, 0, 1, 1), (62, 0, 1, 1), (63, 0, 0, 1), (94, 0, 0, 1), (95, 0, 0, 0)]:
            assert lib.mvk_conv3x3_fused_ok(2, 4, W, 128, 128) == bf128 and lib.mvk_conv3x3_scaled_ok(2, 4, W, 128, 128) == fp128
            assert lib.mvk_conv3x3_fused_ok(2, 4, W, 64, 64) == c64 and lib.mvk_conv3x3_wgrad_scaled_ok(2, 4, W, 256, 256) == c64
        # byte offsets into the tensors are 32 bits wide: 64 x 64 x 256 channels x 4 bytes = 2^22 per image
        assert lib.mvk_conv3x3_wgrad_scaled_ok(1023, 64, 64, 256, 256) == 1 and lib.mvk_conv3x3_wgrad_scaled_ok(1024, 64, 64, 256, 256) == 0
        assert lib.mvk_conv3x3_scaled_ok(2047, 64, 64, 64, 128) == 1 and lib.mvk_conv3x3_scaled_ok(2048, 64, 64, 64, 128) == 0
        assert lib.mvk_conv3x3_fused_ok(1, 4, 30, 192, 64) == 0  # no forward kernel has 192 channels
        assert R3.wgrad_shape_ok(1023, 64, 64, 256, 256) and not R3.wgrad_shape_ok(1024, 64, 64, 256, 256)
        assert lib.mvk_conv3x3_scaled_ok(0, 16, 16, 64, 64) == 0
        D._flags(TILED)
        assert lib.mvk_conv3x3_scaled_ok(8, 16, 16, 64, 64) == 0 and lib.mvk_conv3x3_fused_ok(8, 16, 16, 64, 64) == 0
    finally:
        D._flags(0)


def test_entries_refuse_what_they_do_not_cover():
    """No silent fall-back from the fused / scaled entry points: past the reach (W = 63 on 128 scaled channels) and with a scratch one
    float short of the weight gradient's slabs they return MVK_EINVAL."""
    from multivae_amd._lib import MvkError

    D._flags(RS)
    try:
        for kw in (F_(1, 4, 63, 128, 128, entry="s"), F_(1, 4, 31, 128, 64, entry="f", x_act=LEAKY), F_(1, 4, 95, 64, 64, entry="s")):
            p = D.p_conv3(1, **kw)
            bufs, _ = D.execute(p)
            with pytest.raises(MvkError):
                p.call(bufs)
        need = 256 * 9 * 64 * 64
        for kw in (dict(entry="f", dy_scale=0.1, ws=need - 1), dict(entry="s", ws=need - 1), dict(entry="f", db=True, ws=need + 256 * 64 - 1)):
            p = D.p_conv3_wgrad(1, 2, 7, 7, 64, 64, **kw)
            bufs, _ = D.execute(p)
            with pytest.raises(MvkError):
                p.call(bufs)
        torch.cuda.synchronize()
    finally:
        D._flags(0)


def test_zero_tensor_scaled():
    """An all-zero X under the bound 0 (the scale clamps): the scaled launch stores the bias exactly, column sums and the second store
    included."""
    from multivae_amd._lib import call, ptr, stream_ptr

    n, H, W, Cin, Cout = 2, 7, 7, 128, 256
    d = D.dev()
    gn = R3.g(9)
    w, b = torch.randn(Cout, Cin, 3, 3, generator=gn), torch.randn(Cout, generator=gn)
    res = torch.randn(n, H, W, Cout, generator=gn)
    Xd, Wd, bd, rd = torch.zeros(n, H, W, Cin, device=d), R3.pack_fwd(w).to(d), b.to(d), res.to(d)
    xam, wam, yam = torch.zeros(1, device=d), w.abs().max().reshape(1).to(d), torch.zeros(1, device=d)
    Y, A = torch.full((n, H, W, Cout), float("nan"), device=d), torch.full((n, H, W, Cout), float("nan"), device=d)
    wsp, wsn = D.WS("ws")
    D._flags(RS)
    try:
        call("mvk_conv3x3_s2", ptr(Xd), ptr(Wd), ptr(bd), ptr(Y), ptr(A), n, H, W, Cin, Cout, NONE, ptr(rd), 0.5, ptr(xam), ptr(wam),
             ptr(yam), wsp, wsn, stream_ptr())
    finally:
        D._flags(0)
    assert torch.equal(A.cpu(), b.view(1, 1, 1, -1).expand(n, H, W, Cout))
    assert torch.equal(Y.cpu(), torch.addcmul(res, torch.tensor(0.5), b.view(1, 1, 1, -1).expand(n, H, W, Cout)))
    assert float(yam) == float(Y.abs().max())


# ---- the 1024-slab cap of conv3_small_wgrad ------------------------------------------------------------------------------------------------
GRIDCAP = dict(n=1025, H=4, W=4, Cin=1, Cout=4)  # 1025 work items on 1024 workgroups: workgroup 0 re-stages its tile for image 1024


def gridcap_refs(want_h=False):
    """Operands, initial dW and the float64 references of every workgroup's slab (shared with the host test): slab b = the weight
    gradient over the images b, b + 1024, ... alone, [1024][Cout][Cin][3][3]."""
    c = GRIDCAP
    x, dy, init, _ = R3.wgrad_operands(1025, c["n"], c["H"], c["W"], c["Cin"], c["Cout"])

    def op(a, b):  # per-image weight gradients, added per workgroup
        cols = torch.nn.functional.unfold(a, 3, padding=1).view(c["n"], c["Cin"], 9, -1)
        per = torch.einsum("nckp,nop->nock", cols, b.flatten(2)).reshape(c["n"], c["Cout"], c["Cin"], 3, 3)
        slabs = per[:1024].clone()
        slabs[:c["n"] - 1024] += per[1024:]
        return slabs

    return x, dy, init, R3.bilinear(op, x, dy, want_h=want_h)


def test_small_wgrad_grid_cap():
    """conv3_small_wgrad above its 1024-slab cap: the grid-stride loop (a workgroup that takes a second work item re-stages its tile
    and keeps accumulating).  A 16400-term sum leaves a per-entry bound without teeth (the two-piece emulation stays at 0.2x), so the
    launch is checked at the two levels it computes: (1) every entry of every workgroup's slab, read back from the scratch, against
    the float64 sum over that workgroup's one or two images at C_ENTRY * sum |x dy| (the two-piece emulation must leave this bound);
    (2) dW - initial against the float64 sum of the kernel's OWN slabs at C_ENTRY * (sum |slab| + |initial|); plus the end-to-end
    result at C_ENTRY * bound, the exact kernel set and bit-identity of a repeat."""
    from multivae_amd._lib import call, ptr, stream_ptr

    c = GRIDCAP
    plan = R3.small_wgrad_plan(**c)
    assert plan["grid"] == 1024 and plan["items"] == 1025 and plan["loop"] == "row"
    x, dy, init, blk = gridcap_refs()
    d = D.dev()
    Xd, dYd = D._nhwc(x).to(d), D._nhwc(dy).to(d)
    ws, total = D._ws(), 9 * c["Cin"] * c["Cout"]

    def launch():
        dW = init.to(d)
        ws[:1024 * total].fill_(float("nan"))
        names = D.launched_kernels(lambda: call("mvk_conv3x3_wgrad", ptr(Xd), ptr(dYd), ptr(dW), c["n"], c["H"], c["W"], c["Cin"], c["Cout"],
                                                ptr(ws), ws.numel(), stream_ptr()))
        return names, dW, ws[:1024 * total].view(1024, c["Cout"], c["Cin"], 3, 3).clone()

    names, dW, slabs = launch()
    assert names == sorted([k_swg(1), D.FIN])
    s64 = slabs.double().cpu()
    assert bool(torch.isfinite(s64).all())
    tol = D.C_ENTRY * blk.bound + 1e-30
    worst, deg = float(((s64 - blk.ref).abs() / tol).max()), float(((blk.deg2 - blk.ref).abs() / tol).max())
    print(f"slabs: worst {worst:.3f}x the bound, two-piece {deg:.2f}x")
    assert worst <= 1.0 and deg > 1.0
    got = dW.double().cpu() - init.double()
    r2 = float(((got - s64.sum(0)).abs() / (D.C_ENTRY * (s64.abs().sum(0) + init.double().abs()))).max())
    r3 = float(((got - blk.ref.sum(0)).abs() / (D.C_ENTRY * (blk.bound.sum(0) + init.double().abs()))).max())
    print(f"slab sum: worst {r2:.3f}x its bound; end to end {r3:.4f}x C_ENTRY * bound")
    assert r2 <= 1.0 and r3 <= 1.0
    names2, dW2, slabs2 = launch()
    assert torch.equal(dW, dW2) and torch.equal(slabs, slabs2)


# ---- the deferral arena ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,note", [(F_(1, 1, 257, 3, 8), "W > 256"), (F_(1, 5, 5, 3, 12), "CB = 12"), (F_(1, 1, 178, 4, 8), "LDS")],
                         ids=["W257", "CB12", "lds"])
def test_declined_small_wgrad_takes_no_arena(kw, note):
    """A weight gradient with an image on one side that conv3_small_wgrad declines must not leave a reservation of the deferral arena
    behind: inside deferred_reductions, mvk_defer_wanted afterwards is what the tiled engine's ordered split K asked for (z slabs of
    9 Cin Cout floats, in 256-byte regions) and nothing else: a region that is reserved and never pushed stays taken until the scope
    ends."""
    from multivae_amd import _lib

    p = D.p_conv3_wgrad(17, deferred=True, **kw)
    bufs, run = D.execute(p)
    run()
    torch.cuda.synchronize()
    M, N, K = 9 * kw["Cin"], kw["Cout"], kw["n"] * kw["H"] * kw["W"]
    z = R3.splitk_slabs(M, N, K)
    want = (z * M * N + 63) // 64 * 64 if z > 1 else 0
    assert int(_lib.load().mvk_defer_wanted()) == want, (note, z)
    o = p.outs[0]
    err = (bufs[0].cpu().double() - o.init.double() - o.ref).abs() / (D.C_ENTRY * o.bound)
    assert float(err.max()) <= 1.0


def test_taken_small_wgrad_reserves_its_slabs_only():
    """... and a taken one reserves min(n * bands, 1024) slabs, not 1024."""
    from multivae_amd import _lib

    p = D.p_conv3_wgrad(18, 2, 9, 13, 3, 64, deferred=True)
    bufs, run = D.execute(p)
    assert D.launched_kernels(run) == sorted([k_swg(3), D.BATCH])
    assert int(_lib.load().mvk_defer_wanted()) == 4 * 9 * 3 * 64
