"""CPU checks of tests/conv3_ref.py, the float64 reference behind tests/test_gpu_conv3x3.py and the 3x3 cases of
tests/test_gpu_gemm_dispatch.py:

- on tiny shapes the references agree with float64 autograd and with a direct numpy loop over (channel, channel, tap);
- the derived epilogues (input activation, pre_scale, mask, both residual placements, column sums) are what they state;
- for EVERY case of both tables each degraded emulation that is defined for the case leaves the case's tolerance on at least one
  product output (the per-case ratios are printed): the per-entry check has teeth before any GPU run;
- every case that names a regime of the position stream (reach D, tiles per worker) or of the small weight gradient (single / row
  loop, grid, items per workgroup, a decline) produces it under the Python restatement of the host arithmetic;
- the tables hold the leaves they are meant to hold.
"""
import re
import zlib

import pytest
import torch

import conv3_ref as R3
import test_gpu_conv3x3 as G
import test_gpu_gemm_dispatch as D

F64 = torch.float64


def _close(a, b, bound, what):
    """Two float64 evaluations of one formula in different operation orders: rounding alone, 1e-12 of the term magnitude."""
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    r = float(((a - b).abs() / (1e-12 * bound + 1e-300)).max())
    assert r <= 1.0, f"{what}: {r:.3g} x 1e-12 of the term magnitude"


@pytest.mark.parametrize("n,H,W,Cin,Cout", [(2, 3, 2, 3, 5), (1, 1, 1, 2, 4), (2, 4, 5, 1, 3)])
def test_references_agree_with_autograd_and_loops(n, H, W, Cin, Cout):
    x, w, b, src, res, _ = R3.fwd_operands(1, n, H, W, Cin, Cout)
    dy = torch.randn(n, Cout, H, W, generator=R3.g(2))
    y, dx, dw, db = R3.conv3_autograd(x, w, b, dy)
    r = R3.conv3_fwd(x, w, b)["y"]
    _close(r.ref, y, r.bound, "forward vs autograd")
    _close(r.ref, R3.conv3_loops(x, w) + b.double().view(1, -1, 1, 1), r.bound, "forward vs loops")
    _close(r.bound, R3.conv3_loops(x.abs(), w.abs()) + b.double().abs().view(1, -1, 1, 1), r.bound, "forward bound vs loops")
    g_ = R3.conv3_wgrad(x, dy)
    _close(g_["dw"].ref, dw, g_["dw"].bound, "weight gradient vs autograd")
    _close(g_["db"].ref, db, g_["db"].bound, "bias gradient vs autograd")
    # backward data = the same launch on the flipped, channel-swapped weight
    wb = w.flip(2, 3).transpose(0, 1).contiguous()
    rb = R3.conv3_fwd(dy, wb)["y"]
    _close(rb.ref, dx, rb.bound, "backward data vs autograd")
    # the GEMM pack is a permutation: conv = im2col (tap-major, channel-minor) @ pack
    cols = torch.nn.functional.unfold(x.double(), 3, padding=1).transpose(1, 2).reshape(n * H * W, Cin, 9).transpose(1, 2)
    yp = (cols.reshape(n * H * W, 9 * Cin) @ R3.pack_fwd(w).double()).view(n, H, W, Cout).permute(0, 3, 1, 2)
    _close(yp, r.ref - b.double().view(1, -1, 1, 1), r.bound, "pack layout")


def test_derived_epilogues():
    n, H, W, Cin, Cout = 2, 4, 3, 3, 4
    x, w, b, src, res, _ = R3.fwd_operands(5, n, H, W, Cin, Cout)
    bb = b.double().view(1, -1, 1, 1)
    for x_act, slope in ((R3.LEAKY, R3.F02), (R3.RELU, 0.0), (R3.NONE, 1.0)):
        xa = torch.where(x > 0, x.double(), x.double() * slope)
        conv = R3.op_conv3(xa, w.double())
        m = R3.actgrad64(src, R3.LEAKY)
        r = R3.conv3_fwd(x, w, b, x_act=x_act, pre_scale=0.1, mask_src=src, mask_act=R3.LEAKY, res=res, res_alpha=-1.5, colsum=True)
        ps = float(torch.tensor(0.1, dtype=torch.float32))
        a = (ps * conv + bb) * m
        # the input activation is an fp32 product (x * 0.2f rounds once): 2^-24 of the bound
        tol = r["a"].bound * 2.0 ** -23
        assert bool(((r["a"].ref - a).abs() <= tol).all())
        assert bool(((r["y"].ref - (res.double() - 1.5 * a)).abs() <= tol * 1.5).all())
        assert bool((r["y"].bound >= res.double().abs() + 1.5 * r["a"].bound * (1 - 1e-12)).all())
        _close(r["colsum"].ref, r["a"].ref.sum((0, 2, 3)), r["colsum"].bound, "column sums")
        _close(r["colsum"].bound, (r["a"].bound + r["a"].ref.abs()).sum((0, 2, 3)), r["colsum"].bound, "column-sum tolerance")
        rp = R3.conv3_fwd(x, w, b, x_act=x_act, res=res, res_pre=True)
        assert bool(((rp["y"].ref - (conv + bb + res.double())).abs() <= rp["y"].bound * 2.0 ** -23).all())
    g_ = R3.conv3_wgrad(x, src, x_act=R3.LEAKY, dy_scale=0.1)
    ds = float(torch.tensor(0.1, dtype=torch.float32))
    ref = ds * R3.op_wgrad3(R3.in_act32(x, R3.LEAKY).double(), src.double())
    _close(g_["dw"].ref, ref, g_["dw"].bound, "scaled weight gradient")
    _close(g_["db"].ref, ds * src.double().sum((0, 2, 3)), g_["db"].bound, "scaled bias gradient")
    fl = R3.conv3_fwd(x, w, None, floor_bounds=(2.0, 3.0))["y"].bound - R3.conv3_fwd(x, w, None)["y"].bound
    assert torch.allclose(fl, torch.full_like(fl, R3.FLOOR * 6.0 * 9 * Cin / R3.C_ENTRY), rtol=1e-9)
    assert float(R3.in_act32(torch.tensor([-1.0]), R3.LEAKY)) == -R3.F02


# ---- teeth ---------------------------------------------------------------------------------------------------------------------
GEMM3 = [c for c in D.CASES if c.id.startswith("c3")]
ALL = G.CASES + GEMM3
_HOST = {}


def host_outs(c):
    if c.id not in _HOST:
        _HOST[c.id] = c.fn(zlib.crc32(c.id.encode()) % 100003, host=True, **c.kw)
    return _HOST[c.id]


@pytest.mark.parametrize("c", ALL, ids=[c.id for c in ALL])
def test_degraded_emulations_leave_the_tolerance(c):
    """The GPU check of a case is |got - ref| <= C_ENTRY * bound on every entry of every output; an emulation is rejected when it
    breaks that on any output.  Both emulations must be rejected; f16_drop is defined for the products only (not for db)."""
    p = host_outs(c)
    r2, rh = [], []
    for o in p.outs:
        assert o.ref.dtype == F64 and o.bound.dtype == F64 and o.ref.shape == o.bound.shape == o.deg.shape
        assert bool((o.bound + 1e-300 >= o.ref.abs() * (1 - 1e-12)).all()), "the bound is below its own reference"
        tol = D.C_ENTRY * o.bound + 1e-30
        r2.append(float(((o.deg - o.ref).abs() / tol).max()))
        if o.degh is not None:
            rh.append(float(((o.degh - o.ref).abs() / tol).max()))
    print(f"{c.id}: two_piece {['%.2f' % r for r in r2]}, f16_drop {['%.1f' % r for r in rh]}")
    assert max(r2) > 1.0, f"two-piece operands pass every output: {r2}"
    assert rh and max(rh) > 1.0, f"fp16 pairs without a cross term pass every output: {rh}"


def test_cpu_fp32_stays_inside():
    """torch's fp32 conv2d / conv2d_weight on the CPU (a correct fp32 implementation) stays inside the tolerance the emulations leave."""
    for n, H, W, Cin, Cout in [(1, 6, 4, 64, 64), (2, 9, 13, 1, 32), (1, 9, 40, 16, 1), (2, 4, 63, 64, 64)]:
        x, w, b, *_ = R3.fwd_operands(7, n, H, W, Cin, Cout)
        r = R3.conv3_fwd(x, w, b)["y"]
        got = torch.nn.functional.conv2d(x, w, b, 1, 1).double()
        assert float(((got - r.ref).abs() / (R3.C_ENTRY * r.bound)).max()) <= 1.0
        x, dy, *_ = R3.wgrad_operands(8, n, H, W, Cin, Cout)
        g_ = R3.conv3_wgrad(x, dy)["dw"]
        got = R3.op_wgrad3(x, dy).double()
        assert float(((got - g_.ref).abs() / (R3.C_ENTRY * g_.bound)).max()) <= 1.0


# ---- regimes ---------------------------------------------------------------------------------------------------------------------
def _tpw_class(v):
    return "lt1" if v < 1 else "1to2" if v < 2 else "2to3" if v < 3 else "ge3"


STREAM = [c for c in G.CASES if c.regime and "kind" in c.regime]
SMALLWG = [c for c in G.CASES if c.id.startswith("swg") and c.regime]


@pytest.mark.parametrize("c", STREAM, ids=[c.id for c in STREAM])
def test_stream_regime(c):
    kw, rg = c.kw, c.regime
    n, H, W, Cin, Cout = (kw[k] for k in ("n", "H", "W", "Cin", "Cout"))
    fwd = rg["kind"] == "fwd"
    np_ = 2 if kw.get("entry") in ("s", "s2", "s_part") else 3
    assert (R3.fwd_shape_ok(n, H, W, Cin, Cout, np_) if fwd else R3.wgrad_shape_ok(n, H, W, Cin, Cout)), "the case's own gate"
    if fwd and kw.get("entry") == "f":
        assert R3.fused_ok(n, H, W, Cin, Cout)
    workers = R3.fwd_workers(Cin, Cout) if fwd else R3.wgrad_workers(Cin, Cout)
    assert R3.reach(W) == rg["D"] and f"-D{rg['D']}-" in c.id + "-" or "part" in c.id
    assert R3.reach(W) == rg["D"]
    assert _tpw_class(R3.tiles_per_worker(n, H, W, workers)) == rg["tpw"]
    sp = R3.split(R3.tiles(n, H, W), workers)
    assert sp[0][0] == 0 and sp[-1][1] == R3.tiles(n, H, W) and all(a[1] == b[0] for a, b in zip(sp, sp[1:]))
    most = max(t1 - t0 for t0, t1 in sp)
    assert {"lt1": most <= 1, "1to2": 1 <= most <= 2, "2to3": 2 <= most <= 3, "ge3": most >= 3}[rg["tpw"]]
    assert R3.ring(W) % 32 == 0 and R3.ring(W) >= 32 * (2 * rg["D"] + 2) and R3.ring(W) > 32 * rg["D"] + 63 + W + 2


def test_stream_regimes_cover_the_issue():
    fw = {(c.regime["D"], c.regime["tpw"]) for c in STREAM if c.regime["kind"] == "fwd"}
    wg = {(c.regime["D"], c.regime["tpw"]) for c in STREAM if c.regime["kind"] == "wgrad"}
    for s in (fw, wg):
        assert {d for d, _ in s} == {1, 2, 3} and {t for _, t in s} == {"lt1", "1to2", "2to3", "ge3"}
    shapes = {(c.kw["H"], c.kw["W"]) for c in STREAM if c.kw["n"] == 1}
    assert {(6, 4), (4, 6), (5, 5)} <= shapes
    widths = {c.kw["W"] for c in STREAM}
    assert {30, 31, 62, 63, 94} <= widths
    for pair in R3.RS_PAIRS:  # tiles-per-worker classes of the two pairs the issue names
        got = {c.regime["tpw"] for c in STREAM if c.regime["kind"] == "fwd" and (c.kw["Cin"], c.kw["Cout"]) == pair}
        if pair in ((128, 256), (64, 64)):
            assert {"lt1", "1to2", "ge3"} <= got, (pair, got)
    assert {R3.wgrad_types(c.kw["Cin"], c.kw["Cout"]) for c in STREAM if c.regime["kind"] == "wgrad"} == {1, 2, 3, 4, 6, 8, 9, 12, 16}
    assert R3.wgrad_workers(192, 64) * 3 == 255 and R3.wgrad_workers(192, 192) * 9 == 252  # grids without the XCD remap
    assert [R3.fwd_types(*p) for p in R3.RS_PAIRS] == [1, 2, 2, 4, 8]
    # the reach limits of the three ring sizes
    for W, d in ((30, 1), (31, 2), (62, 2), (63, 3), (94, 3), (95, 4)):
        assert R3.reach(W) == d
    assert R3.fwd_shape_ok(1, 4, 30, 128, 128, 3) and not R3.fwd_shape_ok(1, 4, 31, 128, 128, 3)
    assert R3.fwd_shape_ok(1, 4, 62, 128, 128, 2) and not R3.fwd_shape_ok(1, 4, 63, 128, 128, 2)
    assert R3.fwd_shape_ok(1, 4, 94, 64, 64, 3) and not R3.fwd_shape_ok(1, 4, 95, 64, 64, 3)
    assert not R3.fwd_shape_ok(1, 5, 4, 64, 64) and not R3.fwd_shape_ok(1, 3, 8, 64, 64) and not R3.fwd_shape_ok(1, 4, 5, 64, 64)


@pytest.mark.parametrize("c", SMALLWG, ids=[c.id for c in SMALLWG])
def test_small_wgrad_regime(c):
    kw, rg = c.kw, c.regime
    scratch = rg.get("scratch", 1 << 40)
    plan = R3.small_wgrad_plan(kw["n"], kw["H"], kw["W"], kw["Cin"], kw["Cout"], scratch)
    if rg.get("declined"):
        assert plan is None
        return
    assert plan is not None and plan["loop"] == rg["loop"] and plan["grid"] == rg["grid"]
    assert plan["items"] == rg.get("items", rg["grid"])
    assert k_cs(c) == plan["CS"]


def k_cs(c):
    return int(re.search(r"conv3_small_wgrad_kernel<(\d)>", "".join(c.expect)).group(1))


def test_small_wgrad_limits():
    P = R3.small_wgrad_plan
    assert P(1, 1, 177, 4, 8)["lds"] <= 65536 and P(1, 1, 178, 4, 8) is None and P(1, 1, 256, 3, 8) is not None
    assert P(1, 4, 4, 3, 12) is None and P(1, 4, 4, 512, 3) is None and P(1, 4, 4, 3, 256) is not None and P(1, 4, 4, 5, 8) is None
    assert P(1025, 4, 4, 1, 4)["grid"] == 1024 and P(2, 9, 13, 3, 16, 2 * 432 + 5)["grid"] == 2 and P(2, 9, 13, 3, 16, 431) is None
    assert {c.regime["loop"] for c in SMALLWG if "loop" in c.regime} == {"single", "row"}
    cb = {max(c.kw["Cin"], c.kw["Cout"]) for c in SMALLWG if "loop" in c.regime}
    assert {4, 8, 16, 64, 256} <= cb
    assert R3.splitk_slabs(27, 16, 234) == 8 and R3.splitk_slabs(36, 8, 178) == 6 and R3.splitk_slabs(576, 128, 1024) == 32


def test_grid_cap_slabs_have_teeth():
    """The 1025-image weight gradient is checked slab by slab on the GPU: both emulations leave the per-entry bound of the slabs, the
    slabs add up to the whole gradient, and end to end the two-piece operands would pass."""
    x, dy, _, blk = G.gridcap_refs(want_h=True)
    r2, rh = blk.ratios()
    print(f"grid cap: slabs two_piece {r2:.2f}, f16_drop {rh:.1f}")
    assert r2 > 1.0 and rh > 1.0
    whole = R3.conv3_wgrad(x, dy)["dw"]
    _close(blk.ref.sum(0), whole.ref, whole.bound, "sum of the slabs")
    _close(blk.bound.sum(0), whole.bound, whole.bound, "sum of the slab bounds")
    assert whole.ratios()[0] < 1.0
    assert R3.small_wgrad_plan(**G.GRIDCAP)["grid"] == 1024


# ---- the tables hold their leaves -----------------------------------------------------------------------------------------------
def test_tables_hold_their_leaves():
    ks = {k for c in G.CASES for k in c.expect}
    for cs in (1, 2, 3, 4):
        assert {G.k_cin(cs), G.k_cout(cs), G.k_swg(cs)} <= ks, cs
    for cin, cout in R3.RS_PAIRS:
        for np_ in (3, 2):
            for src in (False, True):
                for res in (False, True):
                    assert G.k_rs(cin, cout, src, res, np_) in ks, (cin, cout, src, res, np_)
        assert G.k_rs(cin, cout, False, True, 2, True) in ks
    assert {G.k_wg(2), G.k_wg(3)} <= ks
    entries = {c.kw.get("entry", "plain") for c in G.CASES if c.fn is D.p_conv3}
    assert entries == {"plain", "y", "res", "f", "s", "s2", "s_part"}
    assert {c.kw.get("entry", "plain") for c in G.CASES if c.fn is D.p_conv3_wgrad} == {"plain", "f", "s"}
    g3 = {k for c in GEMM3 for k in c.expect}
    assert {D.bf(128, 32, "ROW", "N"), D.bf(128, 64, "ROW", "N"), D.bf(128, 64, "COL", "N"), D.gen(128, 32), D.RED, D.BATCH, D.FIN} <= g3
    assert len(G.IDS) == len(set(G.IDS))
