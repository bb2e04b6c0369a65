"""CPU checks of tests/skinny_ref.py, the references and tables behind tests/test_gpu_skinny.py:

- the `*_plan` functions are pinned to hand-computed rows read off skinny.hip (slices and slice widths of the split, the caps, the
  LDS of the heads' backward, K4 / R / weight-load branch of the short-reduction kernel, every decline);
- the references are pinned to torch's float64 autograd of the same modules: two Linear heads on a ReLU / sigmoid / LeakyReLU
  layer, and two Conv2d(C, L, 4, 2, 0) heads on a 4 x 4 map behind a convolution's channel bias for flat_c;
- every `check_*` routine of the GPU file runs on every case with a stand-in backend: the plain fp32 CPU evaluation in the kernels'
  summation order (waves, slices, row groups on their own, then added in order).  Each of them asserts, per output, that the
  two-piece bf16 emulation leaves the bound on at least one entry: no case and no output is exempt;
- the case tables hold the edges the kernel text has.
"""
import pytest
import torch
import torch.nn.functional as F

import skinny_ref as R
import test_gpu_gemm_dispatch as D
import test_gpu_skinny as G

F64 = torch.float64


# ---- host arithmetic on hand-computed rows ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,tiles_shape,nz,kz", [
    (2048, (32, 32), 8, 256),      # 2048 / 256 = 8 slices of 256
    (2052, (32, 32), 8, 272),      # 8 slices of ceil(2052 / 8) = 257 -> 272; 7 x 272 = 1904, the last is 148 wide
    (2304, (32, 32), 9, 256),
    (2816, (32, 32), 11, 256),
    (16384, (512, 16), 64, 256),   # exactly the cap of 64: not capped
    (16640, (512, 16), 62, 272),   # 65 -> 64 slices of 260 -> 272; ceil(16640 / 272) = 62
    (16640, (496, 16), 65, 256),   # 31 tiles: cap 128
    (32768, (16, 16), 128, 256),
    (33024, (16, 16), 122, 272),   # 129 -> 128 slices of 258 -> 272; ceil(33024 / 272) = 122
])
def test_heads_plan_split(K, tiles_shape, nz, kz):
    M, N = tiles_shape
    p = R.heads_plan(M, N, K, ws_floats=1 << 40)
    assert (p.nz, p.kz) == (nz, kz) and p.kernels == [R.H16, R.HFIN] and p.grid == (R.cdiv(M, 16), R.cdiv(N, 16), nz)
    assert nz * kz >= K > (nz - 1) * kz and kz % 16 == 0
    need = nz * M * N
    assert R.heads_plan(M, N, K, ws_floats=need).nz == nz and R.heads_plan(M, N, K, ws_floats=need - 1).nz == 1
    assert R.heads_plan(M, N, K, ws_floats=0).kernels == [R.H16]


def test_heads_plan_rules():
    big = 1 << 40
    assert R.heads_plan(32, 32, 2047 - 3, ws_floats=big).nz == 1          # K < 2048
    assert R.heads_plan(256, 64, 2048, ws_floats=big).nz == 8 and R.heads_plan(208, 80, 2048, ws_floats=big).nz == 1  # 64 | 65 tiles
    assert R.heads_plan(512, 16, 2048, ws_floats=big).grid == (32, 1, 8) and R.heads_plan(528, 16, 2048, ws_floats=big).grid == (33, 1, 8)
    assert R.heads_plan(1024, 17, 64).kernels == [R.NARROW] and R.heads_plan(1023, 17, 64).kernels == [R.H4]
    assert R.heads_plan(1024, 16, 64).kernels == [R.H4] and R.heads_plan(1024, 33, 64).kernels == [R.H4]
    assert R.heads_plan(17, 20, 1020).kernels == [R.H4] and R.heads_plan(17, 20, 1024).kernels == [R.H16]
    assert R.heads_plan(1025, 20, 64).declines == ["M > 1024"] and R.heads_plan(17, 20, 60).declines == ["K < 64"]
    assert R.heads_plan(17, 1024, 2052).declines == ["N K > 2^21"] and R.heads_plan(17, 20, 66).declines == ["K % 4 != 0"]
    assert R.heads_plan(17, 20, 64, aligned=(False, True)).declines == ["X unaligned"]
    assert R.heads_plan(17, 33, 64, heads=2, via="heads").declines == ["N > 32", "two heads and N > 32"]
    assert R.heads_plan(17, 20, 400, heads=2, via="heads", ws_floats=big).grid == (2, 4, 1)
    # wvec: torch Linear rows, K % 4 == 0 rows, both bases on 16 bytes
    assert R.heads_plan(17, 20, 64, w_sk=1, w_sn=64).wvec == 1 and R.heads_plan(17, 20, 64, w_sk=1, w_sn=64, aligned=(True, False)).wvec == 0
    assert R.heads_plan(17, 20, 64, w_sk=20, w_sn=1).wvec == 0
    # the last slice of K = 2052 is 148 wide: kw = 16, waves 10 .. 15 start past its end
    last = R.heads_waves(2052, 8, 272, 16)[-1]
    assert last[0] == (1904, 1920) and last[9] == (2048, 2052) and all(a >= e for a, e in last[10:])
    assert R.heads_waves(4, 1, 0, 4)[0] == [(0, 4), (16, 4), (32, 4), (48, 4)]
    assert R.heads_waves(60, 1, 0, 4)[0][-1] == (48, 60)


def test_heads_bwd_plan_rows():
    p = R.heads_bwd_plan(300, 32, 48, 2)
    assert p.lds_bytes == 61952 == 4 * (128 * 65 + 64 * 16 + 2 * 128 * 20 + 1024) and p.grid == (3, 3) and not p.declines
    assert R.heads_bwd_plan(512, 20, 2048, 2).lds_bytes == 4 * (128 * 41 + 40 * 16 + 5120 + 1024)  # 48 KB for the 2 x 20 heads
    assert R.heads_bwd_plan(1, 1, 16, 1).lds_bytes == 4 * (128 + 16 + 5120 + 1024)  # NN = 1 = NNP
    assert R.heads_bwd_plan(1, 1, 16, 2).lds_bytes == 4 * (384 + 32 + 5120 + 1024)  # NN = 2, NNP = 3
    assert [R.heads_bwd_plan(M, 4, 16, 1).rgs for M in (1, 127, 128, 129, 8192)] == [1, 1, 1, 2, 64]
    assert R.heads_bwd_plan(8193, 4, 16, 1).declines == ["more than 64 row groups"]
    assert R.heads_bwd_plan(17, 33, 48, 1).declines == ["N > 32"] and R.heads_bwd_plan(17, 20, 24, 1).declines == ["K % 16 != 0"]
    assert R.heads_bwd_plan(17, 20, 48, 2, 5).declines == ["flat_c does not divide K"]
    assert R.heads_bwd_plan(17, 20, 48, 2, x_aligned=False).declines == ["X unaligned"]
    s = R.heads_bwd_plan(129, 17, 48, 2, 4).slabs  # two row groups, 12 partial rows of 4 channels per group
    assert s == dict(dW0=1632, dW1=1632, db0=36, db1=36, dbprev=96, prow=12, pc=4)
    assert R.heads_bwd_plan(129, 17, 48, 1).slabs == dict(dW0=1632, db0=36, dbprev=96, prow=1, pc=48)
    assert R.bwd_ws_need(R.BWD_BY_NAME["nobias"]) == 2 * 2 * 20 * 48 + 2 * 40 + 96  # the NULL bias targets still take their slabs
    assert R.bwd_ws_need(R.BWD_BY_NAME["mixed"]) == 3 * 20 * 48 + 2 * 60 + 144 and R.bwd_ws_need(R.BWD_BY_NAME["nodx"]._replace(targets="deferred")) == 0
    assert R.bwd_kernels(R.BWD_BY_NAME["n17-2h-M129"]) == sorted([R.HBWD, R.FIN, R.FINS])  # dW (816) and dbprev (48) float4, db (17) scalar
    assert R.bwd_kernels(R.BWD_BY_NAME["n1-1h-M1-K16"]) == sorted([R.HBWD, R.FIN, R.FINS])
    assert R.bwd_kernels(R.BWD_BY_NAME["nobias"]) == sorted([R.HBWD, R.FIN])


def test_python_estimate_covers_the_c_side():
    """kernels.heads_bwd returns None (separate launches) above its own estimate of the scratch; the C side declines with MVK_EINVAL,
    which the wrapper raises, above the rounded sum of the slabs.  The first must never be the smaller one, with or without flat_c."""
    for M in (1, 127, 129, 300, 8192):
        for N in (1, 17, 20, 32):
            for K in (16, 48, 512, 2048):
                for nh in (1, 2):
                    for flat_c in (0, 4, K):
                        s = R.heads_bwd_plan(M, N, K, nh, flat_c).slabs
                        c_need = sum(v for k, v in s.items() if k not in ("prow", "pc"))
                        assert R.python_ws_estimate(M, N, K, nh) >= c_need, (M, N, K, nh, flat_c)


def test_smallk_plan_rows():
    P = R.smallk_plan
    assert [P(19, 12, K, "kn").K4 for K in (1, 4, 5, 12, 13, 24, 25, 28, 29, 32)] == [1, 1, 2, 3, 4, 6, 7, 7, 8, 8]
    assert {P(19, 12, K, "nk").branch for K in range(1, 33) if K % 4} == {"scalar"} and {P(19, 12, K, "nk").branch for K in range(4, 33, 4)} == {"rows_nk"}
    assert {P(19, 12, K, "kn").branch for K in range(1, 33)} == {"rows_kn"}
    assert P(19, 12, 20, "kn", dict(W=False)).branch == "scalar" and P(19, 12, 20, "nk", dict(W=False)).branch == "scalar"
    assert P(19, 12, 20, "kn", dict(X=False)).branch == "rows_kn" and not P(19, 12, 20, "kn", dict(X=False)).declines
    assert P(19, 12, 20, "kn", dict(Y=False)).declines == ["Y unaligned"]
    assert P(19, 12, 33, "kn").declines == ["K outside 1 .. 32"] and P(19, 6, 20, "kn").declines == ["N % 4 != 0"]
    # R: want = (M gy + 255) / 256 <= 8
    assert (P(2048, 400, 20, "kn").R, P(2049, 400, 20, "kn").R) == (8, 16) and P(2049, 400, 20, "kn").grid == (129, 1)
    assert (P(1024, 2048, 20, "kn").R, P(1025, 2048, 20, "kn").R) == (8, 16) and P(1025, 2048, 20, "kn").grid == (65, 2)
    assert P(37, 1024, 20, "kn").grid == (5, 1) and P(37, 1028, 20, "kn").grid == (5, 2) and P(5120, 2048, 20, "kn").R == 16


# ---- the references against torch's float64 autograd ---------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [R.RELU, R.SIGMOID, R.LEAKY, R.NONE])
def test_linear_heads_reference_is_autograd(act):
    g = R.gen(f"autograd{act}")
    M, K, N = 37, 48, 17
    z = torch.randn(M, K, generator=g, dtype=F64)
    bprev = torch.randn(K, generator=g, dtype=F64).requires_grad_(True)
    Ws = [torch.randn(N, K, generator=g, dtype=F64).requires_grad_(True) for _ in range(2)]
    bs = [torch.randn(N, generator=g, dtype=F64).requires_grad_(True) for _ in range(2)]
    dys = [torch.randn(M, N, generator=g, dtype=F64) for _ in range(2)]
    fn = {R.RELU: torch.relu, R.SIGMOID: torch.sigmoid, R.LEAKY: lambda t: F.leaky_relu(t, D.F02), R.NONE: lambda t: t}[act]
    x = fn(z + bprev)
    x.retain_grad()
    ys = [x @ W.t() + b for W, b in zip(Ws, bs)]
    sum((y * dy).sum() for y, dy in zip(ys, dys)).backward()
    x32 = x.detach().float()  # the kernel reads the stored fp32 output: its mask is act'(x32)
    mine = R.heads_bwd_ref(x32, act, [d.float() for d in dys], [W.detach().float() for W in Ws])
    close = lambda a, b: torch.allclose(a, b, rtol=1e-5, atol=1e-6)  # noqa: E731  (fp32 casts of the operands)
    for h in range(2):
        assert close(mine[f"dW{h}"].ref, Ws[h].grad) and close(mine[f"db{h}"].ref, bs[h].grad)
    assert close(mine["dbprev"].ref, bprev.grad)
    fwd = R.fwd_ref(x32, Ws[0].detach().float().t(), bs[0].detach().float(), act)
    assert close(fwd.ref, fn(ys[0].detach()))
    # dX: the gradient that reaches the pre-activation
    pre_grad = bprev.grad  # column sums of it
    assert close(mine["dX"].ref.sum(0), pre_grad)
    assert bool((mine["dX"].bound + 1e-12 >= mine["dX"].ref.abs()).all())


def test_conv_heads_reference_is_autograd():
    """Two Conv2d(C, L, 4, 2, 0) heads on a 4 x 4 map: X is the NHWC map flattened (k = tap * C + c), the weight gradient comes in
    the [L][C][4][4] layout, the bias gradient of the layer below per channel."""
    g = R.gen("convheads")
    M, C, L = 9, 8, 5
    z = torch.randn(M, C, 4, 4, generator=g, dtype=F64)
    bprev = torch.randn(C, generator=g, dtype=F64).requires_grad_(True)
    Wc = [torch.randn(L, C, 4, 4, generator=g, dtype=F64).requires_grad_(True) for _ in range(2)]
    dys = [torch.randn(M, L, generator=g, dtype=F64) for _ in range(2)]
    h = torch.relu(z + bprev.view(1, C, 1, 1))
    sum((F.conv2d(h, W, None, stride=2).view(M, L) * dy).sum() for W, dy in zip(Wc, dys)).backward()
    x = h.detach().permute(0, 2, 3, 1).reshape(M, 16 * C).float()
    ws = [W.detach().permute(0, 2, 3, 1).reshape(L, 16 * C).float() for W in Wc]  # W(n, k = tap * C + c)
    mine = R.heads_bwd_ref(x, R.RELU, [d.float() for d in dys], ws, flat_c=C)
    close = lambda a, b: torch.allclose(a, b, rtol=1e-5, atol=1e-6)  # noqa: E731
    for i in range(2):
        assert close(mine[f"dW{i}"].ref.view(L, C, 4, 4), Wc[i].grad)
    assert close(mine["dbprev"].ref, bprev.grad)


# ---- the stand-in backend: fp32 on the CPU in the kernels' summation order ------------------------------------------------------------
class Standin:
    def fwd(self, c, inp, ws_floats, names=True):
        plan, _ = R.fwd_plan(c)
        Y = [R.heads_fwd_f32(inp["x"], w, b, c.act, plan) for w, b in zip(inp["w"], inp["b"])]
        ws = None
        if ws_floats > 0:
            ws = torch.zeros(ws_floats) if plan.nz > 1 else torch.full((ws_floats,), float("nan"))
        return dict(Y=Y, guards=True, kernels=None, rc=0, ws=ws)

    def smallk(self, c, inp, preset=None, launches=1, names=True):
        al = dict(W=c.off != "W", Y=c.off != "Y", X=c.off != "X")
        if c.via == "amax" and R.smallk_plan(c.M, c.N, c.K, c.layout, al).declines:
            return dict(Y=torch.full((c.M, c.N), float("nan")), amax=[torch.tensor([preset])], guards=True, kernels=None, rc=G.EINVAL)
        Y = R.smallk_f32(inp["x"], inp["w"], inp["bias_full"], c.act)
        amax = [torch.tensor([max(float(Y.abs().max()), preset)], dtype=torch.float32)] * launches if c.via == "amax" else []
        return dict(Y=Y, amax=amax, guards=True, kernels=None, rc=0)

    def bwd(self, c, inp, inits, ws_floats, off=None, names=True):
        p = R.heads_bwd_plan(c.M, c.N, c.K, c.nh, c.flat_c, x_aligned=off != "X", dx_aligned=off != "dX")
        if p.declines or ws_floats < R.bwd_ws_need(c):
            out = {k: v.clone() for k, v in inits.items()}
            out["dX"] = torch.full((c.M, c.K), float("nan"))
            return dict(out=out, guards=True, kernels=None, rc=G.EINVAL, ws=None)
        out = R.heads_bwd_f32(inp["x"], c.x_act, inp["dys"], inp["ws"], c.flat_c, inits)
        if not c.dx:
            out["dX"] = None
        return dict(out=out, guards=True, kernels=None, rc=0, ws=None)


BE = Standin()
WORST = {}


@pytest.mark.parametrize("c", R.FWD_CASES, ids=[c.name for c in R.FWD_CASES])
def test_check_fwd(c):
    G.check_fwd(c, BE, WORST)


@pytest.mark.parametrize("c", R.SK_CASES, ids=[c.name for c in R.SK_CASES])
def test_check_smallk(c):
    G.check_smallk(c, BE, WORST)


@pytest.mark.parametrize("c", R.AMAX_CASES, ids=[c.name for c in R.AMAX_CASES])
def test_check_amax(c):
    G.check_amax(c, BE, WORST)
    G.check_amax_declines(BE)


@pytest.mark.parametrize("c", R.BWD_CASES, ids=[c.name for c in R.BWD_CASES])
def test_check_bwd(c):
    G.check_bwd(c, BE, WORST)


@pytest.mark.parametrize("d", R.BWD_DECLINES, ids=[d.name for d in R.BWD_DECLINES])
def test_check_bwd_decline(d):
    G.check_bwd_decline(d, BE)
    plan = R.heads_bwd_plan(d.M, d.N, d.K, d.nh, d.flat_c, x_aligned=d.off != "X", dx_aligned=d.off != "dX")
    assert bool(plan.declines) != d.ws_short, d.name  # one reason each: the shape, or the workspace alone


def test_bounds_reject_a_wrong_kernel():
    """What a subtly wrong kernel would give leaves the bound: a quiet term dropped, the last slice dropped, a row group added
    twice, the flat_c permutation left out, the activation mask of the wrong code."""
    c = R.FWD_BY_NAME["fin-K2052"]
    inp, (plan, _) = R.fwd_inputs(c), R.fwd_plan(c)
    ref = R.fwd_ref(inp["x"], inp["w"][0], inp["b"][0], c.act)
    quiet = int((inp["x"].abs().mean(0) < 0.01).nonzero()[5])
    x = inp["x"].clone()
    x[:, quiet] = 0
    assert R.ratios(R.heads_fwd_f32(x, inp["w"][0], inp["b"][0], c.act, plan), ref)[0] > 1
    assert R.ratios(R.heads_fwd_f32(inp["x"], inp["w"][0], inp["b"][0], c.act, plan._replace(nz=7)), ref)[0] > 1
    b = R.BWD_BY_NAME["flat4-2h-def"]
    bi, inits = R.bwd_inputs(b.M, b.N, b.K, b.nh, b.x_act, b.name), R.bwd_inits(b)
    r = R.heads_bwd_ref(bi["x"], b.x_act, bi["dys"], bi["ws"], b.flat_c)
    good = R.heads_bwd_f32(bi["x"], b.x_act, bi["dys"], bi["ws"], b.flat_c, inits)
    assert all(R.ratios(good[k], r[k], inits.get(k))[0] <= 1 for k in r)
    noperm = R.heads_bwd_f32(bi["x"], b.x_act, bi["dys"], bi["ws"], 0, {k: v for k, v in inits.items() if k != "dbprev"})
    assert R.ratios(noperm["dW0"], r["dW0"], inits["dW0"])[0] > 1
    leaky = R.heads_bwd_f32(bi["x"], R.NONE, bi["dys"], bi["ws"], b.flat_c, inits)
    assert R.ratios(leaky["dX"], r["dX"])[0] > 1 and R.ratios(leaky["dbprev"], r["dbprev"], inits["dbprev"])[0] > 1
    twice = {k: good[k] + (good[k] - inits[k]) / 3 for k in inits}  # one of three row groups counted twice, on average
    assert all(R.ratios(twice[k], r[k], inits[k])[0] > 1 for k in inits)


def test_case_tables_hold_the_edges():
    """The shapes the issue asks for, read off the launch code of skinny.hip."""
    bw = R.BWD_CASES
    assert {(c.nh, c.N) for c in bw} >= {(2, 32), (1, 1), (2, 1), (1, 17), (2, 17), (1, 32), (2, 20)}
    assert {c.M for c in bw} >= {1, 127, 128, 129, 300, 8192} and {c.K for c in bw} >= {16, 48, 512}
    assert {c.x_act for c in bw} == set(R.ACTS) and {c.layout for c in bw} == {"nk", "kn"}
    assert {(c.nh, c.flat_c == c.K, c.flat_c > 0) for c in bw if c.flat_c} >= {(1, False, True), (2, False, True), (1, True, True), (2, True, True)}
    assert {c.targets for c in bw} == {"plain", "deferred", "mixed"} and {c.via for c in bw} == {"c", "py"}
    assert {(c.dx, c.dbprev, c.bias) for c in bw} >= {(True, True, True), (False, True, True), (True, False, True), (True, True, False)}
    assert any(c.flat_c and c.nh == 1 and c.dbprev and c.targets == "plain" for c in bw)  # nrows = nz * prow in colsum_finish_any
    assert all(c.why for c in bw) and all(bool((t != 0).all()) for c in bw for t in R.bwd_inits(c).values())
    assert {d.name for d in R.BWD_DECLINES} == {"N33", "K24", "M8193", "flat5", "ws-short", "x-off", "dx-off"}
    fw = {c.name: R.fwd_plan(c)[0] for c in R.FWD_CASES}
    assert {fw[n].nz for n in ("fin-K2048", "fin-K2304", "fin-K2816", "fin-K2052", "fin-cap64", "fin-cap128")} == {8, 9, 11, 62, 122}
    assert fw["fin-K4096-short"].kernels == [R.H16] and fw["fin-K4096"].nz == 16 and fw["fin-65tiles"].nz == 1 and fw["fin-64tiles"].nz == 8
    assert fw["hf-nk-woff-2h"].wvec == 0 and fw["hf-nk-2h-N16"].wvec == 1 and fw["hf-kn-2h-N1"].wvec == 0
    assert {c.act for c in R.FWD_CASES if R.HFIN in fw[c.name].kernels} == set(R.ACTS)
    assert {c.M for c in R.FWD_CASES if c.via == "heads"} >= {1, 15, 16, 17} and {c.K for c in R.FWD_CASES if c.via == "heads"} >= {4, 60}
    sk = R.SK_CASES
    assert {R.smallk_plan(c.M, c.N, c.K, c.layout).K4 for c in sk} == set(range(1, 9))
    assert {c.N for c in sk} >= {4, 400, 1024, 1028, 2048} and {c.bias_mod for c in sk} >= {None, 0, 1, 128, 1028}
    assert {c.off for c in sk} == {None, "W", "X", "Y"} and {c.via for c in sk} == {"gemm", "linear"}
    assert {(R.smallk_plan(c.M, c.N, c.K, c.layout).R, c.M % 16 != 0) for c in sk} >= {(8, True), (16, True)}
    assert {c.peak for c in R.AMAX_CASES} == {"first", "last", "tail", "neg"} and any(c.M == 1 for c in R.AMAX_CASES)
    for c in R.AMAX_CASES:
        if c.peak == "tail":
            assert c.M % R.smallk_plan(c.M, c.N, c.K, c.layout).R != 0
        if c.act in (R.RELU, R.LEAKY):  # a maximum taken in front of the activation would be twice the right one
            i = R.amax_inputs(c)
            pre = R.smallk_f32(i["x"], i["w"], i["bias_full"], R.NONE)
            assert float(pre.abs().max()) > 1.5 * float(R.act32(pre, c.act).abs().max()), c.name
    names = [c.name for t in (R.FWD_CASES, R.SK_CASES, R.AMAX_CASES, R.BWD_CASES) for c in t]
    assert len(names) == len(set(names))


def test_zz_standin_report():
    print("STANDIN_WORST", {k: (round(v[0], 3), v[1], round(v[2], 2)) for k, v in sorted(WORST.items())})
