"""CPU checks of tests/dense16_ref.py, the float64 reference behind tests/test_gpu_dense16.py.  For EVERY case of its table, built
with host=True:

- the degraded emulation (the hi lo' cross term dropped; for plane outputs of fp32 arithmetic, the lo plane dropped) FAILS the
  per-entry check on at least one output: the check has teeth before any GPU run (the per-case ratios are printed);
- a float32 evaluation on the CPU PASSES it on every output;
- the exact-arithmetic value of the shipped three-product form stays at or below 0.8 of it on every output;
- the regime the case names (the slice rule of the weight gradient, R / K4 of the first layer, the k-tile count) is the one its
  shape produces under the restated launcher arithmetic.

Plus: the plane arithmetic on the bit patterns, the yardstick C_TAIL is set from, the references against float64 autograd, and the
coverage the table is meant to have.
"""
import math

import pytest
import torch

import dense16_ref as R
import test_gpu_dense16 as G

F16, F32, F64 = torch.float16, torch.float32, torch.float64
_HOST = {}


def host(c):
    if c.id not in _HOST:
        _HOST.clear()  # one case at a time
        _HOST[c.id] = c.host()
    return _HOST[c.id]


@pytest.mark.parametrize("c", G.CASES, ids=G.IDS)
def test_case_on_the_host(c):
    p = host(c)
    deg, cpu, ship = [], [], []
    for label, rd in p.checks:
        assert rd["ref"].dtype == F64 and rd["tol"].dtype == F64 and rd["ref"].shape == rd["tol"].shape == rd["deg"].shape, label
        tol = rd["tol"] + 1e-30
        deg.append(R.ratio(rd["deg"], rd["ref"], tol))
        if "cpu" in rd:
            cpu.append(R.ratio(rd["cpu"], rd["ref"], tol))
            ship.append(R.ratio(rd["ship"], rd["ref"], tol))
    print(f"{c.id}: degraded {['%.3g' % r for r in deg]}, cpu fp32 {['%.3f' % r for r in cpu]}, shipped form {['%.3f' % r for r in ship]}")
    if p.checks:
        assert max(deg) > 1.0, f"the degraded emulation passes every output: {deg}"
    assert all(r <= 1.0 for r in cpu), f"a float32 evaluation leaves the tolerance: {cpu}"
    assert all(r <= 0.8 for r in ship), f"the exact shipped form is above 0.8 of the tolerance: {ship}"
    kw = c.kw
    if c.fn is G.p_first:
        k4, r_, ct, rgn = R.first_cfg(kw["M"], kw["N"], kw["K"])
        assert R.first_ok(kw["M"], kw["N"], kw["K"]) and f"-K4_{k4}-R{r_}-" in c.id and c.expect == (f"d16_first_kernel<{k4},{r_}>",)
        assert ct * rgn == 256 and kw["K"] == 4 * k4
        assert (r_ == 8) == (kw["M"] <= 2048) and (r_ == 40) == (kw["M"] > 5120)
        assert p.meta["hmax"] <= p.meta["bound_exact"]
    if c.fn in (G.p_fwd, G.p_bwd):
        nt = R.nt_tiles(kw["K"])
        assert f"-nt{nt}-" in c.id + "-" and p.meta["nt"] == nt and kw["K"] <= 1024
    if c.fn is G.p_wgrad:
        S, per, empty, mapping = R.wgrad_slices(kw["M"], kw["N"], kw["K"])
        assert f"-S{S}-per{per}-empty{len(empty)}-{mapping}-" in c.id and p.meta["chain"] <= 1024 and S <= 16
    if c.fn is G.p_pack:
        W = p.meta["W"]
        for w, inv in ((W, p.meta["want"]["nk_inv"]), (W.t(), p.meta["want"]["kn_inv"])):
            xs = w.double().abs() / inv.double()[:, None]
            assert float(xs[xs > 0].min()) >= 2.0 ** -14, "a non-zero scaled element is an fp16 subnormal"
            assert float(xs.max()) < 2.0 ** 14
        assert bool((W[kw["N"] // 2] == 0).all() and (W[:, kw["K"] // 3] == 0).all())
        amax = W.abs().amax(1)
        assert float(amax[amax > 0].max() / amax[amax > 0].min()) > (1e2 if kw["N"] > 8 else 1.0)


def test_wgrad_regimes_of_the_issue():
    want = {(17, 8, 16): (1, 1, [], "plain"), (150, 136, 136): (5, 1, [], "plain"), (300, 904, 904): (4, 3, [], "plain"),
            (300, 136, 72): (8, 2, [5, 6, 7], "xcd"), (264, 784, 512): (8, 2, [5, 6, 7], "xcd"),
            (520, 136, 72): (16, 2, list(range(9, 16)), "xcd"), (1024, 200, 256): (16, 2, [], "xcd")}
    for shape, w in want.items():
        assert R.wgrad_slices(*shape) == w, shape
    assert 520 - 8 * 2 * 32 == 8  # slice 8 of (520, 136, 72) holds 8 rows
    assert 5 * 2 * 32 > 264       # slice 5 of the workload's shape begins behind M
    assert {tuple(c.kw[k] for k in "MNK") for c in G.CASES if c.fn is G.p_wgrad} == set(want)
    # the workgroup -> (tile, slice) mapping runs every pair exactly once; under the XCD mapping a slice stays on one XCD
    for tiles, S in ((4, 5), (64, 4), (2, 8), (28, 8), (2, 16), (4, 16), (1, 1)):
        roles = [R.wgrad_block(L, tiles, S) for L in range(tiles * S)]
        assert sorted(roles) == [(t, z) for t in range(tiles) for z in range(S)]
        if S % 8 == 0:
            assert all(len({L % 8 for L, r in enumerate(roles) if r[1] == z}) == 1 for z in range(S))


def test_first_regimes_of_the_issue():
    shapes = [tuple(c.kw[k] for k in "MNK") for c in G.CASES if c.fn is G.p_first]
    assert shapes == [(9, 8, 4), (70, 16, 4), (300, 64, 12), (2048, 32, 20), (2049, 16, 8), (5121, 16, 4), (5130, 1024, 32),
                      (131, 512, 20), (40, 256, 28)]
    cfgs = [R.first_cfg(*s) for s in shapes]
    assert {c[0] for c in cfgs} == {1, 2, 3, 5, 7, 8} and [c[1] for c in cfgs] == [8, 8, 8, 8, 20, 40, 40, 8, 8]
    assert R.first_cfg(5130, 1024, 32)[2:] == (256, 1)
    assert not R.first_ok(64, 16, 36) and not R.first_ok(64, 16, 6) and not R.first_ok(64, 24, 8)
    opts = [(c.kw["bias"], c.kw["act"]) for c in G.CASES if c.fn is G.p_first]
    assert {b for b, _ in opts} == {True, False} and {a for _, a in opts} == {R.NONE, R.RELU, R.LEAKY}


def test_table_coverage():
    fwd = [c for c in G.CASES if c.fn is G.p_fwd]
    assert [(c.kw["M"], c.kw["N"], c.kw["K"], c.kw["xrows"]) for c in fwd] == [
        (1, 8, 8, 1), (65, 8, 32, 65), (64, 128, 40, 7), (129, 136, 72, 200), (63, 264, 96, 9), (200, 136, 200, 131), (70, 784, 512, 70)]
    for key, vals in (("bias", {True, False}), ("colsum", {True, False}), ("x_loose", {True, False}), ("scale", {0.75, 1.0})):
        default = dict(bias=True, colsum=True, x_loose=False, scale=0.75)[key]
        assert {c.kw.get(key, default) for c in fwd} == vals, key
    sat = [c for c in fwd if c.kw.get("sat")]
    assert sat and all(host(c).meta["premax"] > 12.0 for c in sat[:1])
    bwd = [c for c in G.CASES if c.fn is G.p_bwd]
    assert {(c.kw["M"], c.kw["N"], c.kw["K"]) for c in bwd} == {(1, 8, 8), (65, 16, 8), (129, 136, 72), (200, 64, 200), (70, 512, 784)}
    assert {c.kw["mask"] for c in bwd} == {True, False} and {c.kw["db"] for c in bwd} == {"off", "ws", "deferred"}
    mk = host(next(c for c in bwd if c.kw["mask"] and c.kw["M"] > 64)).meta["mask"]
    bits = {int(b) & 0xFFFF for b in mk.view(torch.int16).flatten().tolist()}
    assert set(G.MASK_BITS) <= bits
    wg = [c for c in G.CASES if c.fn is G.p_wgrad]
    assert {c.kw["finish"] for c in wg} == {"ws", "deferred"} and {c.kw["cs"] for c in wg} == {None, 1, 5}
    assert {(c.kw["N"], c.kw["K"]) for c in G.CASES if c.fn is G.p_pack} == {(8, 16), (96, 48), (200, 256), (72, 64)}
    un = [c.kw for c in G.CASES if c.fn is G.p_unsplit]
    assert {(k.get("rowf", False), k.get("tile", 0)) for k in un} == {(False, 0), (True, 0), (True, 8), (True, 128)}
    ks = {k for c in G.CASES for k in c.expect}
    assert {G.PACK, G.NT_FWD, G.NT_BWD, G.TN, G.SUM, G.UNSPLIT, G.D.BATCH} <= ks
    assert any(c.kw.get("loose") or c.kw.get("h_loose") for c in G.CASES) and len(G.IDS) == len(set(G.IDS))


def test_c_tail():
    """C_TAIL = twice the worst ratio of the float32 CPU tail over the forward table, and at least 4."""
    yard = {c.id: host(c).meta["yard"] for c in G.CASES if c.fn is G.p_fwd}
    print({k: round(v, 3) for k, v in yard.items()})
    need = max(4.0, 2 * max(yard.values()))
    assert need <= R.C_TAIL <= need + 0.5, (need, R.C_TAIL)


# ---- the plane arithmetic ------------------------------------------------------------------------------------------------------------------
def test_scale_functions():
    s = lambda v: float(R.f16_scale_of(v))  # noqa: E731
    assert s(0.0) == 2.0 ** 126 and s(1e-45) == 2.0 ** 126 and s(1e-39) == 2.0 ** 126, "zero and denormals"
    for k in (-100, -20, -1, 0, 1, 13, 14, 60, 100):
        x = 2.0 ** k
        up, dn = float(torch.nextafter(torch.tensor(x, dtype=F32), torch.tensor(math.inf))), \
            float(torch.nextafter(torch.tensor(x, dtype=F32), torch.tensor(0.0)))
        assert s(x) == s(up) == 2.0 ** (13 - k) and s(dn) == 2.0 ** (14 - k), k
        for v in (x, up, dn):
            assert 2.0 ** 13 <= v * s(v) < 2.0 ** 14
            assert float(R.f16_inv_scale(R.f16_scale_of(v))) * s(v) == 1.0
    assert s(2.0 ** 127) == 2.0 ** -114 and s(3e38) == 2.0 ** -114 and s(2.0 ** -126) == 2.0 ** 126  # the clamps
    assert float(R.f16_inv_scale(2.0 ** 126)) == 2.0 ** -126
    v = torch.tensor([0.0, 3.0, 1e-3], dtype=F32)
    assert R.f16_scale_of(v).tolist() == [2.0 ** 126, 2.0 ** 12, 2.0 ** 23]


def test_split_decode_round_trip():
    gen = R.g(5)
    bound = 3.0
    mag = torch.pow(2.0, -torch.rand(200000, generator=gen) * 28)  # down to 2^-28 of the bound
    x = (bound * mag * (torch.randint(0, 2, mag.shape, generator=gen) * 2 - 1)).float()
    hi, lo, inv = R.tensor_planes(x, bound)
    s = float(R.f16_scale_of(bound))
    xs = (x.double() * s).abs()
    err = (R.decode(hi, lo, inv) - x.double()).abs() * s
    # 2^-23 |x s| wherever the pre-scaled lo is a normal fp16 number for certain: |x s| >= 2^-13.  In the binade below (down to 2^-28 of
    # a bound with bound s = 2^14) hi is still normal but lo = (x s - hi) 2048 <= 2^-14 is an fp16 subnormal, rounded to 2^-25: an
    # absolute 2^-36 of the scaled value (measured: up to 2.67 x 2^-23 |x s| there), still 2^-49 of the bound.
    assert bool((err[xs >= 2.0 ** -13] <= 2.0 ** -23 * xs[xs >= 2.0 ** -13]).all())
    assert bool((xs >= 2.0 ** -14.5).all()) and bool((err[xs < 2.0 ** -13] <= 2.0 ** -36).all()) and int((xs < 2.0 ** -13).sum()) > 1000
    assert bool(torch.isfinite(hi.float()).all() and torch.isfinite(lo.float()).all())
    # far below: the absolute floor, 2^-39 of the bound
    tiny = (bound * torch.pow(2.0, -28 - torch.rand(1000, generator=gen) * 30)).float()
    hi, lo, inv = R.tensor_planes(tiny, bound)
    assert float((R.decode(hi, lo, inv) - tiny.double()).abs().max()) <= R.FLOOR * bound
    # per-row scales
    W = R.spread_rows(16, 32, gen, 3.0)
    hi, lo, inv = R.row_planes(W)
    assert bool(((R.decode(hi, lo, inv[:, None]) - W.double()).abs() <= 2.0 ** -23 * W.double().abs() + 1e-300).all())
    assert bool((hi.float().abs().amax(1) >= 2.0 ** 13).all() and (hi.float().abs().amax(1) <= 2.0 ** 14).all())


# ---- the references ------------------------------------------------------------------------------------------------------------------------
def test_references_agree_with_autograd():
    gen = R.g(9)
    M, N, K, xrows, scale, gw = 5, 8, 8, 3, 0.75, 0.2
    a = R.spread_rows(M, K, gen, 1.0)
    A = R.tensor_planes(a, float(a.abs().max()))
    B = R.row_planes(R.spread_rows(N, K, gen, 1.0) * 0.3)
    b = torch.randn(N, generator=gen)
    X = torch.rand(xrows, N, generator=gen)
    r = R.gemm_nt(A, B, float(a.abs().max()))
    A64 = R.decode(*A)
    B64 = R.decode(B[0], B[1], B[2][:, None])
    assert torch.allclose(r["ref"], A64 @ B64.t(), rtol=1e-13) and torch.allclose(r["ship"], r["ref"], rtol=0, atol=float(2.0 ** -21 * r["absum"].max()))
    t = R.nll_tail(r, b, X, xrows, scale, gw, 1.0)
    inv_s2, k, row_const, _ = R.nll_consts(scale, gw, N, 1.0)
    pre = (r["ref"] + b.double()).requires_grad_()
    rows = (0.5 * inv_s2 * (torch.sigmoid(pre) - X.double()[torch.arange(M) % xrows]) ** 2).sum(1)
    (rows.sum() * float(torch.tensor(gw, dtype=F32))).backward()
    assert torch.allclose(t["G"]["ref"], pre.grad, rtol=1e-12, atol=1e-18)
    assert torch.allclose(t["rows"]["ref"][0], rows.detach() + row_const, rtol=1e-13)
    assert abs(row_const - N * (math.log(scale) + 0.5 * math.log(2 * math.pi))) <= 4 * 2.0 ** -24 * abs(row_const)
    assert torch.allclose(t["colsum"]["ref"][0], t["G"]["ref"].sum(0), rtol=1e-13)
    d = R.spread_rows(M, N, gen, 1.0)
    Dp = R.tensor_planes(d, float(d.abs().max()))
    assert torch.allclose(R.gemm_tn(Dp, A, 1.0, 1.0)["ref"], R.decode(*Dp).t() @ A64, rtol=1e-13)
    mk = torch.tensor([[0x0000, 0x8000 - 0x10000, 0x0001, 0x8001 - 0x10000, 0x3C00, 0xBC00 - 0x10000, 0x03FF, 0x7BFF]], dtype=torch.int16)
    assert R.relu_mask(mk.view(F16)).tolist() == [[0, 0, 1, 0, 1, 0, 1, 1]]
    assert R.relu_mask(mk.view(F16)).tolist() == (mk.view(F16).float() > 0).double().tolist()
