"""CPU checks of tests/conv4s2_rs_ref.py, the float64 reference behind tests/test_gpu_conv4s2_rs.py.  For EVERY case of its table:

- the degraded emulation of the case's form (bf16 pieces: two pieces per operand; scaled fp16: the hi lo' cross term dropped) FAILS
  the per-entry check on at least one output: the check has teeth before any GPU run (the per-case ratios are printed);
- torch's float32 conv2d / conv_transpose2d / conv2d_weight on the CPU PASSES it on every output: the tolerance admits a correct
  fp32 implementation, and the reference alone stays inside it;
- the case's named regime (the set of tiles-per-worker counts, or the accumulator chain of a weight gradient) is the one its batch
  produces under the restated host arithmetic.

Plus: the restated arithmetic against the numbers the kernels' configuration structs fix, the XCD remap as a permutation, the
references against float64 autograd, and the coverage the table is meant to have.
"""
import pytest
import torch
import torch.nn.functional as F

import conv4s2_rs_ref as R
import test_gpu_conv4s2_rs as G
import test_gpu_gemm_dispatch as D

F64 = torch.float64
_HOST = {}


def host_outs(c):
    if c.id not in _HOST:
        _HOST.clear()  # one case at a time: the largest hold a few hundred MB of float64
        _HOST[c.id] = c.host()
    return _HOST[c.id]


@pytest.mark.parametrize("c", G.CASES, ids=G.IDS)
def test_case_on_the_host(c):
    p = host_outs(c)
    deg, cpu = [], []
    for o in p.outs:
        assert o.ref.dtype == F64 and o.bound.dtype == F64 and o.ref.shape == o.bound.shape == o.deg.shape == o.cpu.shape
        assert bool((o.bound + 1e-300 >= o.ref.abs() * (1 - 1e-12)).all()), "the bound is below its own reference"
        tol = D.C_ENTRY * o.bound + 1e-30
        deg.append(float(((o.deg - o.ref).abs() / tol).max()))
        cpu.append(float(((o.cpu - o.ref).abs() / tol).max()))
    scaled = c.kw.get("scaled", False)
    print(f"{c.id}: {'f16_drop' if scaled else 'two_piece'} {['%.2f' % r for r in deg]}, cpu fp32 {['%.3f' % r for r in cpu]}")
    assert max(deg) > 1.0, f"the degraded emulation passes every output: {deg}"
    assert max(cpu) <= 1.0, f"a float32 convolution leaves the tolerance: {cpu}"
    if scaled:
        assert p.outs[0].deg is p.outs[0].degh or torch.equal(p.outs[0].deg, p.outs[0].degh)
    # the regime the id names
    if isinstance(c.regime, set):
        assert R.regime(c.kw["n"], c.kw["kind"], c.kw["pair"]) == c.regime
        if "-tpw" in c.id:
            assert c.id.endswith("tpw" + "_".join(map(str, sorted(c.regime))))
    elif isinstance(c.regime, dict):
        assert R.wgrad_chain(c.kw["n"], c.kw["pair"]) == c.regime["chain"] <= 1024
        if "-chain" in c.id:
            assert c.id.endswith(f"chain{c.regime['chain']}")


# ---- the restated arithmetic -----------------------------------------------------------------------------------------------------------------
def test_configuration_numbers():
    """ICfg / WCfg of csrc/imgconv.hip for the four forward instantiations and the two weight-gradient ones."""
    P8, P4 = R.PAIRS
    want = {("down", P8): dict(kind=1, cin=32, cout=64, ksplit=2, nct=2, roles=4, types=1, su=1, tpu=2, products=512),
            ("up", P8): dict(kind=0, cin=64, cout=32, ksplit=1, nct=1, roles=4, types=1, su=1, tpu=2, products=256),
            ("down", P4): dict(kind=1, cin=64, cout=128, ksplit=4, nct=4, roles=16, types=4, su=2, tpu=1, products=1024),
            ("up", P4): dict(kind=0, cin=128, cout=64, ksplit=2, nct=2, roles=16, types=4, su=2, tpu=1, products=512)}
    for (kind, pair), w in want.items():
        c = R.cfg(kind, pair)
        assert {k: c[k] for k in w} == w, (kind, pair)
        assert R.workers(kind, pair) == (256 if pair == P8 else 64)
        assert R.frag_bytes(kind, pair) == 16 * pair[1] * pair[2] * 3 * 2  # every weight element on three bf16 pieces
    assert R.wcfg(*P8) == dict(pix=64, types=1, su=1, ks=4) and R.wcfg(*P4) == dict(pix=16, types=4, su=2, ks=2)
    assert R.workers("wgrad", P8) == 256 and R.workers("wgrad", P4) == 64
    assert R.min_wgrad_scratch(P8) == 256 * 16 * 32 * 64 and R.min_wgrad_scratch(P4) == 64 * 16 * 64 * 128
    assert R.kernel_name("down", P8, True, 2) == "imgconv_kernel<1,8,32,64,true,true,2>"
    assert R.kernel_name("up", P4, False, 3) == "imgconv_kernel<0,4,128,64,false,true,3>"
    assert R.wgrad_kernel_name(P4, 2) == "imgwgrad_kernel<4,64,128,2>"


def test_regimes_of_the_issue():
    P8, P4 = R.PAIRS
    for kind in ("down", "up"):
        assert [R.regime(n, kind, P8) for n in (1, 256, 300, 768)] == [{0, 2}, {2}, {2, 4}, {6}]
        assert [R.regime(n, kind, P4) for n in (2, 128, 130, 256, 384, 700)] == [{0, 1}, {1}, {1, 2}, {2}, {3}, {5, 6}]
        for pair in R.PAIRS:
            for n in (1, 2, 5, 130, 300, 700, 5120):
                rng = R.unit_ranges(n, kind, pair)
                assert rng[0][0] == 0 and rng[-1][1] == R.units(n, kind, pair) and all(a[1] == b[0] for a, b in zip(rng, rng[1:]))
    assert R.wgrad_chain(4, P8) == 64 and R.wgrad_chain(300, P8) == 128 and R.wgrad_chain(1024, P8) == 256
    assert R.wgrad_chain(4, P4) == 32 and R.wgrad_chain(130, P4) == 64 and R.wgrad_chain(2048, P4) == 512
    assert R.wgrad_chain(5120, P8) == 1280 and R.wgrad_chain(5120, P4) == 1280  # the workload's batch: longer than the table reaches
    busy = [i for i, (_, k, _) in enumerate(R.wgrad_chains(4, P8)) if k]
    assert busy == [63, 127, 191, 255]  # n = 4: most workers own nothing
    # every image of a launch is summed by exactly one worker
    for pair, n in ((P8, 300), (P4, 130)):
        ch = R.wgrad_chains(n, pair)
        assert sum(k for _, k, _ in ch) == n and all(a[0] + a[1] == b[0] for a, b in zip(ch, ch[1:]))


def test_xcd_remap_is_a_permutation():
    """Under the remap (4 workgroup types, grid 256) every (worker, type) runs exactly once, and the four types of a worker sit on
    one XCD (b % 8); a grid that is no multiple of 32 keeps the plain division."""
    roles = [R.block_role(b, 4) for b in range(256)]
    assert sorted(roles) == [(w, t) for w in range(64) for t in range(4)]
    for w in range(64):
        assert len({b % 8 for b, r in enumerate(roles) if r[0] == w}) == 1
    assert roles[0] == (0, 0) and roles[8] == (0, 1) and roles[32] == (1, 0) and roles[1] == (8, 0)
    assert [R.block_role(b, 4, 252) for b in (0, 1, 4, 251)] == [(0, 0), (0, 1), (1, 0), (62, 3)]
    assert [R.block_role(b, 1) for b in (0, 9, 255)] == [(0, 0), (9, 0), (255, 0)]


# ---- the references ---------------------------------------------------------------------------------------------------------------------------
def _close(a, b, bound, what):
    r = float(((a - b).abs() / (1e-12 * bound + 1e-300)).max())
    assert r <= 1.0, f"{what}: {r:.3g} x 1e-12 of the term magnitude"


@pytest.mark.parametrize("kind", ["down", "up"])
def test_references_agree_with_autograd(kind):
    n, h, Cu, Cv = 3, 2, 3, 5
    x, W, b, src, cinit = R.fwd_operands(1, kind, n, h, h, Cu, Cv)
    r = R.conv_fwd(kind, x, W, b, act=R.RELU, mask_src=src, mask_act=R.RELU, colsum=True)
    f = F.conv2d if kind == "down" else F.conv_transpose2d
    y = torch.relu(f(x.double(), W.double(), b.double(), stride=2, padding=1)) * (src > 0)
    _close(r["y"].ref, y, r["y"].bound + 1e-30, "forward")
    _close(r["colsum"].ref, y.sum((0, 2, 3)), r["colsum"].bound, "column sums")
    _close(r["colsum"].bound, (r["y"].bound + r["y"].ref.abs()).sum((0, 2, 3)), r["colsum"].bound, "column-sum tolerance")
    none = R.conv_fwd(kind, x, W, b, act=R.RELU, mask_src=src, mask_act=R.NONE)["y"]
    assert torch.equal(none.ref, R.conv_fwd(kind, x, W, b, act=R.RELU)["y"].ref), "a `none` mask multiplies by 1"
    fl = R.conv_fwd(kind, x, W, floor_bounds=(2.0, 3.0))["y"].bound - R.conv_fwd(kind, x, W)["y"].bound
    prod = 4 * Cv if kind == "up" else 16 * Cu
    assert torch.allclose(fl, torch.full_like(fl, R.FLOOR * 6.0 * prod / R.C_ENTRY), rtol=1e-9)
    if kind == "down":
        U, dV, _ = R.wgrad_operands(2, n, h, h, Cu, Cv)
        Wr = torch.zeros(Cv, Cu, 4, 4, dtype=F64, requires_grad=True)
        (F.conv2d(U.double(), Wr, None, stride=2, padding=1) * dV.double()).sum().backward()
        g_ = R.conv_wgrad(U, dV)
        _close(g_.ref, Wr.grad, g_.bound, "weight gradient")


def test_operand_variants():
    x, W, *_ = R.fwd_operands(3, "down", 6, 4, 4, 64, 128, data="tiny")
    amx, amw = x.abs().amax((1, 2, 3)), W.abs().amax((1, 2, 3))
    assert float(amx[3]) < 2.0 ** -26 * float(amx.max()) and float(amw[64]) < 2.0 ** -26 * float(amw.max())
    x, W, *_ = R.fwd_operands(3, "up", 300, 8, 8, 32, 64, data="spread")
    amx, amw = x.abs().amax((1, 2, 3)), W.abs().amax((0, 2, 3))
    assert float(amx.max() / amx.min()) > 1e4 and float(amw.max() / amw.min()) > 1e2


# ---- the table holds what the issue lists --------------------------------------------------------------------------------------------------
def test_table_coverage():
    P8, P4 = R.PAIRS
    fwd = [c for c in G.CASES if c.fn is G.p_fwd and c.kw.get("flags", G.TAKE) == G.TAKE and isinstance(c.regime, set)]
    want = {P8: [{0, 2}, {2}, {2, 4}, {6}], P4: [{0, 1}, {1}, {1, 2}, {2}, {3}, {5, 6}]}
    for pair in R.PAIRS:
        for kind in ("down", "up"):
            bf = [c for c in fwd if c.kw["pair"] == pair and c.kw["kind"] == kind and not c.kw["scaled"] and not c.kw.get("yam_only")
                  and c.kw.get("frag") is not False]
            fp = [c for c in fwd if c.kw["pair"] == pair and c.kw["kind"] == kind and c.kw["scaled"]]
            assert sorted(map(sorted, (c.regime for c in bf))) == sorted(map(sorted, want[pair])), (pair, kind)
            for cs in (bf, fp):
                assert {c.kw["form"] for c in cs} == set(G.FORMS), (pair, kind)
                assert any(c.kw["form"] == "maskcs" and len(c.regime) > 1 for c in cs), "column sums in a multi-count regime"
            regs = [c.regime for c in fp]
            assert len(regs) >= 3 and min(want[pair], key=max) in regs and any(max(r) >= 3 for r in regs)
        wg = [c for c in G.CASES if c.fn is G.p_wgrad and c.kw["pair"] == pair and c.kw.get("flags", G.TAKE) == G.TAKE
              and "ws" not in c.kw and "w" not in c.kw and c.kw["n"] % 2 == 0]
        for scaled in (False, True):
            ns = {(c.kw["n"], c.kw["deferred"]) for c in wg if c.kw["scaled"] == scaled}
            assert {n for n, _ in ns} == ({4, 300, 1024} if pair == P8 else {4, 130, 2048})
            assert {d for _, d in ns} == {False, True}
    sc = [c for c in fwd if c.kw["scaled"]]
    assert {"spread", "tiny"} <= {c.kw.get("data") for c in sc} and any(c.kw.get("loose") for c in sc)
    cs = [c for c in fwd if c.kw["form"] == "maskcs"]
    assert {c.kw["deferred"] for c in cs} == {False, True}
    ks = {k for c in G.CASES for k in c.expect}
    for pair in R.PAIRS:
        for kind in ("down", "up"):
            for src in (False, True):
                for np_ in (2, 3):
                    assert R.kernel_name(kind, pair, src, np_) in ks, (kind, pair, src, np_)
        assert {R.wgrad_kernel_name(pair, 2), R.wgrad_kernel_name(pair, 3)} <= ks
    assert {D.FIN, D.BATCH, D.RED} <= ks
    assert any(c.kw.get("yam_only") for c in G.CASES)
    assert any(c.kw.get("frag") is False for c in G.CASES)
    assert len(G.IDS) == len(set(G.IDS))
