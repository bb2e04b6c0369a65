"""CPU checks of tests/conv_small_ref.py, the float64 reference behind tests/test_gpu_conv4s2_small.py:

- on one tiny case every reference agrees with a second, torch-free statement of the same operation (oracle/nets.py conv2d_np /
  conv_transpose2d_np, a numpy loop for the weight gradient) and with float64 autograd;
- the degraded operands are what they claim to be (16 significant bits; bf3.hpp's pair to 2^-23);
- for EVERY case of the GPU table each degraded emulation that is defined for the case leaves the case's tolerance on at least
  one output: the per-entry check has teeth before any GPU run;
- the table holds the leaves it is meant to hold (12 channel pairs per kernel, both activation instantiations, both forms).
"""
import re

import numpy as np
import pytest
import torch

import conv_small_ref as R
import test_gpu_conv4s2_small as G
from oracle import nets

F64 = torch.float64


def _close(a, b, bound, what):
    """Two float64 evaluations of one formula in different operation orders: rounding alone, 1e-12 of the term magnitude."""
    a = torch.as_tensor(a, dtype=F64)
    b = torch.as_tensor(b, dtype=F64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    r = float(((a - b).abs() / (1e-12 * bound + 1e-300)).max())
    assert r <= 1.0, f"{what}: {r:.3g} x 1e-12 of the term magnitude"


def _wgrad_np(U, dV):
    """dW[cv][cu][kh][kw] = sum_{n,i,j} Upad[n][cu][2 i + kh][2 j + kw] dV[n][cv][i][j] (pad 1), in numpy."""
    U, dV = np.asarray(U, np.float64), np.asarray(dV, np.float64)
    n, Cu, H, W = U.shape
    _, Cv, h, w = dV.shape
    Up = np.zeros((n, Cu, H + 2, W + 2))
    Up[:, :, 1:-1, 1:-1] = U
    out = np.zeros((Cv, Cu, 4, 4))
    for kh in range(4):
        for kw in range(4):
            out[:, :, kh, kw] = np.einsum("nchw,nohw->oc", Up[:, :, kh:kh + 2 * h:2, kw:kw + 2 * w:2], dV)
    return out


def test_references_agree_with_numpy_and_autograd():
    n, h, w, Cu, Cv = 2, 3, 2, 3, 5
    V, W, b = R.up_operands(1, n, h, w, Cu, Cv)
    r = R.up_pre(V, W, b)
    _close(r.ref, nets.conv_transpose2d_np(V, W, b, 2, 1), r.bound, "up pre-activation")
    _close(r.bound, nets.conv_transpose2d_np(V.abs(), W.abs(), b.abs(), 2, 1), r.bound, "up bound")
    U, Wd, bd = R.down_operands(2, n, h, w, Cu, Cv)
    r = R.down_pre(U, Wd, bd)
    _close(r.ref, nets.conv2d_np(U, Wd, bd, 2, 1), r.bound, "down pre-activation")
    _close(r.bound, nets.conv2d_np(U.abs(), Wd.abs(), bd.abs(), 2, 1), r.bound, "down bound")
    for u_act, v_act in [(R.SIGMOID, R.RELU), (R.NONE, R.NONE), (R.NONE, R.RELU), (R.SIGMOID, R.LEAKY)]:
        dU, Uout, V, W, _ = R.bwd_operands(3 + u_act + v_act, n, h, w, Cu, Cv, u_act, v_act)
        r = R.up_bwd(dU, Uout, u_act, V, v_act, W)
        a = R.up_bwd_autograd(dU, Uout, u_act, V, v_act, W)
        for k in ("dV", "dW", "db", "dbv"):
            _close(r[k].ref, a[k], r[k].bound, f"{k} vs autograd (u_act {u_act}, v_act {v_act})")
        dpre = dU.double().numpy() * R.actgrad64(Uout, u_act).numpy()
        vm = R.actgrad64(V, v_act).numpy()
        dV = nets.conv2d_np(dpre, W, np.zeros(Cv), 2, 1) * vm
        _close(r["dV"].ref, dV, r["dV"].bound, "dV vs numpy")
        _close(r["dW"].ref, _wgrad_np(dpre, V), r["dW"].bound, "dW vs numpy")
        _close(r["db"].ref, dpre.sum((0, 2, 3)), r["db"].bound, "db vs numpy")
        _close(r["dbv"].ref, dV.sum((0, 2, 3)), r["dbv"].bound, "dbv vs numpy")
        _close(r["dV"].bound, nets.conv2d_np(np.abs(dpre), W.abs(), np.zeros(Cv), 2, 1) * vm, r["dV"].bound, "dV bound")
    U, dV, _ = R.wgrad_operands(9, n, h, w, Cu, Cv)
    r = R.down_wgrad(U, dV)
    _close(r.ref, _wgrad_np(U, dV), r.bound, "smallcin wgrad vs numpy")
    _close(r.ref, R.down_wgrad_autograd(U, dV), r.bound, "smallcin wgrad vs autograd")
    _close(r.bound, _wgrad_np(U.abs(), dV.abs()), r.bound, "smallcin wgrad bound")


def test_activation_helpers():
    y = torch.tensor([-1.5, -0.0, 0.0, 1e-30, 2.0])
    assert R.actgrad64(y, R.RELU).tolist() == [0, 0, 0, 1, 1]
    assert R.actgrad64(y, R.LEAKY).tolist() == [R.F02, R.F02, R.F02, 1, 1]
    assert R.actgrad64(y, R.NONE).tolist() == [1] * 5
    s = torch.tensor([0.25, 0.5])
    assert R.actgrad64(s, R.SIGMOID).tolist() == [0.1875, 0.25]
    assert R.act64(y.double(), R.LEAKY).tolist() == [-1.5 * R.F02, -0.0, 0.0, float(y[3]), 2.0]


def test_degraded_operands_are_what_they_claim():
    x = torch.randn(4096, generator=R.g(3)) * torch.logspace(-3, 3, 4096)
    e2 = ((R.two_piece(x) - x.double()).abs() / x.double().abs()).max()
    assert 2.0 ** -19 < float(e2) <= 2.0 ** -16  # 16 significant bits: what is lost is visible, and no more than that
    hi, lo, s = R.f16_pair(x)
    amax = float(x.abs().max())
    assert 2.0 ** 13 <= amax * s < 2.0 ** 14
    xs = x.double() * s
    big = xs.abs() >= amax * s * 2.0 ** -28  # bf3.hpp: full precision down to 2^-28 of the maximum
    err = ((hi + lo / 2048.0) - xs).abs()
    assert float((err[big] / xs.abs()[big]).max()) <= 2.0 ** -22
    assert float(err.max()) <= amax * s * 2.0 ** -39 + float((xs.abs() * 2.0 ** -22).max())


_HOST = {}


def host_outs(c):
    if c.id not in _HOST:
        _HOST[c.id] = c.host()
    return _HOST[c.id]


@pytest.mark.parametrize("c", G.CASES, ids=G.IDS)
def test_degraded_emulations_leave_the_tolerance(c):
    """The GPU check of a case is |got - ref| <= C_ENTRY * bound (+ slack |ref|) on every entry of every output; an emulation is
    rejected when it breaks that on any output.  Both emulations must be rejected; f16_drop is defined for the products only."""
    p = host_outs(c)
    r2, rh = [], []
    for o in p.outs:
        assert o.ref.dtype == F64 and o.bound.dtype == F64 and o.ref.shape == o.bound.shape == o.deg.shape
        assert o.derived or bool((o.bound + 1e-300 >= o.ref.abs() * (1 - 1e-12)).all()), "the bound is below its own reference"
        tol = G.D.C_ENTRY * o.bound + o.slack * o.ref.abs() + 1e-30
        r2.append(float(((o.deg - o.ref).abs() / tol).max()))
        if o.degh is not None:
            rh.append(float(((o.degh - o.ref).abs() / tol).max()))
    assert max(r2) > 1.0, f"two-piece operands pass every output: {r2}"
    assert rh and max(rh) > 1.0, f"fp16 pairs without a cross term pass every output: {rh}"


def test_block_cap_slabs_have_teeth():
    """The 263680-position weight gradient is checked slab by slab (320 positions each) on the GPU: both emulations leave the
    per-entry bound of the slabs, and the slabs add up to the whole gradient.  End to end the two-piece operands would pass."""
    U, dV, _, nb, ppb, blk = G.blockcap_refs(want_h=True)
    assert (nb, ppb) == (824, 320) and nb * ppb == U.shape[0] * 256
    r2, rh = blk.ratios()
    assert r2 > 1.0 and rh > 1.0, (r2, rh)
    whole = R.down_wgrad(U, dV)
    _close(R.slabs_to_ref_layout(blk.ref, 3, 32), whole.ref, whole.bound, "sum of the slabs")
    _close(R.slabs_to_ref_layout(blk.bound, 3, 32), whole.bound, whole.bound, "sum of the slab bounds")
    assert whole.ratios()[0] < 1.0  # why the slabs are checked: no per-entry teeth on the 263680-term sum
    assert G.cin_blocks(255) == (1, 256) and G.cin_blocks(257) == (2, 192) and G.cin_blocks(1600) == (7, 256)


def _kernels(prefix):
    return {k for c in G.CASES for k in c.expect if k.startswith(prefix)}


def test_table_holds_its_leaves():
    pairs = {f"{cu},{cv}" for cu, cv in G.PAIRS}
    inst = lambda ks: {",".join(re.match(r"\w+<(\d+),(\d+)", k).groups()) for k in ks}  # noqa: E731
    up, bwd, down = _kernels("small_up_fwd_kernel"), _kernels("small_up_bwd_kernel"), _kernels("small_down_fwd_kernel")
    assert inst(up) == pairs and inst(bwd) == pairs and inst(down) == pairs
    assert {k.split(",")[-1] for k in up} == {"true>", "false>"}
    assert inst({k for k in up if k.endswith("true>")}) == pairs - {"3,32"}  # 16x16 at (3, 32) is the split-bf16 kernel's
    for spec in ("2,1", "-1,-1"):
        for dense in ("true", "false"):
            assert any(k.endswith(f",{spec},{dense}>") for k in bwd), (spec, dense)
    assert inst({k for k in bwd if k.endswith("true>")}) == pairs and inst({k for k in bwd if k.endswith("false>")}) == pairs
    wg = _kernels("smallcin_wgrad_kernel")
    assert {re.match(r"\w+<(\d),(\d)>", k).groups() for k in wg} == {(str(cu), str(cv // 16)) for cu, cv in G.PAIRS}
    assert _kernels("smallcin_fwd_kernel") == {f"smallcin_fwd_kernel<{c}>" for c in (1, 2, 3, 4)}
    for acts in ("-u0v0", "-u0v1", "-u2v3"):  # generic activations: none/none, none/ReLU, sigmoid/LeakyReLU
        assert any(acts in c.id and "-1,-1" in "".join(c.expect) for c in G.CASES if c.id.startswith("upbwd")), acts
    assert len(G.IDS) == len(set(G.IDS))
