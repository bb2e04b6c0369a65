"""csrc/skinny.hip leaf by leaf against float64: heads_fwd_kernel<4|16>, narrow_fwd_kernel, heads_finish_kernel, heads_bwd_kernel and
smallk_fwd_kernel<K4,R>, through mvk_linear_fwd, mvk_heads_fwd, mvk_gemm, mvk_gemm_smallk_amax, mvk_heads_bwd and kernels.heads_bwd.

tests/skinny_ref.py holds the launchers' host arithmetic as plain Python (`*_plan`), the float64 references with their per-entry
bounds, the case tables (every case names the edge it is there for) and the fp32 evaluations in the kernels' summation order;
tests/test_skinny_ref_host.py pins all of it on the CPU and runs every `check_*` routine below with that fp32 stand-in, including
the proof that the two-piece bf16 operands leave the bound on at least one entry of EVERY output of EVERY case (dbprev: the
summation fault skinny_ref's docstring puts in their place).

Every output, and every scratch region whose size the C ABI lets the caller state, sits between 64 sentinel floats with a NaN
prefill (accumulated targets: their non-zero initial content); every entry of every output is compared; a touched sentinel or a NaN
left behind fails; where a case exists to reach a leaf the launched kernel names are asserted against the plan; a second launch from
the same initial buffers is bit-identical.  Tolerance: rule (a) of tests/test_gpu_gemm_dispatch.py with its C_ENTRY (imported), its
slack only for sigmoid evaluation.  Every chain here is shorter than the 1024 terms C_ENTRY was derived for: a wave's k range of a
slice (<= 272), 128 rows of a row group plus <= 64 ordered slabs, NN <= 64 terms of dX, K <= 32 of the short-reduction kernel.

Measured on an MI355X (test_zz_report; worst |got - ref| / tolerance over every entry, per stage; `degraded` = the two-piece
emulation at the same case, for dbprev the reference with row 0 of X left out; profiles/NOTES_skinny.md has every case):
    stage              worst   degraded   case
    heads_fwd          0.412      9.90    hf-nk-woff-2h (head 1)
    narrow             0.248      6.62    narrow-M1024-N17
    finish             0.433     10.72    fin-M528-N16
    heads_bwd.dX       0.583      9.11    n20-2h-M8192
    heads_bwd.dW       0.397     18.03    nn64-M129-K512-def (dW0)
    heads_bwd.db       0.226      2.71    flat4-2h-def (db0)
    heads_bwd.dbprev   0.190    441.61    n1x2-M127
    smallk             0.803     12.12    R8-M1021-N2048 (one entry of 2 091 008; the fp32 CPU chain of 20 products gives the same 0.803)
    smallk.tiled       0.202      7.24    yoff-linear (Y 4 bytes off: the tiled engine)
Weakest rejection of the degraded emulation over all 265 checked outputs: 1.30x (linear-M1: K = 1, products of one term).
Wall time of this file on an MI355X: 2.5 s for the 97 tests (4.8 s with start-up and collection; the first profiler session is 1.6 s
of that); on the CPU with the stand-in backend (tests/test_skinny_ref_host.py, 176 tests): 4 s.

Suspects read from the kernel text, the case that exercises each, and the verdict of the first run on an MI355X:
 1. heads_bwd_kernel's barriers when pslab is absent but the workgroup is the bias block: `red` is first written behind the
    "Ds complete" barrier, and with pslab the extra barrier in front of its reuse is taken by the bias block only, which is
    uniform per workgroup (noprev, noprev-K16, n1-1h-M1-K16 where the only column block is the bias block): cleared.
 2. colsum_finish_any's scalar form for slabs with N % 4 != 0 behind a 4-float-rounded workspace offset (n17-2h-M129: db of 17 on
    colsum_finish_scalar_kernel, dW of 816 and dbprev of 48 on colsum_finish_kernel, by name; flat4-1h: nrows = nz prow): cleared.
 3. heads_fwd_kernel's part index `gridDim.y / tiles_per_head` (fin-64tiles: four column tiles of one head; the scratch is exactly
    nz M N floats between sentinels and every float of it is written): cleared for one head; two heads never split (below).
 4. kernels.heads_bwd's estimate of the scratch against the C side's rounded sum (test_python_estimate_covers_the_c_side, on the
    CPU: the estimate's 64 spare floats cover five slabs rounded up by at most 3): the estimate is never the smaller one: cleared.
 5. heads_finish_kernel's z tail at nz % 4 != 0 and its caps (fin-K2304, fin-K2816, fin-cap64: nz = 62, fin-cap128-tiles31:
    nz = 65, fin-cap128: nz = 122): cleared.
 6. waves with an empty k range, k0 >= k1 (fin-K2052: waves 10 .. 15 of the last slice; hf-K4: waves 1 .. 3): cleared.
 7. smallk_fwd_kernel's idle threads (rg >= rgn, cg >= CT) and rows past M in the published maximum, and `continue` inside the
    row loop in front of a call that synchronises (amax-*: the slot equals max(|Y|, preset) of the same launch bit for bit, also
    with a pre-activation of twice the size that the activation removes): cleared.
 8. amax_publish's relaxed read in front of its atomic (presets above and below the maximum, a second launch without a reset): cleared.
 9. 61952 bytes of dynamic LDS at NN = 64 and the 64-wide load (nn64-M300-K48, nn64-M129-K512-def): cleared.
10. scalar weight loads with w_sk = 1 (hf-nk-woff-2h, hf-nk-woff-1h, narrow-M1024-N32-woff, woff-nk, woff-kn): cleared.
11. every K4 of smallk_fwd_kernel, R = 8 | 16 on both sides of want = 8, an unaligned Y declined and an unaligned X taken
    (test_smallk_every_K, R8-M2048-N400 / R16-M2049-N400, yoff, xoff: by name): cleared.
Verdict: all eleven cleared; csrc/skinny.hip, csrc/igemm.hip and kernels.py are unchanged.  Two things the first runs did show:
the issue's "M = 512 against 528 at N = 16" is 32 against 33 tiles, both on the cap of 64 (`tiles >= 32`); the boundary of the
cap is 31 | 32 tiles, which fin-cap128-tiles31 against fin-cap64 crosses; and an fp32 chain over operands with a loud term EARLY in
the chain leaves C_ENTRY on its own (1.4x over 128 rows on the CPU), which is why skinny_ref puts the loud terms last.

Leaves these entry points cannot reach (and why):
- smallk_fwd_kernel's mask_src / accumulate arguments: mvk_gemm enters smallk_fwd only with `!accumulate && !c_act_src` (igemm.hip,
  "measured +10 us per step: the tiled engine"), mvk_linear_fwd and mvk_gemm_smallk_amax pass neither.
- split-K over workgroups with two heads (heads_fwd_kernel's `gridDim.y / tiles_per_head` part index with heads = 2, and
  heads_finish_kernel with heads = 2): only mvk_heads_fwd launches two heads, and it passes no scratch (ws = NULL: nz = 1).
- `bias_mod <= 0` with a bias: smallk_fwd clamps bias_mod to 1 before the launch (`bias_mod > 0 ? bias_mod : 1`), so the kernel's
  `% g.bias_mod` never sees 0; the clamp itself is the case N4 (bias_mod = 0 with a bias: every column reads bias[0]).
- heads_fwd_kernel<16> with one slice and K < 1024, and <4> with K >= 1024: the launcher chooses by K alone.
"""
import time
import types

import pytest
import torch

import skinny_ref as R
import test_gpu_gemm_dispatch as D
from test_gpu_misc import EINVAL, GUARD, SENTINEL, Guarded

pytestmark = pytest.mark.gpu

MEASURED = {}
_T0 = time.time()
same_bits = lambda a, b: a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))  # noqa: E731


def dev():
    return torch.device("cuda:0")


def _lib():
    from multivae_amd import _lib as L

    return L


def hold(measured, stage, name, got, ref, init=None):
    """One output: no NaN, every entry inside rule (a), and the two-piece emulation outside it on at least one entry."""
    assert got.shape == ref.ref.shape, (name, stage, got.shape, ref.ref.shape)
    assert not bool(torch.isnan(got).any()), f"{name}: {stage}: a NaN is left: an entry the kernel did not write"
    worst, deg = R.ratios(got, ref, init)
    two = "" if ref.deg2 is None else f": row 0 left out; two-piece {R.deg_ratio(ref, ref.deg2, init):.2f}"
    print(f"{name}: {stage} {worst:.3f} (degraded {deg:.2f}{two})")
    if measured is not None and worst > measured.get(stage, (-1.0,))[0]:
        measured[stage] = (worst, name, deg)
    assert worst <= 1.0, f"{name}: {stage}: worst |got - ref| = {worst:.3f}x the bound ({D.C_ENTRY:g} sum|a b|)"
    assert deg > 1.0, f"{name}: {stage}: no teeth: the degraded emulation stays inside the bound ({deg:.3f}x)"


def _profiled(fn, names):
    if names:
        return D.launched_kernels(fn)
    fn()
    torch.cuda.synchronize()
    return None


def _lay(w_kn, layout):
    """Logical [K][N] -> the stored layout."""
    return (w_kn.t() if layout == "nk" else w_kn).contiguous()


# ---- the HIP backend: CPU tensors in, CPU tensors out ---------------------------------------------------------------------------
class Hip:
    def fwd(self, c, inp, ws_floats, names=True):
        lib, sp = _lib().load(), _lib().stream_ptr
        M, N, K = c.M, c.N, c.K
        X = Guarded(M * K, src=inp["x"])
        W = [Guarded(K * N, off=c.w_off, src=_lay(w, c.layout)) for w in inp["w"]]
        Bs = [None if b is None else Guarded(N, src=b) for b in inp["b"]]
        Y = [Guarded(M * N) for _ in range(c.heads)]
        ws = Guarded(ws_floats) if ws_floats > 0 else None
        bp = [None if b is None else b.p for b in Bs]
        rc = []

        def go():
            if c.via == "linear":
                rc.append(lib.mvk_linear_fwd(X.p, W[0].p, bp[0], Y[0].p, M, N, K, c.act, ws.p if ws else None, ws_floats, sp()))
            else:
                two = c.heads == 2
                sk, sn = R.fwd_strides(c)
                rc.append(lib.mvk_heads_fwd(X.p, W[0].p, bp[0], Y[0].p, W[1].p if two else None, bp[1] if two else None,
                                            Y[1].p if two else None, M, N, K, sk, sn, sp()))

        kernels = _profiled(go, names)
        held = [X] + W + Y + [b for b in Bs if b is not None] + ([ws] if ws else [])
        return dict(Y=[y.cpu(M, N) for y in Y], guards=all(g.intact() for g in held), kernels=kernels, rc=rc[0],
                    ws=None if ws is None else ws.cpu(ws_floats))

    def smallk(self, c, inp, preset=None, launches=1, names=True):
        """-> Y, the amax slot after each launch (via="amax"), guards, kernels, rc."""
        lib, sp = _lib().load(), _lib().stream_ptr
        M, N, K = c.M, c.N, c.K
        X = Guarded(M * K, off=c.off == "X", src=inp["x"])
        W = Guarded(K * N, off=c.off == "W", src=_lay(inp["w"], c.layout))
        Bv = None if inp["bias"] is None else Guarded(inp["bias"].numel(), src=inp["bias"])
        Y = Guarded(M * N, off=c.off == "Y")
        slot = Guarded(1, fill=preset) if c.via == "amax" else None
        bp, tb = (None if Bv is None else Bv.p), int(c.layout == "nk")
        bm = 0 if c.bias_mod is None else c.bias_mod
        wsp, wsn = D.WS("ws")
        rc, seen = [], []

        def go():
            if c.via == "gemm":
                rc.append(lib.mvk_gemm(X.p, W.p, Y.p, M, N, K, 0, tb, bp, bm, c.act, 0, None, 0, None, 0, wsp, wsn, sp()))
            elif c.via == "linear":
                rc.append(lib.mvk_linear_fwd(X.p, W.p, bp, Y.p, M, N, K, c.act, wsp, wsn, sp()))
            else:
                rc.append(lib.mvk_gemm_smallk_amax(X.p, W.p, Y.p, M, N, K, tb, bp, bm, c.act, slot.p, sp()))

        kernels = _profiled(go, names)
        for i in range(launches):
            if i:
                _profiled(go, False)
            if slot is not None:
                seen.append(slot.cpu(1))
        held = [X, W, Y] + ([Bv] if Bv else []) + ([slot] if slot else [])
        return dict(Y=Y.cpu(M, N), amax=seen, guards=all(g.intact() for g in held), kernels=kernels, rc=rc[0])

    def bwd(self, c, inp, inits, ws_floats, off=None, names=True):
        """c: a BwdCase.  Targets live in ONE buffer, 64 sentinels between them; deferred / mixed: the flat gradient buffer of the
        scope is that buffer / its head up to dW0.  -> out (name -> tensor, dX None when absent), guards, kernels, rc, ws."""
        from multivae_amd import kernels as K_
        from multivae_amd import schedule

        lib, sp = _lib().load(), _lib().stream_ptr
        M, N, K, nh = c.M, c.N, c.K, c.nh
        X = Guarded(M * K, off=off == "X", src=inp["x"])
        dY = [Guarded(M * N, src=t) for t in inp["dys"]]
        W = [Guarded(N * K, src=(w if c.layout == "nk" else w.t()).contiguous()) for w in inp["ws"]]
        sk, sn = (1, K) if c.layout == "nk" else (N, 1)
        dX = Guarded(M * K, off=off == "dX") if c.dx else None
        # the targets
        spans, n = {}, GUARD
        for k, t in inits.items():
            spans[k] = (n, t.numel(), tuple(t.shape))
            n += (t.numel() + 63) // 64 * 64 + GUARD
        flat = torch.full((n,), SENTINEL, device=dev())
        view = {k: flat[o:o + cnt].view(shp) for k, (o, cnt, shp) in spans.items()}
        for k, t in inits.items():
            view[k].copy_(t)
        free = torch.ones(n, dtype=torch.bool)
        for o, cnt, _ in spans.values():
            free[o:o + cnt] = False
        ws = Guarded(max(ws_floats, 1)) if c.via == "c" else None
        if c.targets == "deferred":
            scope_grad = flat
        elif c.targets == "mixed":
            scope_grad = flat[:spans["dW0"][0] + spans["dW0"][1] + GUARD]
        else:
            scope_grad = None
        tp = lambda k: view[k].data_ptr() if k in view else None  # noqa: E731
        rc, dx_py = [], []

        def launch():
            if c.via == "py":
                params = {}
                for k in view:
                    p = torch.zeros(view[k].shape, device=dev()).requires_grad_(True)
                    p.grad = view[k]
                    params[k] = p
                r = K_.heads_bwd(X.body.view(M, K), c.x_act, [t.body.view(M, N) for t in dY], [w.body for w in W],
                                 [params.get(f"db{h}") for h in range(nh)], sk, sn, flat_c=c.flat_c, want_dx=c.dx,
                                 prev_bias=params.get("dbprev"), dw_params=[params[f"dW{h}"] for h in range(nh)])
                assert r is not None, "kernels.heads_bwd declined a covered shape"
                assert all(t is None for t in r[1] + r[2] + [r[3]]), "a gradient did not go straight into its .grad"
                dx_py.append(r[0])
                rc.append(0)
            else:
                two = nh == 2
                rc.append(lib.mvk_heads_bwd(X.p, c.x_act, dY[0].p, dY[1].p if two else None, W[0].p, W[1].p if two else None, sk, sn,
                                            c.flat_c, dX.p if dX else None, tp("dW0"), tp("dW1"), tp("db0"), tp("db1"), tp("dbprev"),
                                            M, N, K, ws.p, ws_floats, sp()))

        def go():
            if scope_grad is not None:
                with schedule.deferred_reductions(types.SimpleNamespace(grad=scope_grad)):
                    launch()
            else:
                launch()

        kernels = _profiled(go, names)
        out = {k: v.cpu().clone() for k, v in view.items()}
        if c.dx:
            out["dX"] = dx_py[-1].cpu() if c.via == "py" else dX.cpu(M, K)
        else:
            out["dX"] = None
            assert c.via != "py" or dx_py[-1] is None
        held = [X] + dY + W + ([dX] if dX is not None and c.via == "c" else []) + ([ws] if ws else [])
        guards = all(g.intact() for g in held) and bool((flat.cpu()[free] == SENTINEL).all())
        return dict(out=out, guards=guards, kernels=kernels, rc=rc[0], ws=None if ws is None else ws.cpu(ws.n))


HIP = Hip()


# ---- the comparison routines (also run on the CPU by tests/test_skinny_ref_host.py with the fp32 stand-in) -------------------------
def fwd_stage(plan):
    return "finish" if R.HFIN in plan.kernels else "narrow" if plan.kernels == [R.NARROW] else "heads_fwd"


def check_fwd(c, be, measured=None):
    plan, wsf = R.fwd_plan(c)
    assert not plan.declines, (c.name, plan.declines)
    inp = R.fwd_inputs(c)
    got = be.fwd(c, inp, wsf)
    assert got["rc"] == 0, f"{c.name}: return code {got['rc']}"
    assert got["guards"], f"{c.name}: a sentinel next to a buffer was overwritten"
    if got["kernels"] is not None:
        assert got["kernels"] == sorted(plan.kernels), f"{c.name}: launched {got['kernels']}, the plan says {sorted(plan.kernels)} ({c.why})"
    for h in range(c.heads):
        hold(measured, fwd_stage(plan), f"{c.name}[{h}]", got["Y"][h], R.fwd_ref(inp["x"], inp["w"][h], inp["b"][h], c.act))
    if plan.nz > 1 and got["ws"] is not None:  # the scratch is exactly nz M N floats: every slice wrote every entry of its part
        assert not bool(torch.isnan(got["ws"]).any()), f"{c.name}: a part entry of the split was never written"
    if plan.nz == 1 and got["ws"] is not None:
        assert bool(torch.isnan(got["ws"]).all()), f"{c.name}: a launch that does not split wrote into the scratch"
    again = be.fwd(c, inp, wsf, names=False)
    for a, b in zip(got["Y"], again["Y"]):
        assert same_bits(a, b), f"{c.name}: a second launch differs"
    return got


def check_smallk(c, be, measured=None, names=True):
    al = dict(W=c.off != "W", Y=c.off != "Y", X=c.off != "X")
    plan = R.smallk_plan(c.M, c.N, c.K, c.layout, al)
    inp = R.sk_inputs(c)
    got = be.smallk(c, inp, names=names)
    assert got["rc"] == 0 and got["guards"], f"{c.name}: rc {got['rc']}, guards {got['guards']}"
    if got["kernels"] is not None:
        if plan.declines:
            assert plan.declines == ["Y unaligned"], (c.name, plan.declines)
            assert got["kernels"] and all(k.startswith("igemm") for k in got["kernels"]), f"{c.name}: {got['kernels']} is not the tiled engine"
        else:
            assert got["kernels"] == [R.smallk_name(plan.K4, plan.R)], f"{c.name}: launched {got['kernels']}, the plan says K4 = {plan.K4}, R = {plan.R}"
    hold(measured, "smallk.tiled" if plan.declines else "smallk", c.name, got["Y"], R.fwd_ref(inp["x"], inp["w"], inp["bias_full"], c.act))
    assert same_bits(be.smallk(c, inp, names=False)["Y"], got["Y"]), f"{c.name}: a second launch differs"
    return got


def amax_sk(c):
    return R.SkCase(c.name, "amax", c.M, c.N, c.K, c.layout, c.N, c.act, None, c.why)


def check_amax(c, be, measured=None):
    inp = R.amax_inputs(c)
    ref = R.fwd_ref(inp["x"], inp["w"], inp["bias_full"], c.act)
    top = float(ref.ref.abs().max())
    for how in R.AMAX_PRESETS:
        preset = float(torch.tensor({"zero": 0.0, "above": 2.0 * top, "below": 0.25 * top}[how], dtype=torch.float32))
        got = be.smallk(amax_sk(c), inp, preset=preset, launches=2, names=how == "zero")
        name = f"{c.name}-{how}"
        assert got["rc"] == 0 and got["guards"], name
        if got["kernels"] is not None:
            p = R.smallk_plan(c.M, c.N, c.K, c.layout)
            assert got["kernels"] == [R.smallk_name(p.K4, p.R)], (name, got["kernels"])
        hold(measured, "smallk", name, got["Y"], ref)
        Y = got["Y"]
        if c.peak == "neg":
            assert bool((Y < 0).all()), f"{name}: the case wants every Y negative"
        else:
            flat = int(Y.abs().argmax())
            assert (flat // c.N, flat % c.N) == inp["pos"], f"{name}: the maximum is not where the case wants it"
        want = torch.tensor([max(float(Y.abs().max()), preset)], dtype=torch.float32)
        assert same_bits(got["amax"][0], want), f"{name}: published {float(got['amax'][0])}, max(|Y|, preset) = {float(want)}"
        assert same_bits(got["amax"][1], want), f"{name}: the slot changed in a second launch without a reset: {float(got['amax'][1])}"


def check_amax_declines(be):
    """K = 33 and N % 4 != 0: MVK_EINVAL, Y and the slot untouched."""
    for name, N, K in (("amax-K33", 12, 33), ("amax-N6", 6, 20)):
        c = R.SkCase(name, "amax", 19, N, K, "kn", N, R.NONE, None, "declined")
        got = be.smallk(c, R.sk_inputs(c), preset=3.0, names=False)
        assert got["rc"] == EINVAL, f"{name}: accepted (rc {got['rc']})"
        assert got["guards"] and bool(torch.isnan(got["Y"]).all()) and float(got["amax"][0]) == 3.0, f"{name}: something was written"


def bwd_stage(k):
    return "heads_bwd." + (k[:2] if k[:2] in ("dW", "db") and k != "dbprev" else k)


def check_bwd(c, be, measured=None):
    plan = R.heads_bwd_plan(c.M, c.N, c.K, c.nh, c.flat_c)
    assert not plan.declines, (c.name, plan.declines)
    inp, inits = R.bwd_inputs(c.M, c.N, c.K, c.nh, c.x_act, c.name), R.bwd_inits(c)
    ref = R.heads_bwd_ref(inp["x"], c.x_act, inp["dys"], inp["ws"], c.flat_c)
    need = R.bwd_ws_need(c)
    got = be.bwd(c, inp, inits, need)
    assert got["rc"] == 0, f"{c.name}: return code {got['rc']}"
    assert got["guards"], f"{c.name}: a sentinel next to a buffer was overwritten"
    if got["kernels"] is not None:
        if c.targets == "plain" and c.via == "c":
            assert got["kernels"] == R.bwd_kernels(c), f"{c.name}: launched {got['kernels']}, expected {R.bwd_kernels(c)}"
        else:
            assert R.HBWD in got["kernels"], (c.name, got["kernels"])
    if c.dx:
        hold(measured, "heads_bwd.dX", c.name, got["out"]["dX"], ref["dX"])
    else:
        assert got["out"]["dX"] is None
    for k, init in inits.items():
        hold(measured, bwd_stage(k), f"{c.name}/{k}", got["out"][k], ref[k], init)
    again = be.bwd(c, inp, inits, need, names=False)
    for k, v in got["out"].items():
        assert v is None or same_bits(v, again["out"][k]), f"{c.name}: {k} differs in a second launch"
    return got


def check_bwd_decline(d, be):
    """MVK_EINVAL, and every target, dX and the workspace as they were."""
    c = R.B(d.name, d.M, d.N, d.K, d.nh, d.why, flat_c=d.flat_c)
    inp, inits = R.bwd_inputs(d.M, d.N, d.K, d.nh, c.x_act, d.name), R.bwd_inits(c)
    need = R.bwd_ws_need(c)
    got = be.bwd(c, inp, inits, need - 1 if d.ws_short else need + 64, off=d.off, names=False)
    assert got["rc"] == EINVAL, f"{d.name}: accepted (rc {got['rc']})"
    assert got["guards"], d.name
    for k, init in inits.items():
        assert same_bits(got["out"][k], init), f"{d.name}: {k} was written"
    assert bool(torch.isnan(got["out"]["dX"]).all()), f"{d.name}: dX was written"
    assert got["ws"] is None or bool(torch.isnan(got["ws"]).all()), f"{d.name}: the workspace was written"


# ---- forward heads, narrow, finish ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.FWD_CASES, ids=[c.name for c in R.FWD_CASES])
def test_heads_fwd(c):
    check_fwd(c, HIP, MEASURED)


def test_split_and_one_slice_routes():
    """One shape (32 x 4096 -> 32) on the split-K route and, with the scratch one float short, on one slice: different kernels, both
    inside the bound; they need not agree in their bits."""
    a = check_fwd(R.FWD_BY_NAME["fin-K4096"], HIP, MEASURED)
    b = check_fwd(R.FWD_BY_NAME["fin-K4096-short"], HIP, MEASURED)
    assert a["kernels"] == sorted([R.H16, R.HFIN]) and b["kernels"] == [R.H16]
    assert bool(torch.isnan(b["ws"]).all()), "the one-slice route wrote into the scratch it found too small"


def test_heads_fwd_argument_checks():
    """mvk_heads_fwd: N = 33, K = 6, X 4 bytes off -> MVK_EINVAL and nothing written; M = 0 -> MVK_OK and nothing written."""
    lib, sp = _lib().load(), _lib().stream_ptr
    X, W, Y = Guarded(17 * 64 + 4, fill=0.5), Guarded(40 * 64, fill=0.5), Guarded(17 * 40)
    assert lib.mvk_heads_fwd(X.p, W.p, None, Y.p, None, None, None, 17, 33, 64, 1, 64, sp()) == EINVAL
    assert lib.mvk_heads_fwd(X.p, W.p, None, Y.p, None, None, None, 17, 20, 6, 1, 6, sp()) == EINVAL
    assert lib.mvk_heads_fwd(X.p + 4, W.p, None, Y.p, None, None, None, 17, 20, 64, 1, 64, sp()) == EINVAL
    assert lib.mvk_heads_fwd(X.p, W.p, None, Y.p, W.p, None, None, 17, 20, 64, 1, 64, sp()) == EINVAL  # a second head without its Y
    assert lib.mvk_heads_fwd(X.p, W.p, None, Y.p, None, None, None, 0, 20, 64, 1, 64, sp()) == 0
    torch.cuda.synchronize()
    assert Y.untouched() and X.intact() and W.intact()


# ---- short-reduction linear -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["kn", "nk"])
def test_smallk_every_K(layout):
    """K = 1 .. 32 at 19 x 12: every K4, by name; under torch Linear rows K % 4 != 0 takes the scalar weight loads."""
    for K in range(1, 33):
        check_smallk(R.SK_BY_NAME[f"k{K}-{layout}"], HIP, MEASURED)


_SK_REST = [c for c in R.SK_CASES if not c.name.startswith("k")]


@pytest.mark.parametrize("c", _SK_REST, ids=[c.name for c in _SK_REST])
def test_smallk(c):
    check_smallk(c, HIP, MEASURED)


@pytest.mark.parametrize("c", R.AMAX_CASES, ids=[c.name for c in R.AMAX_CASES])
def test_smallk_amax(c):
    check_amax(c, HIP, MEASURED)


def test_smallk_amax_declines():
    check_amax_declines(HIP)


# ---- the heads' backward ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.BWD_CASES, ids=[c.name for c in R.BWD_CASES])
def test_heads_bwd(c):
    check_bwd(c, HIP, MEASURED)


@pytest.mark.parametrize("d", R.BWD_DECLINES, ids=[d.name for d in R.BWD_DECLINES])
def test_heads_bwd_declines(d):
    check_bwd_decline(d, HIP)
    if d.python_none:
        from multivae_amd import kernels as K_

        x = torch.zeros(d.M, d.K, device=dev())
        dys = [torch.zeros(d.M, d.N, device=dev()) for _ in range(d.nh)]
        assert K_.heads_bwd(x, K_.RELU, dys, [None] * d.nh, [None] * d.nh, 1, d.K) is None


def test_zz_report():
    """Prints the worst ratio per stage of this session with its case and the two-piece ratio there, and the file's wall time."""
    print("SKINNY_MEASURED", {k: (round(v[0], 3), v[1], round(v[2], 2)) for k, v in sorted(MEASURED.items())})
    print(f"WALL test_gpu_skinny.py {time.time() - _T0:.1f} s")
