"""The inverse autoregressive flow on the GPU: mvk_iaf_fwd / mvk_iaf_bwd / mvk_iaf_inverse called directly through the C ABI,
entry-wise against float64, and kernels.IAFFlowFn under torch.autograd.

Reference, case table (iaf_ref.CASES: D in {2, 3, 20, 65} x H in {3, 64, 130} x hidden layers in {1, 3} x blocks in {1, 2, 3} x
B in {1, 3, 70}, the optional pointers — rows, dx, weight gradients, the inverse's ladj — and the upstream gradients cycled over it;
plus D = 512, H = 128, B = 3 forward and inverse only) and error model (a first-order running error analysis, carried through the
forward sweep and the backward's triangular solve) live in tests/iaf_ref.py.  Per case:
1. every output of the forward, the backward and the inverse launch, pre-filled with NaN (the accumulated weight gradients: with
   zeros), against the float64 reference: |got - ref| <= C_STAGE[stage] * base for EVERY entry; a NaN left anywhere fails; a
   masked weight's gradient is exactly 0;
2. a second launch from the same buffers is bit-identical;
3. test_masked_weights_are_never_read: NaN in every masked weight changes no bit of any output;
4. test_argument_checks: every MVK_EINVAL branch returns without launching, B = 0 / R = 0 is MVK_OK and writes nothing.

Constants (iaf_ref.C_STAGE = 4x the largest |err| / base of the same formulas in plain torch fp32 on the CPU, backward by fp32
autograd through the forward sweep, over the case table, rounded up; re-derived by test_iaf_host.py::test_error_constants, never
from the HIP kernels):
    stage      torch fp32   C
    z0         0.707        3.0
    ladj       0.110        0.5
    rows       0.168        0.7
    dx         2.338        10.0
    dW         0.197        0.8
    db         0.343        1.4
    x_inv      0.627        2.6
    ladj_inv   0.067        0.3
Largest |err| / base of the HIP kernels on an MI355X (test_zz_report prints HIP_MEASURED); recorded, not a bound:
    z0 0.707 (d20-h3-n3-k1-b70-null-wgrad), ladj 0.110 (d2-h3-n1-k1-b70-null-dx), rows 0.166 (d3-h3-n1-k1-b70), dx 0.435
    (d65-h3-n3-k1-b70-null-rows), dW 0.196 and db 0.249 (d20-h3-n3-k1-b1-null-rows), x_inv 0.497
    (d20-h130-n1-k1-b3-null-dx-null-wgrad), ladj_inv 0.067 (d3-h3-n1-k1-b70).  At most 0.31 of C (ladj_inv, rows: 0.22 ... 0.24).
Factor by which each mutation of the reference exceeded the bound on the kernels' output, weakest named case and stage (HIP_TEETH
lines of test_tolerance_rejects_mutated_reference): flip_first 1.5e5 (z0), ladj_sign 1.8e3 (rows), drop_gl 10.7 (dx, on
d65-h130-n3-k2-b70, where the first-order bound through the triangular solve is at its loosest), out_le 2.2e3 (z0)."""
import pytest
import torch

import iaf_ref as R

pytestmark = pytest.mark.gpu
D = torch.device("cuda:0")
MEASURED = {}
_RUNS = {}


def _lib():
    from multivae_amd import _lib as L

    return L


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=D)


def _flat(nested):
    return [t for per_block in nested for t in per_block]


def launch(case, I, poison=False):
    """Forward, backward and inverse from fresh NaN-filled outputs -> every array written, on the CPU, under the keys of
    iaf_ref.reference (None: not written).  poison: every masked weight is NaN."""
    Lb = _lib()
    sp = Lb.stream_ptr
    Dm, H, nh, nb, B = case.D, case.H, case.nh, case.nb, case.B
    dv = lambda t: None if t is None else t.to(D).contiguous()
    Ws, bs = [dv(w) for w in _flat(I["W"])], [dv(v) for v in _flat(I["b"])]
    if poison:
        mk = R.masks(Dm, H, nh)
        for i, w in enumerate(Ws):
            w[~mk[i % (nh + 1)].to(D)] = float("nan")
    x = dv(I["x"])
    z0, ladj = nan(B, Dm), nan(B)
    rows = None if "rows" in case.null else nan(B)
    n_ws = nb * B * (2 * Dm + nh * H)
    ws = nan(n_ws) if case.backward else None
    Lb.call("mvk_iaf_fwd", Lb.ptr(x), Lb.ptr_array(Ws), Lb.ptr_array(bs), nb, nh, Dm, H, B, Lb.ptr(z0), Lb.ptr(ladj), Lb.ptr(rows),
            Lb.ptr(ws), sp())
    out = dict(z0=z0, ladj=ladj, rows=rows, dx=None, dW=None, db=None)
    if case.backward:
        dx = None if "dx" in case.null else nan(B, Dm)
        wgrad = "wgrad" not in case.null
        deltas = nan(n_ws) if wgrad else None
        dWs = [torch.zeros_like(w) for w in Ws] if wgrad else None
        dbs = [torch.zeros_like(v) for v in bs] if wgrad else None
        grows, dz0, dladj = dv(I["grows"]), dv(I["dz0"]), dv(I["dladj"])  # held: a pointer must not outlive its tensor
        Lb.call("mvk_iaf_bwd", Lb.ptr_array(Ws), nb, nh, Dm, H, Lb.ptr(z0), Lb.ptr(ws), Lb.ptr(grows), Lb.ptr(dz0), Lb.ptr(dladj), B,
                Lb.ptr(dx), Lb.ptr(deltas), Lb.ptr_array(dWs) if wgrad else None, Lb.ptr_array(dbs) if wgrad else None, sp())
        out.update(dx=dx, dW=dWs, db=dbs)
    xi, li = nan(B, Dm), None if "ladj_inv" in case.null else nan(B)
    y = dv(I["y"])
    Lb.call("mvk_iaf_inverse", Lb.ptr(y), Lb.ptr_array(Ws), Lb.ptr_array(bs), nb, nh, Dm, H, B, Lb.ptr(xi), Lb.ptr(li), sp())
    out.update(x_inv=xi, ladj_inv=li)
    torch.cuda.synchronize()
    cpu = lambda v: None if v is None else ([t.cpu().contiguous() for t in v] if isinstance(v, list) else v.cpu().contiguous())
    return {k: cpu(v) for k, v in out.items()}


def _tensors(d):
    for k, v in d.items():
        if v is None:
            continue
        for i, t in enumerate(v if isinstance(v, list) else [v]):
            yield f"{k}[{i}]" if isinstance(v, list) else k, t


def differing(a, b):
    """The first array that both hold and that differs in its bits (None: none)."""
    other = dict(_tensors(b))
    for k, t in _tensors(a):
        if k in other and not torch.equal(t.view(torch.int32), other[k].view(torch.int32)):
            return k
    return None


def run_case(case):
    """(inputs, first launch, second launch, reference, bases) of a case: launched once per session, shared, left unchanged."""
    if case.name not in _RUNS:
        I = R.make_inputs(case)
        ref = R.reference(case, I)
        _RUNS[case.name] = (I, launch(case, I), launch(case, I), ref, R.bases(case, I, ref))
    return _RUNS[case.name]


def check_case(case):
    I, got, got2, ref, base = run_case(case)
    assert differing(got, got2) is None, f"{case.name}: a second launch differs in {differing(got, got2)}"
    for k, t in _tensors(got):
        assert not bool(torch.isnan(t).any()), f"{case.name}: {k} holds a NaN"
    want = set(R.STAGES)
    if "rows" in case.null:
        want -= {"rows"}
    if "dx" in case.null:
        want -= {"dx"}
    if "wgrad" in case.null:
        want -= {"dW", "db"}
    if "ladj_inv" in case.null:
        want -= {"ladj_inv"}
    if not case.backward:
        want -= {"dx", "dW", "db"}
    assert {k for k, v in got.items() if v is not None} == want, case.name
    if got["dW"] is not None:
        mk = R.masks(case.D, case.H, case.nh)
        for i, g in enumerate(got["dW"]):
            assert not bool(g[~mk[i % (case.nh + 1)]].any()), f"{case.name}: a masked weight has a gradient (dW[{i}])"
    ratios = R.ratios(case, I, got, ref=ref, base=base)
    print(case.name, {k: round(v, 3) for k, v in ratios.items()})
    assert set(ratios) == want
    for k, v in ratios.items():
        if v > MEASURED.get(k, (-1.0, ""))[0]:
            MEASURED[k] = (v, case.name)
    for k, v in ratios.items():
        assert v <= R.C_STAGE[k], f"{case.name}: {k} worst |err| / base = {v:.3g} > C = {R.C_STAGE[k]}"


GROUPS = sorted({(c.D, c.H, c.nh) for c in R.CASES})


@pytest.mark.parametrize("Dm,H,nh", GROUPS, ids=[f"d{a}-h{b}-n{c}" for a, b, c in GROUPS])
def test_kernel_cases(Dm, H, nh):
    for case in [c for c in R.CASES if (c.D, c.H, c.nh) == (Dm, H, nh)]:
        check_case(case)


@pytest.mark.parametrize("mut,stages,names", R.TEETH, ids=[t[0] for t in R.TEETH])
def test_tolerance_rejects_mutated_reference(mut, stages, names):
    """The comparison of test_kernel_cases, with one deliberate mistake in the REFERENCE, must fail on the HIP kernels' output in
    every stage named for it on every case named for it (shown against torch fp32 in test_iaf_host.py)."""
    for name in names:
        case = R.CASE_BY_NAME[name]
        I, got, _, _, base = run_case(case)
        bad = R.ratios(case, I, got, mut=(mut,), base=base)
        for s in stages:
            f = bad[s] / R.C_STAGE[s]
            print("HIP_TEETH", mut, name, s, f"{f:.3g}")
            assert f > 1.0, f"{mut} passes {s} on {name}: {f:.3g}x the bound"


@pytest.mark.parametrize("name", ["d2-h3-n1-k1-b1", "d20-h64-n3-k3-b3", "d65-h130-n3-k2-b70"])
def test_masked_weights_are_never_read(name):
    """The kernels take the masks from indices: NaN in every masked weight (torch's `mask * weight` would give NaN) changes no bit."""
    case = R.CASE_BY_NAME[name]
    I, got, _, _, _ = run_case(case)
    assert differing(got, launch(case, I, poison=True)) is None


def _device_inputs(case, I, grad=False):
    Ws = [w.to(D).requires_grad_(grad) for w in _flat(I["W"])]
    bs = [v.to(D).requires_grad_(grad) for v in _flat(I["b"])]
    up = {k: None if I[k] is None else I[k].to(D) for k in ("grows", "dz0", "dladj")}
    return (case.nb, case.nh, case.D, case.H), Ws, bs, up


def test_weight_gradients_accumulate():
    """dW, db are `+=` targets (kernels._grad_target): a second backward into the same buffers doubles every entry exactly."""
    from multivae_amd import kernels

    case = R.CASE_BY_NAME["d20-h64-n3-k3-b3"]
    I, got, _, _, _ = run_case(case)
    dims, Ws, bs, up = _device_inputs(case, I)
    z0, ladj, rows, ws = kernels.iaf_forward(I["x"].to(D), dims, Ws, bs, want_rows=True)
    dWs, dbs = [torch.zeros_like(w) for w in Ws], [torch.zeros_like(v) for v in bs]
    dWs[3] = None  # a null entry: that tensor is skipped
    for _ in range(2):
        kernels.iaf_backward(dims, Ws, z0, ws, dWs=dWs, dbs=dbs, **up)
    for i, (g, r) in enumerate(zip(dWs, got["dW"])):
        assert g is None or torch.equal(g.cpu(), 2 * r), i
    assert all(torch.equal(g.cpu(), 2 * r) for g, r in zip(dbs, got["db"]))


def test_argument_checks():
    """MVK_EINVAL, without a launch (the sentinel-filled buffers stay as they are), for every out-of-range D, H, hidden-layer and
    block count; NULL x / W / b / z0 / ladj / ws / y; a NULL weight or bias entry; no upstream gradient at all; weight gradients
    without deltas; negative B / R.  B = 0 and R = 0 are MVK_OK and write nothing; rows, ws, dx and the inverse's ladj may be
    NULL."""
    Lb = _lib()
    sp = Lb.stream_ptr
    t = torch.full((1 << 16,), 7.0, device=D)
    p = Lb.ptr(t)

    def table(n, hole=None, present=True):
        if not present:
            return None
        arr = Lb.ptr_array([t] * max(n, 1))
        if hole is not None:
            arr[hole] = None
        return arr

    def fwd(x=p, W=True, b=True, w_hole=None, b_hole=None, nb=2, nh=1, Dm=3, H=4, B=3, z0=p, ladj=p, rows=p):
        n = max(nb, 1) * (max(nh, 0) + 1)
        Lb.call("mvk_iaf_fwd", x, table(n, w_hole, W), table(n, b_hole, b), nb, nh, Dm, H, B, z0, ladj, rows, p, sp())

    def bwd(W=True, w_hole=None, nb=2, nh=1, Dm=3, H=4, z0=p, ws=p, grows=p, dz0=None, dladj=None, B=3, deltas=p, dW=True, db=True):
        n = max(nb, 1) * (max(nh, 0) + 1)
        Lb.call("mvk_iaf_bwd", table(n, w_hole, W), nb, nh, Dm, H, z0, ws, grows, dz0, dladj, B, None, deltas, table(n, None, dW),
                table(n, None, db), sp())

    def inv(y=p, W=True, b=True, w_hole=None, b_hole=None, nb=2, nh=1, Dm=3, H=4, Rr=3, x=p):
        n = max(nb, 1) * (max(nh, 0) + 1)
        Lb.call("mvk_iaf_inverse", y, table(n, w_hole, W), table(n, b_hole, b), nb, nh, Dm, H, Rr, x, None, sp())

    shapes = [dict(Dm=1), dict(Dm=513), dict(Dm=0), dict(H=0), dict(H=513), dict(nh=0), dict(nh=5), dict(nb=0), dict(nb=5)]
    bad = [lambda kw=kw: fwd(**kw) for kw in shapes] + [lambda kw=kw: bwd(**kw) for kw in shapes] + \
          [lambda kw=kw: inv(**kw) for kw in shapes]
    bad += [lambda: fwd(x=None), lambda: fwd(W=False), lambda: fwd(b=False), lambda: fwd(w_hole=3), lambda: fwd(b_hole=0),
            lambda: fwd(z0=None), lambda: fwd(ladj=None), lambda: fwd(B=-1),
            lambda: bwd(W=False), lambda: bwd(w_hole=2), lambda: bwd(z0=None), lambda: bwd(ws=None), lambda: bwd(B=-1),
            lambda: bwd(grows=None), lambda: bwd(deltas=None), lambda: bwd(deltas=None, dW=False), lambda: bwd(deltas=None, db=False),
            lambda: inv(y=None), lambda: inv(W=False), lambda: inv(b=False), lambda: inv(w_hole=1), lambda: inv(b_hole=3),
            lambda: inv(x=None), lambda: inv(Rr=-1)]
    for i, f in enumerate(bad):
        with pytest.raises(Lb.MvkError):
            f()
            pytest.fail(f"bad call {i} was accepted")
    fwd(B=0)
    bwd(B=0)
    inv(Rr=0)
    torch.cuda.synchronize()
    assert bool((t == 7.0).all())


def test_autograd_function_matches_the_kernel_reference():
    """kernels.IAFFlowFn under torch.autograd: the kernels' outputs as (rows, z0, ladj) and gradients for x and every parameter
    within the bounds of the float64 reference; kernels.iaf_inverse; the shape checks."""
    from multivae_amd import kernels

    case = R.CASE_BY_NAME["d20-h64-n3-k3-b3"]
    I, got, _, ref, base = run_case(case)
    dims, Ws, bs, up = _device_inputs(case, I, grad=True)
    params = [t for pair in zip(Ws, bs) for t in pair]
    x = I["x"].to(D).requires_grad_(True)
    rows, z0, ladj = kernels.IAFFlowFn.apply(dims, x, *params)
    total = (rows * up["grows"]).sum()
    if up["dz0"] is not None:
        total = total + (z0 * up["dz0"]).sum()
    if up["dladj"] is not None:
        total = total + (ladj * up["dladj"]).sum()
    total.backward()
    fn = dict(z0=z0.detach().cpu(), ladj=ladj.detach().cpu(), rows=rows.detach().cpu(), dx=x.grad.cpu(),
              dW=[w.grad.cpu() for w in Ws], db=[v.grad.cpu() for v in bs])
    ratios = R.ratios(case, I, fn, ref=ref, base=base)
    assert set(ratios) == {"z0", "ladj", "rows", "dx", "dW", "db"}
    for k, v in ratios.items():
        assert v <= R.C_STAGE[k], f"IAFFlowFn: {k} worst |err| / base = {v:.3g} > C = {R.C_STAGE[k]}"
    assert differing(fn, got) is None  # the same launches: the same bits
    # a second backward accumulates into .grad; an input that needs no gradient gets none
    x2 = I["x"].to(D)
    rows2, _, _ = kernels.IAFFlowFn.apply(dims, x2, *params)
    rows2.backward(up["grows"])
    assert x2.grad is None and all(p.grad is not None for p in params)
    xi, li = kernels.iaf_inverse(I["y"].to(D), dims, [w.detach() for w in Ws], [v.detach() for v in bs], want_ladj=True)
    assert torch.equal(xi.cpu(), got["x_inv"]) and torch.equal(li.cpu(), got["ladj_inv"])
    assert kernels.iaf_fused_ok(20, 64, 3, 3) and not kernels.iaf_fused_ok(1, 64, 3, 3) and not kernels.iaf_fused_ok(20, 64, 5, 3)
    with pytest.raises(ValueError, match="expected"):
        kernels.iaf_forward(I["x"].to(D)[:, :5], dims, [w.detach() for w in Ws], [v.detach() for v in bs])
    with pytest.raises(ValueError, match="expected"):
        kernels.iaf_inverse(I["y"].to(D), dims, [w.detach() for w in Ws][:-1], [v.detach() for v in bs][:-1])


def test_zz_report():
    """Prints the head-room the HIP kernels showed in this session: the largest |err| / base per stage, with the case."""
    print("HIP_MEASURED", {k: (round(v, 3), n) for k, (v, n) in sorted(MEASURED.items())})
