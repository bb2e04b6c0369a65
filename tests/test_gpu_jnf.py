"""JNF on the GPU: mvk_maf_fwd / mvk_maf_bwd / mvk_maf_inverse called directly through the C ABI, entry-wise against float64; the
public model against the goldens recorded from the reference and the float64 restatement of tests/jnf_ref.py; and
MultistageTrainer through the stage change.

Kernels.  Reference, case table (jnf_ref.CASES: D in {2, 3, 20, 65} x H in {3, 64, 130} x hidden layers in {1, 3} x blocks in
{1, 2, 3} x B in {1, 3, 70} x M in {1, 2, 3}, the optional pointers — posteriors, dz, weight gradients, the inverse's ladj — and the
upstream gradients cycled over it; plus D = 512, H = 128, B = 3 forward and inverse only) and error model (a first-order running
error analysis) live in tests/jnf_ref.py.  Per case:
1. every output of the forward, the backward and the inverse launch, pre-filled with NaN (the accumulated weight gradients: with
   zeros), against the float64 reference: |got - ref| <= C_STAGE[stage] * base for EVERY entry; a NaN left anywhere fails; a
   masked weight's gradient is exactly 0;
2. a second launch from the same buffers is bit-identical;
3. test_masked_weights_are_never_read: NaN in every masked weight changes no bit of any output;
4. test_argument_checks: every MVK_EINVAL branch returns without launching, B = 0 / R = 0 is MVK_OK and writes nothing.

Constants (jnf_ref.C_STAGE = 4x the largest |err| / base of the same formulas in plain torch fp32 on the CPU, backward by fp32
autograd, over the case table, rounded up; re-derived by test_jnf_host.py::test_error_constants, never from the HIP kernels):
    stage      torch fp32   C     set by
    z0         0.650        3.0   d20-h3-n1-k1-b70-m2-null-dz-null-wgrad
    ladj       0.077        0.4   d20-h3-n3-k1-b70-m3-null-post
    rows       0.232        1.0   d2-h3-n1-k1-b70-m3-null-wgrad
    dmu0       0.551        2.5   d2-h3-n1-k1-b70-m3-null-wgrad
    dlv0       0.519        2.5   d20-h64-n3-k1-b70-m3
    dz         0.390        2.0   d20-h3-n3-k1-b70-m2
    dW         0.201        1.0   d65-h3-n3-k1-b1-m3-null-dz
    db         0.218        1.0   d65-h3-n3-k1-b1-m2-null-post
    x_inv      0.697        3.0   d2-h64-n3-k1-b70-m3-null-wgrad
    ladj_inv   0.098        0.4   d2-h3-n3-k1-b70-m3-null-ladj_inv
The sampler: jnf_ref.C_HMC = 1.0 (torch fp32 drifts by 0.221 of jnf_ref.hmc_base; every |u - alpha| of the seed > 1e-3 in float64).

Largest |err| / base of the HIP kernels on an MI355X (test_zz_report prints HIP_MEASURED); recorded, not a bound:
    z0 0.650 (d20-h3-n1-k1-b70-m2-null-dz-null-wgrad), ladj 0.081 (d2-h3-n1-k2-b70-m3-null-post), rows 0.184
    (d3-h3-n1-k1-b70-m2-null-wgrad), dmu0 0.544 (d65-h64-n3-k1-b70-m1-null-dz-null-wgrad), dlv0 0.695
    (d20-h3-n3-k3-b70-m3-null-dz-null-wgrad), dz 0.390 (d20-h3-n3-k1-b70-m2), dW 0.215 and db 0.221 (d65-h3-n3-k1-b1-m3-null-dz),
    x_inv 0.523 (d65-h64-n3-k1-b70-m3-null-post), ladj_inv 0.072 (d2-h3-n3-k1-b3-m2).  At most 0.28 of C (dlv0).
    The sampler (HIP_HMC): 0.256 of hmc_base against C_HMC = 1.0, 22 of 24 moves accepted as in float64.
Factor by which each mutation of the reference exceeded the bound on the kernels' output, weakest named case and stage (HIP_TEETH
lines of test_tolerance_rejects_mutated_reference): no_flip 1.0e5 (z0), flip_first 612 (ladj), exp_plus 1.1e4 (z0), hidden_gt 567
(ladj), out_le 4.8e3 (x_inv), drop_ladj 23.9 (rows), inv_order 3.5 (x_inv, on d65-h130-n1-k3-b70-m3, where the first-order bound
is at its loosest).

Model.  Every golden case within the 1e-4 relative parity bar (loss, loss_sum, metrics, every gradient against float64 and against
the recorded statistics); in stage one the encoders and the flows have no gradient, in stage two the joint encoder and the
decoders are frozen and have none; the fused and the torch-module paths agree on the same model; encode shapes for N in {1, 3},
both flatten values and return_mean; single-modality encode against the oracle's inverse; `_compute_poe_posterior` value and
gradient against float64; `_sample_from_poe_subset` on fed draws against the float64 sampler; graph replay of a stage-one and of a
stage-two step against the eager step, bit for bit; save + AutoModel.load_from_folder; the folder the reference wrote.

Trainer.  A tiny JNF (warmup 2) for 4 epochs of 3 steps, eager and with use_hip_graph: the reset at epoch 3 with its checkpoint,
which modules move in which stage (bit for bit), and a resume from a stage-two checkpoint."""
import lzma
import math
import os
import shutil

import numpy as np
import pytest
import torch

import golden_cases as G
import jnf_ref as R

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
    return [t for per_flow in nested for per_block in per_flow for t in per_block]


def launch(case, I, poison=False):
    """Forward, backward and inverse from fresh NaN-filled outputs -> every array written, on the CPU, under the keys of
    jnf_ref.reference (None: not written).  poison: every masked weight is NaN."""
    Lb = _lib()
    sp = Lb.stream_ptr
    Dm, H, nh, nb, B, M = case.D, case.H, case.nh, case.nb, case.B, case.M
    dv = lambda t: None if t is None else t.to(D).contiguous()
    Ws, bs = [dv(w) for w in _flat(I["W"])], [dv(v) for v in _flat(I["b"])]
    if poison:
        mk = R.masks(Dm, H, nh)
        for i, w in enumerate(Ws):
            w[~mk[i % (nh + 1)].to(D)] = float("nan")
    post = I["mu0"] is not None
    z = dv(I["z"])
    mu0, lv0 = dv(I["mu0"]), dv(I["lv0"])
    mus = Lb.ptr_array([mu0[m] for m in range(M)]) if post else None
    lvs = Lb.ptr_array([lv0[m] for m in range(M)]) if post else None
    z0, ladj, rows = nan(M, B, Dm), nan(M, B), nan(M, B) if post else None
    n_ws = M * nb * B * (2 * Dm + nh * H)
    ws = nan(n_ws) if case.backward else None
    Lb.call("mvk_maf_fwd", Lb.ptr(z), Lb.ptr_array(Ws), Lb.ptr_array(bs), M, nb, nh, Dm, H, mus, lvs, B, Lb.ptr(z0), Lb.ptr(ladj),
            Lb.ptr(rows), Lb.ptr(ws), sp())
    out = dict(z0=z0, ladj=ladj, rows=rows, dmu0=None, dlv0=None, dz=None, dW=None, db=None)
    if case.backward:
        dmu0, dlv0 = (nan(M, B, Dm), nan(M, B, Dm)) if post else (None, None)
        dz = None if "dz" in case.null else nan(B, Dm)
        wgrad = "wgrad" not in case.null
        deltas = nan(n_ws) if wgrad else None
        dWs = [torch.zeros_like(w) for w in Ws] if wgrad else None
        dbs = [torch.zeros_like(v) for v in bs] if wgrad else None
        grows, dz0, dladj = dv(I["grows"]), dv(I["dz0"]), dv(I["dladj"])  # held: a pointer must not outlive its tensor
        Lb.call("mvk_maf_bwd", Lb.ptr_array(Ws), M, nb, nh, Dm, H, mus, lvs, Lb.ptr(z0), Lb.ptr(ws), Lb.ptr(grows),
                Lb.ptr(dz0), Lb.ptr(dladj), B,
                Lb.ptr_array([dmu0[m] for m in range(M)]) if post else None,
                Lb.ptr_array([dlv0[m] for m in range(M)]) if post else None, Lb.ptr(dz), Lb.ptr(deltas),
                Lb.ptr_array(dWs) if wgrad else None, Lb.ptr_array(dbs) if wgrad else None, sp())
        out.update(dmu0=dmu0, dlv0=dlv0, dz=dz, dW=dWs, db=dbs)
    n1 = nb * (nh + 1)
    x, li = nan(B, Dm), None if "ladj_inv" in case.null else nan(B)
    y = dv(I["y"])
    Lb.call("mvk_maf_inverse", Lb.ptr(y), Lb.ptr_array(Ws[:n1]), Lb.ptr_array(bs[:n1]), nb, nh, Dm, H, B, Lb.ptr(x),
            Lb.ptr(li), sp())
    out.update(x_inv=x, ladj_inv=li)
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


def _named(name):
    return R.CASE_BY_NAME[[n for n in R.CASE_BY_NAME if n.split("-null")[0] == name][0]]


def check_case(case):
    I, got, got2, ref, base = run_case(case)
    assert differing(got, got2) is None, f"{case.name}: a second launch differs in {differing(got, got2)}"
    for k, t in _tensors(got):
        assert not bool(torch.isnan(t).any()), f"{case.name}: {k} holds a NaN"
    want = set(R.STAGES)
    if "post" in case.null:
        want -= {"rows", "dmu0", "dlv0"}
    if "dz" in case.null:
        want -= {"dz"}
    if "wgrad" in case.null:
        want -= {"dW", "db"}
    if "ladj_inv" in case.null:
        want -= {"ladj_inv"}
    if not case.backward:
        want -= {"dmu0", "dlv0", "dz", "dW", "db"}
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


GROUPS = sorted({(c.D, c.H, c.nh, c.nb) for c in R.CASES})


@pytest.mark.parametrize("Dm,H,nh,nb", GROUPS, ids=[f"d{a}-h{b}-n{c}-k{d}" for a, b, c, d in GROUPS])
def test_kernel_cases(Dm, H, nh, nb):
    for case in [c for c in R.CASES if (c.D, c.H, c.nh, c.nb) == (Dm, H, nh, nb)]:
        check_case(case)


@pytest.mark.parametrize("mut,stages,names", R.TEETH, ids=[t[0] for t in R.TEETH])
def test_tolerance_rejects_mutated_reference(mut, stages, names):
    """The comparison of test_kernel_cases, with one deliberate mistake in the REFERENCE, must fail on the HIP kernels' output in
    every stage named for it on every case named for it (shown against torch fp32 in test_jnf_host.py)."""
    for name in names:
        case = _named(name)
        I, got, _, _, base = run_case(case)
        bad = R.ratios(case, I, got, mut=(mut,), base=base)
        for s in stages:
            f = bad[s] / R.C_STAGE[s]
            print("HIP_TEETH", mut, name, s, f"{f:.3g}")
            assert f > 1.0, f"{mut} passes {s} on {name}: {f:.3g}x the bound"


@pytest.mark.parametrize("name", ["d2-h3-n1-k1-b3-m2", "d20-h64-n3-k2-b3-m2", "d65-h130-n3-k3-b3-m1"])
def test_masked_weights_are_never_read(name):
    """The kernels take the masks from indices: NaN in every masked weight (torch's `mask * weight` would give NaN) changes no bit."""
    case = _named(name)
    I, got, _, _, _ = run_case(case)
    assert differing(got, launch(case, I, poison=True)) is None


def test_weight_gradients_accumulate():
    """dW, db are `+=` targets (kernels._grad_target): a second backward into the same buffers doubles every entry exactly."""
    from multivae_amd import kernels

    case = _named("d20-h64-n3-k2-b3-m2")
    I, got, _, _, _ = run_case(case)
    Ws, bs = [w.to(D) for w in _flat(I["W"])], [v.to(D) for v in _flat(I["b"])]
    dims = (case.nb, case.nh, case.D, case.H)
    mus, lvs = list(I["mu0"].to(D)), list(I["lv0"].to(D))
    z0, ladj, rows, ws = kernels.maf_forward(I["z"].to(D), dims, Ws, bs, mus, lvs)
    dWs, dbs = [torch.zeros_like(w) for w in Ws], [torch.zeros_like(v) for v in bs]
    dWs[3] = None  # a null entry: that tensor is skipped
    up = dict(grows=I["grows"].to(D), dz0=None if I["dz0"] is None else I["dz0"].to(D),
              dladj=None if I["dladj"] is None else I["dladj"].to(D))
    for _ in range(2):
        kernels.maf_backward(dims, Ws, z0, ws, mus, lvs, dWs=dWs, dbs=dbs, **up)
    for i, (g, r) in enumerate(zip(dWs, got["dW"])):
        assert g is None or torch.equal(g.cpu(), 2 * r), i
    assert all(torch.equal(g.cpu(), 2 * r) for g, r in zip(dbs, got["db"]))


def test_argument_checks():
    """MVK_EINVAL, without a launch (the sentinel-filled buffers stay as they are), for every out-of-range D, H, hidden-layer,
    block and flow count; NULL z / W / b / z0 / ladj / ws / x / y; a NULL weight or bias entry; posteriors given in part (mu0
    without lv0, rows without posteriors, a NULL entry); grows without posteriors; no upstream gradient at all; weight gradients
    without deltas; negative B / R.  B = 0 and R = 0 are MVK_OK and write nothing; M = 8 is accepted."""
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

    def fwd(z=p, W=True, b=True, w_hole=None, b_hole=None, M=2, nb=2, nh=1, Dm=3, H=4, mu=True, lv=True, mu_hole=None, B=3, z0=p,
            ladj=p, rows=p):
        n = max(M, 1) * max(nb, 1) * (max(nh, 0) + 1)
        Lb.call("mvk_maf_fwd", z, table(n, w_hole, W), table(n, b_hole, b), M, nb, nh, Dm, H, table(M, mu_hole, mu), table(M, None, lv),
                B, z0, ladj, rows, p, sp())

    def bwd(W=True, w_hole=None, M=2, nb=2, nh=1, Dm=3, H=4, mu=True, lv=True, dmu=True, dlv=True, hole=None, z0=p, ws=p, grows=p,
            dz0=None, dladj=None, B=3, deltas=p, dW=True):
        n = max(M, 1) * max(nb, 1) * (max(nh, 0) + 1)
        tabs = [table(M, hole[1] if hole and hole[0] == i else None, present) for i, present in enumerate((mu, lv, dmu, dlv))]
        Lb.call("mvk_maf_bwd", table(n, w_hole, W), M, nb, nh, Dm, H, tabs[0], tabs[1], z0, ws, grows, dz0, dladj, B, tabs[2], tabs[3],
                None, deltas, table(n, None, dW), table(n, None, dW), sp())

    def inv(y=p, W=True, b=True, w_hole=None, b_hole=None, nb=2, nh=1, Dm=3, H=4, Rr=3, x=p):
        n = max(nb, 1) * (max(nh, 0) + 1)
        Lb.call("mvk_maf_inverse", y, table(n, w_hole, W), table(n, b_hole, b), nb, nh, Dm, H, Rr, x, None, sp())

    shapes = [dict(Dm=1), dict(Dm=513), dict(Dm=0), dict(H=0), dict(H=513), dict(nh=0), dict(nh=5), dict(nb=0), dict(nb=5)]
    bad = [lambda kw=kw: fwd(**kw) for kw in shapes] + [lambda kw=kw: bwd(**kw) for kw in shapes] + \
          [lambda kw=kw: inv(**kw) for kw in shapes]
    bad += [lambda: fwd(M=0), lambda: fwd(M=9), lambda: fwd(z=None), lambda: fwd(W=False), lambda: fwd(b=False), lambda: fwd(w_hole=3),
            lambda: fwd(b_hole=0), lambda: fwd(z0=None), lambda: fwd(ladj=None), lambda: fwd(B=-1), lambda: fwd(lv=False),
            lambda: fwd(mu=False), lambda: fwd(rows=None), lambda: fwd(mu=False, lv=False), lambda: fwd(mu_hole=1),
            lambda: bwd(M=0), lambda: bwd(M=9), lambda: bwd(W=False), lambda: bwd(w_hole=2), lambda: bwd(z0=None), lambda: bwd(ws=None),
            lambda: bwd(B=-1), lambda: bwd(lv=False), lambda: bwd(dmu=False), lambda: bwd(dlv=False), lambda: bwd(hole=(0, 1)),
            lambda: bwd(hole=(1, 0)), lambda: bwd(hole=(2, 1)), lambda: bwd(hole=(3, 0)), lambda: bwd(grows=None),
            lambda: bwd(mu=False, lv=False, dmu=False, dlv=False), lambda: bwd(deltas=None),
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
    # M = MVK_MAX_MODALITIES itself is accepted, and so are rows without posteriors left out together
    w, b = torch.full((64,), 0.25, device=D), torch.full((64,), 0.1, device=D)
    x = torch.full((2, 2), 0.5, device=D)
    z0, ladj = nan(8, 2, 2), nan(8, 2)
    Lb.call("mvk_maf_fwd", Lb.ptr(x), Lb.ptr_array([w] * 16), Lb.ptr_array([b] * 16), 8, 1, 1, 2, 3, None, None, 2, Lb.ptr(z0),
            Lb.ptr(ladj), None, None, sp())
    torch.cuda.synchronize()
    assert not bool(torch.isnan(z0).any()) and not bool(torch.isnan(ladj).any()) and bool((t == 7.0).all())
    assert all(torch.equal(z0[0], z0[m]) for m in range(8))


def test_autograd_function_matches_the_kernel_reference():
    """kernels.MAFFlowsFn: the kernels' outputs as (rows, z0, ladj), gradients for z, the posteriors and every parameter;
    kernels.maf_inverse; the shape checks."""
    from multivae_amd import kernels

    case = _named("d20-h64-n3-k2-b3-m2")
    I, got, _, _, _ = run_case(case)
    dims = (case.nb, case.nh, case.D, case.H)
    Ws, bs = [w.to(D).requires_grad_(True) for w in _flat(I["W"])], [v.to(D).requires_grad_(True) for v in _flat(I["b"])]
    params = [t for pair in zip(Ws, bs) for t in pair]
    mus = [I["mu0"][m].to(D).requires_grad_(True) for m in range(2)]
    lvs = [I["lv0"][m].to(D).requires_grad_(True) for m in range(2)]
    z = I["z"].to(D).requires_grad_(True)
    rows, z0, ladj = kernels.MAFFlowsFn.apply(dims, True, z, *mus, *lvs, *params)
    total = (rows * I["grows"].to(D)).sum()
    if I["dz0"] is not None:
        total = total + (z0 * I["dz0"].to(D)).sum()
    if I["dladj"] is not None:
        total = total + (ladj * I["dladj"].to(D)).sum()
    total.backward()
    assert torch.equal(rows.detach().cpu(), got["rows"]) and torch.equal(z0.detach().cpu(), got["z0"])
    assert torch.equal(ladj.detach().cpu(), got["ladj"]) and torch.equal(z.grad.cpu(), got["dz"])
    for m in range(2):
        assert torch.equal(mus[m].grad.cpu(), got["dmu0"][m]) and torch.equal(lvs[m].grad.cpu(), got["dlv0"][m]), m
    assert all(torch.equal(w.grad.cpu(), g) for w, g in zip(Ws, got["dW"])) and all(torch.equal(v.grad.cpu(), g) for v, g in zip(bs, got["db"]))
    # without posteriors: z0 and ladj only; a parameter that asks for no gradient gets none
    Ws[0].requires_grad_(False)
    Ws[0].grad = None
    r2, z02, l2 = kernels.MAFFlowsFn.apply(dims, False, z, *params)
    assert r2 is None and torch.equal(z02.detach().cpu(), got["z0"]) and torch.equal(l2.detach().cpu(), got["ladj"])
    (z02.sum() + l2.sum()).backward()
    assert Ws[0].grad is None
    n1 = case.nb * (case.nh + 1)
    x, li = kernels.maf_inverse(I["y"].to(D), dims, [w.detach() for w in Ws[:n1]], [v.detach() for v in bs[:n1]], want_ladj=True)
    assert torch.equal(x.cpu(), got["x_inv"]) and torch.equal(li.cpu(), got["ladj_inv"])
    with pytest.raises(ValueError):
        kernels.maf_forward(I["z"].to(D), dims, Ws[:-1], bs[:-1])
    with pytest.raises(ValueError):
        kernels.maf_inverse(I["y"].to(D)[:, :5], dims, Ws[:n1], bs[:n1])
    with pytest.raises(ValueError):
        kernels.maf_forward(I["z"].to(D), (case.nb, case.nh, case.D, 600), Ws, bs)


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def _model(cfg):
    from multivae_amd.models import JNF, JNFConfig

    model = JNF(JNFConfig(**R.config_kwargs(cfg)))
    res = model.load_state_dict({k: G.t(v) for k, v in R.case_state_dict(cfg).items()}, strict=False)
    assert not res.unexpected_keys and all(k.endswith(".mask") for k in res.missing_keys)
    return model.to(D).train()


def _inputs(cfg):
    from multivae_amd.data.datasets.base import DatasetOutput

    _, data = R.case_inputs(cfg)
    return DatasetOutput(data={m: G.t(v).to(D) for m, v in data.items()})


@pytest.mark.parametrize("case", R.JNF_CASES)
def test_golden(case):
    cfg, a = G.load_case(case)
    model = _model(cfg)
    model.zero_grad(set_to_none=True)
    stage2 = cfg["epoch"] > cfg["warmup"]
    assert model._binding(list(R.case_dims(cfg))) is not None  # the default flows run fused
    out = model(_inputs(cfg), noise=G.t(a["eps"]).to(D), epoch=cfg["epoch"], some_unknown_kwarg=3)
    out.loss.backward()
    assert list(out.keys()) == ["loss", "loss_sum", "metrics"] and list(out.metrics) == ["kld_prior", "recon_loss", "ljm"]
    for k in ("loss", "loss_sum"):
        print(case, k, float(out[k]), float(a[k]))
        assert abs(float(out[k]) - float(a[k])) <= 1e-4 * abs(float(a[k])), (k, float(out[k]), float(a[k]))
    for k in out.metrics:
        ref = float(a["metric/" + k])
        assert abs(float(out.metrics[k]) - ref) <= 1e-4 * max(1.0, abs(ref)), (k, float(out.metrics[k]), ref)
    params = dict(model.named_parameters())
    for k, p in params.items():
        if k in cfg["nograd"]:
            assert p.grad is None or not bool(p.grad.any()), k
        else:
            assert p.grad is not None, k
    assert [k for k, p in params.items() if not p.requires_grad] == cfg["frozen"]
    if stage2:
        assert sorted(k for k, p in params.items() if p.grad is None) == sorted(cfg["nograd"])
        assert all(k.startswith(("joint_encoder.", "decoders.")) for k in cfg["frozen"]) and len(cfg["frozen"]) > 0
        assert all(p.requires_grad and p.grad is not None for k, p in params.items() if k.startswith(("encoders.", "flows.")))
    else:
        assert all(p.grad is None for k, p in params.items() if k.startswith(("encoders.", "flows.")))
    grads = {k: p.grad for k, p in params.items() if p.grad is not None}
    _, g64 = R.reference_grads(cfg, a)
    for k, g in grads.items():
        ref = g64[k] if g64[k] is not None else torch.zeros(g.shape, dtype=torch.float64)
        err = float((g.double().cpu() - ref).abs().max())
        assert err <= 1e-4 * float(ref.abs().max()) + 1e-9, (k, err, float(ref.abs().max()))
    G.check_grads(a, grads, rtol=1e-4)


def test_fused_and_module_paths_agree():
    """The same model with its flows bound to the kernels and with the torch modules in the same place (what a custom BaseNF,
    or a flow outside kernels.maf_fused_ok, runs): same loss, metrics and gradients within the parity bar."""
    cfg, a = G.load_case("jnf_tiny_stage2_beta_rescale")
    noise = G.t(a["eps"]).to(D)
    res = []
    for fused in (True, False):
        model = _model(cfg)
        if not fused:
            model._binding = lambda names: None
        out = model(_inputs(cfg), noise=noise, epoch=3)
        out.loss.backward()
        res.append((out, {k: p.grad for k, p in model.named_parameters()}))
    (x, gx), (y, gy) = res
    assert abs(float(x.loss) - float(y.loss)) <= 1e-5 * abs(float(y.loss)) and abs(float(x.loss_sum) - float(y.loss_sum)) <= 1e-5 * abs(float(y.loss_sum))
    assert all(abs(float(x.metrics[k]) - float(y.metrics[k])) <= 1e-5 * max(1.0, abs(float(y.metrics[k]))) for k in x.metrics)
    assert [k for k, g in gx.items() if g is None] == [k for k, g in gy.items() if g is None]
    for k, g in gx.items():
        if g is not None:
            assert float((g - gy[k]).abs().max()) <= 1e-4 * float(gy[k].abs().max()) + 1e-9, k


def test_eval_mode_and_refusals():
    cfg, a = G.load_case("jnf_tiny_stage2")
    model = _model(cfg).eval()
    with torch.no_grad():
        out = model(_inputs(cfg), epoch=3)
    assert math.isfinite(float(out.loss)) and abs(float(out.loss_sum) - cfg["B"] * float(out.loss)) <= 1e-5 * abs(float(out.loss_sum))
    assert all(p.requires_grad == k.startswith(("encoders.", "flows.")) for k, p in model.named_parameters())
    with pytest.raises(ValueError):
        model(_inputs(cfg), epoch=3, noise=torch.zeros(3, cfg["B"], cfg["L"], device=D))  # the joint draw is [B, L]
    with pytest.raises(AttributeError):
        from multivae_amd.data.datasets.base import DatasetOutput

        data = _inputs(cfg).data
        model(DatasetOutput(data=data, masks={m: torch.ones(cfg["B"], dtype=torch.bool, device=D) for m in data}))


def test_inference_shapes():
    cfg, _ = G.load_case("jnf_tiny_stage1")
    model = _model(cfg).eval()
    inputs = _inputs(cfg)
    B, L, dims = cfg["B"], cfg["L"], R.case_dims(cfg)
    for N in (1, 3):
        for flatten in (False, True):
            lead = (B,) if N == 1 else ((N * B,) if flatten else (N, B))
            for cm in ("all", list(dims), "m2", ["m3"], ["m1", "m3"]):
                emb = model.encode(inputs, cond_mod=cm, N=N, flatten=flatten, mcmc_steps=2, n_lf=1)
                assert tuple(emb.z.shape) == lead + (L,) and emb.one_latent_space is True, (cm, N, flatten)
                assert bool(torch.isfinite(emb.z).all())
            pred = model.predict(inputs, cond_mod="m1", N=N, flatten=flatten)
            assert {m: tuple(pred[m].shape) for m in dims} == {m: lead + d for m, d in dims.items()}
    mean = model.encode(inputs, N=3, return_mean=True).z
    assert tuple(mean.shape) == (3, B, L) and torch.equal(mean[0], mean[2])
    assert torch.equal(model.encode(inputs, return_mean=True).z, model.joint_encoder(inputs.data).embedding)
    one = model.encode(inputs, cond_mod="m2", N=3, return_mean=True).z
    assert tuple(one.shape) == (3, B, L) and torch.equal(one[0], one[2])
    assert tuple(model.generate_from_prior(4).z.shape) == (4, L)


def test_single_modality_encode_is_the_inverse_flow():
    """encode from one modality: a Gaussian sample of its encoder, pulled back through its flow (mvk_maf_inverse), against the
    float64 inverse of the oracle at the same draw; the torch module gives the same."""
    cfg, _ = G.load_case("jnf_tiny_stage2")
    model = _model(cfg).eval()
    inputs = _inputs(cfg)
    B, L = cfg["B"], cfg["L"]
    eps = torch.randn(3, B, L, generator=torch.Generator().manual_seed(3))
    sd = {k: G.t(v).double() for k, v in R.case_state_dict(cfg).items()}
    data, _ = R.case_tensors(cfg, dict(eps=np.zeros((B, L))))
    for m in R.case_dims(cfg):
        z = model.encode(inputs, cond_mod=m, N=3, noise=eps.to(D)).z
        mu, lv = R.mlp_encoder(sd, f"encoders.{m}.", data[m])
        W, b = R.flow_params(sd, m)
        y = (mu + torch.exp(0.5 * lv) * eps.double()).reshape(-1, L)
        want = R.maf_inverse(W, b, y)[0].reshape(3, B, L)
        err = float((z.double().cpu() - want).abs().max())
        print(m, "encode vs float64 inverse:", err, "of", float(want.abs().max()))
        assert err <= 1e-4 * float(want.abs().max())
        with torch.no_grad():
            assert float((model.flows[m](z.reshape(-1, L)).out.double().cpu() - y).abs().max()) <= 1e-4 * float(y.abs().max())
        model._bound[(m,)] = None  # the torch module in the same place
        z2 = model.encode(inputs, cond_mod=m, N=3, noise=eps.to(D)).z
        assert float((z2 - z).abs().max()) <= 1e-5 * float(want.abs().max())


def _hmc_model():
    cfg = R.CASE_CONFIGS[R.HMC["case"]]
    from multivae_amd.data.datasets.base import DatasetOutput

    model = _model(cfg).eval()
    data, start_mod, start_noise, gamma, acc = R.hmc_draws()
    return model, DatasetOutput(data={m: v.to(D) for m, v in data.items()}), (start_mod, start_noise, gamma, acc)


def test_poe_posterior_value_and_gradient():
    model, inputs, (start_mod, start_noise, gamma, acc) = _hmc_model()
    flows, post, _ = R.hmc_setup(torch.float64)
    K = R.HMC["K"]
    data = {m: torch.cat([v] * K) for m, v in inputs.data.items()}
    z = start_noise.to(D)
    for divide in (True, False):
        want, gwant = R.poe_logdensity(flows, post, start_noise.double(), divide_prior=divide)
        for fused in (True, False):
            if not fused:
                model._bound[tuple(R.HMC["subset"])] = None
            ln, g = model._compute_poe_posterior(R.HMC["subset"], z, data, divide_prior=divide, grad=True)
            only = model._compute_poe_posterior(R.HMC["subset"], z, data, divide_prior=divide, grad=False)
            model._bound.pop(tuple(R.HMC["subset"]), None)
            assert torch.equal(only, ln.detach()) or float((only - ln.detach()).abs().max()) <= 1e-5 * float(want.abs().max())
            e1, e2 = float((ln.double().cpu() - want).abs().max()), float((g.double().cpu() - gwant).abs().max())
            print("poe", divide, fused, e1 / float(want.abs().max()), e2 / float(gwant.abs().max()))
            assert e1 <= 1e-4 * float(want.abs().max()) and e2 <= 1e-4 * float(gwant.abs().max())


def test_hmc_on_fed_draws_matches_float64():
    """`_sample_from_poe_subset` (mcmc_steps = 3, n_lf = 2) on the draws of jnf_ref.hmc_draws against the float64 sampler: no
    accept / reject decision can flip (test_jnf_host.py::test_hmc_oracle_condition), the final z within C_HMC * hmc_base."""
    model, inputs, (start_mod, start_noise, gamma, acc) = _hmc_model()
    want, margin, accepted = R.hmc_run(torch.float64)
    assert margin > R.HMC_MARGIN
    K, n_data, L = R.HMC["K"], R.HMC["n_data"], want.shape[1]
    kw = dict(mcmc_steps=R.HMC["mcmc_steps"], n_lf=R.HMC["n_lf"], eps_lf=R.HMC["eps_lf"], start_mod=start_mod,
              start_noise=start_noise.to(D), gamma=gamma.to(D), acc=acc.to(D))
    z = model.encode(inputs, cond_mod=R.HMC["subset"], N=K, **kw).z
    assert tuple(z.shape) == (K, n_data, L)  # K-major
    v = R.worst_ratio(z.reshape(-1, L).cpu(), want, R.hmc_base(want))
    print("HIP_HMC drift / base", v, "accepted", accepted)
    assert v <= R.C_HMC, v
    flat = model.encode(inputs, cond_mod=R.HMC["subset"], N=K, flatten=True, **kw).z
    assert torch.equal(flat, z.reshape(-1, L))


@pytest.mark.parametrize("epoch", [2, 3], ids=["stage1", "stage2"])
def test_graph_replay_equals_eager(epoch):
    from multivae_amd import kernels, schedule
    from multivae_amd.data.datasets.base import DatasetOutput
    from multivae_amd.models import JNF, JNFConfig
    from multivae_amd.trainers import FlatParams, GraphedStep

    torch.manual_seed(0)
    dims = dict(a=(2, 5), b=(7,), c=(3, 1))
    model = JNF(JNFConfig(n_modalities=3, latent_dim=5, input_dims=dims, warmup=2,
                          decoders_dist=dict(a="normal", b="laplace", c="bernoulli"))).to(D).train()
    assert model.graph_key(epoch=2) != model.graph_key(epoch=3) and model.graph_key(epoch=epoch) == epoch - 1
    B = 64
    inputs = DatasetOutput(data={m: torch.rand(B, *d).to(D) for m, d in dims.items()})
    noise = torch.randn(B, 5, device=D)
    flat = FlatParams(model, params=model.stage_parameters(epoch))
    keys = lambda o: [o.loss.detach().clone()] + [v.clone() for v in o.metrics.values() if torch.is_tensor(v)]
    res = []
    for _ in range(2):
        flat.zero_grad()
        with schedule.deferred_reductions(flat):  # the eager form of the step the graph captures (GraphedStep._body)
            out = model(inputs, noise=noise, epoch=epoch)
            out.loss.backward(gradient=kernels.unit_seed(out.loss))
        res.append(keys(out) + [flat.grad.clone()])
    assert all(torch.equal(a, b) for a, b in zip(res[0], res[1]))  # two eager steps: bit-identical
    assert float(res[0][-1].abs().max()) > 0
    gs = GraphedStep(model, flat, inputs, noise=noise, epoch=epoch)
    o = gs(inputs, noise=noise)
    torch.cuda.synchronize()
    got = keys(o) + [flat.grad]
    for i, (x, y) in enumerate(zip(got, res[0])):
        assert torch.equal(x, y), (i, float((x - y).abs().max()))


def test_save_reload_and_the_reference_folder(tmp_path):
    from multivae_amd.models import JNF, AutoModel
    from multivae_amd.models.nn.flows import MAF, MAFConfig, sequential_masks

    cfg, a = G.load_case("jnf_tiny_stage2_beta_rescale")
    model = _model(cfg)
    model.save(str(tmp_path / "saved"))
    blob = torch.load(str(tmp_path / "saved" / "model.pt"), map_location="cpu")["model_state_dict"]
    assert "flows.m1.net.0.net.0.weight" in blob and "flows.m3.net.1.net.6.mask" in blob
    back = AutoModel.load_from_folder(str(tmp_path / "saved")).to(D).train()
    assert type(back) is JNF and back.model_config == model.model_config and back.beta == 2.5
    noise = G.t(a["eps"]).to(D)
    x, y = model(_inputs(cfg), noise=noise, epoch=3), back(_inputs(cfg), noise=noise, epoch=3)
    assert math.isfinite(float(x.loss)) and torch.equal(x.loss.detach(), y.loss.detach())
    assert all(torch.equal(x.metrics[m], y.metrics[m]) for m in x.metrics)
    # custom flows travel through the custom-architecture pickling
    dims = R.case_dims(cfg)
    mine = {m: MAF(MAFConfig(input_dim=(cfg["L"],), n_made_blocks=1, n_hidden_in_made=2, hidden_size=16)) for m in dims}
    custom = JNF(type(model.model_config)(**R.config_kwargs(cfg)), flows=mine)
    custom.save(str(tmp_path / "custom"))
    assert os.path.exists(str(tmp_path / "custom" / "flows.pkl"))
    again = AutoModel.load_from_folder(str(tmp_path / "custom"))
    assert len(again.flows["m1"].net) == 1 and again.flows["m1"].hidden_size == 16
    assert all(torch.equal(v, again.state_dict()[k]) for k, v in custom.state_dict().items())
    # the folder the reference wrote (make_jnf_golden.py): every parameter holds its periodic pattern, every mask its formula
    src = os.path.join(G.GOLDEN, R.FOLDER)
    dst = tmp_path / "theirs"
    dst.mkdir()
    shutil.copy(os.path.join(src, "model_config.json"), str(dst / "model_config.json"))
    with lzma.open(os.path.join(src, "model.pt.xz"), "rb") as fi, open(str(dst / "model.pt"), "wb") as fo:
        fo.write(fi.read())
    theirs = AutoModel.load_from_folder(str(dst))
    assert type(theirs) is JNF and theirs.warmup == R.FOLDER_CONFIG["warmup"] and theirs.beta == R.FOLDER_CONFIG["beta"]
    assert theirs.reset_optimizer_epochs == [R.FOLDER_CONFIG["warmup"] + 1]
    fresh = JNF(theirs.model_config)
    assert list(theirs.state_dict()) == list(fresh.state_dict())
    for i, (k, v) in enumerate(theirs.named_parameters()):
        want = (((torch.arange(v.numel(), dtype=torch.float64) + 13 * i) % 127) / 32 - 2 + i / 4096).reshape(v.shape).to(v.dtype)
        assert torch.equal(v.detach(), want), k
    masks = sequential_masks(R.FOLDER_CONFIG["L"], [128] * 3)
    for k, v in theirs.state_dict().items():
        if k.endswith(".mask"):
            assert torch.equal(v, masks[int(k.split(".")[-2]) // 2]), k
    assert theirs._binding(list(theirs.flows)) is None and theirs.to(D)._binding(list(theirs.flows)) is not None


# ---- the trainer -------------------------------------------------------------------------------------------------------------------
DIMS = dict(a=(2, 5), b=(7,), c=(3, 1))
STAGE_TWO = ("encoders.", "flows.")


def _tiny():
    from multivae_amd.models import JNF, JNFConfig

    torch.manual_seed(1)
    return JNF(JNFConfig(n_modalities=3, latent_dim=5, input_dims=DIMS, warmup=2))


def _dataset():
    from multivae_amd.data.datasets.base import MultimodalBaseDataset

    g = torch.Generator().manual_seed(5)
    return MultimodalBaseDataset(data={m: torch.rand(12, *d, generator=g) for m, d in DIMS.items()})


def _trainer_config(out, **kw):
    from multivae_amd.trainers import MultistageTrainerConfig

    base = dict(output_dir=str(out), per_device_train_batch_size=4, num_epochs=4, learning_rate=1e-3, optimizer_cls="Adam",
                scheduler_cls="StepLR", scheduler_params=dict(step_size=1, gamma=0.5), steps_saving=1)
    base.update(kw)
    return MultistageTrainerConfig(**base)


def _snapshots():
    """A callback holding the trainer: trainer.model.state_dict() (cloned) and the learning rate after every step and epoch."""
    from multivae_amd.trainers import TrainingCallback

    class Snap(TrainingCallback):
        trainer = None

        def __init__(self):
            self.steps, self.epochs, self.epoch = [], {}, None

        def on_epoch_begin(self, training_config, **kwargs):
            self.epoch = kwargs["epoch"]

        def _state(self):
            return {k: v.detach().cpu().clone() for k, v in self.trainer.model.state_dict().items()}

        def on_train_step_end(self, training_config, **kwargs):
            self.steps.append((self.epoch, self.trainer.optimizer.param_groups[0]["lr"], self._state()))

        def on_epoch_end(self, training_config, **kwargs):
            self.epochs[self.epoch] = self._state()

    return Snap()


def _same(a, b, prefix):
    return all(torch.equal(a[k], b[k]) for k in a if k.startswith(prefix))


def test_base_trainer_refuses_jnf(tmp_path):
    from multivae_amd.trainers import BaseTrainer, BaseTrainerConfig

    with pytest.raises(AttributeError, match="MultistageTrainer"):
        BaseTrainer(_tiny(), _dataset(), training_config=BaseTrainerConfig(output_dir=str(tmp_path)))


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "hipgraph"])
def test_trainer_through_the_stage_change(tmp_path, graph):
    from multivae_amd.trainers import MultistageTrainer

    model = _tiny()
    init = {k: v.detach().clone() for k, v in model.state_dict().items()}
    snap = _snapshots()
    trainer = MultistageTrainer(model, _dataset(), training_config=_trainer_config(tmp_path, use_hip_graph=graph), callbacks=[snap])
    snap.trainer = trainer
    hist = trainer.train()
    assert len(hist) == 4 and all(np.isfinite(h["train_epoch_loss"]) for h in hist)
    assert len(snap.steps) == 12 and [e for e, _, _ in snap.steps] == [1] * 3 + [2] * 3 + [3] * 3 + [4] * 3
    assert all(h["train_ljm"] == 0 for h in hist[:2]) and all(h["train_ljm"] != 0 for h in hist[2:])
    # the reset at epoch `warmup + 1` = 3 wrote the best model so far with the reference's file set
    ckpt = os.path.join(trainer.training_dir, "checkpoint_epoch_2")
    assert sorted(f for f in os.listdir(ckpt) if not f.endswith("_mvk.json")) == [
        "environment.json", "info_checkpoint.json", "metrics_best_model.json", "model.pt", "model_config.json", "optimizer.pt",
        "scheduler.pt", "training_config.json"]
    assert trainer.model is not model
    # stage one: the unimodal encoders and the flows keep their initial bits, the rest trains
    prev = init
    for e, _, st in snap.steps[:6]:
        assert _same(st, init, "encoders.") and _same(st, init, "flows."), e
        assert not _same(st, prev, "joint_encoder.") and not _same(st, prev, "decoders."), e
        prev = st
    # stage two runs on the best model of stage one (the end of epoch 1 or 2): its joint encoder and decoders keep those bits, the
    # encoders and the flows train
    best = torch.load(os.path.join(ckpt, "model.pt"), map_location="cpu")["model_state_dict"]
    assert any(_same(best, snap.epochs[e], "") for e in (1, 2))
    prev = best
    for e, _, st in snap.steps[6:]:
        assert _same(st, best, "joint_encoder.") and _same(st, best, "decoders."), e
        assert not _same(st, prev, "encoders.") and not _same(st, prev, "flows."), e
        assert all(torch.equal(v, best[k]) for k, v in st.items() if k.endswith(".mask")), e
        prev = st
    assert all(p.requires_grad == k.startswith(STAGE_TWO) and (p.grad is None) == (not k.startswith(STAGE_TWO))
               for k, p in trainer.model.named_parameters())
    # the scheduler is made anew at the reset (epoch 3)
    assert [lr for _, lr, _ in snap.steps] == [1e-3] * 3 + [5e-4] * 3 + [1e-3] * 3 + [5e-4] * 3
    # the first stage-two step is a fresh Adam's first step: lr g / (|g| + eps)
    first = snap.steps[6][2]
    moved = torch.cat([(first[k] - best[k]).abs().reshape(-1) for k in first if k.startswith(STAGE_TWO) and not k.endswith(".mask")])
    moved = moved[moved > 0]
    assert moved.numel() > 100
    med = float(moved.double().median())
    print("first stage-two step: median |dp| / lr =", med / 1e-3, "over", moved.numel(), "entries")
    assert abs(med - 1e-3) <= 0.01 * 1e-3, med
    assert set(trainer.optimizer.state_dict()["state"]) == \
        {i for i, (k, _) in enumerate(trainer.model.named_parameters()) if k.startswith(STAGE_TWO)}


def test_resume_from_a_stage_two_checkpoint(tmp_path):
    from multivae_amd.trainers import MultistageTrainer

    t1 = MultistageTrainer(_tiny(), _dataset(), training_config=_trainer_config(tmp_path / "a", num_epochs=3))
    t1.train()
    ckpt = os.path.join(t1.training_dir, "checkpoint_epoch_3")
    saved = torch.load(os.path.join(ckpt, "model.pt"), map_location="cpu")["model_state_dict"]
    opt = torch.load(os.path.join(ckpt, "optimizer.pt"), map_location="cpu")
    names = [k for k, _ in t1.model.named_parameters()]
    assert opt["state"] and all(names[i].startswith(STAGE_TWO) and int(st["step"]) == 3 for i, st in opt["state"].items())
    snap = _snapshots()
    t2 = MultistageTrainer(_tiny(), _dataset(), training_config=_trainer_config(tmp_path / "b", num_epochs=4), callbacks=[snap],
                           checkpoint=ckpt)
    snap.trainer = t2
    hist = t2.train()  # builds the stage-two buffers, then optimizer.load_state_dict: must not raise
    assert len(hist) == 1 and np.isfinite(hist[0]["train_epoch_loss"]) and [e for e, _, _ in snap.steps] == [4] * 3
    assert [id(p) for p in t2.flat.params] == [id(p) for k, p in t2.model.named_parameters() if k.startswith(STAGE_TWO)]
    prev = saved
    for _, lr, st in snap.steps:
        cpu = {k: v.cpu() for k, v in st.items()}
        assert _same(cpu, saved, "joint_encoder.") and _same(cpu, saved, "decoders.")
        assert not _same(cpu, prev, "encoders.") and not _same(cpu, prev, "flows.")
        assert lr == 5e-4
        prev = cpu


def test_zz_report():
    """Prints the head-room the HIP kernels showed in this session: the largest |err| / base per stage, with the case."""
    print("HIP_MEASURED", {k: (round(v, 3), n) for k, (v, n) in sorted(MEASURED.items())})
