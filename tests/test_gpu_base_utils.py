"""The public helper kernels of csrc/utils.hip (mvk_poe_fwd/bwd in both modes, mvk_kl_gauss_fwd/bwd, mvk_logprob_fwd/bwd) called
directly through the C ABI, entry-wise against float64, and models.base.base_utils.kl_divergence once at the wrapper level.

Reference, case table (base_utils_ref.CASES) and error model live in tests/base_utils_ref.py; tests/test_base_utils_ref_host.py
pins that reference to oracle.elbo on the CPU and runs `check_case` below on every case with a stand-in launcher (the fp32
oracle).  Per case:

1. every output, allocated with NaN prefill and 64 sentinel floats before and after, against the float64 reference:
   |got - ref| <= C_STAGE[stage] * base for EVERY entry; a NaN left anywhere fails; the sentinels are untouched;
2. exact properties: stable PoE of one expert returns the expert (and gmu / glv) bit for bit; an expert with lv = +inf gets
   exactly zero gradient; gmu / glv NULL against arrays of zeros agree bit for bit; every optional output of mvk_kl_gauss_bwd
   NULL against given leaves the other three bit-identical; a Laplace tie has gradient exactly 0;
3. a second launch is bit-identical;
4. test_kl_divergence_wrapper: operands [K,B,L], [B,L], [1,L] and a scalar through base_utils.kl_divergence, all four
   gradients against float64 autograd (the column-sum path of _KLFn.backward);
5. test_argument_checks: mvk_kl_gauss_bwd rejects an operand count below 1 as mvk_kl_gauss_fwd does (the kernel indexes
   i % n with it), and launches nothing.

Constants (base_utils_ref.C_STAGE = 4x the largest |err| / base of oracle.elbo in plain torch fp32 on the CPU, backward by fp32
autograd, over the case table, rounded up; re-derived by test_base_utils_ref_host.py::test_error_constants), and the largest
|err| / base of the HIP kernels on an MI355X (test_zz_report):
    stage                     torch fp32  C   set by                                     HIP    set by
    poe.mu                    0.28        2   poe-e3-n1300-wide-nogmu                    0.28   poe-e3-n1300-wide-nogmu
    poe.lv                    0.40        2   poe-e8-n257-benign-noglv                   0.67   poe-e3-n256-eps
    poe.dmu                   0.44        2   poe-e8-n257-benign-noglv                   0.93   poe-e3-n256-eps
    poe.dlv                   0.48        2   poe-e8-n257-benign-noglv                   1.37   poe-e2-n255-wide
    spoe.mu                   0.45        2   spoe-e2-n255-wide                          0.45   spoe-e8-n257-benign-noglv
    spoe.lv                   0.39        2   spoe-e8-n257-benign-noglv                  0.58   spoe-e8-n257-benign-noglv
    spoe.dmu                  0.61        3   spoe-e8-n257-benign-noglv                  0.37   spoe-e8-n257-benign-noglv
    spoe.dlv                  0.79        4   spoe-e8-n257-benign-noglv                  0.38   spoe-e8-n257-benign-noglv
    kl.fwd                    0.60        3   kl-k3-b85-l1-one-full-bl-l                 0.60   kl-k3-b85-l1-one-full-bl-l
    kl.dmean                  0.72        3   kl-k3-b85-l130-one-full-bl-l               0.88   kl-k1-b257-l130-bl-l-one-full
    kl.dlv                    0.54        3   kl-k1-b257-l130-bl-l-one-full              0.70   kl-k3-b85-l130-l-one-full-bl
    kl.dpmean                 0.72        3   kl-k3-b85-l130-one-full-bl-l               0.88   kl-k1-b257-l130-bl-l-one-full
    kl.dplv                   0.88        4   kl-k1-b257-l130-bl-l-one-full              0.86   kl-k3-b85-l130-l-one-full-bl
    logprob.normal.fwd        0.75        3   logprob-normal1-k4-nx325                   0.75   logprob-normal1-k4-nx325
    logprob.normal.bwd        1.33        6   logprob-normal0.75-k4-nx325                1.14   logprob-normal0.75-k4-nx325
    logprob.laplace.fwd       0.65        3   logprob-laplace0.75-k1-nx1300              0.65   logprob-laplace0.75-k1-nx1300
    logprob.laplace.bwd       0.67        3   logprob-laplace0.75-k1-nx1300              1.33   logprob-laplace0.75-k1-nx1300
    logprob.bernoulli.fwd     0.92        4   logprob-bernoulli1-k4-nx325                0.90   logprob-bernoulli1-k1-nx255
    logprob.bernoulli.bwd     0.97        4   logprob-bernoulli1-k4-nx325                0.99   logprob-bernoulli1-k1-nx1300
    logprob.categorical.fwd   0.55        3   logprob-categorical-c130-k3-rows3          0.51   logprob-categorical-c130-k3-rows3
    logprob.categorical.bwd   0.78        4   logprob-categorical-c65-k1-rows5           0.78   logprob-categorical-c65-k1-rows5
i.e. at most 0.69 of C (poe.dlv: the weights recomputed through a logarithm, suspect 1).  The wrapper-level gradients came out
at 0.17 (mean), 0.15 (log_var), 0.07 (prior_mean) and 0.01 (prior_log_var) of their bounds.  Wall time of this file on an
MI355X: 1.5 s for the 56 tests, 1.0 s of it the first use of the wrapper (3.7 s with start-up and collection); on the CPU with the
stand-in launcher (tests/test_base_utils_ref_host.py, 117 tests): 4 s.
Factor by which each mutation of the reference exceeded the bound on its weakest stage and best case, against torch fp32
(test_base_utils_ref_host.py): no_eps 7.7e4 (poe.mu), mean_not_poe 9.0e6, dlnT_no_eps 4.7e5, kl_no_half 7.3e5 (kl.fwd),
kl_wrap_rows 9.1e6 (kl.fwd), kl_dplv_no_sq 7.0e5, target_no_wrap 1.1e6, laplace_half 4.7e6, xent_no_gx 4.4e4.

Suspects of the kernel text, each with the case that exercises it:
 1. poe_bwd_kernel recomputes the weights as exp(-log(exp(l) + eps) - m) / s instead of T / sum T: the argument-rounding terms
    of the base (Fe) carry it; eps and wide cases.
 2. poe_fwd_kernel mode 1 forms acc = sum exp(-lv_e) mu_e unnormalised (overflow below lv = -88: the cases keep lv >= -80).
 3. `w == 0.f ? 0.f : v` for +inf experts: (gm (mu_e - mu) - gl) * 0 * -1 would be -0 or NaN for infinite operands (inf cases).
 4. the modulo-indexed broadcast of the KL kernels with counts rows * L, B * L, L and 1 on each operand (rotated sizes).
 5. kl_bwd_kernel's grid is blocks_for(rows * L): 130 workgroups at rows = 255, L = 130; g[i / L] per row.
 6. xent_kernel: rows % 4 != 0 leaves waves idle in the last block (rows 1, 3, 5, 9); C = 65 and 130 take two and three
    trips; target rows wrap by row % xrows.
 7. logprob_bwd_kernel's Bernoulli 1 / (1 + expf(-a)) at a = -90: expf overflows to +inf, 1 / inf = 0 (bernoulli cases).
Verdict of the first run on an MI355X: all seven cleared; every stage is inside its bound on every case, no sentinel was
touched and no NaN was left.  The one change to csrc/utils.hip is the argument check: mvk_kl_gauss_bwd now rejects an operand
count below 1 as the forward does (test_argument_checks).
"""
import time

import pytest
import torch

import base_utils_ref as R
from test_gpu_recon_nll import EINVAL, Guarded, _lib, dev, same_bits

pytestmark = pytest.mark.gpu

MEASURED = {}
_T0 = time.time()
KL_OUTS = ("dmean", "dlv", "dpmean", "dplv")


def hip_launch(case, inp, null=frozenset()):
    """Forward, then backward, of the case's family from fresh NaN-filled guarded outputs.  `null`: the optional pointers passed
    as NULL; an optional INPUT the case leaves out (gmu, glv) but `null` does not name is passed as an array of zeros."""
    Lb = _lib()
    sp, d = Lb.stream_ptr, dev()
    if case.fam in ("poe", "spoe"):
        E, n, mode = case.E, case.n, int(case.fam == "spoe")
        eps = R.EPS32 if mode == 0 else 0.0
        mus, lvs = Guarded(E * n, src=inp["mu"]), Guarded(E * n, src=inp["lv"])
        out = dict(mu=Guarded(n), lv=Guarded(n), dmu=Guarded(E * n), dlv=Guarded(E * n))
        Lb.call("mvk_poe_fwd", Lb.ptr(mus.body), Lb.ptr(lvs.body), E, n, eps, mode, Lb.ptr(out["mu"].body), Lb.ptr(out["lv"].body), sp())
        g = {}
        for k in ("gmu", "glv"):
            g[k] = None if k in null else (torch.zeros(n, device=d) if inp[k] is None else inp[k].to(d).contiguous())
        Lb.call("mvk_poe_bwd", Lb.ptr(mus.body), Lb.ptr(lvs.body), E, n, eps, mode, Lb.ptr(g["gmu"]), Lb.ptr(g["glv"]),
                Lb.ptr(out["dmu"].body), Lb.ptr(out["dlv"].body), sp())
        shapes = dict(mu=(n,), lv=(n,), dmu=(E, n), dlv=(E, n))
        guards = [mus, lvs]
    elif case.fam == "kl":
        rows, L = case.K * case.B, case.L
        ops = [Guarded(t.numel(), src=t) for t in inp["ops"]]
        g = inp["g"].to(d).contiguous()
        out = dict(fwd=Guarded(rows))
        out.update({k: Guarded(rows * L) for k in KL_OUTS if k not in null})
        cnt = [a for o in ops for a in (Lb.ptr(o.body), o.n)]
        Lb.call("mvk_kl_gauss_fwd", *cnt, rows, L, Lb.ptr(out["fwd"].body), sp())
        Lb.call("mvk_kl_gauss_bwd", *cnt, rows, L, Lb.ptr(g), *[Lb.ptr(out[k].body) if k in out else None for k in KL_OUTS], sp())
        shapes = dict(fwd=(rows,), **{k: (case.K, case.B, L) for k in KL_OUTS})
        guards = ops
    else:
        K, nx, C = case.K, case.nx, case.C
        n = K * nx
        r, x = Guarded(n, src=inp["r"]), Guarded(nx, src=inp["x"])
        g = inp["g"].to(d).contiguous()
        out = dict(fwd=Guarded(n), bwd=Guarded(n))
        a = (Lb.ptr(r.body), Lb.ptr(x.body), n, nx, Lb.DIST[case.dist], case.scale, C, R.XENT_EPS)
        Lb.call("mvk_logprob_fwd", *a, Lb.ptr(out["fwd"].body), sp())
        Lb.call("mvk_logprob_bwd", *a, Lb.ptr(g), Lb.ptr(out["bwd"].body), sp())
        shapes = dict(fwd=(K, nx), bwd=(K, nx))
        guards = [r, x]
    torch.cuda.synchronize()
    res = {k: v.cpu(*shapes[k]) for k, v in out.items()}
    res["guards"] = all(v.intact() for v in list(out.values()) + guards)
    return res


# ---- the comparison routine (also run on the CPU by tests/test_base_utils_ref_host.py with a stand-in launcher) --------------------------
def check_case(case, launch, measured=None):
    inp = R.make_inputs(case)
    null = frozenset(case.null)
    got = launch(case, inp, null)
    ref, base = R.reference(case, inp), R.bases(case, inp)
    assert got.pop("guards"), f"{case.name}: a sentinel next to a buffer was overwritten"
    assert set(got) == set(ref)
    for k, t in got.items():
        assert not bool(torch.isnan(t).any()), f"{case.name}: {k} holds a NaN: an entry the kernel did not write"
    ratios = R.ratios(case, got, ref, base)
    print(case.name, {k: round(v, 3) for k, v in ratios.items()})
    for k, v in ratios.items():
        if measured is not None and v > measured.get(k, (-1.0, ""))[0]:
            measured[k] = (v, case.name)
    for k, v in ratios.items():
        assert v <= R.C_STAGE[k], f"{case.name}: {k} worst |err| / base = {v:.3g} > C = {R.C_STAGE[k]}"
    # exact properties
    if case.fam == "spoe" and case.E == 1:
        assert same_bits(got["mu"], inp["mu"][0]) and same_bits(got["lv"], inp["lv"][0]), "a single expert is returned as is"
        assert same_bits(got["dmu"][0], inp["gmu"]) and same_bits(got["dlv"][0], inp["glv"])
    if case.fam == "spoe" and case.regime == "inf":
        gone = torch.isinf(inp["lv"])
        assert bool(gone.any()) and bool((got["dmu"][gone] == 0).all()) and bool((got["dlv"][gone] == 0).all()), \
            f"{case.name}: gradient on an expert with lv = +inf"
    if case.fam == "logprob" and case.dist == "laplace":
        tie = inp["r"] == inp["x"].unsqueeze(0)
        assert bool(tie.any()) and bool((got["bwd"][tie] == 0).all())
    for name in sorted(null):  # gmu / glv: NULL against zeros
        alt = launch(case, inp, null - {name})
        assert alt.pop("guards") and all(same_bits(got[k], alt[k]) for k in got), f"{case.name}: {name} NULL differs from zeros"
    if case.fam == "kl":
        for name in KL_OUTS:
            alt = launch(case, inp, frozenset({name}))
            assert alt.pop("guards") and set(alt) == set(got) - {name}
            assert all(same_bits(got[k], alt[k]) for k in alt), f"{case.name}: an output changes with {name} NULL"
    again = launch(case, inp, null)
    assert again.pop("guards") and all(same_bits(got[k], again[k]) for k in got), f"{case.name}: a second launch differs"
    return ratios


@pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
def test_case(case):
    check_case(case, hip_launch, MEASURED)


def test_kl_divergence_wrapper():
    """models.base.base_utils.kl_divergence with operands [K,B,L], [B,L], [1,L] and a scalar: the value and all four gradients
    against float64 autograd.  A broadcast operand's gradient is the ordered column sum (mvk_colsum_acc) of the full-shape
    partials over n = rows * L / numel rows, so its bound is the sum of the partials' bounds C base plus the accumulation term
    (ceil(log2 n) + 1) u sum|partial| of a sum of n addends; every term is computed in float64 from the inputs."""
    from multivae_amd.models.base import base_utils as BU

    K, B, L = 3, 85, 5
    case = R.Case("wrapper", "kl", K=K, B=B, L=L, sizes=("full", "bl", "l", "one"))
    inp = R.make_inputs(case)
    ops = [inp["ops"][0], inp["ops"][1], inp["ops"][2].reshape(1, L), inp["ops"][3].reshape(())]
    ref, base = R.reference(case, inp), R.bases(case, inp)
    dops = [t.to(dev()).clone().requires_grad_() for t in ops]
    kl = BU.kl_divergence(*dops)
    assert kl.shape == (K, B)
    (kl * inp["g"].to(dev()).reshape(K, B)).sum().backward()
    assert R.worst_ratio(kl.detach().cpu().reshape(-1), ref["fwd"], base["fwd"]) <= R.C_STAGE["kl.fwd"]
    for t, key, dims in zip(dops, KL_OUTS, ((), (0,), (0, 1), (0, 1, 2))):
        full, fb = ref[key], R.C_STAGE["kl." + key] * base[key]
        if dims:
            n = full.numel() // t.numel()
            fb = fb.expand_as(full).sum(dims) + R.acc(n) * R.U * full.abs().sum(dims)
            full = full.sum(dims)
        r = R.worst_ratio(t.grad.cpu().reshape(-1), full.reshape(-1), fb.expand_as(full).reshape(-1))
        print("wrapper", key, round(r, 3))
        assert r <= 1.0, f"{key}: {r:.3g} x its bound"


def test_argument_checks():
    """mvk_kl_gauss_fwd and mvk_kl_gauss_bwd return MVK_EINVAL for an operand count below 1 (the kernels compute i % n with it), for
    L = 0 and for a NULL operand, and launch nothing: the NaN-filled outputs stay as they are.  rows = 0 is MVK_OK."""
    Lb = _lib()
    lib, sp = Lb.load(), Lb.stream_ptr
    rows, L = 3, 5
    src = Guarded(rows * L, fill=0.25)
    outs = [Guarded(rows * L) for _ in range(4)]
    p, g = Lb.ptr(src.body), Lb.ptr(src.body)

    def fwd(counts=(15, 15, 15, 15), rows=rows, L=L, hole=None):
        a = [x for j, c in enumerate(counts) for x in (None if hole == j else p, c)]
        return lib.mvk_kl_gauss_fwd(*a, rows, L, Lb.ptr(outs[0].body), sp())

    def bwd(counts=(15, 15, 15, 15), rows=rows, L=L, hole=None):
        a = [x for j, c in enumerate(counts) for x in (None if hole == j else p, c)]
        return lib.mvk_kl_gauss_bwd(*a, rows, L, g, *[Lb.ptr(o.body) for o in outs], sp())

    for f in (fwd, bwd):
        for j in range(4):
            for bad in (0, -1):
                counts = [15, 15, 15, 15]
                counts[j] = bad
                assert f(counts=tuple(counts)) == EINVAL, f"{f.__name__}: count {bad} of operand {j} was accepted"
            assert f(hole=j) == EINVAL
        assert f(L=0) == EINVAL and f(rows=-1) == EINVAL
        assert f(rows=0) == 0
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o.body).all()) and o.intact() for o in outs) and src.intact()


def test_zz_report():
    """Prints the head-room the HIP kernels showed in this session (the largest |err| / base per stage, with the case) and the
    wall time of this file."""
    print("HIP_MEASURED", {k: (round(v, 2), n) for k, (v, n) in sorted(MEASURED.items())})
    print(f"WALL test_gpu_base_utils.py {time.time() - _T0:.1f} s")
