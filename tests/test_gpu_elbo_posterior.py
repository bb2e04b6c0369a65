"""The ten posterior entry points of csrc/elbo.hip (mvk_mopoe_posterior_fwd/bwd, mvk_mvtcae_posterior_fwd/bwd,
mvk_mvae_posterior_fwd/bwd, mvk_jmvae_posterior_fwd/bwd, mvk_gauss_sample_kl_fwd/bwd) called directly through the C ABI,
entry-wise against float64.

Reference, case table (elbo_ref.CASES: every case says which edge it is there for) and error model live in tests/elbo_ref.py;
tests/test_elbo_ref_host.py pins that reference to oracle.elbo on the CPU.  Per case:

1. every output array of the forward and the backward launch, pre-filled with NaN, against the float64 reference:
   |got - ref| <= C_STAGE[stage] * base for EVERY entry (the backward kernels recompute the posterior from the inputs and consume
   no forward output, so both references are evaluated on the fp32 inputs); a NaN left anywhere fails;
2. exact properties: the gradients of a missing modality's rows are exactly 0.0 (MVTCAE, MVAE); an MVAE subset with nothing
   present gives kld == 0.0 and z == eps bit for bit; MoPoE's joint_mu / joint_lv are the selected subset's mus_out / lvs_out bit
   for bit; an MVAE sample has the same bits in every member's slab; the NULL and the non-NULL form of every optional pointer
   agree bit for bit on the arrays both write (outputs: with / without mus_out, joint_*, sub_*; inputs: NULL against an array
   of zeros, weights NULL against an array of float32(1 / S));
3. a second launch from the same buffers is bit-identical;
4. test_argument_checks: every MVK_EINVAL branch returns without launching, B = 0 is MVK_OK and writes nothing.

Constants (elbo_ref.C_STAGE = 4x the largest |err| / base of oracle.elbo in plain torch fp32 on the CPU, backward by fp32
autograd, over the case table, rounded up; re-derived by test_elbo_ref_host.py::test_error_constants):
    stage        torch fp32   C     set by
    mopoe.z      1.49         6     mopoe-m2-k1-b260-l130-wide-graded
    mopoe.kld    0.16         1     mopoe-m3-k11-b9-l64-eps-graded
    mopoe.mu     3.74         15    mopoe-m8-k4-b5-l130-dominated-random
    mopoe.lv     2.12         9     mopoe-m5-k1-b260-l5-routed-graded
    mopoe.dmu    5.21         21    mopoe-m5-k1-b260-l5-routed-graded
    mopoe.dlv    3.66         15    mopoe-m3-k11-b9-l64-eps-graded
    mvtcae.z     1.93         8     mvtcae-m8-k4-b5-l130-dominated-random
    mvtcae.jkl   0.23         1     mvtcae-m3-k11-b4-l5-agree-graded
    mvtcae.ckl   0.49         2     mvtcae-m2-k4-b3-l5-wide
    mvtcae.mu    2.93         12    mvtcae-m8-k4-b5-l130-dominated-random
    mvtcae.lv    2.42         10    mvtcae-m2-k1-b260-l130-wide-graded
    mvtcae.dmu   3.13         13    mvtcae-m2-k1-b260-l130-wide-graded
    mvtcae.dlv   2.59         11    mvtcae-m2-k1-b260-l130-wide-graded
    mvae.z       0.54         3     mvae-m2-b260-l130-wide-graded
    mvae.kld     0.22         1     mvae-m5-b3-l5-max
    mvae.mu      0.50         2     mvae-m2-b260-l130-wide-graded
    mvae.lv      0.73         3     mvae-m2-b260-l5-random
    mvae.dmu     0.82         4     mvae-m2-b260-l130-wide-graded
    mvae.dlv     0.91         4     mvae-m2-b260-l130-wide-graded
    jmvae.z      0.72         3     jmvae-m2-k7-b5-l20-null-gljm
    jmvae.kld    0.46         2     jmvae-m2-k4-b260-l5
    jmvae.ljm    0.33         2     jmvae-m2-k4-b260-l5
    jmvae.djmu   2.31         10    jmvae-m2-k1-b260-l130-wide-graded
    jmvae.djlv   2.59         11    jmvae-m2-k1-b260-l130-wide-graded
    jmvae.dmu    1.05         5     jmvae-m2-k1-b260-l130-wide-graded
    jmvae.dlv    2.05         9     jmvae-m2-k1-b260-l130-wide-graded
    gauss.z      0.74         3     gauss-k4-b260-l5
    gauss.kl     0.31         2     gauss-k4-b260-l5
    gauss.dmu    2.25         10    gauss-k4-b260-l5
    gauss.dlv    2.65         11    gauss-k1-b260-l130-wide-graded

Largest |err| / base of the HIP kernels, mutation factors on the kernels' output and the wall time on an MI355X: NOT RECORDED YET.
This file has not run on a GPU: test_zz_report prints HIP_MEASURED (per stage, with the case) and HIP_WORST_PER_FAMILY,
test_tolerance_rejects_mutated_reference prints HIP_TEETH lines; copy them here from the first run.  What stands in for them:
the kernels' own operation order (first-expert initialisation, sequential sums over K and S, dT = dN mu_m + dD,
log(1 / D) then exp, unnormalised MVAE numerator, per-lane trips then a 64-lane tree) written out in torch fp32 on the CPU,
with correctly rounded exp / log, gave over the case table
    mopoe  z 1.49, kld 0.14, mu 3.74, lv 2.12, dmu 5.09, dlv 4.65       mvtcae z 1.93, jkl 0.29, ckl 0.49, mu 2.93, lv 2.42,
    mvae   z 0.58, kld 0.22, mu 0.61, lv 1.00, dmu 1.07, dlv 0.71              dmu 3.43, dlv 2.00
    jmvae  z 0.72, kld 0.35, ljm 0.33, djmu 3.65, djlv 3.94, dmu 1.17, dlv 1.83       gauss z 0.74, kl 0.29, dmu 2.25, dlv 2.25
i.e. at most 0.37 of C (jmvae.djmu); expf / logf at 1-2 ulp come on top on the GPU.
Factor by which each mutation of the reference exceeded the bound on its weakest stage and best case, against torch fp32
(test_elbo_ref_host.py): no_prior_full 3.6e4 (kld), prior_everywhere 3.9e5 (kld), no_eps 1.4e5 (mvtcae.lv), uniform_w 1.0e5
(kld), sel_off 2.6e7 (z), lv0_missing 1.8e6 (lv), mvae_no_prior 6.9e5 (kld), sd_no_half 1.4e4 (mvtcae.dlv), drop_tail 3.6e5
(mopoe.dmu).  Wall time of the reference side of this file on the CPU (every case, with a stand-in launcher): 12 s.

Suspects of the kernel text, each with the regime that exercises it.  Verdicts are from the emulation above until a GPU run
replaces them; elbo.hip is unchanged:
 1. POE_EPS at exp(lv) ~ 1e-8 (eps cases): cleared in emulation, mopoe.dlv 4.65 of C = 15 on mopoe-m8-k7-b4-l64-chosen-eps.
 2. dT = dN * mu[m] + dD in the MoPoE / MVTCAE backward (agree cases): cleared in emulation; oracle.elbo's fp32 autograd forms
    the same difference of products (g mu_m / D - g N / D^2), so the base carries |g_mu| (|mu_m| + |mu_s|) / D.
 3. the five-term MVTCAE conditional KL with one dominating or one present modality (dominated / one cases): cleared in
    emulation, ckl 0.49 of C = 2; the kernel's terms are the oracle's.
 4. MVAE num += expf(-lv) * mu unnormalised against normalised backward weights: cleared in emulation (mu 0.61 of C = 2,
    dlv 0.71 of C = 4); stable_poe forms the same unnormalised sum, and lv >= -80 keeps it finite.
 5. logf(1 / D) followed by expf(lv_s): cleared in emulation; poe returns log(pd_var) and the KL exponentiates it again too.
 6. B = 260 = 65 x 4 fills its last workgroup: the partial last workgroup comes from B in {1, 3, 5, 9} (the tail cases).
"""
import ctypes

import pytest
import torch

import elbo_ref as R

pytestmark = pytest.mark.gpu

MEASURED = {}
_RUNS = {}


def dev():
    return torch.device("cuda:0")


def _lib():
    from multivae_amd import _lib as L

    return L


def to_dev(ts):
    return [None if t is None else t.to(dev()).contiguous() for t in ts]


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev())


def implied_null(case, inp):
    """The optional pointers a case passes as NULL: the named ones and those its inputs leave out."""
    null = set(case.null)
    if case.fam == "mopoe" and inp["weights"] is None:
        null.add("weights")
    if case.fam == "mvae":
        null |= {f"dzm{m}" for m in range(case.M) if inp["dzm"][m] is None}
    return null


def launch(case, inp, null):
    """Forward, then backward, of the case's family from fresh NaN-filled outputs.  `null`: the optional pointers passed as
    NULL; an optional INPUT the case leaves out but `null` does not name is passed as an array of zeros (weights: float32(1 / S)).
    -> every array written, on the CPU, under the keys of elbo_ref.reference (None: not written)."""
    Lb = _lib()
    d = dev()
    fam, M, K, B, L = case.fam, case.M, case.K, case.B, case.L
    sp = Lb.stream_ptr
    mus, lvs = to_dev(inp["mus"]), to_dev(inp["lvs"])
    pm, pl = Lb.ptr_array(mus), Lb.ptr_array(lvs)
    eps = inp["eps"].to(d).contiguous()
    masks = None if inp["masks"] is None else [m.to(torch.uint8).to(d).contiguous() for m in inp["masks"]]
    marr = None if masks is None else Lb.ptr_array(masks)
    dmu, dlv = [nan(B, L) for _ in range(M)], [nan(B, L) for _ in range(M)]

    def opt(name, t, shape, fill=0.0):
        if name in null:
            return None
        return torch.full(shape, fill, dtype=torch.float32, device=d) if t is None else t.to(d).contiguous()

    if fam == "mopoe":
        S = len(inp["bits"])
        bits = torch.tensor(inp["bits"], dtype=torch.int32, device=d)
        sel = inp["sel"].to(torch.int32).to(d).contiguous()
        w = opt("weights", inp["weights"], (S, B), 1.0 / S)
        z, kld = nan(K, B, L), nan(B)
        mo, lo = (None, None) if "mus_out" in null else (nan(S, B, L), nan(S, B, L))
        jm, jl = (None, None) if "joint" in null else (nan(B, L), nan(B, L))
        Lb.call("mvk_mopoe_posterior_fwd", pm, pl, M, Lb.ptr(bits), S, Lb.ptr(sel), Lb.ptr(w), Lb.ptr(eps), K, B, L, Lb.ptr(z),
                Lb.ptr(kld), Lb.ptr(mo), Lb.ptr(lo), Lb.ptr(jm), Lb.ptr(jl), sp())
        dz, gk = inp["dz"].to(d).contiguous(), opt("gkld", inp["gk"], (B,))
        Lb.call("mvk_mopoe_posterior_bwd", pm, pl, M, Lb.ptr(bits), S, Lb.ptr(sel), Lb.ptr(w), Lb.ptr(eps), Lb.ptr(dz), K, B, L,
                Lb.ptr(gk), Lb.ptr_array(dmu), Lb.ptr_array(dlv), sp())
        out = dict(z=z, kld=kld, mus_out=mo, lvs_out=lo, joint_mu=jm, joint_lv=jl)
    elif fam == "mvtcae":
        z, jkl, ckl = nan(K, B, L), nan(B), nan(M, B)
        jm, jl = (None, None) if "joint" in null else (nan(B, L), nan(B, L))
        Lb.call("mvk_mvtcae_posterior_fwd", pm, pl, marr, M, Lb.ptr(eps), K, B, L, Lb.ptr(z), Lb.ptr(jkl), Lb.ptr(ckl), Lb.ptr(jm),
                Lb.ptr(jl), sp())
        dz, gj, gc = inp["dz"].to(d).contiguous(), opt("gjoint", inp["gj"], (B,)), opt("gcond", inp["gc"], (M, B))
        Lb.call("mvk_mvtcae_posterior_bwd", pm, pl, marr, M, Lb.ptr(eps), Lb.ptr(dz), K, B, L, Lb.ptr(gj), Lb.ptr(gc),
                Lb.ptr_array(dmu), Lb.ptr_array(dlv), sp())
        out = dict(z=z, jkl=jkl, ckl=ckl, joint_mu=jm, joint_lv=jl)
    elif fam == "mvae":
        S = len(inp["bits"])
        bits = (ctypes.c_int32 * S)(*inp["bits"])
        cnt = [sum((b >> m) & 1 for b in inp["bits"]) for m in range(M)]
        zm = [nan(cnt[m], B, L) if cnt[m] else None for m in range(M)]
        kld = nan(S, B)
        sm, sl = (None, None) if "sub" in null else (nan(S, B, L), nan(S, B, L))
        Lb.call("mvk_mvae_posterior_fwd", pm, pl, marr, M, bits, S, Lb.ptr(eps), B, L, Lb.ptr_array(zm), Lb.ptr(kld), Lb.ptr(sm),
                Lb.ptr(sl), sp())
        dzm = [opt(f"dzm{m}", inp["dzm"][m], (cnt[m], B, L)) if cnt[m] else None for m in range(M)]
        gk = opt("gkld", inp["gk"], (S, B))
        Lb.call("mvk_mvae_posterior_bwd", pm, pl, marr, M, bits, S, Lb.ptr(eps), Lb.ptr_array(dzm), B, L, Lb.ptr(gk),
                Lb.ptr_array(dmu), Lb.ptr_array(dlv), sp())
        out = dict(zm=zm, kld=kld, sub_mu=sm, sub_lv=sl)
    elif fam == "jmvae":
        jmu, jlv = inp["jmu"].to(d).contiguous(), inp["jlv"].to(d).contiguous()
        z, kld, ljm = nan(K, B, L), nan(B), nan(B)
        Lb.call("mvk_jmvae_posterior_fwd", Lb.ptr(jmu), Lb.ptr(jlv), pm, pl, M, Lb.ptr(eps), K, B, L, Lb.ptr(z), Lb.ptr(kld),
                Lb.ptr(ljm), sp())
        dz, gk, gl = opt("dz", inp["dz"], (K, B, L)), opt("gkld", inp["gk"], (B,)), opt("gljm", inp["gl"], (B,))
        djmu, djlv = nan(B, L), nan(B, L)
        Lb.call("mvk_jmvae_posterior_bwd", Lb.ptr(jmu), Lb.ptr(jlv), pm, pl, M, Lb.ptr(eps), Lb.ptr(dz), K, B, L, Lb.ptr(gk),
                Lb.ptr(gl), Lb.ptr(djmu), Lb.ptr(djlv), Lb.ptr_array(dmu), Lb.ptr_array(dlv), sp())
        out = dict(z=z, kld=kld, ljm=ljm, djmu=djmu, djlv=djlv)
    else:
        w, kl = nan(K, B, L), nan(B)
        Lb.call("mvk_gauss_sample_kl_fwd", Lb.ptr(mus[0]), Lb.ptr(lvs[0]), Lb.ptr(eps), K, B, L, Lb.ptr(w), Lb.ptr(kl), sp())
        dw, gk = opt("dw", inp["dz"], (K, B, L)), opt("gkl", inp["gk"], (B,))
        Lb.call("mvk_gauss_sample_kl_bwd", Lb.ptr(mus[0]), Lb.ptr(lvs[0]), Lb.ptr(eps), Lb.ptr(dw), Lb.ptr(gk), K, B, L,
                Lb.ptr(dmu[0]), Lb.ptr(dlv[0]), sp())
        out = dict(w=w, kl=kl)
    out.update(dmu=dmu, dlv=dlv)
    torch.cuda.synchronize()
    return {k: (None if v is None else [None if t is None else t.cpu() for t in v] if isinstance(v, list) else v.cpu())
            for k, v in out.items()}


def arrays(got):
    for k, v in got.items():
        for i, t in enumerate(v if isinstance(v, list) else [v]):
            if t is not None:
                yield f"{k}[{i}]", t


def differing(a, b):
    """The first array that both hold and that differs in its bits (None: none)."""
    other = dict(arrays(b))
    for k, x in arrays(a):
        if k in other and not torch.equal(x.view(torch.int32), other[k].view(torch.int32)):
            return k
    return None


def run_case(case):
    """(inputs, first launch, second launch, reference, bases) of a case: launched once per session, shared, left unchanged."""
    if case.name not in _RUNS:
        inp = R.make_inputs(case)
        null = implied_null(case, inp)
        _RUNS[case.name] = (inp, launch(case, inp, null), launch(case, inp, null), R.reference(case, inp), R.bases(case, inp))
    return _RUNS[case.name]


OUTPUT_PAIRS = dict(mopoe=("mus_out", "joint"), mvtcae=("joint",), mvae=("sub",), jmvae=(), gauss=())


@pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
def test_case(case):
    inp, got, got2, ref, base = run_case(case)
    fam, M, B = case.fam, case.M, case.B
    # 3. determinism
    assert differing(got, got2) is None and differing(got2, got) is None
    # 1. every entry of every array; nothing left unwritten
    for k, t in arrays(got):
        assert not bool(torch.isnan(t).any()), f"{case.name}: {k} holds a NaN: an entry the kernel did not write"
    ratios = R.ratios(case, inp, got, ref=ref, base=base)
    print(case.name, {k: round(v, 3) for k, (v, _) in ratios.items()})
    for k, (v, arr) in ratios.items():
        if v > MEASURED.get(k, (-1.0, ""))[0]:
            MEASURED[k] = (v, case.name)
    for k, (v, arr) in ratios.items():
        assert v <= R.C_STAGE[k], f"{case.name}: {k} ({arr}) worst |err| / base = {v:.3g} > C = {R.C_STAGE[k]}"
    # 2. exact properties
    if inp["masks"] is not None and fam in ("mvtcae", "mvae"):
        for m in range(M):
            gone = ~inp["masks"][m]
            assert bool((got["dmu"][m][gone] == 0).all()) and bool((got["dlv"][m][gone] == 0).all()), \
                f"modality {m}: gradient on its missing rows"
    if fam == "mopoe" and got["mus_out"] is not None and got["joint_mu"] is not None:
        sel, rows = inp["sel"].long(), torch.arange(B)
        assert torch.equal(got["joint_mu"].view(torch.int32), got["mus_out"][sel, rows].view(torch.int32))
        assert torch.equal(got["joint_lv"].view(torch.int32), got["lvs_out"][sel, rows].view(torch.int32))
    if fam == "mvae":
        slot = [0] * M
        for s, bt in enumerate(inp["bits"]):
            members = [m for m in range(M) if (bt >> m) & 1]
            zs = [got["zm"][m][slot[m]] for m in members]
            for m in members:
                slot[m] += 1
            assert all(torch.equal(zs[0].view(torch.int32), z.view(torch.int32)) for z in zs[1:]), f"subset {s}: slabs differ"
            if inp["masks"] is not None:
                gone = ~torch.stack([inp["masks"][m] for m in members]).any(0)
                assert bool((got["kld"][s][gone] == 0).all()), f"subset {s}: KL of rows with nothing present"
                assert torch.equal(zs[0][gone].view(torch.int32), inp["eps"][s][gone].view(torch.int32)), f"subset {s}: z != eps"
    # the NULL and the non-NULL form of every optional pointer
    null = implied_null(case, inp)
    for name in OUTPUT_PAIRS[fam]:
        alt = launch(case, inp, null ^ {name})
        k = differing(got, alt)
        assert k is None, f"{case.name}: {k} changes with {name} {'given' if name in null else 'NULL'}"
    for name in sorted(null - set(OUTPUT_PAIRS[fam])):
        alt = launch(case, inp, null - {name})
        k = differing(got, alt) or differing(alt, got)
        assert k is None, f"{case.name}: {k} differs between {name} NULL and {name} = zeros / 1 / S"


@pytest.mark.parametrize("mut,stages,names", R.TEETH, ids=[t[0] for t in R.TEETH])
def test_tolerance_rejects_mutated_reference(mut, stages, names):
    """The comparison of test_case, with one deliberate mistake in the REFERENCE, must fail on the HIP kernels' output in every
    stage named for it on at least one of its cases (the same is shown against torch fp32 in test_elbo_ref_host.py)."""
    best = {s: 0.0 for s in stages}
    for name in names:
        case = R.CASE_BY_NAME[name]
        inp, got, _, _, base = run_case(case)
        bad = R.ratios(case, inp, got, mut=(mut,), base=base)
        for s in stages:
            if s in bad:
                f = bad[s][0] / R.C_STAGE[s]
                print("HIP_TEETH", mut, name, s, f"{f:.3g}")
                best[s] = max(best[s], f)
    for s, f in best.items():
        assert f > 1.0, f"{mut} passes {s} on all of {names}: at most {f:.3g}x the bound"


# ---- argument checks -----------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    """MVK_EINVAL, without a launch (the sentinel-filled outputs stay as they are), for: M = 0; M = 9; K = 0; L = 0; B < 0; a
    NULL member of mu[]; mus_out without lvs_out, joint_mu without joint_lv, sub_mu without sub_lv (and the reverse); S = 0; MVAE
    subset bits outside the modality set, an empty MVAE subset, S above MVK_MVAE_MAX_SUBSETS.  B = 0 is MVK_OK and writes nothing."""
    Lb = _lib()
    d = dev()
    sp = Lb.stream_ptr
    t = torch.full((4096,), 7.0, device=d)
    ints = torch.tensor([3, 1, 0, 0, 0, 0, 0, 0], dtype=torch.int32, device=d)  # subset_masks [2] / sel [<= 8]: all in range
    p, pi = Lb.ptr(t), Lb.ptr(ints)

    def arr(n, hole=None):
        a = Lb.ptr_array([t] * n)
        if hole is not None:
            a[hole] = None
        return a

    def hbits(bits):
        return (ctypes.c_int32 * len(bits))(*bits)

    def mopoe_f(M=2, S=2, K=2, B=3, L=5, hole=None, mo=True, lo=True, jm=True, jl=True):
        n = max(M, 1)
        Lb.call("mvk_mopoe_posterior_fwd", arr(n, hole), arr(n), M, pi, S, pi, None, p, K, B, L, p, p, p if mo else None,
                p if lo else None, p if jm else None, p if jl else None, sp())

    def mopoe_b(M=2, S=2, K=2, B=3, L=5, hole=None):
        n = max(M, 1)
        Lb.call("mvk_mopoe_posterior_bwd", arr(n), arr(n, hole), M, pi, S, pi, None, p, p, K, B, L, None, arr(n), arr(n), sp())

    def mvtcae_f(M=2, K=2, B=3, L=5, hole=None, jm=True, jl=True):
        n = max(M, 1)
        Lb.call("mvk_mvtcae_posterior_fwd", arr(n, hole), arr(n), None, M, p, K, B, L, p, p, p, p if jm else None,
                p if jl else None, sp())

    def mvtcae_b(M=2, K=2, B=3, L=5, hole=None):
        n = max(M, 1)
        Lb.call("mvk_mvtcae_posterior_bwd", arr(n), arr(n), None, M, p, p, K, B, L, None, None, arr(n, hole), arr(n), sp())

    def mvae_f(M=2, bits=(3, 1), S=None, B=3, L=5, hole=None, sm=True, sl=True):
        n = max(M, 1)
        Lb.call("mvk_mvae_posterior_fwd", arr(n, hole), arr(n), None, M, hbits(bits), len(bits) if S is None else S, p, B, L,
                arr(n), p, p if sm else None, p if sl else None, sp())

    def mvae_b(M=2, bits=(3, 1), S=None, B=3, L=5, hole=None):
        n = max(M, 1)
        Lb.call("mvk_mvae_posterior_bwd", arr(n), arr(n, hole), None, M, hbits(bits), len(bits) if S is None else S, p, arr(n), B,
                L, None, arr(n), arr(n), sp())

    def jmvae_f(M=2, K=2, B=3, L=5, hole=None):
        n = max(M, 1)
        Lb.call("mvk_jmvae_posterior_fwd", p, p, arr(n, hole), arr(n), M, p, K, B, L, p, p, p, sp())

    def jmvae_b(M=2, K=2, B=3, L=5, hole=None):
        n = max(M, 1)
        Lb.call("mvk_jmvae_posterior_bwd", p, p, arr(n), arr(n), M, p, None, K, B, L, None, None, p, p, arr(n), arr(n, hole), sp())

    def gauss_f(K=2, B=3, L=5):
        Lb.call("mvk_gauss_sample_kl_fwd", p, p, p, K, B, L, p, p, sp())

    def gauss_b(K=2, B=3, L=5):
        Lb.call("mvk_gauss_sample_kl_bwd", p, p, p, None, None, K, B, L, p, p, sp())

    multi = [mopoe_f, mopoe_b, mvtcae_f, mvtcae_b, mvae_f, mvae_b, jmvae_f, jmvae_b]
    with_k = [mopoe_f, mopoe_b, mvtcae_f, mvtcae_b, jmvae_f, jmvae_b, gauss_f, gauss_b]
    bad = []
    for f in multi:
        bad += [lambda f=f: f(M=0), lambda f=f: f(M=9), lambda f=f: f(hole=1)]
    for f in with_k:
        bad.append(lambda f=f: f(K=0))
    for f in multi + [gauss_f, gauss_b]:
        bad += [lambda f=f: f(L=0), lambda f=f: f(B=-1)]
    bad += [lambda: mopoe_f(mo=False), lambda: mopoe_f(lo=False), lambda: mopoe_f(jm=False), lambda: mopoe_f(jl=False),
            lambda: mopoe_f(S=0), lambda: mopoe_b(S=0), lambda: mvtcae_f(jm=False), lambda: mvtcae_f(jl=False),
            lambda: mvae_f(sm=False), lambda: mvae_f(sl=False)]
    for f in (mvae_f, mvae_b):
        bad += [lambda f=f: f(bits=(3, 4)), lambda f=f: f(bits=(3, 0)), lambda f=f: f(bits=(3,) * 33), lambda f=f: f(S=0),
                lambda f=f: f(bits=(3, 256))]
    for i, f in enumerate(bad):
        with pytest.raises(Lb.MvkError):
            f()
            pytest.fail(f"bad call {i} was accepted")
    for f in multi + [gauss_f, gauss_b]:  # zero rows: OK, nothing written
        f(B=0)
    mvae_f(bits=(3,) * 32, B=0)  # S = MVK_MVAE_MAX_SUBSETS itself is accepted
    torch.cuda.synchronize()
    assert bool((t == 7.0).all())


def test_zz_report():
    """Prints the head-room the HIP kernels showed in this session: the largest |err| / base per stage and per family."""
    print("HIP_MEASURED", {k: (round(v, 2), n) for k, (v, n) in sorted(MEASURED.items())})
    fam = {}
    for k, (v, n) in MEASURED.items():
        f = k.split(".")[0]
        if v / R.C_STAGE[k] > fam.get(f, (-1.0,))[0]:
            fam[f] = (v / R.C_STAGE[k], k, round(v, 2), n)
    print("HIP_WORST_PER_FAMILY (fraction of C, stage, |err| / base, case)", fam)
