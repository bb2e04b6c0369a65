"""The importance-sampling entries of csrc/mmvae.hip (mvk_iwae_sample, mvk_iwae_logw, mvk_iwae_reduce: the kernels under every
compute_joint_nll of the package) called directly through the C ABI, entry by entry against float64.

References, case tables (CASES: chains sample -> logw -> reduce; REDUCE_CASES: the reduction alone), error model and mutations live
in tests/iwae_ref.py; tests/test_iwae_ref_host.py pins them on the CPU and runs the `check_*` routines below with a stand-in
backend (the same formulas in plain torch fp32).  Per case:

1. every output (z, lw, ll) is allocated with NaN prefill and 64 sentinel floats before and after; |got - ref| <= C_STAGE[stage] *
   U * base + SUB for EVERY entry; an entry whose reference is not finite must be in the same non-finite class, and a NaN anywhere
   else fails; no sentinel is touched;
2. lw is checked against the reference on the z the sample entry wrote and ll on the lw the logw entry wrote, and lw once more
   from the inputs (`lw.e2e`);
3. exact properties: z == loc where the noise is 0; family 2 (NORMAL_SOFTPLUS) gives the bits of family 0 in all three entries;
   the NaN of a NaN expert density is on row 1 alone; all experts at -inf give lw = +inf and ll = +inf; a column of -inf gives
   ll = -inf; a +inf entry gives +inf; a NaN entry gives NaN, also when the rest of the column is -inf;
4. a second launch is bit-identical;
5. test_argument_checks: every MVK_EINVAL branch of the three entries, which launch nothing;
6. test_tolerance_rejects_mutated_reference: the HIP output against each wrong reference of TEETH leaves the bound.

Constants (iwae_ref.C_STAGE): 4x the largest |err| / (U base) of the plain-torch-fp32 stand-in on the CPU, rounded up, or derived
(d); next to them the largest |err| / (U base) of the HIP kernels on an MI355X (test_zz_report):
    stage     torch fp32  C      set by                     HIP     set by
    z         1.73        7      iw-laplace-k3-b4-l130-e3-r1-sd    1.66    iw-laplace-k12-b4-l20-e2-r2-both
    lw        2.65        11     iw-laplace-k3-b4-l130-e3-r1-sd    2.64    iw-laplace-k3-b4-l130-e3-r1-sd
    ll        1.13        5      iw-normal-k7-b5-l5-e1-r2          1.13    iw-normal-k7-b5-l5-e1-r2
    lw.e2e    1.57        18 (d) iw-normal-k1000-b3-l8-e5-r2       1.57    iw-normal-k1000-b3-l8-e5-r2
i.e. at most 0.24 of C.  Wall time of this file on an MI355X: 0.3 s for the 39 tests (2.3 s with start-up and collection); the CPU
twin (62 tests): 2 s.
Factor by which each mutation of the reference leaves the bound on its weakest named case, HIP output: no_log_E 2.4e3
(iw-normal-k5-b3-l64-e2-r8), prior_ignored 2.2e4 (iw-softplus-k9-b4-l6-e2-r1-loc), skip_expert 2.2e4 (iw-normal-k2-b3-l3-e32-r0),
log_K 800 (red-big-n2-k65-b5).  Deliberate break of a scratch copy of the kernel and what failed: `- logf((float)E)` dropped:
test_chain on every case with E > 1 (13 of 14).
Suspects of the issue, each with the case that decides it, and the verdict of the run on an MI355X:
    9.  a NaN expert density (iw-nan-expert-*, iw-nan-first-expert-*): the running logsumexp of iwae_logw_kernel dropped it (lw came
        out finite); FIXED in csrc/mmvae.hip (a NaN lq now sets s).  One expert at -inf (iw-one-expert-minf-*), E = 32
        (iw-normal-k2-b3-l3-e32-r0): cleared.  All experts at -inf (iw-all-experts-minf-*): lw = +inf was right, ll came out NaN: 10.
    10. iwae_reduce_kernel: an all -inf column gives -inf (red-minf-column-*): cleared.  A +inf entry gave NaN (expf(inf - inf)) where
        torch.logsumexp gives +inf (red-pinf-entry-*), and a NaN entry in a column that is otherwise -inf gave -inf (fmaxf drops the
        NaN and the sum was skipped; red-nan-entry-*, column 3): both FIXED in csrc/mmvae.hip (a non-finite maximum is not
        subtracted).  n = 8, K in 1, 63, 64, 65, 1000, B in 1, 3, 4, 5, |lw| ~ 3e3 with a spread of 100 (red-big-*): cleared.
    11. Laplace noise at 0, +-(1 - 2^-24), subnormals (iw-laplace-edges-*), K B L no multiple of 256 (iw-normal-k33-b9-l20-*),
        family 2 (iw-softplus-*: the bits of family 0 in all three entries): cleared.
    12. R = 0 and 8, prior_loc alone, prior_sd alone, L in 1, 64, 130, K B = 297, every rejected argument combination
        (test_argument_checks): cleared.
    Cases that failed before the two kernel changes (run against a build of the parent's kernels): test_chain[iw-nan-expert-*],
    test_chain[iw-nan-first-expert-*], test_chain[iw-all-experts-minf-*] (ll), test_reduce[red-pinf-entry-*],
    test_reduce[red-nan-entry-*]; the operations on finite operands are the same as before (every finite case passed on both builds).
"""
import math
import time

import pytest
import torch

import iwae_ref as R
from test_gpu_nexus_kernels import no_nan, note
from test_gpu_recon_nll import EINVAL, Guarded, _lib, dev, same_bits

pytestmark = pytest.mark.gpu

MEASURED = {}
_T0 = time.time()
_RUNS = {}


def hold(measured, stage, ratio, name):
    """Print, record and assert one stage's worst |err| / base."""
    print(f"{name}: {stage} {ratio:.3f}")
    note(measured, stage, ratio, name)
    assert ratio <= R.C_STAGE[stage], f"{name}: {stage} worst |err| / (U base) = {ratio:.3g} > C = {R.C_STAGE[stage]}"


def _d(t):
    return None if t is None else t.to(torch.float32).to(dev()).contiguous()


class Hip:
    def sample(self, fam, loc, sd, noise):
        Lb = _lib()
        K, B, L = noise.shape
        a = [Guarded(t.numel(), src=t) for t in (loc, sd, noise)]
        z = Guarded(K * B * L)
        Lb.call("mvk_iwae_sample", *[Lb.ptr(t.body) for t in a], K, B, L, fam, Lb.ptr(z.body), Lb.stream_ptr())
        torch.cuda.synchronize()
        return dict(z=z.cpu(K, B, L), guards=all(t.intact() for t in a + [z]))

    def logw(self, fam, z, rows, locs, sds, ploc, psd):
        Lb = _lib()
        K, B, L = z.shape
        zd, rd, ld, sd = Guarded(z.numel(), src=z), [_d(t) for t in rows], [_d(t) for t in locs], [_d(t) for t in sds]
        pl, ps = _d(ploc), _d(psd)
        lw = Guarded(K * B)
        Lb.call("mvk_iwae_logw", Lb.ptr(zd.body), Lb.ptr_array(rd) if rd else None, len(rd), Lb.ptr_array(ld), Lb.ptr_array(sd), len(ld),
                Lb.ptr(pl), Lb.ptr(ps), K, B, L, fam, Lb.ptr(lw.body), Lb.stream_ptr())
        torch.cuda.synchronize()
        return dict(lw=lw.cpu(K, B), guards=zd.intact() and lw.intact())

    def reduce(self, lws):
        Lb = _lib()
        K, B = lws[0].shape
        a = [Guarded(K * B, src=t) for t in lws]
        ll = Guarded(B)
        Lb.call("mvk_iwae_reduce", Lb.ptr_array([t.body for t in a]), len(a), K, B, Lb.ptr(ll.body), Lb.stream_ptr())
        torch.cuda.synchronize()
        return dict(ll=ll.cpu(B), guards=all(t.intact() for t in a + [ll]))


HIP = Hip()


def ref_family(case):
    return "laplace" if case.family == "laplace" else "normal"


def run_case(case, be):
    """The chain of one case, every entry launched twice from fresh buffers (and family 2 a third time as family 0)."""
    key = (id(be), case.name)
    if key not in _RUNS:
        inp = R.make_inputs(case)
        out = []
        for fam in [R.FAMILY[case.family]] * 2 + ([0] if case.family == "softplus" else []):
            s = be.sample(fam, inp["sloc"], inp["ssd"], inp["noise"])
            w = be.logw(fam, s["z"], inp["rows"], inp["locs"], inp["sds"], inp["ploc"], inp["psd"])
            r = be.reduce([w["lw"]])
            out.append(dict(z=s["z"], lw=w["lw"], ll=r["ll"], guards=s["guards"] and w["guards"] and r["guards"]))
        _RUNS[key] = (inp, out)
    return _RUNS[key]


def case_ratios(case, inp, got, mut=()):
    fam = ref_family(case)
    zref, zb = R.z_of(fam, inp["sloc"], inp["ssd"], inp["noise"])
    a = (inp["rows"], inp["locs"], inp["sds"], inp["ploc"], inp["psd"], mut)
    lw, base, _ = R.lw_of(fam, got["z"], *a)
    lwe, basee, td = R.lw_of(fam, zref, *a, zmag=zb)
    ll, lb = R.ll_of([got["lw"]], mut)
    return {"z": R.worst_ratio(got["z"], zref, R.U * zb + R.SUB), "lw": R.worst_ratio(got["lw"], lw, R.U * base + R.SUB),
            "lw.e2e": R.worst_ratio(got["lw"], lwe, R.U * (basee + td) + R.SUB), "ll": R.worst_ratio(got["ll"], ll, R.U * lb + R.SUB)}


def check_case(case, be, measured=None):
    inp, out = run_case(case, be)
    got = out[0]
    for o in out:
        assert o["guards"], f"{case.name}: a sentinel next to a buffer was overwritten"
        for k in ("z", "lw", "ll"):
            assert same_bits(o[k], got[k]), f"{case.name}: {k} differs between two launches" + (" or between family 2 and family 0" if len(out) > 2 else "")
    no_nan(got["z"], f"{case.name} z")
    if case.finite:
        no_nan(got["lw"], f"{case.name} lw"), no_nan(got["ll"], f"{case.name} ll")
        assert bool(torch.isfinite(got["lw"]).all()) and bool(torch.isfinite(got["ll"]).all())
    for k, v in case_ratios(case, inp, got).items():
        hold(measured, k, v, case.name)
    zero = inp["noise"] == 0
    assert bool((got["z"][zero] == inp["sloc"].expand_as(got["z"])[zero]).all()), f"{case.name}: z != loc where the noise is 0"
    row1 = torch.zeros(case.K, case.B, dtype=torch.bool)
    row1[:, 1 if case.B > 1 else 0] = True
    if case.special in ("nan", "nan0"):
        assert torch.equal(torch.isnan(got["lw"]), row1), f"{case.name}: the NaN expert density did not give NaN on exactly the (k, b) of row 1"
        assert torch.equal(torch.isnan(got["ll"]), row1[0]) and bool(torch.isfinite(got["lw"][~row1]).all())
    if case.special == "minf":
        assert torch.equal(got["lw"] == math.inf, row1) and torch.equal(got["ll"] == math.inf, row1[0])
        assert bool(torch.isfinite(got["lw"][~row1]).all()) and bool(torch.isfinite(got["ll"][~row1[0]]).all())


@pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
def test_chain(case):
    check_case(case, HIP, MEASURED)


def run_reduce(case, be):
    key = (id(be), case.name)
    if key not in _RUNS:
        lws = R.reduce_inputs(case)
        _RUNS[key] = (lws, be.reduce(lws), be.reduce(lws))
    return _RUNS[key]


def reduce_ratios(case, lws, got, mut=()):
    ll, lb = R.ll_of(lws, mut)
    return {"ll": R.worst_ratio(got["ll"], ll, R.U * lb + R.SUB)}


def check_reduce(case, be, measured=None):
    lws, got, again = run_reduce(case, be)
    assert got["guards"] and again["guards"], f"{case.name}: a sentinel next to a buffer was overwritten"
    assert same_bits(got["ll"], again["ll"]), f"{case.name}: ll differs between two launches"
    ll = got["ll"]
    if case.finite:
        no_nan(ll, case.name)
        assert bool(torch.isfinite(ll).all())
    for k, v in reduce_ratios(case, lws, got).items():
        hold(measured, k, v, case.name)
    cls = R.klass(ll).tolist()
    if case.kind == "minf":
        assert cls == [3, 0, 0, 0, 0], f"{case.name}: classes {cls}: an all -inf column must give -inf and nothing else may leave the finite"
    if case.kind == "pinf":
        assert cls == [0, 2, 0, 2, 0], f"{case.name}: classes {cls}: a +inf entry must give +inf"
    if case.kind == "nan":
        assert cls == [0, 1, 0, 1, 1], f"{case.name}: classes {cls}: a NaN entry must give NaN for its column alone"


@pytest.mark.parametrize("case", R.REDUCE_CASES, ids=[c.name for c in R.REDUCE_CASES])
def test_reduce(case):
    check_reduce(case, HIP, MEASURED)


# ---- teeth ------------------------------------------------------------------------------------------------------------------------------------
def teeth_factor(mut, stages, name, be):
    m = (mut,)
    if name in R.BY_NAME:
        case = R.BY_NAME[name]
        inp, out = run_case(case, be)
        clean, bad = case_ratios(case, inp, out[0]), case_ratios(case, inp, out[0], m)
    else:
        case = R.REDUCE_BY_NAME[name]
        lws, got, _ = run_reduce(case, be)
        clean, bad = reduce_ratios(case, lws, got), reduce_ratios(case, lws, got, m)
    assert all(clean[k] <= R.C_STAGE[k] for k in stages), clean
    return min(bad[k] / R.C_STAGE[k] for k in stages)


TEETH_IDS = [(mut, stages, name) for mut, stages, names in R.TEETH for name in names]


@pytest.mark.parametrize("mut,stages,name", TEETH_IDS, ids=[f"{t[0]}-{t[2]}" for t in TEETH_IDS])
def test_tolerance_rejects_mutated_reference(mut, stages, name):
    f = teeth_factor(mut, stages, name, HIP)
    print(mut, name, f"{f:.3g}x the bound")
    assert f > 1.0, f"{mut} passes on {name}: {f:.3g}x the bound"


# ---- argument checks ------------------------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    """Every MVK_EINVAL branch: sample: a NULL loc, sd, noise or z, K or B -1, L 0, family -1 or 3; logw: a NULL z, loc, sd or lw, rows
    NULL with n_rows 1, n_rows -1 or 9, E 0 or 33, K or B -1, L 0, family -1 or 3, a NULL rows[r], loc[e] or sd[e]; reduce: a NULL
    lw or ll, n 0 or 9, K 0, B -1, a NULL lw[j].  Nothing is launched: the NaN-filled outputs stay as they are.  K = 0 or B = 0 is
    MVK_OK and writes nothing; E = 32, n_rows = 8 and n = 8 are accepted (test_chain, test_reduce)."""
    Lb = _lib()
    lib, sp, pa, p = Lb.load(), Lb.stream_ptr, Lb.ptr_array, Lb.ptr
    K, B, L = 2, 3, 4
    src = Guarded(K * B * L, fill=0.5)
    z, lw, ll = Guarded(K * B * L), Guarded(K * B), Guarded(B)
    s = src.body

    def smp(loc=p(s), sd=p(s), noise=p(s), K=K, B=B, L=L, fam=0, out=p(z.body)):
        return lib.mvk_iwae_sample(loc, sd, noise, K, B, L, fam, out, sp())

    def lgw(zz=p(s), rows=pa([s]), nr=1, loc=pa([s, s]), sd=pa([s, s]), E=2, K=K, B=B, L=L, fam=0, out=p(lw.body)):
        return lib.mvk_iwae_logw(zz, rows, nr, loc, sd, E, None, None, K, B, L, fam, out, sp())

    def red(a=pa([s, s]), n=2, K=K, B=B, out=p(ll.body)):
        return lib.mvk_iwae_reduce(a, n, K, B, out, sp())

    bad = [smp(loc=None), smp(sd=None), smp(noise=None), smp(out=None), smp(K=-1), smp(B=-1), smp(L=0), smp(fam=-1), smp(fam=3),
           lgw(zz=None), lgw(loc=None), lgw(sd=None), lgw(out=None), lgw(rows=None), lgw(nr=-1), lgw(rows=pa([s] * 9), nr=9), lgw(E=0),
           lgw(loc=pa([s] * 33), sd=pa([s] * 33), E=33), lgw(K=-1), lgw(B=-1), lgw(L=0), lgw(fam=-1), lgw(fam=3),
           lgw(rows=pa([s, None]), nr=2), lgw(loc=pa([s, None])), lgw(sd=pa([None, s])),
           red(a=None), red(out=None), red(n=0), red(a=pa([s] * 9), n=9), red(K=0), red(B=-1), red(a=pa([s, None]))]
    for i, rc in enumerate(bad):
        assert rc == EINVAL, f"bad call {i} was accepted ({rc})"
    assert smp(K=0) == 0 and smp(B=0) == 0 and lgw(K=0) == 0 and lgw(B=0) == 0 and red(B=0) == 0
    assert lgw(rows=None, nr=0, K=0) == 0
    torch.cuda.synchronize()
    for t in (z, lw, ll):
        assert bool(torch.isnan(t.body).all()) and t.intact()
    assert src.intact()


def test_zz_report():
    """Prints the head-room the HIP kernels showed in this session (the largest |err| / (U base) per stage, with the case) and the
    wall time of this file."""
    print("HIP_MEASURED", {k: (round(v, 3), n) for k, (v, n) in sorted(MEASURED.items())})
    print(f"WALL test_gpu_iwae.py {time.time() - _T0:.1f} s")
