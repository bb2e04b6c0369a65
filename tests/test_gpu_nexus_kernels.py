"""The four entries of csrc/nexus.hip (mvk_nexus_aggregate_fwd/bwd, mvk_nexus_top_nll_fwd/bwd; six kernels) called directly through
the C ABI, entry by entry against float64, and the forced perceptual dropout (FPD) of nexus_keep bit for bit against a float32 model.

References, case tables (AGG_CASES, TOP_CASES, the FPD tables), error model and mutations live in tests/nexus_kernels_ref.py;
tests/test_nexus_kernels_ref_host.py pins them on the CPU and runs the `check_*` routines below with a stand-in backend (the same
formulas in plain torch fp32).  Per case:

1. every output (agg, keep_out, dmsgs, q, s2, rows, dr, and the scratch `work`) is allocated with NaN prefill and 64 sentinel floats
   before and after; |got - ref| <= C_STAGE[stage] * U * base + SUB for EVERY entry; a NaN left anywhere fails (outside the one
   s2 = 0 case, where the non-finite class of every entry must equal that of the fp32 formula on the CPU); no sentinel is touched;
2. s2 is checked against the reference on the q the kernel wrote, rows and dr against the reference on its q and s2, and all three
   once more from the inputs (`*.e2e`);
3. exact properties: keep_out against the keep model bit for bit (0.5, -3 and a subnormal in keep_in give 1.0); a row with nothing
   kept has message and gradient exactly 0; dmsgs of a dropped modality exactly 0 and those of the kept modalities of one row
   bit-identical to each other; rows of masked rows exactly 0; s2 of an unadapted modality exactly 1; dr of a modality whose
   grows[m] is NULL exactly 0; with no adapted modality the backward pass leaves `work` untouched (still NaN);
4. a second launch is bit-identical;
5. test_fpd_*: keep_out bit for bit against nexus_kernels_ref.fpd_keep on crafted uniforms (u0 at p and its float32 neighbours,
   u1 and every shuffle uniform at 0, 1 - 2^-24 and 1.0, p in 0, 0.3, 1) and on 3000 random rows for each M in 2, 3, 5, 8;
6. test_argument_checks: every MVK_EINVAL branch of the four entries, which launch nothing;
7. test_tolerance_rejects_mutated_reference: the HIP output against each wrong reference of TEETH leaves the bound.

Constants (nexus_kernels_ref.C_STAGE): 4x the largest |err| / base of the plain-torch-fp32 stand-in on the CPU, rounded up, or
derived from the count of roundings (d); next to them the largest |err| / base of the HIP kernels on an MI355X (test_zz_report):
    stage     torch fp32  C      set by                     HIP     set by
    agg       2.17        9      agg-u-m3-b3-d65            2.17    agg-u-m3-b3-d65
    dmsgs     0.84        1 (d)  agg-keepin-m8-b5-d130      0.84    agg-keepin-m8-b5-d130
    q         3.77        16     top-b1025                  3.77    top-b1025
    s2        2.38        10     top-maskmost-b300          2.15    top-sign-b300
    rows      2.27        10     top-sign-b300              2.27    top-sign-b300
    dr        2.34        32 (d) top-wide-adapted           2.34    top-wide-adapted
    s2.e2e    2.34        26 (d) top-maskmost-b300          2.20    top-sign-b300
    rows.e2e  2.32        78 (d) top-b65537                 2.28    top-sign-b300
    dr.e2e    4.30        126 (d) top-maskmost-b300         2.46    top-b3
    c_m       0.68        3      top-b5-m8                  0.59    top-b1
i.e. at most 0.84 of C (dmsgs, one division) and 0.24 of C on every measured stage; the elementwise stages come out with the bits of
the CPU evaluation.  c_m is what the partial sums of C_m left in `work` add up to, against the float64 C_m of the same q and s2,
over U times the sum of the magnitudes.  On the all-ones case (top-ones-b300, C_m = 0 in real arithmetic) the
residue is 0.37 U sum|.| on the MI355X, and the worst dr entry of that case sits at 0.88 U of its per-entry base: suspect 1 is cleared.
Wall time of this file on an MI355X: 0.9 s for the 50 tests (4.2 s with start-up and collection); the CPU twin (64 tests): 4 s.
Factor by which each mutation of the reference leaves the bound on its weakest named case and stage, HIP output (the stand-in
gives the same figures): s2_unmasked_only 4.2e3 (top-wide-adapted), no_cterm 307 (top-sign-b300), mean_over_M 3.7e6
(agg-keepin-m3-b37-d70); the bit-exact FPD model: no_swap changes 624 of 6000 rows (fpd-random-m3), u0_le_p 28 rows
(fpd-crafted-m2).  Deliberate breaks of a scratch copy of the kernels and what failed: `2.f *` of cterm dropped: test_top_nll on every
case with an adapted modality whose C_m does not vanish (11 of 15); the `j > M - 1` clamp replaced by `j = i`: all four fpd-crafted
tables.
Suspects of the issue, each with the case that decides it, and the verdict of the run on an MI355X:
    1. C_m as rounding residue (top-ones-b300, top-sign-b300, top-maskmost-b300; base from the sum of magnitudes): cleared, see above.
    2. the second and third trip of the forward partial loop (top-b1025, top-b2049) and the second trip of the backward one
       (top-b65537, nparts = 257) against float64: cleared.
    3. the grid sized by Dmax (top-narrow-adapted, top-wide-adapted) and the skipped first backward launch (top-none-adapted: `work`
       is still all NaN after the backward pass): cleared.
    4. a NULL masks[m] in a given array and a NULL grows[m] (top-mixed-null, top-b3): accepted, the modality is complete / its dr is
       exactly 0: cleared; include/mvk.h now says so.
    5. precedence keep_in > masks > u (agg-all-three-m3-b37-d7, agg-masks-u-m3-b37-d7), keep_in of 0.5, -3 and 1e-40 (agg-keepin-odd-*),
       an empty row (row 0 of every keep_in / masks case), M = 1 with u (agg-u-m1-b9-d3), M = 8 (agg-u-m8-b37-d5,
       agg-keepin-m8-b5-d130): cleared.
    6. FPD bit for bit (test_fpd_keep_is_the_float32_model, 8 tables): cleared; the clamps are reached by u = 1.0 only (the CPU twin
       shows that (1 - 2^-24) n never rounds up to n for n <= 7).
    7. B in 1, 3, 4, 5 and D in 1, 63, 64, 65, 130 (top-b1 .. top-b5-m8, agg-*): cleared.
    8. s2 = 0 (top-s2-zero): rows and dr of that modality are all NaN, s2 = 0, exactly the classes of the fp32 formula on the CPU; the
       other modalities are untouched.  Documented in include/mvk.h, not changed.
    No change to csrc/nexus.hip.
"""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import nexus_kernels_ref as R
from test_gpu_recon_nll import EINVAL, Guarded, _lib, dev, same_bits

pytestmark = pytest.mark.gpu

MEASURED = {}
_T0 = time.time()
_RUNS = {}


def note(measured, stage, ratio, name):
    if measured is not None and ratio > measured.get(stage, (-1.0, ""))[0]:
        measured[stage] = (ratio, name)


def hold(measured, stage, ratio, name):
    """Print, record and assert one stage's worst |err| / base."""
    print(f"{name}: {stage} {ratio:.3f}")
    note(measured, stage, ratio, name)
    assert ratio <= R.C_STAGE[stage], f"{name}: {stage} worst |err| / (U base) = {ratio:.3g} > C = {R.C_STAGE[stage]}"


def no_nan(t, what):
    assert not bool(torch.isnan(t).any()), f"{what}: a NaN is left: an entry the kernel did not write"


def _u8(t):
    return None if t is None else t.to(torch.uint8).to(dev()).contiguous()


def _d(t):
    return None if t is None else t.to(torch.float32).to(dev()).contiguous()


# ---- the HIP backend ------------------------------------------------------------------------------------------------------------------------
class Hip:
    def agg_fwd(self, msgs, masks, keep_in, u, p):
        Lb = _lib()
        M, (B, D) = len(msgs), msgs[0].shape
        gm = [Guarded(B * D, src=t) for t in msgs]
        mk = None if masks is None else [_u8(t) for t in masks]
        ki, ud = _d(keep_in), _d(u)
        agg, keep = Guarded(B * D), Guarded(B * M)
        Lb.call("mvk_nexus_aggregate_fwd", Lb.ptr_array([g.body for g in gm]), None if mk is None else Lb.ptr_array(mk), Lb.ptr(ki),
                Lb.ptr(ud), float(p), M, B, D, Lb.ptr(agg.body), Lb.ptr(keep.body), Lb.stream_ptr())
        torch.cuda.synchronize()
        return dict(agg=agg.cpu(B, D), keep=keep.cpu(B, M), guards=all(g.intact() for g in gm + [agg, keep]))

    def agg_bwd(self, keep, g):
        Lb = _lib()
        (B, M), D = keep.shape, g.shape[1]
        kd, gd = Guarded(B * M, src=keep), Guarded(B * D, src=g)
        dm = [Guarded(B * D) for _ in range(M)]
        Lb.call("mvk_nexus_aggregate_bwd", Lb.ptr(kd.body), Lb.ptr(gd.body), M, B, D, Lb.ptr_array([t.body for t in dm]), Lb.stream_ptr())
        torch.cuda.synchronize()
        return dict(dmsgs=torch.stack([t.cpu(B, D) for t in dm]), guards=all(t.intact() for t in dm + [kd, gd]))

    @staticmethod
    def _top_args(inp, dims, adapt):
        Lb = _lib()
        M = len(dims)
        keepalive = dict(z=[_d(t) for t in inp["z"]], r=[_d(t) for t in inp["r"]],
                         masks=None if inp["masks"] is None else [_u8(t) for t in inp["masks"]])
        args = (Lb.ptr_array(keepalive["z"]), Lb.ptr_array(keepalive["r"]), None if keepalive["masks"] is None else Lb.ptr_array(keepalive["masks"]),
                (C.c_int * M)(*dims), (C.c_float * M)(*inp["gamma"]), (C.c_int * M)(*[int(a) for a in adapt]), M, inp["z"][0].shape[0])
        return keepalive, args

    def top_fwd(self, inp, dims, adapt):
        Lb = _lib()
        M, B = len(dims), inp["z"][0].shape[0]
        keepalive, args = self._top_args(inp, dims, adapt)
        rows = [Guarded(B) for _ in range(M)]
        q, s2, work = Guarded(M * B), Guarded(M), Guarded(M * ((B + 3) // 4))
        Lb.call("mvk_nexus_top_nll_fwd", *args, Lb.ptr_array([t.body for t in rows]), Lb.ptr(q.body), Lb.ptr(s2.body), Lb.ptr(work.body),
                Lb.stream_ptr())
        torch.cuda.synchronize()
        return dict(rows=torch.stack([t.cpu(B) for t in rows]), q=q.cpu(M, B), s2=s2.cpu(M), work=work.cpu(-1),
                    guards=all(t.intact() for t in rows + [q, s2, work]))

    def top_bwd(self, inp, dims, adapt, q, s2):
        Lb = _lib()
        M, B = len(dims), inp["z"][0].shape[0]
        keepalive, args = self._top_args(inp, dims, adapt)
        gr = [_d(t) for t in inp["g"]]
        qd, sd = Guarded(M * B, src=q), Guarded(M, src=s2)
        work = Guarded(M * ((B + 3) // 4))
        dr = [Guarded(B * d) for d in dims]
        Lb.call("mvk_nexus_top_nll_bwd", *args, Lb.ptr_array(gr), Lb.ptr(qd.body), Lb.ptr(sd.body), Lb.ptr(work.body),
                Lb.ptr_array([t.body for t in dr]), Lb.stream_ptr())
        torch.cuda.synchronize()
        return dict(dr=[t.cpu(B, d) for t, d in zip(dr, dims)], work=work.cpu(-1), guards=all(t.intact() for t in dr + [qd, sd, work]))


HIP = Hip()


# ---- aggregation ------------------------------------------------------------------------------------------------------------------------------
def run_agg(case, be):
    key = (id(be), case.name)
    if key not in _RUNS:
        inp = R.agg_inputs(case)
        a = (inp["msgs"], inp["masks"], inp["keep_in"], inp["u"], case.p)
        f, f2 = be.agg_fwd(*a), be.agg_fwd(*a)
        b, b2 = be.agg_bwd(f["keep"], inp["gout"]), be.agg_bwd(f["keep"], inp["gout"])
        _RUNS[key] = (inp, f, f2, b, b2)
    return _RUNS[key]


def agg_ratios(case, inp, f, b, mut=()):
    keep = R.keep_set(case.M, case.B, inp["keep_in"], inp["masks"], inp["u"], case.p)
    ref, base = R.agg(inp["msgs"], keep, mut)
    dref, dbase = R.dmsgs(keep, inp["gout"], mut)
    return {"agg": R.worst_ratio(f["agg"], ref, R.U * base + R.SUB), "dmsgs": R.worst_ratio(b["dmsgs"], dref, R.U * dbase + R.SUB)}


def check_agg(case, be, measured=None):
    inp, f, f2, b, b2 = run_agg(case, be)
    M, B = case.M, case.B
    assert f["guards"] and b["guards"], f"{case.name}: a sentinel next to a buffer was overwritten"
    for k in ("agg", "keep"):
        no_nan(f[k], f"{case.name} {k}")
        assert same_bits(f[k], f2[k]), f"{case.name}: {k} differs between two launches"
    no_nan(b["dmsgs"], f"{case.name} dmsgs")
    assert same_bits(b["dmsgs"], b2["dmsgs"]), f"{case.name}: dmsgs differs between two launches"
    keep = R.keep_set(M, B, inp["keep_in"], inp["masks"], inp["u"], case.p)
    assert same_bits(f["keep"], keep), f"{case.name}: keep_out is not the keep model bit for bit"
    for k, v in agg_ratios(case, inp, f, b).items():
        hold(measured, k, v, case.name)
    empty = keep.sum(1) == 0
    assert bool((f["agg"][empty] == 0).all()) and bool((b["dmsgs"][:, empty] == 0).all()), f"{case.name}: a row with nothing kept is not exactly 0"
    first = b["dmsgs"][keep.argmax(1), torch.arange(B)]  # [B, D]: the gradient of the first kept modality of each row
    for m in range(M):
        sel = keep[:, m] != 0
        assert bool((b["dmsgs"][m][~sel] == 0).all()), f"{case.name}: dmsgs[{m}] of a dropped modality is not exactly 0"
        assert same_bits(b["dmsgs"][m][sel], first[sel]), f"{case.name}: dmsgs of the kept modalities of one row differ in bits"


@pytest.mark.parametrize("case", R.AGG_CASES, ids=[c.name for c in R.AGG_CASES])
def test_aggregate(case):
    check_agg(case, HIP, MEASURED)


# ---- forced perceptual dropout ---------------------------------------------------------------------------------------------------------------------
def fpd_table(name):
    """name = fpd-crafted-mM or fpd-random-mM -> [(p, u)]."""
    kind, M = name.split("-")[1], int(name.split("-m")[1])
    if kind == "crafted":
        return M, [(p, R.fpd_crafted(M, p)) for p in R.FPD_P]
    return M, [(p, R.fpd_random(M)) for p in (0.3, 1.0)]


FPD_TABLES = [f"fpd-{k}-m{M}" for k in ("crafted", "random") for M in R.FPD_M]


def run_fpd(name, be):
    key = (id(be), name)
    if key not in _RUNS:
        M, tabs = fpd_table(name)
        out = []
        for p, u in tabs:
            msgs = [torch.full((u.shape[0], 1), float(m + 1)) for m in range(M)]
            out.append((p, u, be.agg_fwd(msgs, None, None, torch.from_numpy(u), p)))
        _RUNS[key] = (M, out)
    return _RUNS[key]


def fpd_mismatches(name, be, mut=()):
    M, out = run_fpd(name, be)
    bad = 0
    for p, u, f in out:
        assert f["guards"]
        no_nan(f["keep"], name)
        no_nan(f["agg"], name)
        want = torch.from_numpy(R.fpd_keep(u, p, M, mut))
        bad += int((f["keep"].view(torch.int32) != want.view(torch.int32)).any(1).sum())
    return bad


def check_fpd(name, be):
    assert fpd_mismatches(name, be) == 0, f"{name}: keep_out differs from the float32 model of nexus_keep"
    M, out = run_fpd(name, be)
    for p, u, f in out:  # the message of the kept set: msgs are the constants m + 1, so agg names the subset's mean
        k = f["keep"].double()
        want = (k * torch.arange(1, M + 1, dtype=R.F64)).sum(1) / k.sum(1)
        assert bool((k.sum(1) >= 1).all()) and R.worst_ratio(f["agg"][:, 0], want, R.C_STAGE["agg"] * R.U * want) <= 1.0


@pytest.mark.parametrize("name", FPD_TABLES)
def test_fpd_keep_is_the_float32_model(name):
    check_fpd(name, HIP)


# ---- top-level likelihood ---------------------------------------------------------------------------------------------------------------------------
def run_top(case, be):
    key = (id(be), case.name)
    if key not in _RUNS:
        inp = R.top_inputs(case)
        f, f2 = be.top_fwd(inp, case.dims, case.adapt), be.top_fwd(inp, case.dims, case.adapt)
        b, b2 = be.top_bwd(inp, case.dims, case.adapt, f["q"], f["s2"]), be.top_bwd(inp, case.dims, case.adapt, f["q"], f["s2"])
        _RUNS[key] = (inp, f, f2, b, b2)
    return _RUNS[key]


def top_ratios(case, inp, f, b, mut=()):
    """stage -> the worst |err| / (U base) over the modalities ("c_m": what the partial sums left in `work` by the backward pass
    add up to against C_m of the q and s2 it was given, over the sum of the magnitudes)."""
    out = {}
    B = case.B
    nb = (B + 255) // 256

    def put(k, v):
        out[k] = max(out.get(k, 0.0), v)

    for m, D in enumerate(case.dims):
        z, r, gamma, ad = inp["z"][m], inp["r"][m], inp["gamma"][m], case.adapt[m]
        mask = None if inp["masks"] is None else inp["masks"][m]
        g = inp["g"][m]
        qref, qb = R.q_rows(z, r)
        put("q", R.worst_ratio(f["q"][m], qref, R.U * qb + R.SUB))
        stages = [("", f["q"][m], None)] + ([(".e2e", qref, None)] if case.e2e else [])
        for suffix, qq, _ in stages:
            s2ref = R.s2_of(qq, D, ad, mask, mut)
            if ad:
                put("s2" + suffix, R.worst_ratio(f["s2"][m], s2ref, R.U * s2ref + R.SUB))
            s2u = f["s2"][m] if suffix == "" else s2ref
            rref, rb = R.rows_of(qq, s2u, D, gamma, mask)
            put("rows" + suffix, R.worst_ratio(f["rows"][m], rref, R.U * rb + R.SUB))
            dref, db = R.dr_of(z, r, qq, s2u, gamma, ad, g, mask, mut)
            put("dr" + suffix, R.worst_ratio(b["dr"][m], dref, R.U * db + R.SUB))
        if ad and g is not None and not mut and case.name not in R.NONFINITE_CASES:
            Cm, Sm = R.c_m(f["q"][m], f["s2"][m], D, g, mask)
            put("c_m", abs(float(b["work"][m * nb:(m + 1) * nb].double().sum()) - float(Cm)) / (R.U * float(Sm)))
    return out


def check_top(case, be, measured=None):
    inp, f, f2, b, b2 = run_top(case, be)
    M, B = len(case.dims), case.B
    assert f["guards"] and b["guards"], f"{case.name}: a sentinel next to a buffer was overwritten"
    for k in ("rows", "q", "s2", "work"):
        assert same_bits(f[k], f2[k]), f"{case.name}: {k} differs between two launches"
    assert same_bits(b["work"], b2["work"]) and all(same_bits(x, y) for x, y in zip(b["dr"], b2["dr"])), f"{case.name}: dr differs between two launches"
    if case.name in R.NONFINITE_CASES:
        for m, D in enumerate(case.dims):
            mask = None if inp["masks"] is None else inp["masks"][m]
            fp = R.top_fp32(inp["z"][m], inp["r"][m], D, inp["gamma"][m], case.adapt[m], mask, inp["g"][m])
            for k, got in (("q", f["q"][m]), ("s2", f["s2"][m]), ("rows", f["rows"][m]), ("dr", b["dr"][m])):
                assert torch.equal(R.klass(got), R.klass(fp[k])), f"{case.name}: {k}[{m}] is not in the non-finite class of the fp32 formula"
            if case.zero[m]:
                assert float(f["s2"][m]) == 0.0 and bool(torch.isnan(f["rows"][m]).all()) and bool(torch.isnan(b["dr"][m]).all())
            else:
                no_nan(f["rows"][m], case.name), no_nan(b["dr"][m], case.name)
    else:
        for k in ("rows", "q", "s2", "work"):
            no_nan(f[k], f"{case.name} {k}")
        for t in b["dr"]:
            no_nan(t, f"{case.name} dr")
    ratios = top_ratios(case, inp, f, b)
    for k, v in ratios.items():
        hold(measured, k, v, case.name)
    for m in range(M):
        if not case.adapt[m]:
            assert float(f["s2"][m]) == 1.0, f"{case.name}: s2 of an unadapted modality is not exactly 1"
        if inp["masks"] is not None and inp["masks"][m] is not None and not (case.zero and case.zero[m]):
            assert bool((f["rows"][m][~inp["masks"][m]] == 0).all()), f"{case.name}: rows of masked rows are not exactly 0"
        if inp["g"][m] is None and not (case.zero and case.zero[m]):
            assert bool((b["dr"][m] == 0).all()), f"{case.name}: dr of a modality without grows is not exactly 0"
    nb = (B + 255) // 256
    if any(case.adapt):
        assert bool(torch.isnan(b["work"][M * nb:]).all()), f"{case.name}: the backward pass wrote `work` beyond its M x ceil(B / 256) partials"
    else:
        assert bool(torch.isnan(b["work"]).all()), f"{case.name}: `work` was written although no modality is adapted"


@pytest.mark.parametrize("case", R.TOP_CASES, ids=[c.name for c in R.TOP_CASES])
def test_top_nll(case):
    check_top(case, HIP, MEASURED)


# ---- teeth ------------------------------------------------------------------------------------------------------------------------------------
def teeth_factor(mut, family, stages, name, be):
    """The factor by which the backend's output leaves the bound of the reference mutated by `mut` on case `name` (its weakest named
    stage); for the bit-exact FPD model: the number of rows that differ."""
    m = (mut,)
    if family == "fpd":
        assert fpd_mismatches(name, be) == 0
        return float(fpd_mismatches(name, be, m))
    if family == "agg":
        case = R.AGG_BY_NAME[name]
        inp, f, _, b, _ = run_agg(case, be)
        clean, bad = agg_ratios(case, inp, f, b), agg_ratios(case, inp, f, b, m)
    else:
        case = R.TOP_BY_NAME[name]
        inp, f, _, b, _ = run_top(case, be)
        clean, bad = top_ratios(case, inp, f, b), top_ratios(case, inp, f, b, m)
    assert all(clean[k] <= R.C_STAGE[k] for k in stages), clean
    return min(bad[k] / R.C_STAGE[k] for k in stages)


TEETH_IDS = [(mut, fam, stages, name) for mut, fam, stages, names in R.TEETH for name in names]


@pytest.mark.parametrize("mut,family,stages,name", TEETH_IDS, ids=[f"{t[0]}-{t[3]}" for t in TEETH_IDS])
def test_tolerance_rejects_mutated_reference(mut, family, stages, name):
    f = teeth_factor(mut, family, stages, name, HIP)
    print(mut, name, f"{f:.3g}x the bound" if family != "fpd" else f"{f:.0f} rows differ")
    assert f > 1.0 if family != "fpd" else f >= 1.0, f"{mut} passes on {name}"


# ---- argument checks ------------------------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    """Every MVK_EINVAL branch of the four entries: a NULL array or output, M 0 or 9, B -1, D 0, a NULL msgs[m], masks[m] (aggregate
    only: the top NLL takes a NULL masks[m] as "complete"), dmsgs[m], z[m], r[m], rows[m] or dr[m], D[m] 0.  Nothing is launched:
    the NaN-filled outputs stay as they are.  B = 0 is MVK_OK and writes nothing."""
    Lb = _lib()
    lib, sp, pa, p = Lb.load(), Lb.stream_ptr, Lb.ptr_array, Lb.ptr
    M, B, D = 3, 5, 4
    src = [Guarded(B * D, fill=0.5) for _ in range(M)]
    mk = [_u8(torch.ones(B)) for _ in range(M)]
    outs = [Guarded(B * D) for _ in range(M)]
    small = Guarded(M * B)
    work = Guarded(M * 2)
    sb = [t.body for t in src]
    ob = [t.body for t in outs]

    def fwd(msgs=pa(sb), masks=None, M=M, B=B, D=D, agg=p(outs[0].body), keep=p(small.body)):
        return lib.mvk_nexus_aggregate_fwd(msgs, masks, None, None, 0.0, M, B, D, agg, keep, sp())

    def bwd(keep=p(src[0].body), g=p(src[1].body), M=M, B=B, D=D, dm=pa(ob)):
        return lib.mvk_nexus_aggregate_bwd(keep, g, M, B, D, dm, sp())

    def ints(v):
        return (C.c_int * len(v))(*v)

    gam = (C.c_float * M)(1.0, 1.0, 1.0)

    def tfwd(z=pa(sb), r=pa(sb), masks=None, Ds=ints([D] * M), gamma=gam, adapt=ints([1] * M), M=M, B=B, rows=pa(ob), q=p(small.body),
             s2=p(small.body), wk=p(work.body)):
        return lib.mvk_nexus_top_nll_fwd(z, r, masks, Ds, gamma, adapt, M, B, rows, q, s2, wk, sp())

    def tbwd(z=pa(sb), r=pa(sb), masks=None, Ds=ints([D] * M), gamma=gam, adapt=ints([1] * M), M=M, B=B, grows=pa(sb), q=p(src[0].body),
             s2=p(src[0].body), wk=p(work.body), dr=pa(ob)):
        return lib.mvk_nexus_top_nll_bwd(z, r, masks, Ds, gamma, adapt, M, B, grows, q, s2, wk, dr, sp())

    hole = lambda a: pa([a[0], None, a[2]])  # noqa: E731
    bad = [fwd(msgs=None), fwd(agg=None), fwd(keep=None), fwd(M=0), fwd(msgs=pa(sb * 3), M=9), fwd(B=-1), fwd(D=0), fwd(msgs=hole(sb)),
           fwd(masks=hole(mk)),
           bwd(keep=None), bwd(g=None), bwd(dm=None), bwd(M=0), bwd(dm=pa(ob * 3), M=9), bwd(B=-1), bwd(D=0), bwd(dm=hole(ob))]
    for fn, extra in ((tfwd, [dict(rows=None), dict(q=None), dict(s2=None), dict(wk=None), dict(rows=hole(ob))]),
                      (tbwd, [dict(grows=None), dict(q=None), dict(s2=None), dict(wk=None), dict(dr=None), dict(dr=hole(ob))])):
        common = [dict(z=None), dict(r=None), dict(Ds=None), dict(gamma=None), dict(adapt=None), dict(M=0), dict(M=9), dict(B=-1),
                  dict(z=hole(sb)), dict(r=hole(sb)), dict(Ds=ints([D, 0, D]))]
        bad += [fn(**kw) for kw in common + extra]
    for i, rc in enumerate(bad):
        assert rc == EINVAL, f"bad call {i} was accepted ({rc})"
    assert fwd(B=0) == 0 and bwd(B=0) == 0 and tfwd(B=0) == 0 and tbwd(B=0) == 0
    torch.cuda.synchronize()
    for t in outs + [small, work]:
        assert bool(torch.isnan(t.body).all()) and t.intact()
    assert all(t.intact() for t in src)
    # accepted: a NULL masks[m] in the top NLL's array and a NULL grows[m] (test_top_nll: top-mixed-null), M = 8 (agg-*-m8, top-b5-m8)


def test_zz_report():
    """Prints the head-room the HIP kernels showed in this session (the largest |err| / (U base) per stage, with the case) and the
    wall time of this file."""
    print("HIP_MEASURED", {k: (round(v, 3), n) for k, (v, n) in sorted(MEASURED.items())})
    print(f"WALL test_gpu_nexus_kernels.py {time.time() - _T0:.1f} s")
