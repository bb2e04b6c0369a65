"""mvk_recon_nll_fwd / mvk_recon_nll_bwd (csrc/elbo.hip) and the two loss-seed kernels mvk_loss_backward_seed /
mvk_scale_by_device_scalar (csrc/misc.hip) called directly through the C ABI, entry-wise against float64.

Reference, case table (nll_ref.CASES: every case says which edge it is there for) and error model live in tests/nll_ref.py;
tests/test_nll_ref_host.py pins that reference to oracle.elbo._row_nll on the CPU and runs `check_case` below on every case
with a stand-in launcher (the fp32 oracle), so the table and the bounds are proven before any GPU time is spent.  Per case:

1. rows and drecon, allocated with NaN prefill and 64 sentinel floats before and after, against the float64 reference:
   |got - ref| <= C_STAGE[stage] * base for EVERY entry; a NaN left anywhere fails; the sentinels are untouched (dead and
   tail lanes write nothing outside the row);
2. exact properties: drecon of a masked-out row and of a Laplace tie is exactly 0; rows are bit-identical with every option
   toggled (mask, rowcoef, drecon given / NULL, another coef); mask = NULL against all-ones and rowcoef = NULL against ones
   agree bit for bit; the gradient of the fused forward and of mvk_recon_nll_bwd with rows = NULL agree bit for bit (both
   instantiations run recon_vec_body / the scalar loop with the same operands in the same order; FWD only adds the row store);
3. a second launch is bit-identical;
4. test_one_launch_of_eight: one call with n_mod = 8 that mixes the scalar, Normal / Laplace float4, Bernoulli float4 and
   categorical groups gives every descriptor the bits it gets when launched alone;
5. test_argument_checks: every MVK_EINVAL branch of launch_recon (its validation loop precedes every launch, so a rejected
   call launches nothing), B = 0 is MVK_OK and writes nothing;
6. the seed kernels against float64 with sentinels, across the grid cap of 4096 blocks.

Constants (nll_ref.C_STAGE = 4x the largest |err| / base of oracle.elbo in plain torch fp32 on the CPU, backward by fp32
autograd, over the case table, rounded up; re-derived by test_nll_ref_host.py::test_error_constants), and the largest
|err| / base of the HIP kernels on an MI355X (test_zz_report):
    stage               torch fp32  C   set by                                     HIP    set by
    normal.rows         0.38        2   normal-k33-b1-d4-rc                        0.46   normal-k33-b1-d4-rc
    normal.drecon       1.74        7   normal.75-k10-b5-d1020-random-rc           2.44   normal.75-k10-b5-d1020-random-rc
    laplace.rows        0.32        2   laplace-k10-b9-d3-random-rc                0.26   laplace.3-k10-b3-d8
    laplace.drecon      1.52        7   laplace-k10-b9-d3-random-rc                1.39   laplace-k10-b9-d3-random-rc
    bernoulli.rows      0.23        1   bernoulli-k16-b5-d255-soft                 0.13   bernoulli-k10-b9-d784-soft-random-fwd
    bernoulli.drecon    1.38        6   bernoulli-k17-b3-d4100-soft-rc             1.60   bernoulli-k10-b5-d784-off-x
    categorical.rows    0.16        1   categorical-k33-b1-c130-p1-soft            0.16   categorical-k10-b5-c2-p32-soft-random-rc
    categorical.drecon  1.17        5   categorical-k17-b3-c64-p4-soft-rc          1.22   categorical-k17-b3-c64-p4-soft-rc
i.e. at most 0.35 of C (normal.drecon).  Wall time of this file on an MI355X: 0.8 s for the 47 tests (2.8 s with start-up and
collection); on the CPU with the stand-in launcher (tests/test_nll_ref_host.py, 86 tests): 4 s.
Factor by which each mutation of the reference exceeded the bound on its weakest named case, against torch fp32
(test_nll_ref_host.py): no_row_const 259 (normal.01-k1-b9-d4099-fwd), mask_rows 7.8e5, no_rescale_grad 4.9e5, rowcoef_bk 7.4e10,
drop_last_vec 4.7e3 (bernoulli-k17-b3-d4100-soft-rc: one float4 of 1025), chunk_8_9 2.9e10, bern_no_x 1.4e6, cat_no_sx 1.5e36
(a padding position has base TINY); no_shift is not rejected and cannot be (test_softmax_shift_is_not_rejected_and_cannot_be).

Suspects of the kernel text, each with the case that exercises it:
 1. dead lanes of recon_vec_body load element 0 and compute on it; `live` masks the sum and the store
    (normal-k1-b1-d4: 255 dead lanes; laplace-k17-b3-d1028-rc: one live lane in slot 1; sentinels + NaN prefill).
 2. red[k][wave] accumulates across column tiles (bernoulli-k17-b3-d4100-soft-rc, laplace-k33-b1-d4100-random: two tiles).
 3. balanced chunks kper = ceil(K / kchunks) with rowcoef indexed by k0 + k (K = 17: 9 + 8; K = 33: 3 x 11; the chunk_8_9 and
    rowcoef_bk mutations show the bound sees a wrong index).
 4. nll_row_const in fp32 at scale 0.4, where log s + 0.919 cancels to 0.0026 (normal.4-k16-b3-d1024, one-normal-d4).
 5. Bernoulli sig = e / (1 + e) with e = expf(-90) subnormal (bernoulli-*-hard): inside TINY (1 + w).
 6. categorical: sx = 0 positions write gw * (softmax * 0 - 0) = +-0 (zeros cases); C = 1 (lse = v exactly).
 7. the block_start scan over up to 8 descriptors (test_one_launch_of_eight).
 8. a misaligned drecon moves only the second pass to the scalar group (laplace-k10-b5-d784-off-drecon).
Verdict of the first run on an MI355X: all eight cleared, csrc/elbo.hip is unchanged.  Every stage is inside its bound on
every case, no sentinel was touched, no NaN was left, the fused and the second-pass gradients agree bit for bit on every case
(the assertion stands unrelaxed), and every descriptor of the eight-descriptor launch has the bits of its launch alone.
"""
import time

import pytest
import torch

import nll_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64
EINVAL = -1  # MVK_EINVAL
SENTINEL = 12345.0
MEASURED = {}
_T0 = time.time()


def dev():
    return torch.device("cuda:0")


def _lib():
    from multivae_amd import _lib as L

    return L


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# ---- guarded device buffers --------------------------------------------------------------------------------------------------------------
class Guarded:
    """n floats with GUARD sentinel floats before and after; `off`: the body starts 4 bytes past a 16-byte boundary."""

    def __init__(self, n, off=False, fill=float("nan"), src=None):
        self.n, self.lo = n, GUARD + (1 if off else 0)
        self.buf = torch.full((self.lo + n + GUARD,), SENTINEL, dtype=torch.float32, device=dev())
        self.body = self.buf[self.lo:self.lo + n]
        if src is not None:
            self.body.copy_(src.reshape(-1))
        else:
            self.body.fill_(fill)
        assert (self.body.data_ptr() % 16 == 4) == bool(off) and self.body.data_ptr() % 16 in (0, 4)

    def intact(self):
        b = self.buf.cpu()
        return bool((b[:self.lo] == SENTINEL).all()) and bool((b[self.lo + self.n:] == SENTINEL).all())

    def cpu(self, *shape):
        return self.body.cpu().reshape(*shape).clone()


class Prepared:
    """The device buffers of one descriptor."""

    def __init__(self, case, recon, x, mask, rowcoef, drecon, coef, via):
        K, B, D = case.K, case.B, case.D
        self.case, self.via, self.coef = case, via, coef
        self.recon = Guarded(K * B * D, off=case.misalign == "recon", src=recon)
        self.x = Guarded(B * D, off=case.misalign == "x", src=x)
        self.mask = None if mask is None else mask.to(torch.uint8).to(dev()).contiguous()
        self.rowcoef = None if rowcoef is None else rowcoef.to(dev()).contiguous()
        self.rows = Guarded(K * B) if via == "fwd" else None
        self.drecon = Guarded(K * B * D, off=case.misalign == "drecon") if drecon else None
        assert via == "fwd" or drecon

    def fill(self, e, with_drecon=True, with_rows=True):
        Lb, c = _lib(), self.case
        e.recon, e.x = self.recon.body.data_ptr(), self.x.body.data_ptr()
        e.mask = None if self.mask is None else self.mask.data_ptr()
        e.rowcoef = None if self.rowcoef is None else self.rowcoef.data_ptr()
        e.rows = self.rows.body.data_ptr() if (self.rows is not None and with_rows) else None
        e.drecon = self.drecon.body.data_ptr() if (self.drecon is not None and with_drecon) else None
        e.D, e.dist, e.scale, e.rescale, e.coef, e.n_classes = c.D, Lb.DIST[c.dist], c.scale, c.rescale, self.coef, c.C

    def collect(self):
        c = self.case
        gs = [g for g in (self.recon, self.x, self.rows, self.drecon) if g is not None]
        return dict(rows=None if self.rows is None else self.rows.cpu(c.K, c.B),
                    drecon=None if self.drecon is None else self.drecon.cpu(c.K, c.B, c.D), guards=all(g.intact() for g in gs))


def hip_launch(case, recon, x, mask, rowcoef, drecon, coef, via):
    """One descriptor launched alone.  via = "fwd": mvk_recon_nll_fwd (with drecon: the fused gradient; a case whose drecon is
    misaligned runs the forward with drecon = NULL and then mvk_recon_nll_bwd); via = "bwd": mvk_recon_nll_bwd with rows = NULL."""
    Lb = _lib()
    p = Prepared(case, recon, x, mask, rowcoef, drecon, coef, via)
    desc = (Lb.ReconDesc * 1)()
    two_pass = case.misalign == "drecon" and drecon
    if via == "fwd":
        p.fill(desc[0], with_drecon=not two_pass)
        Lb.call("mvk_recon_nll_fwd", desc, 1, case.K, case.B, Lb.stream_ptr())
    if via == "bwd" or two_pass:
        p.fill(desc[0], with_rows=False)
        Lb.call("mvk_recon_nll_bwd", desc, 1, case.K, case.B, Lb.stream_ptr())
    torch.cuda.synchronize()
    return p.collect()


# ---- the comparison routine (also run on the CPU by tests/test_nll_ref_host.py with a stand-in launcher) --------------------------------
def check_case(case, launch, measured=None):
    """Everything that is asserted about one case; `launch` has the signature of hip_launch.  -> {stage: |err| / base}."""
    inp = R.make_inputs(case)
    recon, x, mask, rowcoef = inp["recon"], inp["x"], inp["mask"], inp["rowcoef"]
    K, B, D = case.K, case.B, case.D
    args = (case, recon, x, mask, rowcoef, case.drecon, case.coef)
    got = launch(*args, "fwd")
    ref, base = R.reference(case, inp), R.bases(case, inp)
    # 1. every entry; nothing left unwritten; nothing written outside
    assert got["guards"], f"{case.name}: a sentinel next to a buffer was overwritten"
    assert (got["drecon"] is not None) == case.drecon
    for k in ("rows", "drecon"):
        if got[k] is not None:
            assert not bool(torch.isnan(got[k]).any()), f"{case.name}: {k} holds a NaN: an entry the kernel did not write"
    ratios = R.ratios(case, got, ref, base)
    print(case.name, {k: round(v, 3) for k, v in ratios.items()})
    for k, v in ratios.items():
        if measured is not None and v > measured.get(k, (-1.0, ""))[0]:
            measured[k] = (v, case.name)
    for k, v in ratios.items():
        assert v <= R.C_STAGE[k], f"{case.name}: {k} worst |err| / base = {v:.3g} > C = {R.C_STAGE[k]}"
    # 2. exact properties
    if case.drecon and mask is not None:
        assert bool((got["drecon"][:, ~mask] == 0).all()), f"{case.name}: gradient on a masked-out row"
    if case.drecon and case.dist == "laplace":
        tie = recon == x.unsqueeze(0)
        assert bool(tie.any()) and bool((got["drecon"][tie] == 0).all()), f"{case.name}: gradient at a tie recon == x"
    gen = torch.Generator().manual_seed(K * 1000 + B)
    other_mask = None if mask is not None else torch.rand(B, generator=gen) > 0.5
    other_rc = None if rowcoef is not None else torch.randn(K, B, generator=gen)
    tog = launch(case, recon, x, other_mask, other_rc, not case.drecon, R.f32(case.coef * 0.77 + 0.1), "fwd")
    assert tog["guards"] and same_bits(got["rows"], tog["rows"]), f"{case.name}: rows change with mask / rowcoef / drecon / coef"
    if mask is None or rowcoef is None:
        one = launch(case, recon, x, torch.ones(B, dtype=torch.bool) if mask is None else mask,
                     torch.ones(K, B) if rowcoef is None else rowcoef, case.drecon, case.coef, "fwd")
        assert one["guards"] and same_bits(got["rows"], one["rows"])
        if case.drecon:
            assert same_bits(got["drecon"], one["drecon"]), f"{case.name}: NULL mask / rowcoef differ from explicit ones"
    if case.drecon:
        sec = launch(*args, "bwd")
        assert sec["guards"] and sec["rows"] is None
        assert same_bits(got["drecon"], sec["drecon"]), f"{case.name}: fused and second-pass gradients differ in their bits"
    # 3. determinism
    again = launch(*args, "fwd")
    assert same_bits(got["rows"], again["rows"]) and (not case.drecon or same_bits(got["drecon"], again["drecon"]))
    return ratios


@pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
def test_case(case):
    check_case(case, hip_launch, MEASURED)


def test_one_launch_of_eight():
    """n_mod = MVK_MAX_MODALITIES in one call: 4 descriptors in the Normal / Laplace float4 group, 2 in the scalar group, 1 in
    the Bernoulli float4 group, 1 categorical; every output has the bits of the same descriptor launched alone."""
    Lb = _lib()
    cases = R.ONE_LAUNCH
    assert len(cases) == Lb.MAX_MODALITIES and len({(c.K, c.B) for c in cases}) == 1
    K, B = cases[0].K, cases[0].B
    preps, alone = [], []
    desc = (Lb.ReconDesc * len(cases))()
    for i, c in enumerate(cases):
        inp = R.make_inputs(c)
        a = (c, inp["recon"], inp["x"], inp["mask"], inp["rowcoef"], c.drecon, c.coef, "fwd")
        alone.append(hip_launch(*a))
        preps.append(Prepared(*a))
        preps[-1].fill(desc[i])
    Lb.call("mvk_recon_nll_fwd", desc, len(cases), K, B, Lb.stream_ptr())
    torch.cuda.synchronize()
    for c, p, a in zip(cases, preps, alone):
        got = p.collect()
        assert got["guards"], c.name
        assert same_bits(got["rows"], a["rows"]), f"{c.name}: rows differ from the descriptor launched alone"
        assert (got["drecon"] is None) == (a["drecon"] is None)
        if got["drecon"] is not None:
            assert same_bits(got["drecon"], a["drecon"]), f"{c.name}: drecon differs from the descriptor launched alone"
    # the second pass over the descriptors that take a gradient, again in one call
    sub = [(c, a) for c, a in zip(cases, alone) if c.drecon]
    desc2 = (Lb.ReconDesc * len(sub))()
    preps2 = []
    for i, (c, _) in enumerate(sub):
        inp = R.make_inputs(c)
        preps2.append(Prepared(c, inp["recon"], inp["x"], inp["mask"], inp["rowcoef"], True, c.coef, "bwd"))
        preps2[-1].fill(desc2[i])
    Lb.call("mvk_recon_nll_bwd", desc2, len(sub), K, B, Lb.stream_ptr())
    torch.cuda.synchronize()
    for (c, a), p in zip(sub, preps2):
        got = p.collect()
        assert got["guards"] and same_bits(got["drecon"], a["drecon"]), f"{c.name}: second pass in one call"


def test_argument_checks():
    """Every MVK_EINVAL branch of launch_recon: descs NULL; n_mod 0 or 9; K 0; B -1; recon or x NULL; D 0; forward without rows;
    backward without drecon; dist -1 or 4; categorical with n_classes 0 or D % n_classes != 0 -- also as the LAST of two
    descriptors, whose valid first one must not have been launched.  The validation loop of launch_recon returns before the
    first hipLaunchKernelGGL, so these calls launch nothing: the NaN-filled outputs stay as they are.  B = 0 is MVK_OK and writes
    nothing either."""
    Lb = _lib()
    sp = Lb.stream_ptr
    K, B, D = 2, 3, 8
    src = Guarded(K * B * D, fill=0.5)
    rows, drecon = Guarded(K * B), Guarded(K * B * D)

    def make(n=1, bad=None, **kw):
        desc = (Lb.ReconDesc * n)()
        for i in range(n):
            e = desc[i]
            e.recon, e.x, e.rows, e.drecon = (src.body.data_ptr(), src.body.data_ptr(), rows.body.data_ptr(),
                                              drecon.body.data_ptr())
            e.mask = e.rowcoef = None
            e.D, e.dist, e.scale, e.rescale, e.coef, e.n_classes = D, 0, 1.0, 1.0, 1.0, 0
        for k, v in kw.items():
            setattr(desc[n - 1 if bad is None else bad], k, v)
        return desc

    def rc(fn, desc, n, k=K, b=B):
        return getattr(Lb.load(), fn)(desc, n, k, b, sp())

    f, bw = "mvk_recon_nll_fwd", "mvk_recon_nll_bwd"
    bad = []
    for fn in (f, bw):
        bad += [(fn, None, 1, K, B), (fn, make(), 0, K, B), (fn, make(9), 9, K, B), (fn, make(), 1, 0, B), (fn, make(), 1, K, -1)]
        for n in (1, 2):
            bad += [(fn, make(n, recon=None), n, K, B), (fn, make(n, x=None), n, K, B), (fn, make(n, D=0), n, K, B),
                    (fn, make(n, dist=-1), n, K, B), (fn, make(n, dist=4), n, K, B),
                    (fn, make(n, dist=3, n_classes=0), n, K, B), (fn, make(n, dist=3, n_classes=3), n, K, B)]
    bad += [(f, make(rows=None), 1, K, B), (f, make(2, rows=None), 2, K, B), (bw, make(drecon=None), 1, K, B),
            (bw, make(2, drecon=None), 2, K, B)]
    for i, (fn, desc, n, k, b) in enumerate(bad):
        assert rc(fn, desc, n, k, b) == EINVAL, f"bad call {i} ({fn}) was accepted"
    assert rc(f, make(), 1, K, 0) == 0 and rc(bw, make(2), 2, K, 0) == 0
    assert rc(f, make(8), 8, K, 0) == 0  # n_mod = MVK_MAX_MODALITIES itself is accepted
    torch.cuda.synchronize()
    assert bool(torch.isnan(rows.body).all()) and bool(torch.isnan(drecon.body).all())
    assert rows.intact() and drecon.intact() and src.intact()


# ---- mvk_loss_backward_seed / mvk_scale_by_device_scalar ----------------------------------------------------------------------------------
SEED_LENGTHS = [1, 255, 256, 257, 4096 * 256 + 3]  # the last: beyond the grid cap of 4096 blocks (the grid-stride loop runs twice)


def _seed_jobs(n_jobs):
    """(length, coef, fill) of up to 12 jobs: every length with fill 0 and nonzero."""
    jobs = []
    for i in range(n_jobs):
        jobs.append((SEED_LENGTHS[i % len(SEED_LENGTHS)], R.f32(0.3 + 0.7 * i), (i % len(SEED_LENGTHS) + i // len(SEED_LENGTHS)) % 2))
    return jobs


@pytest.mark.parametrize("gscale", [1.0, 0.37])
@pytest.mark.parametrize("n_jobs", [1, 12])
def test_loss_backward_seed(gscale, n_jobs):
    """buf = float32(gscale * coef) where fill != 0, buf *= gscale where fill == 0: one rounding each, so |got - ref| <= u |ref|
    against float64 (+ TINY for a flushed subnormal); with gscale == 1 the fill == 0 buffers keep their bits and the fill != 0
    buffers hold float32(coef) exactly."""
    Lb = _lib()
    gs = torch.tensor([gscale], dtype=torch.float32, device=dev())
    g32 = float(gs.cpu()[0])
    jobs = _seed_jobs(n_jobs)
    assert {j[2] for j in jobs} == ({0, 1} if n_jobs > 1 else {0})
    gen = torch.Generator().manual_seed(n_jobs)
    srcs = [torch.randn(n, generator=gen) * 10.0 ** float(torch.randint(-3, 4, (1,), generator=gen)) for n, _, _ in jobs]
    bufs = [Guarded(n, src=s) for (n, _, _), s in zip(jobs, srcs)]
    desc = (Lb.SeedDesc * n_jobs)()
    for e, b, (n, coef, fill) in zip(desc, bufs, jobs):
        e.buf, e.n, e.coef, e.fill = b.body.data_ptr(), n, coef, fill
    Lb.call("mvk_loss_backward_seed", desc, n_jobs, Lb.ptr(gs), Lb.stream_ptr())
    torch.cuda.synchronize()
    for b, s, (n, coef, fill) in zip(bufs, srcs, jobs):
        got = b.cpu(n)
        assert b.intact(), f"job of length {n}: sentinel overwritten"
        ref = torch.full((n,), g32 * coef, dtype=torch.float64) if fill else s.double() * g32
        r = R.worst_ratio(got, ref, R.U * ref.abs() + R.TINY)
        assert r <= 1.0, f"length {n} fill {fill}: {r:.3g} roundings"
        if gscale == 1.0:
            assert same_bits(got, torch.full((n,), coef) if fill else s), f"length {n} fill {fill}: bits change at gscale 1"


@pytest.mark.parametrize("gscale", [1.0, 0.37])
def test_scale_by_device_scalar(gscale):
    Lb = _lib()
    gs = torch.tensor([gscale], dtype=torch.float32, device=dev())
    g32 = float(gs.cpu()[0])
    gen = torch.Generator().manual_seed(7)
    for n in SEED_LENGTHS:
        s = torch.randn(n, generator=gen)
        b = Guarded(n, src=s)
        Lb.call("mvk_scale_by_device_scalar", Lb.ptr(b.body), n, Lb.ptr(gs), Lb.stream_ptr())
        torch.cuda.synchronize()
        got = b.cpu(n)
        assert b.intact()
        ref = s.double() * g32
        assert R.worst_ratio(got, ref, R.U * ref.abs() + R.TINY) <= 1.0
        if gscale == 1.0:
            assert same_bits(got, s)


def test_seed_argument_checks():
    """n = 0 and n = MVK_SEED_MAX + 1 are MVK_EINVAL (as are NULL jobs, NULL gscale, a NULL buffer, a negative length) and launch
    nothing; n = 12 with empty buffers and a zero-length scale are MVK_OK."""
    Lb = _lib()
    lib, sp = Lb.load(), Lb.stream_ptr
    gs = torch.tensor([0.5], dtype=torch.float32, device=dev())
    b = Guarded(16, fill=3.0)

    def jobs(n, length=16, buf=True):
        d = (Lb.SeedDesc * max(n, 1))()
        for e in d:
            e.buf, e.n, e.coef, e.fill = (b.body.data_ptr() if buf else None), length, 2.0, 1
        return d

    assert lib.mvk_loss_backward_seed(jobs(1), 0, Lb.ptr(gs), sp()) == EINVAL
    assert lib.mvk_loss_backward_seed(jobs(13), 13, Lb.ptr(gs), sp()) == EINVAL
    assert lib.mvk_loss_backward_seed(None, 1, Lb.ptr(gs), sp()) == EINVAL
    assert lib.mvk_loss_backward_seed(jobs(1), 1, None, sp()) == EINVAL
    assert lib.mvk_loss_backward_seed(jobs(2, buf=False), 2, Lb.ptr(gs), sp()) == EINVAL
    assert lib.mvk_loss_backward_seed(jobs(2, length=-1), 2, Lb.ptr(gs), sp()) == EINVAL
    assert lib.mvk_loss_backward_seed(jobs(12, length=0), 12, Lb.ptr(gs), sp()) == 0
    assert lib.mvk_scale_by_device_scalar(None, 4, Lb.ptr(gs), sp()) == EINVAL
    assert lib.mvk_scale_by_device_scalar(Lb.ptr(b.body), 4, None, sp()) == EINVAL
    assert lib.mvk_scale_by_device_scalar(Lb.ptr(b.body), 0, Lb.ptr(gs), sp()) == 0
    torch.cuda.synchronize()
    assert bool((b.body == 3.0).all()) and b.intact()


def test_zz_report():
    """Prints the head-room the HIP kernels showed in this session (the largest |err| / base per stage, with the case) and the
    wall time of this file."""
    print("HIP_MEASURED", {k: (round(v, 2), n) for k, (v, n) in sorted(MEASURED.items())})
    print(f"WALL test_gpu_recon_nll.py {time.time() - _T0:.1f} s")
