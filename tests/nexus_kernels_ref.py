"""Float64 references, the float32 model of forced perceptual dropout (FPD), case tables, error model and reference mutations for
the kernels of csrc/nexus.hip (mvk_nexus_aggregate_fwd/bwd, mvk_nexus_top_nll_fwd/bwd), written from the formulas of
include/mvk.h.  Used by tests/test_gpu_nexus_kernels.py (HIP) and tests/test_nexus_kernels_ref_host.py (CPU).

Stages, one function each: keep set (`keep_set`, `fpd_keep`), `agg`, `dmsgs`, `q`, `s2`, `rows`, `c_m`, `dr`.  C_m is no output of
its own: the stage is what the partial sums the backward pass leaves in `work` ([m][block of 256 rows]) add up to.

Error model: |got - ref| <= C_STAGE[stage] * U * base + SUB per entry, U = 2^-24, base = the sum of the magnitudes of the terms
that enter the entry (below, per stage), SUB = 2^-126 (a result below the smallest normal number may be flushed).  Later stages
are checked against the reference evaluated on the float32 arrays the kernel produced itself (s2 from q; rows and dr from q and
s2), so the bound of a stage holds the roundings of that stage alone and no entry is excluded; `*.e2e` stages repeat the
comparison from the inputs with the constants of the stages in between added up.
"""
import math
from dataclasses import dataclass

import numpy as np
import torch

F64 = torch.float64
U = 2.0 ** -24
SUB = 2.0 ** -126
LOG_2PI = math.log(2 * math.pi)
MAXM = 8  # MVK_MAX_MODALITIES

# C = 4x the largest |err| / base of the plain-torch-fp32 stand-in over the case table on the CPU, rounded up
# (tests/test_nexus_kernels_ref_host.py::test_error_constants), or `derived` from the count of roundings:
#   dmsgs  one division: 1.
#   dr     term of C_m: D/(2 s2) (1), s2 s2 (1), q / . (1), the difference (1), times g (1) = 5 relative to the magnitudes;
#          the sum: 8 levels of the LDS tree, up to 2 trips of the partial loop, 8 levels again = 18; 2 C / (B D): 3;
#          g / s2 (1), the sum of the two (1), z - r (1), two products (2): 32 in all, first order.
#   *.e2e  the staged constant plus those of the stages in between: s2.e2e = s2 + q; rows.e2e = rows + q + 2 s2.e2e (s2 enters
#          q / (2 s2) and D/2 ln s2, whose absolute error D/2 d s2 / s2 the D/2 ln 2 pi term of the base carries);
#          dr.e2e = dr + q + 3 s2.e2e (1 / s2 and 1 / s2^2).
C_STAGE = {"agg": 9, "dmsgs": 1, "q": 16, "s2": 10, "rows": 10, "c_m": 3, "dr": 32}
DERIVED = {"dmsgs", "dr", "s2.e2e", "rows.e2e", "dr.e2e"}
C_STAGE["s2.e2e"] = C_STAGE["s2"] + C_STAGE["q"]
C_STAGE["rows.e2e"] = C_STAGE["rows"] + C_STAGE["q"] + 2 * C_STAGE["s2.e2e"]
C_STAGE["dr.e2e"] = C_STAGE["dr"] + C_STAGE["q"] + 3 * C_STAGE["s2.e2e"]
MEASURED_STAGES = sorted(set(C_STAGE) - DERIVED)


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- comparison -------------------------------------------------------------------------------------------------------------------------
def klass(t):
    """0 finite, 1 NaN, 2 +inf, 3 -inf."""
    t = t.double()
    return torch.isnan(t) * 1 + (t == math.inf) * 2 + (t == -math.inf) * 3


def worst_ratio(got, ref, bound):
    """max over ALL entries of |got - ref| / bound; an entry whose reference is not finite must be of the same non-finite class
    (ratio 0) and a non-finite entry where the reference is finite counts as infinitely wrong."""
    got, ref, bound = got.double().reshape(-1), ref.double().reshape(-1), bound.double().reshape(-1)
    assert got.shape == ref.shape == bound.shape and got.numel() > 0
    fin = torch.isfinite(ref)
    r = torch.where(fin, (got - ref).abs() / bound, torch.where(klass(got) == klass(ref), 0.0, math.inf).double())
    r = torch.where(fin & ~torch.isfinite(got), torch.full_like(r, math.inf), r)
    return float(r.max())


# ---- keep set -----------------------------------------------------------------------------------------------------------------------------
def fpd_keep(u, p, M, mut=()):
    """The float32 model of nexus_keep's FPD branch.  u [B, M + 1] float32 (numpy), p the drop probability (rounded to float32 as
    the C ABI does).  Row b is dropped when u0 < p (and M > 1); then size = 1 + floorf(u1 * float(M - 1)) clamped to [1, M - 1]
    and the kept modalities are the first `size` of a partial Fisher-Yates shuffle, j = i + floorf(u[2 + i] * float(M - i))
    clamped to M - 1.  `fpd_keep64` evaluates the same formula without the float32 rounding of the products."""
    return _fpd(u, p, M, np.float32, mut)


def fpd_keep64(u, p, M):
    return _fpd(u, p, M, np.float64, ())


def _fpd(u, p, M, ft, mut):
    u = np.asarray(u, dtype=np.float32)
    B = u.shape[0]
    keep = np.ones((B, M), dtype=np.float32)
    p = np.float32(p)
    if M < 2:
        return keep
    for b in range(B):
        ub = u[b]
        drop = ub[0] <= p if "u0_le_p" in mut else ub[0] < p
        if not drop:
            continue
        size = 1 + int(np.floor(ft(ub[1]) * ft(M - 1)))
        size = min(max(size, 1), M - 1)
        perm = list(range(M))
        for i in range(size):
            j = min(i + int(np.floor(ft(ub[2 + i]) * ft(M - i))), M - 1)
            if "no_swap" in mut:
                perm[i] = perm[j]
            else:
                perm[i], perm[j] = perm[j], perm[i]
        keep[b] = 0.0
        for i in range(size):
            keep[b, perm[i]] = 1.0
    return keep


def keep_set(M, B, keep_in=None, masks=None, u=None, p=0.0, mut=()):
    """The keep matrix [B, M] of 0. / 1., by the precedence keep_in over masks over u; nothing given keeps everything."""
    if keep_in is not None:
        return (keep_in != 0).float()
    if masks is not None:
        return torch.stack([m.bool() for m in masks], 1).float()
    if u is not None:
        return torch.from_numpy(fpd_keep(u.numpy(), p, M, mut))
    return torch.ones(B, M)


# ---- aggregation ----------------------------------------------------------------------------------------------------------------------------
def agg(msgs, keep, mut=()):
    """agg [B, D] = sum_m keep msg_m / count (0 for a row with nothing kept) and its base sum_m keep |msg_m| / count."""
    m64 = torch.stack([t.double() for t in msgs], 1)  # [B, M, D]
    k = keep.double()[:, :, None]
    cnt = k.sum(1)
    den = torch.full_like(cnt, float(len(msgs))) if "mean_over_M" in mut else cnt
    inv = torch.where(cnt > 0, 1.0 / den.clamp_min(1), torch.zeros_like(cnt))
    return (m64 * k).sum(1) * inv, (m64.abs() * k).sum(1) * inv


def dmsgs(keep, g, mut=()):
    """d msg_m [M, B, D] = keep / count * g and its base |.|."""
    k = keep.double().t()[:, :, None]  # [M, B, 1]
    cnt = k.sum(0, keepdim=True)
    den = torch.full_like(cnt, float(keep.shape[1])) if "mean_over_M" in mut else cnt
    out = torch.where(cnt > 0, k / den.clamp_min(1), torch.zeros_like(k)) * g.double()[None]
    return out, out.abs()


# ---- top-level likelihood ---------------------------------------------------------------------------------------------------------------------
def q_rows(z, r):
    """q [B] = sum_d (z - r)^2; every term is positive: base = q."""
    q = ((z.double() - r.double()) ** 2).sum(1)
    return q, q


def s2_of(q, D, adapt, mask=None, mut=()):
    """s2 = mean over the WHOLE [B, D] block (masked rows included) of (z - r)^2 when adapted, else 1."""
    if not adapt:
        return torch.ones((), dtype=F64)
    q = q.double()
    if "s2_unmasked_only" in mut and mask is not None:
        return (q * mask.double()).sum() / (mask.double().sum() * D)
    return q.sum() / (q.numel() * D)


def rows_of(q, s2, D, gamma, mask=None):
    """rows [B] = gamma mask (q / (2 s2) + D/2 ln s2 + D/2 ln 2 pi) and its base."""
    q, s2 = q.double(), s2.double()
    w = gamma * (torch.ones_like(q) if mask is None else mask.double())
    ls = torch.log(s2)
    return w * (q / (2 * s2) + 0.5 * D * ls + 0.5 * D * LOG_2PI), gamma * (q / (2 * s2) + 0.5 * D * (ls.abs() + LOG_2PI))


def c_m(q, s2, D, g, mask=None):
    """C_m = sum_b g_b mask_b (D / (2 s2) - q_b / (2 s2^2)) and the sum of the magnitudes sum_b |g_b| mask_b (D / (2 s2) + q_b / (2 s2^2))
    (with an all-ones g and no mask C_m is 0 in real arithmetic: only the second can bound what fp32 leaves of it)."""
    q, s2 = q.double(), s2.double()
    gm = g.double() * (1.0 if mask is None else mask.double())
    return (gm * (0.5 * D / s2 - 0.5 * q / s2 ** 2)).sum(), (gm.abs() * (0.5 * D / s2 + 0.5 * q / s2 ** 2)).sum()


def dr_of(z, r, q, s2, gamma, adapt, g=None, mask=None, mut=()):
    """dr [B, D] = -gamma (z - r) (g_b mask_b / s2 + 2 C_m / (B D)) (the second term for an adapted modality only; g = None is
    a NULL grows[m]: zero) and its base gamma |z - r| (|g_b| mask_b / s2 + 2 sum|.| / (B D))."""
    e = z.double() - r.double()
    B, D = e.shape
    s2 = s2.double()
    g = torch.zeros(B, dtype=F64) if g is None else g.double()
    gm = g * (1.0 if mask is None else mask.double())
    C, S = c_m(q, s2, D, g, mask) if adapt else (torch.zeros((), dtype=F64), torch.zeros((), dtype=F64))
    if "no_cterm" in mut:
        C = torch.zeros((), dtype=F64)
    return -gamma * e * (gm / s2 + 2 * C / (B * D))[:, None], gamma * e.abs() * (gm.abs() / s2 + 2 * S / (B * D))[:, None]


def top_fp32(z, r, D, gamma, adapt, mask, g, q=None, s2=None):
    """The formulas of the two entries in plain torch float32 in the kernels' operation order (sums by torch.sum; the backward
    pass on the given q and s2 when given): the stand-in backend of the CPU twin and, for the s2 = 0 case, the evaluation whose
    non-finite classes the kernel must reproduce.  cpart: the sums of the terms of C_m over blocks of 256 rows."""
    f = torch.float32
    t = lambda v: torch.tensor(float(v), dtype=f)  # noqa: E731
    e = z - r
    B = z.shape[0]
    n = t(B) * t(D)
    q = (e * e).sum(1) if q is None else q
    if s2 is None:
        s2 = q.sum() / n if adapt else torch.ones((), dtype=f)
    half_log = 0.5 * t(D) * (torch.log(s2) + t(1.8378770664093453))
    inv = 0.5 / s2
    w = torch.full((B,), gamma, dtype=f) if mask is None else torch.where(mask.bool(), t(gamma), t(0))
    rows = w * (q * inv + half_log)
    gm = torch.zeros(B, dtype=f) if g is None else (g if mask is None else torch.where(mask.bool(), g, t(0)))
    cterm, cpart = t(0), torch.zeros((B + 255) // 256, dtype=f)
    if adapt:
        c = torch.zeros(B, dtype=f) if g is None else gm * (0.5 * t(D) / s2 - 0.5 * q / (s2 * s2))
        if g is not None and mask is not None:
            c = torch.where(mask.bool(), c, t(0))
        cpart = torch.cat([c, torch.zeros(-B % 256, dtype=f)]).reshape(-1, 256).sum(1)
        cterm = 2.0 * cpart.sum() / n
    dr = -t(gamma) * e * (gm / s2 + cterm)[:, None]
    return dict(q=q, s2=s2, rows=rows, dr=dr, cpart=cpart)


# ---- case tables ------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class AggCase:
    name: str
    why: str
    M: int
    B: int
    D: int
    src: tuple  # the keep sources handed to the entry, of "keep_in", "masks", "u"
    p: float = 0.0
    odd: bool = False  # keep_in values 0.5, -3 and a subnormal for "kept"
    seed: int = 0


AGG_CASES = [
    AggCase("agg-keepin-m3-b37-d70", "base case; row 0 keeps nothing (message and gradient exactly 0), row 1 one modality (5)", 3, 37, 70, ("keep_in",)),
    AggCase("agg-keepin-odd-m3-b9-d5", "keep_in of 0.5, -3 and a subnormal normalise to 1 (5)", 3, 9, 5, ("keep_in",), odd=True),
    AggCase("agg-all-three-m3-b37-d7", "keep_in, masks and u all given: keep_in wins (5)", 3, 37, 7, ("keep_in", "masks", "u"), p=1.0),
    AggCase("agg-masks-u-m3-b37-d7", "masks and u given: masks win over a certain FPD drop (5)", 3, 37, 7, ("masks", "u"), p=1.0),
    AggCase("agg-masks-m4-b5-d64", "dataset masks; B = 5: the second workgroup holds one row (7)", 4, 5, 64, ("masks",)),
    AggCase("agg-none-m2-b4-d63", "all three NULL keep everything; B = 4 fills one workgroup, D = 63 (7)", 2, 4, 63, ()),
    AggCase("agg-u-m1-b9-d3", "M = 1 with u and p = 1: never dropped (5)", 1, 9, 3, ("u",), p=1.0),
    AggCase("agg-u-m8-b37-d5", "M = 8: the lane < M write of keep_out at its widest; FPD (5, 6)", 8, 37, 5, ("u",), p=0.6),
    AggCase("agg-u-m5-b1-d1", "B = 1, D = 1 (7)", 5, 1, 1, ("u",), p=1.0),
    AggCase("agg-u-m3-b3-d65", "B = 3, D = 65: a second trip of the lane loop for one lane (7)", 3, 3, 65, ("u",), p=0.5),
    AggCase("agg-keepin-m8-b5-d130", "M = 8, D = 130: three trips (5, 7)", 8, 5, 130, ("keep_in",)),
    AggCase("agg-u-p0-m3-b300-d2", "p = 0: nothing is ever dropped; 75 workgroups (6)", 3, 300, 2, ("u",), p=0.0),
]
AGG_BY_NAME = {c.name: c for c in AGG_CASES}


def agg_inputs(case):
    g = gen(100 + AGG_CASES.index(case))
    M, B, D = case.M, case.B, case.D
    inp = dict(msgs=[torch.randn(B, D, generator=g) for _ in range(M)], gout=torch.randn(B, D, generator=g), keep_in=None, masks=None, u=None)
    k = (torch.rand(B, M, generator=g) > 0.4).float()
    k[0] = 0.0
    if B > 1:
        k[1] = 0.0
        k[1, M // 2] = 1.0
    if "keep_in" in case.src:
        inp["keep_in"] = k.clone()
        if case.odd:
            odd = torch.tensor([0.5, -3.0, 1e-40])
            inp["keep_in"] = torch.where(k != 0, odd[torch.arange(B * M).reshape(B, M) % 3], torch.zeros(()))
            assert bool((inp["keep_in"][k != 0] != 0).all())
    if "masks" in case.src:
        km = (torch.rand(B, M, generator=g) > 0.5) if "keep_in" in case.src else k.bool()
        inp["masks"] = [km[:, m].contiguous() for m in range(M)]
    if "u" in case.src:
        inp["u"] = torch.rand(B, M + 1, generator=g)
    return inp


@dataclass(frozen=True)
class TopCase:
    name: str
    why: str
    B: int
    dims: tuple
    adapt: tuple
    g: str = "randn"  # rows' gradient: "ones", "sign", "randn"
    masks: tuple = ()  # per modality the kept fraction, None for a NULL entry; () for a NULL array
    gnull: tuple = ()  # modalities whose grows[m] is NULL
    zero: tuple = ()  # modalities with z == r ("eq") or a difference whose square underflows ("tiny")
    e2e: bool = True
    gammas: tuple = (0.5, 2.0, 1.25, 1.0, 0.75, 3.0, 0.25, 1.5)  # exact in float32


TOP_CASES = [
    TopCase("top-ones-b300", "all-ones g, no mask: C_m is pure rounding residue (1)", 300, (5, 70, 3), (1, 1, 1), g="ones"),
    TopCase("top-sign-b300", "random-sign g: C_m cancels only partly (1)", 300, (5, 70, 3), (1, 1, 0), g="sign"),
    TopCase("top-maskmost-b300", "masks that remove 9 rows in 10; s2 still runs over every row (1)", 300, (5, 70, 3), (1, 1, 1), masks=(0.1, 0.1, 0.1)),
    TopCase("top-b1025", "forward nparts = 257: a second trip of the partial loop (2)", 1025, (3, 1), (1, 1)),
    TopCase("top-b2049", "forward nparts = 513: a third trip (2)", 2049, (2,), (1,), g="ones"),
    TopCase("top-b65537", "backward nparts = 257 > 256: a second trip in the backward pass (2)", 65537, (1, 2), (1, 1)),
    TopCase("top-narrow-adapted", "the grid is sized by D = 70, the adapted modality has D = 1 (3)", 37, (1, 70, 3), (1, 0, 0)),
    TopCase("top-wide-adapted", "only the widest modality is adapted (3)", 37, (1, 70, 3), (0, 1, 0), masks=(0.6, 0.6, 0.6)),
    TopCase("top-none-adapted", "no adapted modality: the first backward launch is skipped, work stays untouched (3)", 37, (1, 70, 3), (0, 0, 0)),
    TopCase("top-mixed-null", "masks[1] NULL in a given array; grows[0], grows[2] NULL: dr exactly 0 (4)", 37, (5, 70, 3), (1, 1, 0), masks=(0.7, None, 0.7), gnull=(0, 2)),
    TopCase("top-b1", "B = 1 over D in 1, 63, 64, 65, 130: three waves of the workgroup idle (7)", 1, (1, 63, 64, 65, 130), (1, 1, 0, 1, 1)),
    TopCase("top-b3", "B = 3 (7)", 3, (1, 63, 64, 65, 130), (1, 0, 1, 1, 1), masks=(0.5, None, 0.5, None, 0.5)),
    TopCase("top-b4", "B = 4 (7)", 4, (1, 63, 64, 65, 130), (0, 1, 1, 1, 0), g="sign"),
    TopCase("top-b5-m8", "B = 5: a second, partly empty workgroup feeds part; M = 8 (7)", 5, (1, 63, 64, 65, 130, 2, 7, 33), (1, 1, 1, 0, 1, 1, 0, 1)),
    TopCase("top-s2-zero", "z == r and a difference whose square underflows on adapted modalities: s2 = 0 (8)", 9, (4, 3, 5), (1, 1, 1), zero=("eq", "tiny", None), masks=(0.5, None, 0.5), e2e=False),
]
TOP_BY_NAME = {c.name: c for c in TOP_CASES}
NONFINITE_CASES = {"top-s2-zero"}


def top_inputs(case):
    g = gen(200 + TOP_CASES.index(case))
    B, M = case.B, len(case.dims)
    zs = [torch.randn(B, d, generator=g) for d in case.dims]
    rs = [z + 0.3 * torch.randn(z.shape, generator=g) for z in zs]
    for m, kind in enumerate(case.zero):
        if kind == "eq":
            rs[m] = zs[m].clone()
        elif kind == "tiny":
            zs[m] = torch.full_like(zs[m], 1e-25)
            rs[m] = torch.zeros_like(zs[m])
    masks = None
    if case.masks:
        masks = [None if f is None else (torch.rand(B, generator=g) < f) for f in case.masks]
        for mk in masks:
            if mk is not None:
                mk[0] = True  # never an empty mask
    if case.g == "ones":
        gr = [torch.ones(B) for _ in range(M)]
    elif case.g == "sign":
        gr = [torch.where(torch.rand(B, generator=g) < 0.5, -1.0, 1.0) for _ in range(M)]
    else:
        gr = [torch.randn(B, generator=g) for _ in range(M)]
    gr = [None if m in case.gnull else t for m, t in enumerate(gr)]
    return dict(z=zs, r=rs, masks=masks, g=gr, gamma=list(case.gammas[:M]))


# ---- crafted FPD rows ---------------------------------------------------------------------------------------------------------------------------
ONE_M = float(np.float32(1.0) - np.float32(2.0 ** -24))  # the largest float32 below 1


def fpd_crafted(M, p):
    """Rows of uniforms on the edges of nexus_keep for M modalities and drop probability p: u0 at p and its float32 neighbours,
    u1 at 0, 1 - 2^-24 and 1.0 (the size clamp), each shuffle uniform at 0, 1 - 2^-24 and 1.0 (the j clamp)."""
    pf = np.float32(p)
    rows = []
    base = np.full(M + 1, 0.37, dtype=np.float32)
    for u0 in (np.nextafter(pf, np.float32(-1)), pf, np.nextafter(pf, np.float32(2)), np.float32(0), np.float32(ONE_M)):
        row = base.copy()
        row[0] = u0
        rows.append(row)
    for u1 in (0.0, ONE_M, 1.0, 0.5):
        for us in (0.0, ONE_M, 1.0):
            for i in range(2, M + 1):
                row = base.copy()
                row[0], row[1], row[i] = 0.0, u1, us
                rows.append(row)
            row = base.copy()
            row[0], row[1] = 0.0, u1
            row[2:] = us
            rows.append(row)
    return np.stack(rows).astype(np.float32)


FPD_M = (2, 3, 5, 8)
FPD_P = (0.0, 0.3, 1.0)
FPD_RANDOM_ROWS = 3000


def fpd_random(M):
    return torch.rand(FPD_RANDOM_ROWS, M + 1, generator=gen(300 + M)).numpy()


# ---- reference mutations: (name, family, stages that must reject it, cases) ------------------------------------------------------------------------
TEETH = [
    ("s2_unmasked_only", "top", ("s2", "s2.e2e"), ("top-maskmost-b300", "top-wide-adapted")),
    ("no_cterm", "top", ("dr", "dr.e2e"), ("top-sign-b300", "top-maskmost-b300", "top-b65537")),
    ("mean_over_M", "agg", ("agg", "dmsgs"), ("agg-keepin-m3-b37-d70", "agg-masks-m4-b5-d64")),
    ("no_swap", "fpd", ("keep",), ("fpd-random-m3", "fpd-random-m5", "fpd-random-m8")),
    ("u0_le_p", "fpd", ("keep",), ("fpd-crafted-m2", "fpd-crafted-m3", "fpd-crafted-m8")),
]
