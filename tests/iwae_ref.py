"""Float64 references, case tables, error model and reference mutations for the importance-sampling entries of csrc/mmvae.hip
(mvk_iwae_sample, mvk_iwae_logw, mvk_iwae_reduce), written from the formulas of include/mvk.h.  Used by tests/test_gpu_iwae.py
(HIP) and tests/test_iwae_ref_host.py (CPU).

Stages, one function each: `z`, `lpz`, `lq_e`, `lqz`, `lw`, `ll`.  The entries write z, lw and ll; lpz, lq_e and lqz are the
intermediate stages of lw and supply its base.

Error model: |got - ref| <= C_STAGE[stage] * U * base + SUB per entry, U = 2^-24, SUB = 2^-126, base = the sum of the magnitudes of
the terms that enter the entry:
  z    |loc| + |sd t(noise)|
  lw   sum_r |rows_r| + T(prior) + sum_e w_e T(e) + |lqz| + ln E, with T(.) = sum_l (d^2 / (2 sd^2) + |ln sd| + ln sqrt(2 pi))
       (Laplace: |ln 2 sd| + |d| / sd) the magnitude sum of a log-density row and w_e the softmax weights of the experts
  ll   |m| + |ln s| + ln(n K) + 1 + sum_k w_k |lw_k - m|, m the column maximum, s = sum_k exp(lw_k - m), w_k = exp(lw_k - m) / s
lw is checked against the reference evaluated on the float32 z the sample entry produced (and ll on the float32 lw), so no entry
needs excluding; the end-to-end stages repeat the comparison from the inputs: a rounding of z moves a log-density term by its
derivative, which the bases below carry as T'(.) = sum_l |z| (|d| / sd^2) (Laplace: |z| / sd).
An entry whose reference is not finite must come out in the same non-finite class (NaN, +inf, -inf).
"""
import math
from dataclasses import dataclass

import torch

from nexus_kernels_ref import F64, SUB, U, gen, klass, worst_ratio  # noqa: F401  (one comparison routine for both families)

HALF_LOG_2PI = 0.5 * math.log(2 * math.pi)
FAMILY = {"normal": 0, "laplace": 1, "softplus": 2}  # MVK_FAMILY_NORMAL, _LAPLACE_SOFTMAX, _NORMAL_SOFTPLUS (scored as NORMAL)
MAXE = 32  # MVK_IWAE_MAX_EXPERTS

# C = 4x the largest |err| / base of the plain-torch-fp32 stand-in over the case table on the CPU, rounded up
# (tests/test_iwae_ref_host.py::test_error_constants); `derived`: lw.e2e = lw + z (one z rounding per term, through T').
C_STAGE = {"z": 7, "lw": 11, "ll": 5}
DERIVED = {"lw.e2e"}
C_STAGE["lw.e2e"] = C_STAGE["lw"] + C_STAGE["z"]
MEASURED_STAGES = sorted(set(C_STAGE) - DERIVED)


def is_laplace(family):
    return family == "laplace"


# ---- stages -------------------------------------------------------------------------------------------------------------------------------
def t_of(family, noise):
    n = noise.double()
    return -torch.sign(n) * torch.log1p(-n.abs()) if is_laplace(family) else n


def z_of(family, loc, sd, noise):
    """z [K, B, L] = loc + sd t(noise) and its base |loc| + |sd t|."""
    st = sd.double() * t_of(family, noise)
    return loc.double() + st, loc.double().abs() + st.abs()


def logp(family, z, loc, sd, zmag=None):
    """Log-density terms [..., L], the magnitude sum of each and the magnitude of its derivative times zmag (the base of z;
    |z| when not given)."""
    z, loc, sd = z.double(), loc.double(), sd.double()
    zmag = z.abs() if zmag is None else zmag.double()
    d = z - loc
    if is_laplace(family):
        return -torch.log(2 * sd) - d.abs() / sd, torch.log(2 * sd).abs() + d.abs() / sd, zmag / sd
    return (-(d * d) / (2 * sd * sd) - torch.log(sd) - HALF_LOG_2PI, (d * d) / (2 * sd * sd) + torch.log(sd).abs() + HALF_LOG_2PI,
            zmag * d.abs() / (sd * sd))


def lpz_of(family, z, prior_loc, prior_sd, mut=(), zmag=None):
    """lpz [K, B] = sum_l log p(z_l), the prior family(prior_loc or 0, prior_sd or 1)."""
    L = z.shape[-1]
    pl = torch.zeros(L, dtype=F64) if prior_loc is None or "prior_ignored" in mut else prior_loc.double()
    ps = torch.ones(L, dtype=F64) if prior_sd is None or "prior_ignored" in mut else prior_sd.double()
    v, T, Td = logp(family, z, pl, ps, zmag)
    return v.sum(-1), T.sum(-1), Td.sum(-1)


def lq_e_of(family, z, locs, sds, zmag=None):
    """lq [E, K, B] = sum_l log q_e(z_l) with the expert parameters [B, L] broadcast over K."""
    out = [logp(family, z, lo[None], sd[None], zmag) for lo, sd in zip(locs, sds)]
    return tuple(torch.stack([o[i].sum(-1) for o in out]) for i in range(3))


def lqz_of(lq, mut=()):
    """lqz [K, B] = logsumexp_e lq_e - ln E and the softmax weights of the experts (0 where the mixture is not finite)."""
    E = lq.shape[0]
    use = lq[1:] if "skip_expert" in mut and E > 1 else lq
    lse = torch.logsumexp(use, 0)
    lse = torch.where(torch.isnan(use).any(0), torch.full_like(lse, math.nan), lse)  # (a NaN expert: NaN, by definition)
    w = torch.nan_to_num(torch.exp(lq - torch.logsumexp(lq, 0)[None]), nan=0.0, posinf=0.0)  # (of the full mixture, whatever `mut`)
    return lse - (0.0 if "no_log_E" in mut else math.log(E)), w


def lw_of(family, z, rows, locs, sds, prior_loc, prior_sd, mut=(), zmag=None):
    """lw [K, B] = -sum_r rows_r + lpz - lqz with its base and the extra base of the end-to-end comparison (z rounded once, by
    U times its own base zmag)."""
    lpz, Tp, Tdp = lpz_of(family, z, prior_loc, prior_sd, mut, zmag)
    lq, Tq, Tdq = lq_e_of(family, z, locs, sds, zmag)
    lqz, w = lqz_of(lq, mut)
    lpx = -sum(r.double() for r in rows) if rows else torch.zeros_like(lpz)
    ra = sum(r.double().abs() for r in rows) if rows else torch.zeros_like(lpz)
    fin = lambda t: torch.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0)  # noqa: E731  (bases of non-finite entries are not used)
    base = ra + Tp + fin((w * fin(Tq)).sum(0)) + fin(lqz).abs() + math.log(len(locs))
    return lpx + lpz - lqz, base, Tdp + fin((w * fin(Tdq)).sum(0))


def ll_of(lws, mut=()):
    """ll [B] = logsumexp over the n arrays x K samples - ln(n K) and its base."""
    n, K = len(lws), lws[0].shape[0]
    x = torch.cat([t.double() for t in lws], 0)  # [n K, B]
    lse = torch.logsumexp(x, 0)
    lse = torch.where(torch.isnan(x).any(0), torch.full_like(lse, math.nan), lse)
    cnt = K if "log_K" in mut else n * K
    m = x.max(0).values
    fin = torch.isfinite(m)
    mm = torch.where(fin, m, torch.zeros_like(m))
    e = torch.exp(x - mm[None])
    s = e.sum(0)
    spread = torch.nan_to_num(e * (x - mm[None]).abs(), nan=0.0).sum(0) / s.clamp_min(1e-300)
    base = mm.abs() + torch.nan_to_num(torch.log(s), nan=0.0, posinf=0.0, neginf=0.0).abs() + math.log(n * K) + 1 + torch.nan_to_num(spread, posinf=0.0)
    return lse - math.log(cnt), base


# ---- the formulas in plain torch float32 (stand-in backend of the CPU twin) ----------------------------------------------------------------------
def t32(family, noise):
    return -torch.sign(noise) * torch.log1p(-noise.abs()) if is_laplace(family) else noise


def logp32(family, z, loc, sd):
    d = z - loc
    if is_laplace(family):
        return -torch.log(2.0 * sd) - d.abs() / sd
    return -(d * d) / (2.0 * sd * sd) - torch.log(sd) - torch.tensor(0.918938533204672742, dtype=torch.float32)


def seqsum(t):
    """Sum over the last axis in index order, as the one-thread-per-(k, b) kernel adds."""
    acc = torch.zeros(t.shape[:-1], dtype=t.dtype)
    for l in range(t.shape[-1]):
        acc = acc + t[..., l]
    return acc


def lw32(family, z, rows, locs, sds, prior_loc, prior_sd):
    L = z.shape[-1]
    f = torch.float32
    lpz = seqsum(logp32(family, z, torch.zeros(L, dtype=f) if prior_loc is None else prior_loc, torch.ones(L, dtype=f) if prior_sd is None else prior_sd))
    lq = torch.stack([seqsum(logp32(family, z, lo[None], sd[None])) for lo, sd in zip(locs, sds)])
    lse = torch.logsumexp(lq, 0)
    lse = torch.where(torch.isnan(lq).any(0), torch.full_like(lse, math.nan), lse)
    lqz = lse - torch.log(torch.tensor(float(len(locs)), dtype=f))
    lpx = torch.zeros_like(lpz)
    for r in rows:
        lpx = lpx - r
    return lpx + lpz - lqz


def ll32(lws):
    x = torch.cat(list(lws), 0)
    lse = torch.logsumexp(x, 0)
    lse = torch.where(torch.isnan(x).any(0), torch.full_like(lse, math.nan), lse)
    return lse - torch.log(torch.tensor(float(len(lws)), dtype=torch.float32) * torch.tensor(float(lws[0].shape[0]), dtype=torch.float32))


# ---- case tables ----------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    """One chain sample -> logw -> reduce."""
    name: str
    why: str
    family: str
    K: int
    B: int
    L: int
    E: int
    R: int
    prior: str = "none"  # "none", "loc", "sd", "both"
    noise: str = "plain"  # "plain", "edges": Laplace noise at 0, +-(1 - 2^-24), subnormals
    special: str = ""  # "nan": sd = 0 at z == loc for one expert of one row; "minf1": one expert at -inf; "minf": all of them
    finite: bool = True


CASES = [
    Case("iw-normal-k7-b5-l5-e1-r2", "base case, one expert", "normal", 7, 5, 5, 1, 2),
    Case("iw-normal-k33-b9-l20-e3-r2-both", "K B L = 5940, no multiple of 256: the i % BL broadcast (11); K B = 297 (12)", "normal", 33, 9, 20, 3, 2, "both"),
    Case("iw-laplace-k12-b4-l20-e2-r2-both", "Laplace with a prior", "laplace", 12, 4, 20, 2, 2, "both"),
    Case("iw-laplace-edges-k5-b3-l7-e2-r1", "Laplace noise at 0, +-(1 - 2^-24) and subnormal values (11)", "laplace", 5, 3, 7, 2, 1, "none", "edges"),
    Case("iw-softplus-k9-b4-l6-e2-r1-loc", "family 2 (NORMAL_SOFTPLUS) behaves as NORMAL in all three entries (11); prior_loc alone (12)", "softplus", 9, 4, 6, 2, 1, "loc"),
    Case("iw-normal-k3-b5-l1-e4-r0-sd", "L = 1, R = 0, prior_sd alone (12)", "normal", 3, 5, 1, 4, 0, "sd"),
    Case("iw-normal-k5-b3-l64-e2-r8", "L = 64, R = 8 likelihood rows (12)", "normal", 5, 3, 64, 2, 8),
    Case("iw-laplace-k3-b4-l130-e3-r1-sd", "L = 130; Laplace with prior_sd alone (12)", "laplace", 3, 4, 130, 3, 1, "sd"),
    Case("iw-normal-k2-b3-l3-e32-r0", "E = 32 = MVK_IWAE_MAX_EXPERTS (9)", "normal", 2, 3, 3, 32, 0),
    Case("iw-normal-k1000-b3-l8-e5-r2", "K = 1000: 16 trips of the reduce loop (10)", "normal", 1000, 3, 8, 5, 2),
    Case("iw-nan-expert-k4-b3-l5-e3-r1", "sd = 0 for expert 1 of row 1, z == loc at sample 2: NaN in, NaN out for the (k, b) of row 1 alone (9)", "normal", 4, 3, 5, 3, 1, special="nan", finite=False),
    Case("iw-nan-first-expert-k4-b3-l5-e3-r1", "the same with the NaN on the FIRST expert, while the running maximum is still -inf (9)", "normal", 4, 3, 5, 3, 1, special="nan0", finite=False),
    Case("iw-one-expert-minf-k4-b3-l5-e3-r1", "one expert at -inf (sd = inf): it drops out of the mixture, everything stays finite (9)", "normal", 4, 3, 5, 3, 1, special="minf1"),
    Case("iw-all-experts-minf-k4-b3-l5-e2-r1", "all experts of row 1 at -inf: lqz = -inf, lw = +inf, ll = +inf (9, 10)", "normal", 4, 3, 5, 2, 1, special="minf", finite=False),
]
BY_NAME = {c.name: c for c in CASES}


def make_inputs(case):
    g = gen(400 + CASES.index(case))
    K, B, L, E = case.K, case.B, case.L, case.E
    locs = [torch.randn(B, L, generator=g) for _ in range(E)]
    sds = [torch.rand(B, L, generator=g) * 0.8 + 0.3 for _ in range(E)]
    if is_laplace(case.family):
        noise = torch.rand(K, B, L, generator=g) * 1.98 - 0.99
        if case.noise == "edges":
            one_m = 1.0 - 2.0 ** -24
            edges = torch.tensor([0.0, -0.0, one_m, -one_m, 1e-40, -1e-40, 2.0 ** -126, -(2.0 ** -149)])
            noise.view(-1)[:2 * edges.numel()] = edges.repeat(2)
            locs[0].view(-1)[8:16] = 0.0  # z = sd t alone on the second copy of the edges
    else:
        noise = torch.randn(K, B, L, generator=g)
    rows = [torch.rand(K, B, generator=g) * 50 for _ in range(case.R)]
    ploc = torch.randn(L, generator=g) * 0.1 if case.prior in ("loc", "both") else None
    psd = torch.rand(L, generator=g) + 0.5 if case.prior in ("sd", "both") else None
    sloc, ssd = locs[0].clone(), sds[0].clone()  # the sampling distribution: expert 0 before the special entries below
    if case.special in ("nan", "nan0"):
        e = 1 if case.special == "nan" else 0
        sds[e][1, 2] = 0.0
        noise[2, 1, 2] = 0.0  # z[2, 1, 2] = sloc[1, 2] exactly: -0 / 0; the other samples of row 1: -inf + inf
        locs[e][1, 2] = sloc[1, 2]
    elif case.special == "minf1":
        sds[1][:, 0] = math.inf
    elif case.special == "minf":
        for e in range(E):
            sds[e][1, 0] = math.inf
    return dict(locs=locs, sds=sds, sloc=sloc, ssd=ssd, noise=noise, rows=rows, ploc=ploc, psd=psd)


@dataclass(frozen=True)
class ReduceCase:
    name: str
    why: str
    n: int
    K: int
    B: int
    kind: str = "plain"  # "plain"; "big": |lw| ~ 3e3 with a spread of ~100; "minf": column 0 all -inf; "pinf": a +inf entry; "nan": a NaN entry
    finite: bool = True


REDUCE_CASES = [ReduceCase(f"red-n{n}-k{K}-b{B}", f"K = {K}, B = {B}, n = {n} (10)", n, K, B)
                for n, K, B in ((1, 1, 1), (1, 63, 3), (2, 64, 4), (3, 65, 5), (1, 1000, 3), (8, 7, 5))]
REDUCE_CASES += [
    ReduceCase("red-big-n2-k65-b5", "|lw| around 3e3 with a spread of about 100 (10)", 2, 65, 5, "big"),
    ReduceCase("red-big-n1-k1000-b4", "the same over K = 1000 (10)", 1, 1000, 4, "big"),
    ReduceCase("red-minf-column-n2-k65-b5", "a column that is all -inf gives -inf, not NaN; single -inf entries elsewhere (10)", 2, 65, 5, "minf", False),
    ReduceCase("red-pinf-entry-n2-k65-b5", "a +inf entry gives +inf as torch.logsumexp does (10)", 2, 65, 5, "pinf", False),
    ReduceCase("red-nan-entry-n2-k65-b5", "a NaN entry gives NaN for that column alone, also next to -inf only (10)", 2, 65, 5, "nan", False),
]
REDUCE_BY_NAME = {c.name: c for c in REDUCE_CASES}


def reduce_inputs(case):
    g = gen(500 + REDUCE_CASES.index(case))
    lws = [torch.randn(case.K, case.B, generator=g) * 3 - 40 for _ in range(case.n)]
    if case.kind == "big":
        lws = [-3e3 + 100 * torch.rand(case.K, case.B, generator=g) * (1 if j % 2 == 0 else -1) for j in range(case.n)]
    if case.kind == "minf":
        for t in lws:
            t[:, 0] = -math.inf
        lws[0][3, 1] = -math.inf
        lws[-1][64, 2] = -math.inf
    if case.kind == "pinf":
        lws[-1][64, 1] = math.inf
        lws[0][0, 3] = math.inf
        lws[0][1, 3] = math.inf
    if case.kind == "nan":
        lws[-1][64, 1] = math.nan
        for t in lws:
            t[:, 3] = -math.inf
        lws[0][5, 3] = math.nan
        lws[0][0, 4] = math.inf
        lws[0][1, 4] = math.nan
    return lws


# ---- reference mutations: (name, stages that must reject it, cases) -------------------------------------------------------------------------------
TEETH = [
    ("no_log_E", ("lw",), ("iw-normal-k33-b9-l20-e3-r2-both", "iw-laplace-k12-b4-l20-e2-r2-both", "iw-normal-k5-b3-l64-e2-r8")),
    ("prior_ignored", ("lw",), ("iw-normal-k33-b9-l20-e3-r2-both", "iw-softplus-k9-b4-l6-e2-r1-loc", "iw-laplace-k3-b4-l130-e3-r1-sd")),
    ("skip_expert", ("lw",), ("iw-normal-k33-b9-l20-e3-r2-both", "iw-normal-k2-b3-l3-e32-r0", "iw-laplace-k3-b4-l130-e3-r1-sd")),
    ("log_K", ("ll",), ("red-n2-k64-b4", "red-n8-k7-b5", "red-big-n2-k65-b5")),
]
