"""Float64 torch reference of the reconstruction-likelihood kernels of csrc/elbo.hip (mvk_recon_nll_fwd / mvk_recon_nll_bwd: the
row kernel recon_nll_kernel in its three launch groups and the class-row kernel recon_categorical_kernel), written from the
formulas of oracle.elbo.recon_log_prob / _row_nll with the semantics of mvk_recon_desc; plus the case table, the seeded inputs
and the error model of tests/test_gpu_recon_nll.py.  CPU only: no GPU, no libmvk.so.  tests/test_nll_ref_host.py pins the
reference to oracle.elbo._row_nll evaluated in float64.

With recon [K,B,D], x [B,D] broadcast over K, d = recon - x, s = scale:
    normal      -log p = d^2 / (2 s^2) + log s + log(2 pi) / 2          d(-log p)/d recon = d / s^2
    laplace     -log p = |d| / s + log(2 s)                              sign(d) / s   (0 at a tie recon == x)
    bernoulli   -log p = max(r, 0) - r x + log1p(exp(-|r|))  (r = recon: logits)       sigmoid(r) - x
    categorical D = P positions of C classes, v = r + 1e-6:  -log p of a position = -(sum_c x_c v_c - lse(v) sum_c x_c)
                d / d r_c = softmax(v)_c sum_c' x_c' - x_c
    rows[k,b]     = rescale * sum_d -log p                                (the mask does NOT apply to rows)
    drecon[k,b,:] = coef * mask[b] * rowcoef[k,b] * rescale * d(-log p)/d recon      (mask, rowcoef: NULL = 1)
The reference is evaluated on the fp32 inputs (scale, rescale and coef as the fp32 values the C ABI carries); drecon is the
float64 autograd gradient of sum_kb rows[k,b] coef mask[b] rowcoef[k,b].

Error model (the form of tests/elbo_ref.py).  u = 2^-24.  Every output has a `base` of its own shape, computed in float64 from
the inputs: u times the sum of the absolute values of what is added or cancelled to form the entry plus u times the entry's
own magnitude.  Per element e (g = the entry of drecon, w = |coef mask rowcoef rescale|):
    normal      rows: (|r| + |x|) |d| / s^2 + |t|  (t = d^2 / 2 s^2)          drecon: w (|r| + |x|) / s^2 + |g|
    laplace     rows: (|r| + |x|) / s + |t|        (t = |d| / s)              drecon: |g|   (the sign of d is exact)
    bernoulli   rows: max(r, 0) + |r x| + log1p(e^-|r|) + |t|                 drecon: w (sig + |x|) + |g|
    categorical position p: EL = |lse| + |max v| + acc(C) + 2 + sum_c softmax_c (|v_c - max v| + |v_c|)  (the error of lse: fl(r +
                1e-6), the shifted exponentials, the wave sum of C addends, logf), then
                rows: EL sum|x| + (1 + acc(C)) sum|x v| + acc(C) |lse| sum|x| + |t_p|
                drecon: w (softmax_c |sum x| (|v_c| + |lse| + EL + 3 + acc(C)) + |x_c|) + |g|
A row gets rescale * (the sum of its per-element bases + acc(D) u sum|t|) + u |row| (categorical: acc(P) over the positions); a
Normal or Laplace row also u rescale D (|log s| + 0.919) (|log 2s| for Laplace) for the row constant, which is formed in fp32
as float(D) * (logf(s) + 0.9189..) and cancels near s = 0.3989.  Every base also carries TINY (1 + w): exp(-90) is a subnormal
fp32 that the hardware may flush.  Where a base would otherwise be 0 (a masked-out row, a Laplace tie) the kernel's entry is
additionally required to be exactly 0 by the GPU test.
A comparison passes when |got - ref| <= C_STAGE[stage] * base for EVERY entry; C_STAGE is 4x the largest |err| / base that
oracle.elbo in plain torch fp32 on the CPU (backward: fp32 autograd) shows over the whole case table, rounded up;
tests/test_nll_ref_host.py::test_error_constants re-derives it.  `mut` names deliberate mistakes of the REFERENCE, used only to
show that the bounds reject them (TEETH)."""
import math
import zlib
from dataclasses import dataclass

import torch

from elbo_ref import acc
from mmvae_ref import TINY, U, f32, worst_ratio  # noqa: F401  (re-exported to the tests)
from oracle import elbo

F64 = torch.float64
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
DISTS = ("normal", "laplace", "bernoulli", "categorical")

# one constant per stage: 4x the value measured by tests/test_nll_ref_host.py::test_error_constants, rounded up
C_STAGE = {
    "normal.rows": 2.0, "normal.drecon": 7.0, "laplace.rows": 2.0, "laplace.drecon": 7.0,
    "bernoulli.rows": 1.0, "bernoulli.drecon": 6.0, "categorical.rows": 1.0, "categorical.drecon": 5.0,
}


@dataclass(frozen=True)
class Case:
    name: str
    dist: str
    K: int
    B: int
    D: int
    scale: float = 1.0
    C: int = 0              # categorical: classes per position (D = P * C)
    regime: str = ""        # bernoulli: hard | soft targets; categorical: onehot | soft | zeros (one-hot with all-zero positions)
    mask: str = "none"      # none (NULL) | random | all (every row missing) | last (only the last row missing)
    rowcoef: bool = False   # given, graded over 10^U(-3, 3); else NULL
    drecon: bool = True     # given; else NULL (forward only)
    rescale: float = 1.0
    coef: float = 1.0
    misalign: str = ""      # recon | x | drecon: that buffer starts 4 bytes past a 16-byte boundary
    why: str = ""


def _c(name, dist, K, B, D, why, **kw):
    for k in ("scale", "rescale", "coef"):
        if k in kw:
            kw[k] = f32(kw[k])
    return Case(name, dist, K, B, D, why=why, **kw)


CASES = [
    # float4 path (every buffer 16-byte aligned, D % 4 == 0)
    _c("normal-k1-b1-d4", "normal", 1, 1, 4, "smallest float4 launch: one live lane, 255 dead lanes re-read element 0"),
    _c("normal.75-k10-b5-d1020-random-rc", "normal", 10, 5, 1020, "NV = 1 with 255 live lanes; random mask, graded rowcoef",
       scale=0.75, mask="random", rowcoef=True, rescale=1.7, coef=0.3),
    _c("normal.4-k16-b3-d1024", "normal", 16, 3, 1024, "the last NV = 1 size, all 256 lanes live; K = 16: one full chunk; "
       "scale 0.4: the row constant D (log s + 0.919) nearly cancels", scale=0.4, rescale=0.5),
    _c("laplace-k17-b3-d1028-rc", "laplace", 17, 3, 1028, "the first NV = 3 size: one live lane in the second slot; K = 17: "
       "chunks 9 + 8; planted ties", scale=0.5, rowcoef=True, coef=1.0 / 51),
    _c("normal.01-k10-b5-d3072-last", "normal", 10, 5, 3072, "exactly one NV = 3 tile; scale 0.01; only the last row missing",
       scale=0.01, mask="last", rescale=1.0 / 3.0),
    _c("bernoulli-k1-b9-d3076-hard", "bernoulli", 1, 9, 3076, "one NV = 3 tile and one float4 of a second; hard targets, logits to "
       "+-90", regime="hard", coef=1.0 / 9),
    _c("bernoulli-k17-b3-d4100-soft-rc", "bernoulli", 17, 3, 4100, "two tiles with a tail (768 + 257 float4) on the Bernoulli "
       "group; 9 + 8", regime="soft", rowcoef=True, rescale=3.92),
    _c("laplace-k33-b1-d4100-random", "laplace", 33, 1, 4100, "K = 33: three chunks of 11 on NV = 3; B = 1", scale=0.5,
       mask="random", coef=0.3),
    _c("laplace.3-k10-b3-d8", "laplace", 10, 3, 8, "scale 0.3: at the scale 0.5 of the other Laplace cases the row constant D log(2 s) "
       "is exactly 0", scale=0.3, rescale=1.7),
    _c("normal-k33-b1-d4-rc", "normal", 33, 1, 4, "three chunks on the shortest row", rowcoef=True),
    # scalar path (D % 4 != 0)
    _c("normal-k1-b1-d1", "normal", 1, 1, 1, "smallest scalar launch: one element"),
    _c("laplace-k10-b9-d3-random-rc", "laplace", 10, 9, 3, "D = 3, nine rows; ties", scale=0.5, mask="random", rowcoef=True,
       rescale=1.7, coef=0.3),
    _c("bernoulli-k16-b5-d255-soft", "bernoulli", 16, 5, 255, "one short of a block's stride", regime="soft", coef=0.0125),
    _c("normal.75-k17-b3-d257-rc", "normal", 17, 3, 257, "one past a block's stride: lane 0 takes two elements; 9 + 8 on the scalar "
       "path", scale=0.75, rowcoef=True, rescale=2.0),
    _c("bernoulli-k10-b5-d1023-hard-all", "bernoulli", 10, 5, 1023, "every row missing: drecon all zero, rows unaffected",
       regime="hard", mask="all"),
    _c("laplace-k33-b1-d4099-rc", "laplace", 33, 1, 4099, "long scalar row, K = 33 (D > 1024: 3 x 11)", scale=0.5, rowcoef=True),
    _c("normal.01-k1-b9-d4099-fwd", "normal", 1, 9, 4099, "long scalar row, drecon NULL", scale=0.01, drecon=False, rescale=0.19),
    # D = 784 (D % 4 == 0) with one buffer 4 bytes off: the scalar group
    _c("normal-k10-b5-d784-off-recon", "normal", 10, 5, 784, "recon misaligned", misalign="recon", mask="random", rescale=3.92),
    _c("bernoulli-k10-b5-d784-off-x", "bernoulli", 10, 5, 784, "x misaligned", regime="hard", misalign="x", rowcoef=True),
    _c("laplace-k10-b5-d784-off-drecon", "laplace", 10, 5, 784, "drecon misaligned: forward with drecon NULL on the float4 path, "
       "then mvk_recon_nll_bwd on the scalar path", scale=0.5, misalign="drecon", mask="last", rowcoef=True, coef=0.02),
    _c("bernoulli-k10-b9-d784-soft-random-fwd", "bernoulli", 10, 9, 784, "drecon NULL on the Bernoulli float4 group",
       regime="soft", mask="random", drecon=False),
    # categorical: one block per (k, b), one wave per position
    _c("categorical-k1-b3-c1-p5", "categorical", 1, 3, 5, "C = 1: lse = v, every term and gradient cancels", C=1, regime="onehot"),
    _c("categorical-k10-b5-c2-p32-soft-random-rc", "categorical", 10, 5, 64, "C = 2, 32 positions: eight per wave", C=2,
       regime="soft", mask="random", rowcoef=True, rescale=1.7, coef=0.3),
    _c("categorical-k16-b3-c63-p3-zeros", "categorical", 16, 3, 189, "C one short of a wave; P = 3: wave 3 idle; padding "
       "positions (sx = 0)", C=63, regime="zeros"),
    _c("categorical-k17-b3-c64-p4-soft-rc", "categorical", 17, 3, 256, "C = one full wave trip, one position per wave", C=64,
       regime="soft", rowcoef=True, coef=1.0 / 51),
    _c("categorical-k10-b9-c65-p5-zeros-last-rc", "categorical", 10, 9, 325, "C one past a trip; P = 5: wave 0 takes two", C=65,
       regime="zeros", mask="last", rowcoef=True, rescale=2.5),
    _c("categorical-k33-b1-c130-p1-soft", "categorical", 33, 1, 130, "three trips, a single position, B = 1", C=130, regime="soft"),
    _c("categorical-k1-b5-c1590-p3-zeros", "categorical", 1, 5, 4770, "the vocabulary size of the CUB captions, 25 trips", C=1590,
       regime="zeros", coef=0.2),
    _c("categorical-k10-b3-c65-p4-onehot-fwd", "categorical", 10, 3, 260, "drecon NULL", C=65, regime="onehot", drecon=False),
]
# the eight descriptors of ONE launch with n_mod = 8 (K and B belong to the launch: K = 17, B = 3); each is also a case of its own
ONE_LAUNCH = [
    _c("one-normal-d784", "normal", 17, 3, 784, "float4 group, slot 0", mask="random", rowcoef=True, rescale=3.92, coef=0.1),
    _c("one-laplace-d3", "laplace", 17, 3, 3, "scalar group, slot 0", scale=0.5, rowcoef=True),
    _c("one-bernoulli-d784", "bernoulli", 17, 3, 784, "Bernoulli group, slot 0; drecon NULL", regime="hard", drecon=False),
    _c("one-categorical-c65-p5", "categorical", 17, 3, 325, "class-row kernel launched from the same call", C=65, regime="zeros",
       mask="last", coef=0.5),
    _c("one-normal-d3072", "normal", 17, 3, 3072, "float4 group, slot 1: NV = 3 next to NV = 1 rows, found by the block_start "
       "scan", scale=0.75, mask="last"),
    _c("one-bernoulli-d1024-off-recon", "bernoulli", 17, 3, 1024, "scalar group, slot 1: a Bernoulli row next to a Laplace one",
       regime="soft", misalign="recon", rowcoef=True, rescale=2.0),
    _c("one-laplace-d1028", "laplace", 17, 3, 1028, "float4 group, slot 2: Laplace behind two Normal rows", scale=0.5,
       mask="random", drecon=False),
    _c("one-normal-d4", "normal", 17, 3, 4, "float4 group, slot 3: the last entry of the table", scale=0.4, coef=2.0),
]
CASES += ONE_LAUNCH
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)

TEETH = [  # (mutation of the REFERENCE, the stage kind it must show in, the cases named for it)
    ("no_row_const", "rows", ["normal.75-k10-b5-d1020-random-rc", "laplace.3-k10-b3-d8", "normal.01-k1-b9-d4099-fwd",
                              "normal-k1-b1-d1"]),
    ("mask_rows", "rows", ["normal.75-k10-b5-d1020-random-rc", "bernoulli-k10-b5-d1023-hard-all",
                           "categorical-k10-b9-c65-p5-zeros-last-rc"]),
    ("no_rescale_grad", "drecon", ["normal.75-k10-b5-d1020-random-rc", "bernoulli-k17-b3-d4100-soft-rc",
                                   "categorical-k10-b5-c2-p32-soft-random-rc"]),
    ("rowcoef_bk", "drecon", ["laplace-k17-b3-d1028-rc", "bernoulli-k10-b5-d784-off-x", "categorical-k17-b3-c64-p4-soft-rc"]),
    ("drop_last_vec", "rows", ["normal-k1-b1-d4", "normal.4-k16-b3-d1024", "laplace-k17-b3-d1028-rc",
                               "bernoulli-k17-b3-d4100-soft-rc"]),
    ("chunk_8_9", "drecon", ["laplace-k17-b3-d1028-rc", "bernoulli-k17-b3-d4100-soft-rc", "normal.75-k17-b3-d257-rc"]),
    ("bern_no_x", "drecon", ["bernoulli-k1-b9-d3076-hard", "bernoulli-k16-b5-d255-soft"]),
    ("cat_no_sx", "drecon", ["categorical-k16-b3-c63-p3-zeros", "categorical-k1-b5-c1590-p3-zeros"]),
]
NOOP_MUT = "no_shift"  # log_softmax without the 1e-6: log_softmax is shift-invariant, so this is the same function


# ---- seeded inputs ---------------------------------------------------------------------------------------------------------------------
def make_inputs(case):
    """Seeded fp32 inputs of one case (CPU tensors; None where the case passes NULL)."""
    gen = torch.Generator().manual_seed(zlib.crc32(case.name.encode()))
    K, B, D = case.K, case.B, case.D
    rn = lambda *s: torch.randn(*s, generator=gen)
    ru = lambda *s: torch.rand(*s, generator=gen)
    if case.dist in ("normal", "laplace"):
        recon, x = rn(K, B, D), ru(B, D)
        if case.dist == "laplace":  # exact ties recon == x: gradient 0 in the reference and in the kernel
            tie = ru(K, B, D) < 0.05
            tie[0, 0, 0] = tie[-1, -1, -1] = True
            recon = torch.where(tie, x.expand(K, B, D), recon)
    elif case.dist == "bernoulli":
        recon = 3.0 * rn(K, B, D)
        far = ru(K, B, D) < 0.1
        recon = torch.where(far, 180.0 * ru(K, B, D) - 90.0, recon)  # logits spread to +-90
        recon.view(-1)[0], recon.view(-1)[-1] = 90.0, -90.0
        x = ru(B, D)
        if case.regime == "hard":
            x = (x > 0.5).float()
    else:
        C, P = case.C, D // case.C
        recon = 2.0 * rn(K, B, P, C)
        far = ru(K, B, P, C) < 0.1
        recon = torch.where(far, 80.0 * ru(K, B, P, C) - 40.0, recon)  # spread to +-40: the max subtraction matters
        if case.regime == "soft":
            x = torch.softmax(rn(B, P, C), -1)
        else:
            x = torch.nn.functional.one_hot(torch.randint(0, C, (B, P), generator=gen), C).float()
            if case.regime == "zeros":  # padding positions: the whole target row of a position is 0
                pad = ru(B, P) < 0.4
                pad[0, -1], pad[-1, 0] = True, False
                x = x * (~pad).float().unsqueeze(-1)
        recon, x = recon.reshape(K, B, D), x.reshape(B, D)
    mask = None
    if case.mask == "random":
        mask = ru(B) > 0.3
        mask[0] = False
        if B > 1:
            mask[-1] = True
    elif case.mask == "all":
        mask = torch.zeros(B, dtype=torch.bool)
    elif case.mask == "last":
        mask = torch.ones(B, dtype=torch.bool)
        mask[-1] = False
    rowcoef = (10.0 ** (6 * ru(K, B) - 3) * torch.where(ru(K, B) < 0.5, -1.0, 1.0)).float() if case.rowcoef else None
    return dict(recon=recon.float().contiguous(), x=x.float().contiguous(), mask=mask, rowcoef=rowcoef)


# ---- the float64 reference -----------------------------------------------------------------------------------------------------------
def _sg(value, grad_like):
    """`value` with the gradient of `grad_like` (both the same shape)."""
    return value.detach() + (grad_like - grad_like.detach())


def _elem_nll(case, r, x, mut):
    """-log p per element [K,B,D] (categorical: per position [K,B,P]) without the row constant, in r's dtype."""
    s = case.scale
    if case.dist == "normal":
        return (r - x) ** 2 / (2.0 * s * s)
    if case.dist == "laplace":
        return (r - x).abs() / s
    if case.dist == "bernoulli":
        t = r.clamp(min=0) - r * x + torch.log1p(torch.exp(-r.abs()))
        if "bern_no_x" in mut:  # d/dr = sigmoid(r) instead of sigmoid(r) - x (values unchanged)
            t = t + (r - r.detach()) * x
        return t
    K, B = r.shape[:2]
    C = case.C
    v = r.reshape(K, B, -1, C) + (0.0 if NOOP_MUT in mut else 1e-6)
    xx = x.reshape(B, -1, C)
    lse = torch.logsumexp(v, -1)
    sx = xx.sum(-1).expand_as(lse)
    term = lse * sx
    if "cat_no_sx" in mut:  # d/dr_c = softmax_c - x_c: the factor sum_c' x_c' left out (values unchanged)
        term = _sg(term, lse)
    return -((xx * v).sum(-1) - term)


def _row_const(case):
    if case.dist == "normal":
        return case.D * (math.log(case.scale) + HALF_LOG_2PI)
    if case.dist == "laplace":
        return case.D * math.log(2.0 * case.scale)
    return 0.0


def _weights(case, inp, dtype, mut=()):
    """coef * mask[b] * rowcoef[k,b] [K,B]."""
    K, B = case.K, case.B
    w = torch.full((K, B), case.coef, dtype=dtype)
    if inp["mask"] is not None:
        w = w * inp["mask"].to(dtype)
    if inp["rowcoef"] is not None:
        rc = inp["rowcoef"].to(dtype)
        if "rowcoef_bk" in mut:  # the [K,B] array read as [B,K]
            rc = rc.reshape(-1)[(torch.arange(B)[None, :] * K + torch.arange(K)[:, None]) % (K * B)]
        if "chunk_8_9" in mut and K == 17:  # chunks of 8 + 9 samples whose rowcoef stays with the chunks of 9 + 8
            rc = rc[torch.tensor(list(range(8)) + [(9 + j) % K for j in range(9)])]
        w = w * rc
    return w


def reference(case, inp, mut=(), dtype=F64):
    """rows [K,B] and drecon [K,B,D] (None where the case passes drecon = NULL) in `dtype`, from the fp32 inputs."""
    r = inp["recon"].to(dtype).clone().requires_grad_()
    x = inp["x"].to(dtype)
    t = _elem_nll(case, r, x, mut)
    if "drop_last_vec" in mut and case.dist != "categorical":  # the last float4 of every row left out
        t = torch.cat([t[..., :-4], 0.0 * t[..., -4:]], -1)
    rows = (t.sum(-1) + (0.0 if "no_row_const" in mut else _row_const(case))) * case.rescale
    out_rows = rows
    if "mask_rows" in mut and inp["mask"] is not None:
        out_rows = rows * inp["mask"].to(dtype)
    drecon = None
    if case.drecon:
        (drecon,) = torch.autograd.grad((rows * _weights(case, inp, dtype, mut)).sum(), r)
        if "no_rescale_grad" in mut:
            drecon = drecon / case.rescale
    return dict(rows=out_rows.detach(), drecon=drecon)


def oracle_eval(case, inp, dtype):
    """The same arrays by oracle.elbo._row_nll in `dtype`, the gradient by autograd of sum rows * coef * mask * rowcoef (float64:
    pins the reference; float32: what the constants are measured on and what the stand-in launcher returns)."""
    r = inp["recon"].to(dtype).clone().requires_grad_()
    x = inp["x"].to(dtype)
    if case.dist == "categorical":
        rows = elbo._row_nll(case.dist, r.reshape(case.K, case.B, -1, case.C), x.reshape(case.B, -1, case.C), case.rescale)
    else:
        rows = elbo._row_nll(case.dist, r, x, case.rescale, case.scale)
    drecon = None
    if case.drecon:
        tot = rows * case.coef
        if inp["mask"] is not None:
            tot = tot * inp["mask"].to(dtype)
        if inp["rowcoef"] is not None:
            tot = tot * inp["rowcoef"].to(dtype)
        (drecon,) = torch.autograd.grad(tot.sum(), r)
    return dict(rows=rows.detach(), drecon=drecon)


def run_torch32(case, inp):
    return oracle_eval(case, inp, torch.float32)


# ---- the error model -------------------------------------------------------------------------------------------------------------------
def bases(case, inp):
    """base of rows [K,B] and of drecon [K,B,D] (None: drecon NULL), float64."""
    ref = reference(case, inp)
    with torch.no_grad():
        r, x = inp["recon"].to(F64), inp["x"].to(F64)
        K, B, D, s = case.K, case.B, case.D, case.scale
        w = (_weights(case, inp, F64) * case.rescale).abs().unsqueeze(-1)  # [K,B,1]
        g = None if ref["drecon"] is None else ref["drecon"].abs()
        t = _elem_nll(case, r, x, ()).abs()
        const = 0.0
        if case.dist == "normal":
            d = (r - x).abs()
            eb = (r.abs() + x.abs()) * d / (s * s) + t
            gb = w * (r.abs() + x.abs()) / (s * s)
            const = D * (abs(math.log(s)) + 0.919)
        elif case.dist == "laplace":
            eb = (r.abs() + x.abs()) / s + t
            gb = torch.zeros_like(r)
            const = D * abs(math.log(2.0 * s))
        elif case.dist == "bernoulli":
            eb = r.clamp(min=0) + (r * x).abs() + torch.log1p(torch.exp(-r.abs())) + t
            gb = w * (torch.sigmoid(r) + x.abs())
        else:
            C = case.C
            v = r.reshape(K, B, -1, C) + 1e-6
            xx = x.reshape(B, -1, C).expand(K, B, -1, C)
            mx, lse = v.amax(-1), torch.logsumexp(v, -1)
            p = torch.exp(v - lse.unsqueeze(-1))
            EL = lse.abs() + mx.abs() + acc(C) + 2 + (p * ((v - mx.unsqueeze(-1)).abs() + v.abs())).sum(-1)
            sax, sxv = xx.abs().sum(-1), (xx * v).abs().sum(-1)
            eb = EL * sax + (1 + acc(C)) * sxv + acc(C) * lse.abs() * sax + t  # per position [K,B,P]
            gb = w.unsqueeze(-1) * (p * xx.sum(-1, keepdim=True).abs() * (v.abs() + (lse.abs() + EL + 3 + acc(C)).unsqueeze(-1))
                                    + xx.abs())
            gb = gb.reshape(K, B, D)
        n = t.shape[-1]
        rows = U * (case.rescale * (eb.sum(-1) + acc(n) * t.sum(-1) + const) + ref["rows"].abs()) + TINY
        drecon = None if g is None else U * (gb + g) + TINY * (1 + w)
        return dict(rows=rows, drecon=drecon)


def ratios(case, got, ref, base):
    """max |got - ref| / base over EVERY entry, per stage -> {stage: ratio}; compare with C_STAGE[stage]."""
    out = {}
    for k in ("rows", "drecon"):
        if got.get(k) is not None:
            assert got[k].shape == ref[k].shape == base[k].shape, (k, got[k].shape, ref[k].shape)
            out[f"{case.dist}.{k}"] = worst_ratio(got[k], ref[k], base[k])
    return out
