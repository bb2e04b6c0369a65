"""References, host arithmetic and case tables for csrc/skinny.hip (tests/test_gpu_skinny.py runs them on the GPU,
tests/test_skinny_ref_host.py pins them on the CPU).  Nothing here touches the GPU path of the package.

1. The host arithmetic of the launchers as plain Python (`heads_plan`, `heads_bwd_plan`, `smallk_plan`): which kernels a shape
   launches, on which grid, with how many K slices, which weight-load branch, and what makes the launcher decline.  Every case
   below states the leaf it is there for; the GPU file asserts the kernel names the plan gives.
2. float64 references with per-entry bounds in the form of tests/test_gpu_gemm_dispatch.py: bound = sum |a b| + |bias| + |initial|
   (column sums of dX: the column sums of dX's own bounds), and the same formulas on operands rounded to a two-piece bf16 split
   (`D.two_piece`), which the bound must reject on at least one entry of EVERY output of EVERY case.
3. fp32 CPU evaluations in the kernels' summation order (`*_f32`): slices, waves and row groups are summed on their own and then
   added in the kernels' order.  They are the stand-in backend of the host test.

Operands.  A per-entry rejection of the two-piece operands needs a rounding error of ~2^-17 per term that does not average out:
over n equal terms it shrinks like 1 / sqrt(n) against the bound (about 19 / sqrt(n) times the bound for normal operands), and beyond
a few hundred terms it passes.  Reductions longer than 64 terms therefore run on a LOUD / QUIET scale along the reduction axis: the
LAST 8 positions at scale ~1, every other at 2^-10.  A quiet term is still ~50x the tolerance of its entry, so a skipped, doubled
or misplaced quiet term fails the entry as a loud one does; the loud ones keep the sum short enough for the two-piece operands to
leave the bound.  The loud positions are the last ones because every kernel here adds along its axis in ascending order (k inside
a wave, the waves, the slices; the rows of a group, the groups): a loud term EARLY in a chain makes each later addition round at
the loud magnitude, n u |S| in all, which is the fp32 chain's own error on such operands (the stand-in shows 1.4x the bound over
128 rows) and not what C_ENTRY's basis, partial sums of random sign, covers.

dbprev.  The column sums of dX add M x taps x NN two-piece terms per entry: no operand scale short of a handful of non-zero rows
lets their rounding leave the bound, and what the launch adds to dX to get dbprev is a SUM, not a product of operands.  Its
degraded emulation is therefore a summation fault: the reference with the contribution of row 0 of X left out (a quiet row at
M > 64).  That must leave the bound on at least one entry in every case; the two-piece figure is still computed and printed
(`Ref.deg2`).  The two-piece operands themselves are rejected on dX's own entries, from which dbprev is summed, in the same case.
"""
import math
import zlib
from collections import namedtuple

import torch

import test_gpu_gemm_dispatch as D

NONE, RELU, SIGMOID, LEAKY = D.NONE, D.RELU, D.SIGMOID, D.LEAKY
ACTS = (NONE, RELU, SIGMOID, LEAKY)
C_ENTRY = D.C_ENTRY
SIG_SLACK = 2e-7  # the dispatch table's slack: a sigmoid evaluation is allowed 2 ulp of its own value
H4, H16, HFIN, NARROW, HBWD = D.H4, D.H16, D.HFIN, D.NARROW, "heads_bwd_kernel"
FIN, FINS = D.FIN, D.FINS
HB_KC, HB_MR, HB_XS = 16, 128, 20
QUIET = 2.0 ** -10
LOUD = 8


def smallk_name(K4, R):
    return f"smallk_fwd_kernel<{K4},{R}>"


def cdiv(a, b):
    return -(-a // b)


def gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()) & 0x7FFFFFFF)


# ---- host arithmetic ------------------------------------------------------------------------------------------------------
HeadsPlan = namedtuple("HeadsPlan", "kernels grid nz kz wvec declines")


def heads_plan(M, N, K, heads=1, w_sk=1, w_sn=None, aligned=True, ws_floats=0, via="linear"):
    """heads_launch (skinny.hip) and, via="linear", the conditions of mvk_linear_fwd around it (via="heads": mvk_heads_fwd, which
    passes no scratch).  aligned: X and W on 16 bytes (a bool, or (X, W)).  declines: why the kernels are not taken ([] = taken)."""
    w_sn = K if w_sn is None else w_sn
    xa, wa = aligned if isinstance(aligned, tuple) else (aligned, aligned)
    dec = []
    if via == "linear":
        if M > 1024:
            dec.append("M > 1024")
        if K < 64:
            dec.append("K < 64")
        if N * K > 2 ** 21:
            dec.append("N K > 2^21")
    else:
        ws_floats = 0
        if N > 32:
            dec.append("N > 32")
    if heads == 2 and N > 32:
        dec.append("two heads and N > 32")
    if N < 1 or M < 1:
        dec.append("empty")
    if K % 4 != 0 or K < 4:
        dec.append("K % 4 != 0")
    if not xa:
        dec.append("X unaligned")
    wvec = int(w_sk == 1 and w_sn % 4 == 0 and wa)
    if dec:
        return HeadsPlan([], None, 0, 0, wvec, dec)
    tph = cdiv(N, 16)
    gx, gy = cdiv(M, 16), heads * tph
    tiles, nz, kz = gx * gy, 1, 0
    if ws_floats > 0 and tiles <= 64 and K >= 2048:
        nz = K // 256
        nz = min(nz, 64 if tiles >= 32 else 128)
        kz = (cdiv(K, nz) + 15) & ~15
        nz = cdiv(K, kz)
        if nz < 2 or nz * heads * M * N > ws_floats:
            nz = 1
    if heads == 1 and 16 < N <= 32 and M >= 1024:
        return HeadsPlan([NARROW], (gx, 1, 1), 1, 0, wvec, [])
    if nz > 1:
        return HeadsPlan([H16, HFIN], (gx, gy, nz), nz, kz, wvec, [])
    return HeadsPlan([H16 if K >= 1024 else H4], (gx, gy, 1), 1, 0, wvec, [])


def heads_waves(K, nz, kz, NW):
    """[(k0, k1) per wave] per slice, as heads_fwd_kernel<NW> cuts them (empty waves have k0 >= k1)."""
    out = []
    for z in range(nz):
        kbeg, kend = (z * kz, min(K, z * kz + kz)) if nz > 1 else (0, K)
        kw = cdiv(kend - kbeg, 16 * NW) * 16
        out.append([(kbeg + w * kw, min(kend, kbeg + w * kw + kw)) for w in range(NW)])
    return out


BwdPlan = namedtuple("BwdPlan", "grid rgs lds_bytes slabs declines")


def heads_bwd_plan(M, N, K, nh, flat_c=0, x_aligned=True, dx_aligned=True):
    """heads_bwd_launch and the slab bookkeeping of mvk_heads_bwd.  slabs: floats of each slab region (rounded up to 4) in the
    order the C side lays them into the workspace: dW0, dW1, db0, db1, dbprev; plus prow (partial rows of dbprev per row group)."""
    dec = []
    if M < 1 or N < 1:
        dec.append("empty")
    if N > 32:
        dec.append("N > 32")
    if K % HB_KC != 0 or K < HB_KC:
        dec.append("K % 16 != 0")
    if not x_aligned:
        dec.append("X unaligned")
    if not dx_aligned:
        dec.append("dX unaligned")
    if flat_c > 0 and K % flat_c != 0:
        dec.append("flat_c does not divide K")
    rgs = cdiv(M, HB_MR)
    if rgs > 64:
        dec.append("more than 64 row groups")
    nn = nh * N
    lds = 4 * (((HB_MR * (nn | 1) + 3) & ~3) + nn * HB_KC + 2 * HB_MR * HB_XS + 16 * 64)
    pc = flat_c if flat_c > 0 else K
    prow = K // pc if (flat_c <= 0 or K % flat_c == 0) else 0
    r4 = lambda v: (v + 3) & ~3  # noqa: E731
    slabs = dict(dW0=r4(N * K * rgs), db0=r4(N * rgs), dbprev=r4(pc * rgs * prow), prow=prow, pc=pc)
    if nh == 2:
        slabs.update(dW1=r4(N * K * rgs), db1=r4(N * rgs))
    return BwdPlan((K // HB_KC, rgs), rgs, lds, slabs, dec)


SLAB_ORDER = ("dW0", "dW1", "db0", "db1", "dbprev")


def python_ws_estimate(M, N, K, nh):
    """kernels.heads_bwd's own estimate of the scratch (it returns None above it instead of calling the C side)."""
    return (nh * (N * K + N) + K) * cdiv(M, 128) + 64


SmallkPlan = namedtuple("SmallkPlan", "K4 R grid branch declines")


def smallk_plan(M, N, K, layout, aligned=True):
    """smallk_fwd.  layout "kn": W [K][N] (tb = 0), "nk": torch Linear [N][K] (tb = 1).  aligned: bool or dict(W=, Y=, X=)."""
    al = dict(W=True, Y=True, X=True)
    al.update(aligned if isinstance(aligned, dict) else dict(W=aligned, Y=aligned))
    dec = []
    if K > 32 or K < 1:
        dec.append("K outside 1 .. 32")
    if N % 4 != 0 or N < 4:
        dec.append("N % 4 != 0")
    if not al["Y"]:
        dec.append("Y unaligned")
    if M < 1:
        dec.append("empty")
    if dec:
        return SmallkPlan(0, 0, None, None, dec)
    w_sk, w_sn = (N, 1) if layout == "kn" else (1, K)
    if w_sn == 1 and w_sk % 4 == 0 and al["W"]:
        branch = "rows_kn"
    elif w_sk == 1 and w_sn % 4 == 0 and K % 4 == 0 and al["W"]:
        branch = "rows_nk"
    else:
        branch = "scalar"
    CT = N // 4
    ctb = min(CT, 256)
    gy = cdiv(CT, ctb)
    want = (M * gy + 255) // 256
    R = 8 if want <= 8 else 16
    return SmallkPlan(min(8, cdiv(K, 4)), R, (cdiv(M, R), gy), branch, [])


# ---- operands -------------------------------------------------------------------------------------------------------------
def axis_scale(n, g, loud=LOUD):
    """Scale along a reduction axis: short axes every position on its own scale (0.25 .. 4.25), long ones QUIET with the last LOUD
    positions loud (the module docstring says why the last)."""
    if n <= 64:
        return torch.rand(n, generator=g) * 4 + 0.25
    s = torch.full((n,), QUIET)
    s[n - loud:] = 1.0
    return s * (torch.rand(n, generator=g) * 0.5 + 0.75)


def act_out(v, act):
    """A stored output of the activation (what the backward reads): SIGMOID in (0, 1), RELU >= 0."""
    return D.act64(v.double(), act).float()


Ref = namedtuple("Ref", "ref bound deg slack deg2", defaults=(None,))


def fwd_ref(x, wkn, b, act):
    """act(X W + b): W given as [K][N]."""
    ref, bound, deg = D.gemm64(x, wkn, b, act)
    return Ref(ref, bound, deg, SIG_SLACK if act == SIGMOID else 0.0)


def flat_perm(t, flat_c):
    """[N][K] with k = (tap, c) -> the Conv2d layout [N][c][tap] ([L][C][4][4] at 16 taps)."""
    if flat_c <= 0:
        return t
    N, K = t.shape
    return t.reshape(N, K // flat_c, flat_c).permute(0, 2, 1).reshape(N, K)


def prev_sum(t, flat_c):
    """Bias gradient of the layer below: per column of X, or per channel when the layer below is a convolution."""
    if flat_c <= 0:
        return t.sum(0)
    M, K = t.shape
    return t.reshape(M, K // flat_c, flat_c).sum((0, 1))


def heads_bwd_ref(x, x_act, dys, ws, flat_c=0):
    """dys [M][N] per head, ws [N][K] per head (logical).  -> {output name: Ref} of what the launch ADDS to its targets."""
    mask = D.actgrad64(x, x_act)
    ident = lambda t: t.double()  # noqa: E731

    def dx(f, g):
        return sum(f(dy) @ g(w) for dy, w in zip(dys, ws)) * mask

    ab = lambda t: t.double().abs()  # noqa: E731
    out = {"dX": Ref(dx(ident, ident), dx(ab, ab), dx(D.two_piece, D.two_piece), 0.0)}
    for h, dy in enumerate(dys):
        out[f"dW{h}"] = Ref(flat_perm(dy.double().t() @ x.double(), flat_c), flat_perm(ab(dy).t() @ ab(x), flat_c),
                            flat_perm(D.two_piece(dy).t() @ D.two_piece(x), flat_c), 0.0)
        out[f"db{h}"] = Ref(dy.double().sum(0), ab(dy).sum(0), D.two_piece(dy).sum(0), 0.0)
    d = out["dX"]
    full = prev_sum(d.ref, flat_c)
    out["dbprev"] = Ref(full, prev_sum(d.bound, flat_c), full - prev_sum(d.ref[:1], flat_c), 0.0, prev_sum(d.deg, flat_c))
    return out


def deg_ratio(r, deg, init=None):
    """Worst |deg - ref| / tolerance of a degraded emulation `deg` of what the launch adds."""
    bound = r.bound if init is None else r.bound + init.double().abs()
    return float(((deg - r.ref).abs() / (C_ENTRY * bound + r.slack * r.ref.abs() + 1e-30)).max())


def ratios(got, r, init=None):
    """(worst |got - ref| / tolerance, the same for the two-piece emulation) under rule (a) of the dispatch table."""
    bound = r.bound if init is None else r.bound + init.double().abs()
    tol = C_ENTRY * bound + r.slack * r.ref.abs() + 1e-30
    g = got.double() if init is None else got.double() - init.double()
    return float(((g - r.ref).abs() / tol).max()), float(((r.deg - r.ref).abs() / tol).max())


# ---- fp32 evaluations in the kernels' summation order ------------------------------------------------------------------------
def act32(v, act):
    if act == RELU:
        return torch.where(v > 0, v, torch.zeros_like(v))
    if act == SIGMOID:
        return torch.sigmoid(v)
    if act == LEAKY:
        return torch.where(v > 0, v, D.F02 * v)
    return v


def heads_fwd_f32(x, wkn, b, act, plan):
    """heads_fwd_kernel / narrow_fwd_kernel / heads_finish_kernel: waves on their own, added in fours; slices in z order."""
    M, K = x.shape
    N = wkn.shape[1]
    x, wkn = x.float(), wkn.float()
    if plan.kernels == [NARROW]:
        kw = cdiv(K, 64) * 16
        waves = [[(w * kw, min(K, w * kw + kw)) for w in range(4)]]
    else:
        waves = heads_waves(K, plan.nz, plan.kz, 4 if plan.kernels == [H4] else 16)
    total = torch.zeros(M, N)
    for sl in waves:
        p = [x[:, a:e] @ wkn[a:e] if e > a else torch.zeros(M, N) for a, e in sl]
        t = torch.zeros(M, N)
        for w in range(0, len(p), 4):
            t = t + ((p[w] + p[w + 1]) + (p[w + 2] + p[w + 3]))
        total = total + t
    return act32(total + (0 if b is None else b.float()), act)


def smallk_f32(x, wkn, bias_full, act):
    """smallk_fwd_kernel: one chain per output in k order, starting from the bias."""
    M, K = x.shape
    acc = torch.zeros(M, wkn.shape[1]) + (0 if bias_full is None else bias_full.float())
    for k in range(K):
        acc = acc + x[:, k:k + 1].float() * wkn[k].float()
    return act32(acc, act)


def heads_bwd_f32(x, x_act, dys, ws, flat_c, inits):
    """heads_bwd_kernel and the ordered finishes: row groups of 128 on their own, then the groups in order on top of the target."""
    M, K = x.shape
    mask = D.actgrad64(x, x_act).float()
    dycat, wcat = torch.cat([d.float() for d in dys], 1), torch.cat([w.float() for w in ws], 0)
    dX = (dycat @ wcat) * mask
    out = {"dX": dX}
    acc = {k: v.clone().float() for k, v in inits.items()}
    for r0 in range(0, M, HB_MR):
        rows = slice(r0, min(M, r0 + HB_MR))
        for h, dy in enumerate(dys):
            if f"dW{h}" in acc:
                acc[f"dW{h}"] += flat_perm(dy[rows].float().t() @ x[rows].float(), flat_c).reshape(acc[f"dW{h}"].shape)
            if f"db{h}" in acc:
                acc[f"db{h}"] += dy[rows].float().sum(0)
        if "dbprev" in acc:
            ps = dX[rows].sum(0)
            acc["dbprev"] += ps if flat_c <= 0 else ps.reshape(K // flat_c, flat_c).sum(0)
    out.update(acc)
    return out


# ---- forward heads / finish: through mvk_linear_fwd (one head, torch Linear weights, explicit scratch) ----------------------
FwdCase = namedtuple("FwdCase", "name via M N K heads layout bias act ws w_off why")


def F(name, M, N, K, why, via="linear", heads=1, layout="nk", bias=True, act=NONE, ws="exact", w_off=False):
    return FwdCase(name, via, M, N, K, heads, layout, bias, act, ws, w_off, why)


FWD_CASES = [
    F("fin-K2048", 32, 32, 2048, "nz = 8, kz = 256: two rounds of four in the finish, no z tail"),
    F("fin-K2304", 32, 32, 2304, "nz = 9: z tail of 1"),
    F("fin-K2816", 32, 32, 2816, "nz = 11: z tail of 3"),
    F("fin-K2052", 32, 32, 2052, "kz = 272, last slice 148 wide: its waves 10 .. 15 have an empty k range"),
    F("fin-K4096-short", 32, 32, 4096, "scratch one float below nz M N: back to one slice, heads_fwd_kernel<16> alone", ws="short"),
    F("fin-K4096", 32, 32, 4096, "the same shape on the split route (nz = 16): both routes inside the bound"),
    F("fin-K2048-nows", 32, 32, 2048, "no scratch at all: one slice", ws="none"),
    F("fin-M512-N16", 512, 16, 2048, "32 tiles"),
    F("fin-M528-N16", 528, 16, 2048, "33 tiles; M = 528 = 33 x 16"),
    F("fin-64tiles", 256, 64, 2048, "16 x 4 = 64 tiles: the last shape that splits"),
    F("fin-65tiles", 208, 80, 2048, "13 x 5 = 65 tiles: no split although the scratch is there"),
    F("fin-cap64", 512, 16, 16640, "K / 256 = 65 > 64 at 32 tiles: capped, kz = 272, nz = 62"),
    F("fin-cap128-tiles31", 496, 16, 16640, "31 tiles: the cap is 128, so nz = 65 stays (kz = 256)"),
    F("fin-cap128", 16, 16, 33024, "K / 256 = 129 > 128 at one tile: capped, kz = 272, nz = 122"),
    F("fin-K2304-nobias-relu", 17, 5, 2304, "no bias, ReLU in the finish, M and N ragged", bias=False, act=RELU),
    F("fin-K2048-sigmoid", 32, 20, 2048, "sigmoid in the finish", act=SIGMOID),
    F("fin-K2048-leaky", 32, 20, 2048, "LeakyReLU in the finish", act=LEAKY),
    F("h16-K1024-sigmoid-nobias", 33, 17, 1024, "heads_fwd_kernel<16> below the split, its own epilogue: sigmoid, no bias", bias=False,
      act=SIGMOID),
    F("h4-K64-leaky", 17, 33, 64, "heads_fwd_kernel<4>, three column tiles, LeakyReLU", act=LEAKY),
    F("h4-K1020-relu", 100, 40, 1020, "heads_fwd_kernel<4> at its longest K (kw = 256, last wave 252)", act=RELU),
    F("narrow-M1024-N17", 1024, 17, 64, "narrow_fwd_kernel at its first M, one column in the second tile", act=RELU),
    F("narrow-M1024-N32-woff", 1024, 32, 64, "narrow_fwd_kernel with torch Linear rows 4 bytes off: its scalar loads at w_sk = 1, both tiles full",
      w_off=True, act=LEAKY),
    F("narrow-M1023-N17", 1023, 17, 64, "one row below: the two-tile grid of heads_fwd_kernel<4>"),
    # ---- layouts through mvk_heads_fwd (no scratch, no activation) ----
    F("hf-nk-woff-2h", 33, 20, 400, "torch Linear rows 4 bytes off a 16-byte boundary: wvec = 0 with w_sk = 1", via="heads", heads=2, w_off=True),
    F("hf-nk-woff-1h", 17, 32, 64, "the same with one head", via="heads", w_off=True),
    F("hf-nk-2h-N16", 17, 16, 400, "N = 16: one column tile per head", via="heads", heads=2),
    F("hf-nk-2h-N17", 17, 17, 400, "N = 17: two column tiles per head, 15 idle columns", via="heads", heads=2),
    F("hf-kn-2h-N1", 17, 1, 400, "N = 1, packed [K][N] weights", via="heads", heads=2, layout="kn"),
    F("hf-nk-1h-N1", 16, 1, 64, "N = 1 with one head", via="heads"),
    F("hf-M1", 1, 20, 400, "M = 1: every lane reads row 0", via="heads", heads=2),
    F("hf-M15", 15, 20, 400, "M = 15", via="heads", heads=2, layout="kn"),
    F("hf-M16", 16, 20, 400, "M = 16: one full row tile", via="heads", heads=2),
    F("hf-M17", 17, 20, 400, "M = 17: a second row tile with one row", via="heads", heads=2, layout="kn"),
    F("hf-K4", 17, 20, 4, "K = 4: wave 0 has one quad of lanes with data, waves 1 .. 3 are empty", via="heads", heads=2),
    F("hf-K60", 17, 20, 60, "K = 60: the last wave is 12 wide", via="heads", heads=2, layout="kn"),
    F("hf-K1024-2h", 17, 20, 1024, "two heads on heads_fwd_kernel<16>", via="heads", heads=2),
]
FWD_BY_NAME = {c.name: c for c in FWD_CASES}


def fwd_strides(c):
    """(w_sk, w_sn) as the C entry passes them."""
    return (1, c.K) if c.layout == "nk" else (c.N, 1)


def fwd_plan(c):
    sk, sn = fwd_strides(c)
    al = (True, not c.w_off)
    ample = heads_plan(c.M, c.N, c.K, c.heads, sk, sn, al, 1 << 40, c.via)
    # the scratch of the split; where the plan does not split at K >= 2048, what a split would have needed (it must stay untouched)
    exact = (ample.nz if ample.nz > 1 else c.K // 256 if c.K >= 2048 else 0) * c.heads * c.M * c.N
    ws_floats = {"exact": exact, "short": exact - 1, "none": 0}[c.ws] if c.via == "linear" else 0
    return heads_plan(c.M, c.N, c.K, c.heads, sk, sn, al, ws_floats, c.via), ws_floats


def fwd_inputs(c):
    g = gen(c.name)
    ks = axis_scale(c.K, g)
    x = torch.randn(c.M, c.K, generator=g) * ks * (torch.rand(c.M, 1, generator=g) * 4 + 0.25)
    norm = math.sqrt(min(c.K, LOUD) if c.K > 64 else c.K)
    ws = [torch.randn(c.K, c.N, generator=g) * (torch.rand(1, c.N, generator=g) + 0.5) / norm for _ in range(c.heads)]
    bs = [torch.randn(c.N, generator=g) if c.bias else None for _ in range(c.heads)]
    return dict(x=x, w=ws, b=bs)  # w: [K][N] logical; the backend lays it out


# ---- short-reduction linear ---------------------------------------------------------------------------------------------------
SkCase = namedtuple("SkCase", "name via M N K layout bias_mod act off why")


def S(name, M, N, K, why, via="gemm", layout="kn", bias_mod=None, act=NONE, off=None):
    """bias_mod: None = no bias; 0 = a bias with bias_mod = 0 (read as period 1); via="linear": bias_mod is N or None."""
    return SkCase(name, via, M, N, K, layout, bias_mod, act, off, why)


SK_M, SK_N = 19, 12  # every K at one small shape: 19 rows = two workgroups of 8 + a partial one, three column groups
SK_CASES = [S(f"k{K}-{lay}", SK_M, SK_N, K, f"K4 = {cdiv(K, 4)}" + (", scalar weight loads" if lay == "nk" and K % 4 else ""),
              layout=lay, bias_mod=SK_N, act=ACTS[K % 4]) for lay in ("kn", "nk") for K in range(1, 33)]
SK_CASES += [
    S("woff-kn", 19, 12, 20, "[K][N] weights 4 bytes off: the scalar loads", off="W", bias_mod=12),
    S("woff-nk", 19, 12, 20, "torch Linear weights 4 bytes off: the scalar loads", layout="nk", off="W", bias_mod=12),
    S("xoff", 19, 12, 20, "X 4 bytes off: its loads are scalar, the kernel still runs", off="X", bias_mod=12),
    S("yoff", 19, 12, 20, "Y 4 bytes off: declined, the tiled engine writes it", off="Y", bias_mod=12),
    S("xoff-linear", 19, 12, 20, "the same through mvk_linear_fwd", via="linear", layout="nk", off="X", bias_mod=12),
    S("yoff-linear", 19, 12, 20, "the same through mvk_linear_fwd", via="linear", layout="nk", off="Y", bias_mod=12),
    S("N4", 37, 4, 20, "one column group: ctb = 1, 256 row groups for 8 rows", bias_mod=0, act=RELU),
    S("N400", 37, 400, 20, "ctb = 100 does not divide 256: 56 idle threads", bias_mod=1, act=LEAKY),
    S("N1024", 37, 1024, 20, "ctb = 256: one row group, every thread busy", bias_mod=128, act=RELU),
    S("N1028", 37, 1028, 20, "gy = 2 and ONE active column group in the second workgroup", bias_mod=1028, act=SIGMOID),
    S("N2048", 37, 2048, 20, "gy = 2, both full", layout="nk", bias_mod=128),
    S("R8-M2045-N400", 2045, 400, 20, "want = 8: 8 rows per workgroup, five rows in the last one; M = 2048 is the last such M", bias_mod=400, act=RELU),
    S("R8-M2048-N400", 2048, 400, 20, "want = 8: the last M with 8 rows per workgroup", layout="nk", bias_mod=400, act=LEAKY),
    S("R16-M2049-N400", 2049, 400, 20, "want = 9: the first M with 16 rows per workgroup, one row in the last one", bias_mod=400, act=RELU),
    S("R8-M1021-N2048", 1021, 2048, 20, "gy = 2: want = (2 M + 255) / 256 = 8: 8 rows, five in the last workgroup", layout="nk", bias_mod=128, act=RELU),
    S("R16-M1025-N2048", 1025, 2048, 20, "gy = 2: want = 9: 16 rows, one row in the last workgroup", layout="nk", bias_mod=128, act=RELU),
    S("linear-K20", 37, 400, 20, "mvk_linear_fwd: torch Linear rows, bias period N", via="linear", layout="nk", bias_mod=400, act=RELU),
    S("linear-K13-nobias", 600, 64, 13, "mvk_linear_fwd without a bias, scalar loads", via="linear", layout="nk", act=SIGMOID),
    S("linear-M1", 1, 64, 1, "one row, K = 1: seven of eight rows of the workgroup past M", via="linear", layout="nk", bias_mod=64),
]
SK_BY_NAME = {c.name: c for c in SK_CASES}

# mvk_gemm_smallk_amax: (name, M, N, K, layout, act, peak, why): peak = where max |Y| sits ("first", "last", "tail": the last,
# partial row group) or "neg" (every Y negative under NONE)
AmaxCase = namedtuple("AmaxCase", "name M N K layout act peak why")
AMAX_CASES = [
    AmaxCase("amax-first", 37, 1028, 20, "kn", RELU, "first", "the maximum at Y[0][0]; two column workgroups, one nearly idle"),
    AmaxCase("amax-last", 32, 1028, 20, "kn", RELU, "last", "the maximum at the last entry, written by the one-group workgroup"),
    AmaxCase("amax-tail", 37, 400, 13, "nk", LEAKY, "tail", "the maximum in the last, partial row group (37 = 4 x 8 + 5)"),
    AmaxCase("amax-neg", 19, 12, 20, "kn", NONE, "neg", "every Y negative without an activation: |Y| is what counts"),
    AmaxCase("amax-M1", 1, 400, 32, "nk", NONE, "first", "one row: seven of eight rows of the workgroup are past M"),
    AmaxCase("amax-R16", 2050, 400, 20, "kn", RELU, "tail", "16 rows per workgroup, two rows in the last one"),
]
AMAX_PRESETS = ("zero", "above", "below")


def sk_bias(c, g):
    if c.bias_mod is None:
        return None, None
    period = max(c.bias_mod, 1)
    bias = torch.randn(period, generator=g)
    return bias, bias[torch.arange(c.N) % period]


def sk_inputs(c):
    g = gen(c.name)
    x = torch.randn(c.M, c.K, generator=g) * (torch.rand(c.M, 1, generator=g) * 4 + 0.25)
    w = torch.randn(c.K, c.N, generator=g) * (torch.rand(1, c.N, generator=g) + 0.5) / math.sqrt(c.K)
    bias, full = sk_bias(c, g)
    return dict(x=x, w=w, bias=bias, bias_full=full)


def amax_inputs(c):
    g = gen(c.name)
    x = torch.randn(c.M, c.K, generator=g)
    w = torch.randn(c.K, c.N, generator=g) / math.sqrt(c.K)
    bias = torch.randn(c.N, generator=g)
    if c.peak == "neg":
        x, bias = x * 8.0, -32.0 - bias.abs()  # |X W| stays below 32 (asserted by the check: every Y negative)
        pos = None
    else:
        m, n = {"first": (0, 0), "last": (c.M - 1, c.N - 1), "tail": (c.M - 1, c.N // 2)}[c.peak]
        x[m] *= 16.0
        w[:, n] = 4.0 * torch.sign(x[m]) * w[:, n].abs() + torch.sign(x[m]) * 0.5
        bias[n] = bias[n].abs()
        if c.act in (RELU, LEAKY):  # a pre-activation of twice the peak's size and the other sign next to it: the activation takes it
            n2 = (n + 4) % c.N      # out, and a maximum taken in front of the activation would publish it
            w[:, n2], bias[n2] = -2.0 * w[:, n], -bias[n2].abs()
        pos = (m, n)
    return dict(x=x, w=w, bias=bias, bias_full=bias, pos=pos)


# ---- the heads' backward --------------------------------------------------------------------------------------------------------
BwdCase = namedtuple("BwdCase", "name M N K nh x_act layout flat_c dx dbprev bias targets via why")


def B(name, M, N, K, nh, why, x_act=RELU, layout="nk", flat_c=0, dx=True, dbprev=True, bias=True, targets="plain", via="c"):
    """targets: "plain" tensors (workspace slabs, finished by the call), "deferred" (inside deferred_reductions), "mixed" (dW0
    inside the flat buffer, the others outside).  via: "c" = mvk_heads_bwd, "py" = kernels.heads_bwd."""
    return BwdCase(name, M, N, K, nh, x_act, layout, flat_c, dx, dbprev, bias, targets, via, why)


BWD_CASES = [
    B("nn64-M300-K48", 300, 32, 48, 2, "NN = 64: every lane of the 64-wide load, all 256 weight-gradient threads, 61952 bytes of LDS"),
    B("nn64-M129-K512-def", 129, 32, 512, 2, "NN = 64 at K = 512 with a second row group of ONE row; deferred finish", targets="deferred",
      x_act=LEAKY, layout="kn"),
    B("n1-1h-M1-K16", 1, 1, 16, 1, "N = 1, one head, M = 1, K = 16: ONE column block, which is also the bias block", x_act=NONE),
    B("n1x2-M127", 127, 1, 48, 2, "N = 1 with two heads (NN = 2, even: NNP = 3); one row short of a full group; a bias gradient is ONE entry here", x_act=SIGMOID),
    B("n17-1h-M128", 128, 17, 48, 1, "odd NN = 17 = NNP; exactly one full row group", x_act=LEAKY, layout="kn"),
    B("n17-2h-M129", 129, 17, 48, 2, "even NN = 34, NNP = 35; one row in the second group", x_act=NONE),
    B("n32-1h-M300", 300, 32, 48, 1, "one head of 32 (NN = 32, NNP = 33)", x_act=SIGMOID, layout="kn"),
    B("n20-2h-M300-py", 300, 20, 512, 2, "the MnistSvhn heads through kernels.heads_bwd, deferred", targets="deferred", via="py"),
    B("n20-2h-M8192", 8192, 20, 16, 2, "rgs = 64, the limit, at K = 16", targets="deferred"),
    B("n20-2h-M8192-plain", 8192, 20, 16, 2, "rgs = 64 finished by colsum_finish from the workspace", x_act=LEAKY),
    B("nodx", 129, 20, 48, 2, "dX = NULL: nothing but the slabs is written", dx=False),
    B("nodx-py", 129, 20, 48, 2, "want_dx=False through kernels.heads_bwd", dx=False, via="py", layout="kn"),
    B("noprev", 129, 20, 48, 2, "dbprev = NULL: no pslab, the bias block starts right behind the Ds barrier", dbprev=False),
    B("noprev-K16", 300, 17, 16, 1, "dbprev = NULL at one column block", dbprev=False, x_act=NONE),
    B("nobias", 129, 20, 48, 2, "bias targets NULL: their slabs go to the workspace and get no finish", bias=False),
    B("nobias-def", 129, 17, 48, 1, "bias target NULL inside deferred_reductions: a workspace slab beside deferred ones", bias=False,
      targets="deferred"),
    B("flat4-1h", 129, 20, 16, 1, "flat_c = 4 with one head: prow = 4 partial rows per group, nrows = nz prow in colsum_finish", flat_c=4),
    B("flat4-2h-def", 300, 20, 48, 2, "flat_c = 4 with two heads, deferred", flat_c=4, targets="deferred", layout="kn"),
    B("flatK-1h", 129, 17, 48, 1, "flat_c = K: one tap, the permutation is the identity, prow = 1", flat_c=48, x_act=LEAKY),
    B("flatK-2h", 127, 20, 16, 2, "flat_c = K with two heads at one column block", flat_c=16, x_act=NONE),
    B("flat128-svhn", 300, 20, 512, 2, "flat_c = 128 at K = 512: four taps of the Conv2d heads", flat_c=128, layout="kn", targets="deferred"),
    B("mixed", 300, 20, 48, 2, "dW0 inside the flat buffer, every other target outside: one deferred and four workspace slabs",
      targets="mixed"),
    B("mixed-flat4", 129, 17, 16, 1, "the same with flat_c and one head", targets="mixed", flat_c=4, layout="kn"),
]
BWD_BY_NAME = {c.name: c for c in BWD_CASES}

# declines: (name, base case fields changed, what)
BwdDecline = namedtuple("BwdDecline", "name M N K nh flat_c off ws_short python_none why")
BWD_DECLINES = [
    BwdDecline("N33", 17, 33, 48, 1, 0, None, False, True, "N = 33"),
    BwdDecline("K24", 17, 20, 24, 2, 0, None, False, True, "K = 24 is no multiple of 16"),
    BwdDecline("M8193", 8193, 4, 16, 1, 0, None, False, True, "65 row groups"),
    BwdDecline("flat5", 17, 20, 48, 2, 5, None, False, False, "flat_c = 5 does not divide 48"),
    BwdDecline("ws-short", 129, 20, 48, 2, 0, None, True, False, "workspace one float below the slabs"),
    BwdDecline("x-off", 17, 20, 48, 2, 0, "X", False, False, "X 4 bytes off"),
    BwdDecline("dx-off", 17, 20, 48, 2, 0, "dX", False, False, "dX 4 bytes off"),
]


def bwd_inputs(M, N, K, nh, x_act, name):
    g = gen(name)
    ms = axis_scale(M, g)[:, None]
    x = act_out(torch.randn(M, K, generator=g), x_act)
    dys = [torch.randn(M, N, generator=g) * ms for _ in range(nh)]
    ws = [torch.randn(N, K, generator=g) * (torch.rand(N, 1, generator=g) + 0.5) / math.sqrt(nh * N) for _ in range(nh)]
    return dict(x=x, dys=dys, ws=ws)


def bwd_targets(c):
    """Names and shapes of the accumulated targets of a case, in the C side's slab order."""
    pc = c.flat_c if c.flat_c > 0 else c.K
    t = []
    for h in range(c.nh):
        t.append((f"dW{h}", (c.N, c.K)))
    if c.bias:
        for h in range(c.nh):
            t.append((f"db{h}", (c.N,)))
    if c.dbprev:
        t.append(("dbprev", (pc,)))
    return sorted(t, key=lambda kv: SLAB_ORDER.index(kv[0]))


def bwd_inits(c):
    """Non-zero initial content of every target: the launch accumulates."""
    g = gen(c.name + "/init")
    return {k: torch.randn(*s, generator=g) * 0.25 for k, s in bwd_targets(c)}


def bwd_ws_need(c):
    """Workspace floats the C side takes: every slab whose target is not deferred (NULL bias targets included)."""
    p = heads_bwd_plan(c.M, c.N, c.K, c.nh, c.flat_c)
    names = [k for k in SLAB_ORDER if k in p.slabs and (k != "dbprev" or c.dbprev)]
    deferred = {"plain": [], "deferred": [k for k, _ in bwd_targets(c)], "mixed": ["dW0"]}[c.targets]
    return sum(p.slabs[k] for k in names if k not in deferred)


def bwd_kernels(c):
    """Kernels of a plain-target launch (deferred targets are finished by the scope's one launch, whose name is not pinned here)."""
    k = {HBWD}
    if c.targets == "plain":
        pc = c.flat_c if c.flat_c > 0 else c.K
        p = heads_bwd_plan(c.M, c.N, c.K, c.nh, c.flat_c)
        off, cnts = 0, dict(dW0=c.N * c.K, dW1=c.N * c.K, db0=c.N, db1=c.N, dbprev=pc)
        present = {n for n, _ in bwd_targets(c)}
        for n in SLAB_ORDER:
            if n not in p.slabs or (n == "dbprev" and not c.dbprev):
                continue
            if n in present:  # colsum_finish_any: float4 form for N % 4 == 0 at a 16-byte slab (offsets are multiples of 4 floats)
                k.add(FIN if cnts[n] % 4 == 0 and off % 4 == 0 else FINS)
            off += p.slabs[n]
    return sorted(k)
