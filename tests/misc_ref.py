"""Float64 references, exact index / bit models, case tables and error constants for the helper kernels of csrc/misc.hip
(tests/test_gpu_misc.py on the GPU, tests/test_misc_ref_host.py on the CPU).  CPU only: torch and numpy.

Every reference takes `mut`, a tuple of names of deliberately wrong variants (TEETH): test_misc_ref_host.py shows that each of
them leaves the bound on a named case, i.e. that the bounds below can see the defect they are there for.

Error model.  U = 2^-24 is the unit roundoff of fp32; a bound is `C * base` per ENTRY, base in absolute units.
Derived from the number of roundings (C_STAGE entries marked "derived"):
  act_bwd, sigmoid      y (1 - y) dY: the difference, the product, the product = 3 roundings, (1 + U)^3 - 1 < 4 U, base = U |ref|
  act_bwd_scaled, sigm. a g y (1 - y): one product more = 4 roundings < 5 U, base = U |ref|
  axpby                 a x + b y evaluated as two products and a sum or as one product and an FMA (the compiler may contract):
                        at most 3 roundings, each on a quantity <= |a x| + |b y|: 3 U (|a x| + |b y|)
  pooling               at most 9 addends = 8 additions on partial sums <= sum|x|, the rounded constant 1/9 and the product:
                        10 roundings, 10 U sum|x| / 9 (backward: at most 4 addends, the same bound on sum|dy| / 9)
  upsample backward     (p00 + p01) + (p10 + p11): two roundings on any path, 3 U sum|p|
  uniform draws         lo + u (hi - lo): (hi - lo), the product, the sum (or an FMA): 3 U (|lo| + u |hi - lo|); exact at (0, 1)
A result below the normal range carries an absolute rounding error of one subnormal spacing, 2^-149, which every base includes.
Measured (C_STAGE entries of the Adam stages and of the normal draws): 4x the largest |err| / base of a plain fp32 CPU
evaluation of the same formula (torch.optim.Adam(foreach=False); numpy float32 Box-Muller) against the float64 reference over
the case table, rounded up; test_misc_ref_host.py::test_error_constants re-derives them.  Their bases:
  adam.m     U (|m| + |g'|), g' = |g gscale| + wd |p|             (the lerp cancels: the error is relative to its operands)
  adam.v     U (b2 v + (1 - b2) g'^2)                             (both terms non-negative: relative to the result)
  adam.vmax  the base of adam.v, or U vmax where the old maximum stays
  adam.p     U (|p'| + step_size (|m| + |g'|) / denom)            (the errors of m over the denominator, and of the quotient)
  rng.normal U r (1 + theta), r = sqrt(-2 ln u1), theta = 2 pi u2 (the relative error of r and the absolute error U theta of the angle)
"""
import collections
import math

import numpy as np
import torch

F64 = torch.float64
U = 2.0 ** -24
SUB = 2.0 ** -149
NONE, RELU, SIGMOID, LEAKY = 0, 1, 2, 3
F02 = float(torch.tensor(0.2, dtype=torch.float32))  # the kernels' 0.2f
BIG = 2048 * 256  # elements one sweep of a capped 2048-workgroup grid covers

C_STAGE = {
    "act_bwd.sigmoid": 4, "act_bwd_scaled.sigmoid": 5, "axpby": 3, "pool.fwd": 10, "pool.bwd": 10, "up.bwd": 3, "rng.uniform": 3,  # derived
    "adam.m": 4, "adam.v": 16, "adam.vmax": 13, "adam.p": 9, "rng.normal": 9,  # measured (test_error_constants)
}
MEASURED_STAGES = ("adam.m", "adam.v", "adam.vmax", "adam.p", "rng.normal")


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def gen(seed):
    return torch.Generator().manual_seed(seed)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def worst_ratio(got, ref, base):
    """Largest |got - ref| / base over the entries (0 / 0 counts as 0, x / 0 as inf)."""
    err = (got.double() - ref.double()).abs().reshape(-1)
    base = base.double().reshape(-1).expand_as(err)
    r = torch.where(err == 0, torch.zeros_like(err), err / base.clamp_min(1e-300))
    return float(r.max()) if r.numel() else 0.0


# ---- weight packs: pure permutations ------------------------------------------------------------------------------------------------------
PackCase = collections.namedtuple("PackCase", "name kind Cv Cu frags off ld_mul col_off why")


def _pc(kind, Cv, Cu, why, frags=False, off=False, ld_mul=1, col_off=0):
    name = f"k{kind}-cv{Cv}-cu{Cu}" + ("-frag" if frags else "") + ("-off" if off else "") + (f"-ld{ld_mul}-co{col_off}" if ld_mul > 1 else "")
    return PackCase(name, kind, Cv, Cu, frags, off, ld_mul, col_off, why)


PACK_CASES = [
    _pc(0, 8, 8, "one tile of the tiled branch"),
    _pc(0, 16, 24, "several tiles, Cu != Cv"),
    _pc(0, 64, 32, "tiled, first fragment pair of mvk_imgconv_frag_bytes", frags=True),
    _pc(0, 128, 64, "tiled, second fragment pair", frags=True),
    _pc(0, 256, 128, "512 tiles on 256 workgroups: the tile loop strides"),
    _pc(0, 32, 3, "generic branch: Cu % 8 != 0"),
    _pc(0, 3, 32, "generic branch: Cv % 8 != 0"),
    _pc(0, 1, 1, "generic branch, one workgroup with 16 live lanes"),
    _pc(0, 64, 32, "Wref 4 bytes off: generic branch WITH fragments", frags=True, off=True),
    _pc(0, 128, 64, "the same, 131072 elements on 256 x 256 threads: the element loop strides", frags=True, off=True),
    _pc(0, 8, 16, "ld_down = 2 Cv, col_off = Cv: tiled, the other half of the rows stays untouched", ld_mul=2, col_off=8),
    _pc(0, 8, 16, "ld_down = 2 Cv, col_off = 2: generic (col_off % 4 != 0)", ld_mul=2, col_off=2),
    _pc(1, 5, 7, "unflatten pack, odd sizes"),
    _pc(1, 20, 128, "unflatten pack of the MNIST decoder's size"),
    _pc(2, 20, 20, "3x3 pack, one sweep"),
    _pc(2, 128, 128, "3x3 pack, 147456 elements: more than the 65536 one sweep of pack_amax covers"),
]
PACK_BY_NAME = {c.name: c for c in PACK_CASES}
assert len(PACK_BY_NAME) == len(PACK_CASES)


def pack_taps(kind):
    return 9 if kind == 2 else 16


def pack_weight(case):
    """Wref[Cv][Cu][taps]: normal entries (so are the residues of their bf16 split), no two equal in magnitude at the top."""
    return torch.randn(case.Cv, case.Cu, pack_taps(case.kind), generator=gen(case.Cv * 1000 + case.Cu * 10 + case.kind))


def pack_ref(kind, W, mut=()):
    """-> (Wdown or None, Wup): the layouts of include/mvk.h.  W: [Cv][Cu][taps]."""
    Cv, Cu = W.shape[0], W.shape[1]
    if kind == 1:  # Wref[ci][co][tap] -> Wup[ci][tap * Cout + co]
        return None, W.permute(0, 2, 1).reshape(Cv, 16 * Cu).contiguous()
    if kind == 2:  # Wdown[tap * Cu + cu][cv], Wup[(8 - tap) * Cv + cv][cu]
        Wb = W if "k2_not_mirrored" in mut else W.flip(2)
        return W.permute(2, 1, 0).reshape(9 * Cu, Cv).contiguous(), Wb.permute(2, 0, 1).reshape(9 * Cv, Cu).contiguous()
    W4 = W.reshape(Cv, Cu, 4, 4)
    if "khkw_swapped" in mut:
        W4 = W4.transpose(2, 3)
    Wdown = W4.permute(2, 3, 1, 0).reshape(16 * Cu, Cv).contiguous()  # [(kh * 4 + kw) * Cu + cu][cv]
    # kh = (1 - ph) + 2 a: kh = 2 a + rh with rh = 1 - ph, so ph runs against rh
    W6 = W4.reshape(Cv, Cu, 2, 2, 2, 2)  # [cv][cu][a][rh][b][rw]
    if "parity_flipped" not in mut:
        W6 = W6.flip(3, 5)  # [cv][cu][a][ph][b][pw]
    Wup = W6.permute(3, 5, 2, 4, 0, 1).reshape(4, 4 * Cv, Cu).contiguous()  # [ph * 2 + pw][(a * 2 + b) * Cv + cv][cu]
    return Wdown, Wup


def pack_ref_loops(kind, W):
    """The same layouts as plain loops over the definitions (the host test holds pack_ref to it)."""
    Cv, Cu, T = W.shape
    if kind == 1:
        up = W.new_empty(Cv, 16 * Cu)
        for tap in range(16):
            for co in range(Cu):
                up[:, tap * Cu + co] = W[:, co, tap]
        return None, up
    if kind == 2:
        down, up = W.new_empty(9 * Cu, Cv), W.new_empty(9 * Cv, Cu)
        for tap in range(9):
            for cu in range(Cu):
                down[tap * Cu + cu, :] = W[:, cu, tap]
                up[(8 - tap) * Cv:(9 - tap) * Cv, cu] = W[:, cu, tap]
        return down, up
    down, up = W.new_empty(16 * Cu, Cv), W.new_empty(4, 4 * Cv, Cu)
    for ph in range(2):
        for pw in range(2):
            for a in range(2):
                for b in range(2):
                    kh, kw = (1 - ph) + 2 * a, (1 - pw) + 2 * b
                    up[ph * 2 + pw, (a * 2 + b) * Cv:(a * 2 + b + 1) * Cv, :] = W[:, :, kh * 4 + kw]
                    down[(kh * 4 + kw) * Cu:(kh * 4 + kw + 1) * Cu, :] = W[:, :, kh * 4 + kw].t()
    return down, up


def place_down(Wdown, ld, col_off, fill=float("nan")):
    """Wdown written with leading dimension ld at column col_off into a `fill`-prefilled [rows][ld] array."""
    out = torch.full((Wdown.shape[0], ld), fill)
    out[:, col_off:col_off + Wdown.shape[1]] = Wdown
    return out


# ---- the three-piece bf16 split ---------------------------------------------------------------------------------------------------------
def bf3_split(x):
    """x (fp32) -> int16 [3][n]: three round-to-nearest-even bfloat16 casts of successive residues (the residues are exact in fp32)."""
    x = x.reshape(-1).float()
    p0 = x.bfloat16()
    r1 = x - p0.float()
    p1 = r1.bfloat16()
    r2 = r1 - p1.float()
    p2 = r2.bfloat16()
    return torch.stack([p.view(torch.int16) for p in (p0, p1, p2)])


def bf3_join(planes):
    """int16 [3][n] -> fp32 a + (b + c), the expression of bf3_to_f32_kernel."""
    a, b, c = (p.view(torch.bfloat16).float() for p in planes)
    return a + (b + c)


def bf3_input(n, seed=0):
    """Normal values on scales 2^-90 .. 2^90 (|x| >= 2^-100, the range test_bf3_roundtrip_condition proves), plus the hand-picked
    patterns at the front."""
    g = gen(1000 + n + seed)
    x = torch.randn(n, generator=g) * torch.exp2(torch.randint(-90, 91, (n,), generator=g).float())
    x = torch.where(x.abs() < 2.0 ** -100, torch.ones_like(x), x)
    pat = BF3_PATTERNS[:n]
    x[:len(pat)] = pat
    return x


def _bits_to_f32(words):
    return torch.tensor(np.array(words, dtype=np.uint32).view(np.float32).copy())


# (values whose first piece rounds up to infinity, |x| >= 0x7F7F8000, are outside the format's contract and left out)
BF3_PATTERNS = _bits_to_f32([
    0x3FFFFFFF, 0xBFFFFFFF, 0x3F7FFFFF, 0x3F800000, 0x40000000, 0x0D800000, 0x7F000000,   # all-ones mantissa, powers of two
    0x3F808000, 0x3F818000, 0x3F800080, 0x3F800180, 0x3F808080, 0x3F7F8000, 0x3F80FFFF,   # ties of the first / second cast
    0x3F807FFF, 0x3F808001, 0x3F800001, 0xBF808000, 0xBF818000,                           # next to a tie, negative ties
])


# ---- layout -------------------------------------------------------------------------------------------------------------------------------
LAYOUT_SHAPES = [(1, 1, 1, 1), (2, 3, 5, 7), (3, 4, 1, 9), (5, 64, 2, 2)]  # (n, c, h, w)


# ---- activations ---------------------------------------------------------------------------------------------------------------------------
def act_grad64(y, act, mut=()):
    y = y.double()
    if act == RELU:
        return (y > 0).double()
    if act == LEAKY:
        return torch.where(y > 0, torch.ones_like(y), torch.full_like(y, 0.01 if "leaky_001" in mut else F02))
    if act == SIGMOID:
        if "sigmoid_from_pre" in mut:
            s = torch.sigmoid(y)
            return s * (1 - s)
        return y * (1 - y)
    return torch.ones_like(y)


def act_grad32(y, act):
    """The fp32 expression of mvk_act_grad_from_out."""
    if act == RELU:
        return (y > 0).float()
    if act == LEAKY:
        return torch.where(y > 0, torch.ones_like(y), torch.full_like(y, F02))
    if act == SIGMOID:
        return y * (1.0 - y)
    return torch.ones_like(y)


ACT_SPECIAL = [0.0, -0.0, -1.5, 1e-40, 1.0, -1e-40, 0.5, 2.0]  # zero of both signs, negative, subnormal, exactly 1


def act_inputs(n, act, seed=0):
    """(dY, Y): Y is a plausible OUTPUT of the activation (sigmoid: in [0, 1]) with the special values at the front."""
    g = gen(77 + n % 1000 + 7 * act + seed)
    dY = torch.randn(n, generator=g)
    if act == SIGMOID:
        Y = torch.rand(n, generator=g)
        sp = [0.0, 1e-40, 1.0, 0.5, f32(1 - 2.0 ** -24), 2.0 ** -30]
    else:
        Y = torch.randn(n, generator=g)
        sp = ACT_SPECIAL
    k = min(n, len(sp))
    Y[:k] = torch.tensor(sp[:k])
    return dY, Y


ACT_BWD_N = [1, 3, 4, 5, 1023, 1024, 1028]
ACT_SCALED_N = [1, 2, 3, 4, 5, 6, 7, 8, 9, 1023, 1024, 1025, 1027]
ACTS = [NONE, RELU, SIGMOID, LEAKY]


def axpby_ref(x, a, y, b):
    """-> (float64 pre-activation, base / U)."""
    ax = a * x.double() if x is not None else 0.0
    by = b * y.double() if y is not None else 0.0
    ref = ax + by
    mag = (ax.abs() if x is not None else 0.0) + (by.abs() if y is not None else 0.0)
    return ref, mag


def sigmoid_ulps(got, ref64):
    """|got - ref| in units of the fp32 spacing at |ref|."""
    ulp = torch.exp2(torch.floor(torch.log2(ref64.abs().clamp_min(2.0 ** -126))) - 23)
    return float(((got.double() - ref64).abs() / ulp).max())


# ---- pooling and upsampling on NHWC -------------------------------------------------------------------------------------------------------
POOL_SHAPES = [(1, 1, 1, 1), (2, 1, 5, 4), (2, 2, 2, 8), (3, 3, 7, 6), (2, 5, 9, 3), (2, 7, 7, 20)]  # (n, H, W, C)


def pool_name(s, off=False):
    return "x".join(map(str, s)) + ("-off" if off else "")


def pool_inputs(shape, op):
    n, H, W, C = shape
    OH, OW = (H + 1) // 2, (W + 1) // 2
    dims = {"pool.fwd": (n, H, W, C), "pool.bwd": (n, OH, OW, C), "up.fwd": (n, H, W, C), "up.bwd": (n, 2 * H, 2 * W, C)}[op]
    return torch.randn(*dims, generator=gen(sum(shape) + len(op)))


def pool_fwd_ref(x, mut=()):
    """AvgPool2d(3, 2, 1), count_include_pad: y[b, oh, ow] = sum of the valid x[b, 2 oh - 1 + kh, 2 ow - 1 + kw] / 9.
    -> (float64 y, sum|x| of the window)."""
    n, H, W, C = x.shape
    OH, OW = (H + 1) // 2, (W + 1) // 2
    x = x.double()
    y, mag = torch.zeros(n, OH, OW, C, dtype=F64), torch.zeros(n, OH, OW, C, dtype=F64)
    for oh in range(OH):
        for ow in range(OW):
            cnt = 0
            for kh in range(3):
                for kw in range(3):
                    h, w = 2 * oh - 1 + kh, 2 * ow - 1 + kw
                    if 0 <= h < H and 0 <= w < W:
                        y[:, oh, ow] += x[:, h, w]
                        mag[:, oh, ow] += x[:, h, w].abs()
                        cnt += 1
            y[:, oh, ow] /= cnt if "valid_count" in mut else 9
    return y, mag


def pool_bwd_ref(dy, H, W, mut=()):
    """dx[b, h, w] = (1 / 9) sum of dy over the windows that contain (h, w): oh in {h / 2, (h + 1) / 2}, clipped to oh < OH."""
    n, OH, OW, C = dy.shape
    assert (OH, OW) == ((H + 1) // 2, (W + 1) // 2)
    flat = torch.cat([dy.double().reshape(-1), torch.zeros(2 * OW * C + C, dtype=F64)])  # what an unclipped read would run into
    dx, mag = torch.zeros(n, H, W, C, dtype=F64), torch.zeros(n, H, W, C, dtype=F64)
    for b in range(n):
        for h in range(H):
            for w in range(W):
                for oh in sorted({h // 2, (h + 1) // 2}):
                    if oh >= OH and "no_oh_clip" not in mut:
                        continue
                    for ow in sorted({w // 2, (w + 1) // 2}):
                        if ow >= OW:
                            continue
                        o = ((b * OH + oh) * OW + ow) * C
                        dx[b, h, w] += flat[o:o + C]
                        mag[b, h, w] += flat[o:o + C].abs()
    return dx / 9, mag


def up_fwd_ref(x):
    return x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def up_bwd_ref(dy, mut=()):
    d = dy.double()
    taps = [d[:, 0::2, 0::2], d[:, 0::2, 1::2], d[:, 1::2, 0::2], d[:, 1::2, 1::2]]
    if "drop_tap" in mut:
        taps = taps[:3]
    mag = d.abs()
    return sum(taps), mag[:, 0::2, 0::2] + mag[:, 0::2, 1::2] + mag[:, 1::2, 0::2] + mag[:, 1::2, 1::2]


# ---- Adam ---------------------------------------------------------------------------------------------------------------------------------
AdamCase = collections.namedtuple("AdamCase", "name entry n off step wd gscale ams zero regime lr why")
ADAM_HYPER = dict(b1=0.9, b2=0.999, eps=1e-8)


def _ac(entry, n, why, off=None, step=1, wd=0.0, gscale=1.0, ams=None, zero=False, regime="plain", lr=1e-3):
    ams = (entry in ("amsgrad",)) if ams is None else ams
    name = f"{entry}-n{n}-s{step}" + (f"-off_{off}" if off else "") + ("-wd" if wd else "") + ("-gs" if gscale != 1 else "") + \
           ("-ams" if ams else "") + ("-zero" if zero else "") + (f"-{regime}" if regime != "plain" else "")
    return AdamCase(name, entry, n, off, step, wd, gscale, ams, zero, regime, lr, why)


ADAM_CASES = [
    _ac("step", 1, "scalar kernel, one live lane"),
    _ac("step", 3, "scalar kernel, n % 4 != 0", step=2, wd=0.01),
    _ac("step", 4, "float4 kernel, one live lane", step=1000, gscale=0.5),
    _ac("step", 1028, "float4 kernel, second block with one live lane", wd=0.01, gscale=0.5),
    _ac("step", 4 * 256 + 4, "float4 kernel: 257 quads", step=2),
    _ac("step", BIG + 5, "scalar kernel past the 2048-workgroup cap: the grid-stride loop runs twice", step=1000, wd=0.01),
    _ac("amsgrad", 1028, "running maximum above and below the new v", step=2),
    _ac("amsgrad", 3, "amsgrad on the scalar kernel", wd=0.01, gscale=0.5),
    _ac("fused", 1028, "zero_grad: g cleared as it is consumed", zero=True, step=2),
    _ac("fused", 1027, "zero_grad on the scalar kernel", zero=True, ams=True, step=1000),
    _ac("fused", 4 * 256 + 4, "amsgrad + zero_grad, float4", zero=True, ams=True, wd=0.01),
    _ac("fused", 1028, "v = g = m = 0 leaves p bit for bit", regime="zeros"),
    _ac("fused", 1028, "moments at the scale of eps^2: the place of eps in the denominator decides the step", regime="tiny", step=2),
    _ac("pub", 1028, "the scalars are published by the update launch", step=2, wd=0.01, gscale=0.5),
    _ac("pub", 5, "published from the scalar kernel", step=1000),
    _ac("dev", 4, "device scalars, one live lane"),
    _ac("dev", 1028, "device scalars, second block", step=2, wd=0.01, gscale=0.5),
    _ac("dev", 4 * 256 + 4, "device scalars, amsgrad + zero_grad", step=1000, ams=True, zero=True),
] + [_ac("fused", 1028, f"{b} alone 4 bytes off: the scalar kernel", off=b, ams=True, step=2, wd=0.01) for b in ("p", "g", "m", "v", "vmax")]
ADAM_BY_NAME = {c.name: c for c in ADAM_CASES}
assert len(ADAM_BY_NAME) == len(ADAM_CASES)


def adam_inputs(case):
    g_ = gen(len(case.name) * 131 + case.n % 977 + case.step)
    n = case.n
    if case.regime == "zeros":
        return dict(p=torch.randn(n, generator=g_), g=torch.zeros(n), m=torch.zeros(n), v=torch.zeros(n), vmax=None)
    if case.regime == "tiny":
        return dict(p=torch.randn(n, generator=g_) * 1e-3, g=torch.randn(n, generator=g_) * 1e-6, m=torch.randn(n, generator=g_) * 1e-6,
                    v=torch.rand(n, generator=g_) * 1e-12 + 1e-14, vmax=None)
    p = torch.randn(n, generator=g_)
    g = torch.randn(n, generator=g_) * torch.exp2(torch.randint(-8, 3, (n,), generator=g_).float())
    m = torch.randn(n, generator=g_) * 0.1
    v = torch.rand(n, generator=g_) * 0.01 + 1e-6
    vmax = None
    if case.ams:  # half the entries above the new v, half below
        vmax = v * torch.where(torch.arange(n) % 2 == 0, torch.full((n,), 4.0), torch.full((n,), 0.25))
    return dict(p=p, g=g, m=m, v=v, vmax=vmax)


def adam_scalars(lr, step, wd, gscale, b1=0.9, b2=0.999, eps=1e-8):
    """The eight floats of AdamScalars in Python double (step_size, 1 - b1, b2, 1 - b2, eps, wd, sqrt(bc2), gscale)."""
    return [lr / (1.0 - b1 ** step), 1.0 - b1, b2, 1.0 - b2, eps, wd, math.sqrt(1.0 - b2 ** step), gscale]


def adam_ref(case, inp, mut=()):
    """torch's single-tensor Adam rule in float64 from the fp32 inputs.  -> (outputs, bases / 1)."""
    ss, omb1, b2, omb2, eps, wd, bc2s, gs = adam_scalars(case.lr, case.step, case.wd, case.gscale)
    p, g, m, v = (inp[k].double() for k in "pgmv")
    ge = g * gs
    gmag = ge.abs() + wd * p.abs()
    if "wd_after_moments" not in mut:
        ge = ge + wd * p
    m1 = m + (ge - m) * omb1
    v1 = v * b2 + omb2 * ge * ge
    if "wd_after_moments" in mut:
        ge = ge + wd * p
    out, base = {}, {}
    vd = v1
    if case.ams:
        vmax = inp["vmax"].double()
        vd = torch.maximum(vmax, v1)
        out["vmax"] = v1 if "ams_not_kept" in mut else vd
        base["vmax"] = U * vd + SUB
    if "eps_in_sqrt" in mut:
        denom = torch.sqrt(vd + eps) / bc2s
    else:
        denom = torch.sqrt(vd) / (1.0 if "no_bc2" in mut else bc2s) + eps
    p1 = p - ss * (m1 / denom)
    out.update(p=p1, m=m1, v=v1, g=torch.zeros_like(g) if case.zero else inp["g"].double())
    base.update(m=U * (m.abs() + gmag) + SUB, v=U * (v * b2 + omb2 * gmag * gmag) + SUB,
                p=U * (p1.abs() + ss * (m.abs() + gmag) / denom) + SUB)
    return out, base


def adam_torch(case, inp, dtype=torch.float32):
    """torch.optim.Adam(foreach=False) on the CPU; in fp32: the plain evaluation the constants are derived from, and the stand-in
    launcher of the host test.  The gradient scale (which torch does not have) is one product in front, as in adam_one."""
    inp = {k: (None if t is None else t.to(dtype)) for k, t in inp.items()}
    p = inp["p"].clone().requires_grad_(True)
    g = inp["g"].clone()
    p.grad = g * torch.tensor(case.gscale, dtype=dtype)
    opt = torch.optim.Adam([p], lr=case.lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=case.wd, amsgrad=case.ams, foreach=False)
    st = dict(step=torch.tensor(float(case.step - 1)), exp_avg=inp["m"].clone(), exp_avg_sq=inp["v"].clone())
    if case.ams:
        st["max_exp_avg_sq"] = inp["vmax"].clone()
    opt.state[p] = st
    opt.step()
    out = dict(p=p.detach().clone(), m=st["exp_avg"], v=st["exp_avg_sq"], g=torch.zeros_like(g) if case.zero else g)
    if case.ams:
        out["vmax"] = st["max_exp_avg_sq"]
    return out


def adam_ratios(case, got, ref, base):
    return {f"adam.{k}": worst_ratio(got[k], ref[k], base[k]) for k in ("p", "m", "v", "vmax") if k in ref}


# ---- Philox4x32-10 and the two maps ---------------------------------------------------------------------------------------------------------
PHILOX_KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]
M32 = np.uint64(0xFFFFFFFF)


def philox(ctr, key, mut=()):
    """Philox4x32-10 on numpy uint64 arrays.  ctr: four arrays (or scalars), key: two.  -> uint64 [4][n] of 32-bit words."""
    c = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) & M32 for x in ctr]
    n = max(len(x) for x in c)
    c = [np.broadcast_to(x, (n,)).copy() for x in c]
    k0, k1 = (np.uint64(int(k) & 0xFFFFFFFF) for k in key)
    m0 = np.uint64(0xD2511F53 if "round_constant" not in mut else 0xD2511F55)
    m1 = np.uint64(0xCD9E8D57)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]  # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack(c)


def rng_words(seed, offset, n, mut=()):
    """The words behind out[0 .. n): thread t = i / 4 runs counter (offset + t) mod 2^64 split into two words, key = seed.
    -> uint64 [threads][4]."""
    threads = (n + 3) // 4
    t = np.arange(threads, dtype=np.uint64) + np.uint64(1 if "counter_off_by_one" in mut else 0)
    with np.errstate(over="ignore"):
        ctr = np.uint64(offset) + t  # wraps mod 2^64 like the kernel's unsigned long long
    hi = ctr >> np.uint64(32)
    if "no_carry" in mut:
        hi = np.full_like(hi, np.uint64(offset) >> np.uint64(32))
    z = np.zeros(threads, dtype=np.uint64)
    return philox((ctr & M32, hi, z, z), (seed & 0xFFFFFFFF, seed >> 32), mut).T.copy()


def rng_uniform_ref(words, n, lo=0.0, hi=1.0):
    """-> (float64 lo + (c >> 8) 2^-24 (hi - lo), base / U)."""
    u = (words >> np.uint64(8)).astype(np.float64).reshape(-1)[:n] * 2.0 ** -24
    span = float(np.float32(hi) - np.float32(lo))  # the kernel's fp32 difference is part of the formula's input here
    return torch.from_numpy(lo + u * (hi - lo)), torch.from_numpy(abs(lo) + u * abs(span))


def rng_normal_ref(words, n, mut=(), dtype=np.float64):
    """Box-Muller of each thread's word pairs (c0, c1), (c2, c3): u1 = ((c >> 8) + 1) 2^-24 in (0, 1], u2 = (c' >> 8) 2^-24;
    out = r cos(2 pi u2), r sin(2 pi u2), r = sqrt(-2 ln u1).  -> (values, base / U) in `dtype` (float32: the plain fp32 evaluation)."""
    w = (words >> np.uint64(8)).reshape(-1, 2)
    one = 0 if "u1_no_plus_one" in mut else 1
    u1 = ((w[:, 0] + np.uint64(one)).astype(dtype) * dtype(2.0 ** -24)).astype(dtype)
    u2 = (w[:, 1].astype(dtype) * dtype(2.0 ** -24)).astype(dtype)
    with np.errstate(divide="ignore"):
        r = np.sqrt(dtype(-2.0) * np.log(u1)).astype(dtype)
    th = (dtype(6.28318530717958647692) * u2).astype(dtype)
    a, b = (r * np.cos(th)).astype(dtype), (r * np.sin(th)).astype(dtype)
    if "sincos_swapped" in mut:
        a, b = b, a
    val = np.stack([a, b], axis=1).reshape(-1)[:n]
    base = np.repeat(r.astype(np.float64) * (1.0 + th.astype(np.float64)), 2)[:n]
    return torch.from_numpy(val.copy()), torch.from_numpy(base.copy())


RngCase = collections.namedtuple("RngCase", "name seed offset n off why")
SEED_HI = 0x9E3779B97F4A7C15
RNG_CASES = [
    RngCase("s0-o0-n4", 0, 0, 4, False, "the first known answer through the kernel"),
    RngCase("hi-carry-n1", SEED_HI, 2 ** 32 - 3, 1, False, "one thread, three dead lanes of the store"),
    RngCase("hi-carry-n5", SEED_HI, 2 ** 32 - 3, 5, False, "a tail thread with one live value"),
    RngCase("hi-carry-n1024", SEED_HI, 2 ** 32 - 3, 1024, False, "the counter carries into its second word at thread 3"),
    RngCase("hi-carry-n1025", SEED_HI, 2 ** 32 - 3, 4 * 256 + 1, False, "two workgroups: the ticket counts to 2"),
    RngCase("hi-carry-n1025-off", SEED_HI, 2 ** 32 - 3, 4 * 256 + 1, True, "out 4 bytes off: the scalar stores"),
    RngCase("hi-2^40-n1024", SEED_HI, 2 ** 40 + 7, 1024, False, "a high counter word that is set before the launch"),
    RngCase("s1-o5-n65536", 1, 5, 65536, False, "64 workgroups; 32768 pairs reach u1 near 2^-15, where the + 1 of u1 weighs most"),
]
RNG_BY_NAME = {c.name: c for c in RNG_CASES}

# ---- the wrong variants and the case each one must fail on (test_misc_ref_host.py::test_teeth) ----------------------------------------
TEETH = [
    ("khkw_swapped", "pack", "k0-cv8-cu8"), ("parity_flipped", "pack", "k0-cv16-cu24"), ("k2_not_mirrored", "pack", "k2-cv20-cu20"),
    ("no_bc2", "adam", "step-n1-s1"), ("eps_in_sqrt", "adam", "fused-n1028-s2-tiny"), ("wd_after_moments", "adam", "step-n3-s2-wd"),
    ("ams_not_kept", "adam", "amsgrad-n1028-s2-ams"),
    ("valid_count", "pool.fwd", "2x2x2x8"), ("no_oh_clip", "pool.bwd", "2x2x2x8"), ("drop_tap", "up.bwd", "1x1x1x1"),
    ("leaky_001", "act", "n3"), ("sigmoid_from_pre", "act", "n5"),
    ("counter_off_by_one", "rng.uniform", "hi-carry-n1"), ("no_carry", "rng.uniform", "hi-carry-n1024"),
    ("round_constant", "rng.uniform", "s0-o0-n4"), ("u1_no_plus_one", "rng.normal", "s1-o5-n65536"),
    ("sincos_swapped", "rng.normal", "hi-carry-n5"),
]
