"""float64 references of the MLP decoder on pre-split fp16 pair planes (csrc/dense16.hip: d16_pack_kernel, d16_first_kernel<K4, R>,
d16_nt_kernel<BM, EPI>, d16_tn_kernel, d16_sum_kernel, d16_unsplit_kernel) and the host arithmetic of its launchers, restated.

Plane arithmetic (csrc/bf3.hpp): an operand tensor x is held as two fp16 planes under a power-of-two scale s,
x s = hi + lo / 2048 with hi = fp16(x s), lo = fp16((x s - hi) 2048); a product of two such pairs is
hi hi' + (hi lo' + lo hi') / 2048: three MFMAs, the lo lo' term (2^-22 of the product) is left out.  `decode` is exact in float64, so
every kernel is judged on the operands it was ACTUALLY given: the references below start from decoded planes.

Per GEMM output, four float64 tensors (dict keys):

  ref    the exact result of the decoded operands
  tol    C_ENTRY (sum_k |a b| + |bias| + |initial|) + 2^-39 K a_bound rowmax_b   (the second term is bf3.hpp's floor of a scaled
         pair: an absolute 2^-39 of the operand BOUNDS per product; a weight-plane row has its own scale, so its bound is the
         row's maximum)
  deg    the shipped form with the hi lo' cross term dropped (the second operand rounded to its hi plane): must leave tol
  ship   the exact-arithmetic value of the shipped three-product form (ref minus the lo lo' term): must stay at 0.8 tol
  cpu    a float32 evaluation on the CPU: must stay inside tol

C_ENTRY = 5e-7 is the constant of tests/test_gpu_gemm_dispatch.py for fp32 accumulator chains of <= 1024 terms; every chain of
tests/test_gpu_dense16.py stays at or below 1024 (K <= 784 in d16_nt_kernel, <= 96 rows per slice and <= 16 slabs in the weight
gradient: each case states its own).

The NLL tail of d16_nt_kernel<.., D16_NLL> is not linear in the GEMM; with pre = C + bias, r = sigmoid(pre), x = X[m % xrows],
k = gw / s^2:
  G    = k (r - x) r (1 - r)                   tol |dG/dpre| tol_pre + C_TAIL 2^-24 k (|r - x| + r (1 - r)) + 2^-23 |G| + 2^-39 g_bound
  rows = sum_n (r - x)^2 / (2 s^2) + row_const tol sum_n (|r - x| r (1 - r) / s^2 tol_pre + C_TAIL 2^-24 |r - x| / s^2)
                                                   + C_ENTRY sum_n |term| + 2^-24 |row_const| (column tile 0 only)
  colsum_part = sums of the fp32 G over a row tile   tol sum_m (tol_G without its two plane terms) + C_ENTRY sum_m |G|
The tail term is ABSOLUTE in r: near saturation 1 - r carries a fixed absolute error of r.  C_TAIL is set from a yardstick, the
same tail in float32 on the CPU (torch.sigmoid of the fp32 rounding of pre, then the kernel's products): twice the yardstick's
worst |G32 - G| / (2^-24 k (|r - x| + r (1 - r))) over the table, and at least 4 (tests/test_dense16_ref_host.py::test_c_tail
measures it; the factor 2 is the margin tests/test_gpu_conv4s2_small.py::test_activations gives mvk_fast_sigmoid over torch's fp32
sigmoid).
"""
import math

import torch

C_ENTRY = 5e-7       # tests/test_gpu_gemm_dispatch.py
FLOOR = 2.0 ** -39   # csrc/bf3.hpp: absolute error of a scaled pair far below its bound, per product, in units of the bounds
C_TAIL = 4.0         # see above; the yardstick measures 1.49 over the table (twice that is below the floor of 4)
NONE, RELU, SIGMOID, LEAKY = 0, 1, 2, 3
F02 = float(torch.tensor(0.2, dtype=torch.float32))
F10001 = float(torch.tensor(1.0001, dtype=torch.float32))  # the kernels' 1.0001f
F32, F64, F16 = torch.float32, torch.float64, torch.float16
LOOSE = (3.7, 5.3)   # operand bounds this many times the true maxima (no powers of two)


def g(seed):
    return torch.Generator().manual_seed(seed)


# ---- plane arithmetic (csrc/bf3.hpp) ---------------------------------------------------------------------------------------------
def _f32(x):
    return x.to(F32) if isinstance(x, torch.Tensor) else torch.tensor(x, dtype=F32)


def f16_scale_of(amax):
    """Power of two s with amax s in [2^13, 2^14), from the bit pattern; clamped to [2^-126, 2^126] (amax = 0 or denormal: 2^126)."""
    e = (_f32(amax).contiguous().view(torch.int32) >> 23) & 0xFF
    return ((267 - e).clamp(1, 253) << 23).view(F32)


def f16_inv_scale(s):
    return ((254 << 23) - _f32(s).contiguous().view(torch.int32)).view(F32)


def inv_of(bound):
    """1 / f16_scale_of(bound) as float64."""
    return f16_inv_scale(f16_scale_of(bound)).double()


def split(x, s):
    """(hi, lo) fp16 planes of the fp32 tensor x under the scale(s) s (x s is an exact product for a power of two)."""
    xs = _f32(x) * _f32(s)
    hi = xs.to(F16)
    lo = ((xs - hi.float()) * 2048.0).to(F16)
    return hi, lo


def decode(hi, lo, inv):
    """(hi + lo / 2048) inv in float64: exact."""
    return (hi.double() + lo.double() / 2048.0) * (inv.double() if isinstance(inv, torch.Tensor) else inv)


def tensor_planes(x, bound):
    """(hi, lo, inv) of x under ONE scale from `bound` >= max |x| (inv: float64 scalar)."""
    s = f16_scale_of(bound)
    hi, lo = split(x, s)
    return hi, lo, float(f16_inv_scale(s))


def row_planes(W):
    """(hi, lo, inv[rows]) of W with one scale per row from the row's maximum (d16_pack_kernel)."""
    s = f16_scale_of(W.float().abs().amax(1))
    hi, lo = split(W, s[:, None])
    return hi, lo, f16_inv_scale(s)


def ulp32(x):
    """fp32 spacing at |x| (x in float64)."""
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126))) - 23)


def act64(v, act):
    if act == RELU:
        return v.clamp_min(0)
    if act == LEAKY:
        return torch.where(v > 0, v, F02 * v)
    return v


# ---- data ------------------------------------------------------------------------------------------------------------------------
def spread_rows(rows, cols, gen, decades, away_from_zero=False):
    """Normal entries (or, away_from_zero, magnitudes in [0.5, 1) with random signs), row i times 10^u_i, u_i uniform in +-decades."""
    if away_from_zero:
        v = (torch.rand(rows, cols, generator=gen) * 0.5 + 0.5) * (torch.randint(0, 2, (rows, cols), generator=gen) * 2 - 1)
    else:
        v = torch.randn(rows, cols, generator=gen)
    return (v * torch.pow(10.0, (torch.rand(rows, 1, generator=gen) * 2 - 1) * decades)).float()


# ---- d16_pack_kernel -------------------------------------------------------------------------------------------------------------
def pack_operand(seed, N, K):
    """W [N][K]: rows over 10^+-3, magnitudes away from zero (so that no non-zero scaled element is an fp16 subnormal in either
    orientation), row N // 2 and column K // 3 all zero."""
    W = spread_rows(N, K, g(seed), 3.0, away_from_zero=True)
    W[N // 2] = 0.0
    W[:, K // 3] = 0.0
    return W


def pack(W):
    """dict of the six outputs of mvk_dense16_pack: nk planes [N][K] + nk_inv [N], kn planes [K][N] + kn_inv [K]."""
    nk_hi, nk_lo, nk_inv = row_planes(W)
    kn_hi, kn_lo, kn_inv = row_planes(W.t().contiguous())
    return dict(nk_hi=nk_hi, nk_lo=nk_lo, nk_inv=nk_inv, kn_hi=kn_hi, kn_lo=kn_lo, kn_inv=kn_inv)


# ---- d16_first_kernel ------------------------------------------------------------------------------------------------------------
def first_cfg(M, N, K):
    """(K4, R, CT, rgn) of the d16_first_kernel<K4, R> launch: R rows per workgroup, CT column groups, rgn row groups."""
    want = (M + 255) // 256
    R = 8 if want <= 8 else (20 if want <= 20 else 40)
    return K // 4, R, N // 4, 256 // (N // 4)


def first_ok(M, N, K):
    return M > 0 and 4 <= K <= 32 and K % 4 == 0 and 4 <= N <= 1024 and N % 8 == 0 and 256 % (N // 4) == 0


def first_operands(seed, M, N, K):
    gen = g(seed)
    z = spread_rows(M, K, gen, 2.0)
    W = ((torch.rand(N, K, generator=gen) - 0.5) * 2 / K ** 0.5).float()
    b = ((torch.rand(N, generator=gen) - 0.5) * 2 / K ** 0.5).float()
    return z, W, b


def first(z, W, b, act, z_amax):
    """H = act(z W^T + b) and the a-priori bound max_n ||W[n]||_1 z_amax + max |b| in float64 (bound_exact: the kernel publishes
    fp32(l1 z_amax 1.0001 + bm), at most 1.001 of it, and never below max |H|)."""
    z64, W64 = z.double(), W.double()
    b64 = torch.zeros(W.shape[0], dtype=F64) if b is None else b.double()
    pre = z64 @ W64.t() + b64
    absum = z64.abs() @ W64.abs().t() + b64.abs()
    bound_exact = float(W64.abs().sum(1).max()) * float(z_amax) + float(b64.abs().max())
    pre32 = z.float() @ W.float().t() + b64.float()
    return dict(ref=act64(pre, act), absum=absum, bound_exact=bound_exact, cpu32=act64(pre32, act))


def first_tol(r, bound):
    """C_ENTRY (sum |z w| + |b|) + 2^-23 |h| + 2^-39 bound: the fma chain, the pair's quantisation, the pair's floor."""
    return C_ENTRY * r["absum"] + 2.0 ** -23 * r["ref"].abs() + FLOOR * bound


def first_emulations(r, bound):
    """(cpu, ship, deg) as the planes would decode: the fp32 CPU evaluation split under `bound`; the fp32 rounding of the exact
    result split (the plane quantisation alone); and the exact result on its hi plane only (the lo plane dropped)."""
    inv = inv_of(bound)
    s = f16_scale_of(bound)
    cpu = decode(*split(r["cpu32"], s), inv)
    hi, lo = split(r["ref"].float(), s)
    return cpu, decode(hi, lo, inv), decode(hi, torch.zeros_like(lo), inv)


# ---- the plane GEMMs -------------------------------------------------------------------------------------------------------------
def nt_tiles(K):
    """k-tiles of 32 of d16_nt_kernel (an odd count runs one more tile of zeros)."""
    return (K + 31) // 32


def gemm_nt(A, B, a_bound):
    """C[m][n] = sum_k A[m][k] B[n][k] from planes A = (hi, lo, inv scalar) [M][K] and B = (hi, lo, inv[N]) [N][K]."""
    Ah, Al, ia = A
    Bh, Bl, ib = B
    ib = ib.double()[:, None]
    A64, B64 = decode(Ah, Al, ia), decode(Bh, Bl, ib)
    K = A64.shape[1]
    ref = A64 @ B64.t()
    absum = A64.abs() @ B64.abs().t()
    floor = FLOOR * K * float(a_bound) * B64.abs().amax(1)[None, :]
    lolo = (Al.double() * (ia / 2048.0)) @ (Bl.double() * (ib / 2048.0)).t()
    return dict(ref=ref, absum=absum, floor=floor, tol=C_ENTRY * absum + floor, deg=A64 @ (Bh.double() * ib).t(), ship=ref - lolo,
                cpu=(A64.float() @ B64.float().t()).double())


def gemm_tn(Dp, Hp, d_bound, h_bound, init=None, rows_per_slice=None):
    """dW[j][i] (+)= sum_m D[m][j] H[m][i] from planes D [M][N] and H [M][K], each under one tensor scale.  cpu: float32 matrix
    products over the rows of each slice of the launch (the kernel's accumulator chains), then the ordered float32 sum of the slabs."""
    Dh, Dl, idd = Dp
    Hh, Hl, ih = Hp
    D64, H64 = decode(Dh, Dl, idd), decode(Hh, Hl, ih)
    M = D64.shape[0]
    ref = D64.t() @ H64
    absum = D64.abs().t() @ H64.abs()
    tol = C_ENTRY * (absum + (0 if init is None else init.double().abs())) + FLOOR * M * float(d_bound) * float(h_bound)
    lolo = (Dl.double() * (idd / 2048.0)).t() @ (Hl.double() * (ih / 2048.0))
    step = rows_per_slice or M
    cpu = torch.zeros(ref.shape, dtype=F32)
    for m0 in range(0, M, step):
        cpu = cpu + D64[m0:m0 + step].float().t() @ H64[m0:m0 + step].float()
    return dict(ref=ref, absum=absum, tol=tol, deg=D64.t() @ (Hh.double() * ih), ship=ref - lolo, cpu=cpu.double())


def wgrad_slices(M, N, K):
    """(S, per, empty_slices, mapping) of mvk_dense16_wgrad: S slices of `per` 32-row chunks over 128 x 128 tiles; a multiple of 8
    keeps its empty tail slices (they write zero slabs) and maps workgroup -> (tile, slice) so that a slice stays on one XCD."""
    tiles = ((N + 127) // 128) * ((K + 127) // 128)
    chunks = (M + 31) // 32
    S = max(1, min(256 // tiles, chunks))
    if S >= 6 and chunks >= 8:
        S = 16 if (S >= 12 and chunks >= 16) else 8
    per = (chunks + S - 1) // S
    if S % 8 != 0:
        S = (chunks + per - 1) // per
    empty = [z for z in range(S) if z * per * 32 >= M]
    return S, per, empty, "xcd" if S % 8 == 0 else "plain"


def wgrad_block(L, tiles, S):
    """(tile, slice) of workgroup L of the 1-D grid (d16_tn_kernel)."""
    if S % 8 == 0:
        q = L >> 3
        return q % tiles, (q // tiles) * 8 + (L & 7)
    return L % tiles, L // tiles


def relu_mask(mask_hi):
    """ReLU'(h) as d16_nt_kernel reads it from the uploaded hi plane: a positive fp16 number (sign clear, not zero; a positive
    subnormal counts, -0 and +0 do not)."""
    bits = mask_hi.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    return ((bits != 0) & ((bits & 0x8000) == 0)).double()


def bwd_data(A, B, a_bound, mask_hi=None, db_init=None):
    """dA = (G W) * mask (out) and its column sums (db, added to db_init): every tensor of gemm_nt times the mask."""
    r = gemm_nt(A, B, a_bound)
    if mask_hi is not None:
        m = relu_mask(mask_hi)
        r = {k: v * m for k, v in r.items()}
    s = lambda t: t.sum(0)  # noqa: E731
    init = 0 if db_init is None else db_init.double().abs()
    db = dict(ref=s(r["ref"]), tol=s(r["tol"]) + C_ENTRY * (s(r["ref"].abs()) + init), deg=s(r["deg"]), ship=s(r["ship"]),
              cpu=r["cpu"].float().sum(0).double())
    return r, db


# ---- the NLL tail ----------------------------------------------------------------------------------------------------------------
def nll_consts(scale, gw, N, x_amax):
    """(inv_s2, k, row_const, g_bound) as the launcher and the kernel form them: inv_s2 and row_const in fp32 (the operands the
    kernel is given), k = gw inv_s2 and the bound gw (1 + x_amax) / (4 s^2) 1.0001 in float64."""
    s32 = torch.tensor(scale, dtype=F32)
    inv_s2 = float(1.0 / (s32 * s32))
    gw32 = float(torch.tensor(gw, dtype=F32))
    row_const = float(torch.tensor(float(N), dtype=F32) * (torch.log(s32) + torch.tensor(0.918938533204672742, dtype=F32)))
    g_bound = gw32 * (1.0 + float(x_amax)) / (4.0 * float(s32) ** 2) * F10001
    return inv_s2, gw32 * inv_s2, row_const, g_bound


def nll_tail(r, bias, X, xrows, scale, gw, x_amax, bm=64, g_bound=None):
    """From gemm_nt's dict of C: dicts (ref, tol, deg, ship, cpu) of G [M][N], rows_part [ceil(N / 128)][M] and colsum_part
    [ceil(M / bm)][N], and the yardstick ratio of the case.  g_bound: the published bound G's planes are decoded under."""
    M, N = r["ref"].shape
    b64 = torch.zeros(N, dtype=F64) if bias is None else bias.double()
    x = X.double()[torch.arange(M) % xrows]
    inv_s2, k, row_const, gb = nll_consts(scale, gw, N, x_amax)
    g_bound = gb if g_bound is None else g_bound
    tol_pre = r["tol"] + C_ENTRY * b64.abs()
    P, CR = (N + 127) // 128, (M + bm - 1) // bm

    def tail(pre):
        rr = torch.sigmoid(pre)
        d = rr - x
        return k * d * rr * (1 - rr), 0.5 * inv_s2 * d * d

    def rows_of(term):
        t = torch.nn.functional.pad(term, (0, P * 128 - N)).view(M, P, 128).sum(2).t().contiguous()
        return t

    def cols_of(G):
        return torch.nn.functional.pad(G, (0, 0, 0, CR * bm - M)).view(CR, bm, N).sum(1)

    pre = r["ref"] + b64
    rr = torch.sigmoid(pre)
    s1, d = rr * (1 - rr), rr - x
    G, term = tail(pre)
    unit = 2.0 ** -24 * k * (d.abs() + s1)
    tolG_f32 = (k * (s1 + d * (1 - 2 * rr)) * s1).abs() * tol_pre + C_TAIL * unit
    tolG = tolG_f32 + 2.0 ** -23 * G.abs() + FLOOR * g_bound
    tol_term = d.abs() * s1 * inv_s2 * tol_pre + C_TAIL * 2.0 ** -24 * d.abs() * inv_s2
    rc = torch.zeros(P, 1, dtype=F64)
    rc[0] = row_const
    out = {}
    ev = {name: tail(r[name] + b64) for name in ("deg", "ship", "cpu")}
    # the yardstick: the fp32 rounding of the exact pre-activation, torch's fp32 sigmoid, the kernel's products in fp32
    pre32 = pre.float()
    r32 = torch.sigmoid(pre32)
    d32 = r32 - X.float()[torch.arange(M) % xrows]
    k32 = torch.tensor(gw, dtype=F32) * torch.tensor(inv_s2, dtype=F32)
    G32 = (k32 * d32 * (r32 * (1 - r32))).double()
    yard = float(((G32 - G).abs() / unit).max())
    # the cpu evaluation carries the yardstick's fp32 tail on the fp32 GEMM
    prec = (r["cpu"] + b64).float()
    rc32 = torch.sigmoid(prec)
    dc32 = rc32 - X.float()[torch.arange(M) % xrows]
    ev["cpu"] = ((k32 * dc32 * (rc32 * (1 - rc32))).double(), (torch.tensor(0.5 * inv_s2, dtype=F32) * dc32 * dc32).double())
    inv_g, s_g = inv_of(g_bound), f16_scale_of(g_bound)
    quant = lambda t: decode(*split(t.float(), s_g), inv_g)  # noqa: E731  (what G's planes hold of an fp32 value)
    out["G"] = dict(ref=G, tol=tolG, deg=ev["deg"][0], ship=quant(ev["ship"][0]), cpu=quant(ev["cpu"][0]))
    out["rows"] = dict(ref=rows_of(term) + rc, tol=rows_of(tol_term) + C_ENTRY * rows_of(term.abs()) + 2.0 ** -24 * rc.abs(),
                       **{n_: rows_of(ev[n_][1]) + rc for n_ in ev})
    out["colsum"] = dict(ref=cols_of(G), tol=cols_of(tolG_f32) + C_ENTRY * cols_of(G.abs()), **{n_: cols_of(ev[n_][0]) for n_ in ev})
    out["yard"], out["g_bound"], out["pre"] = yard, gb, pre
    return out


# ---- d16_unsplit_kernel ----------------------------------------------------------------------------------------------------------
def unsplit(hi, lo, bound, rowf=None, rowf_scale=1.0, rowf_tile=0):
    """fp32 out[m][n] = fma(lo, 2^-11, hi) inv rf, rf = rowf[(n // tile) M + m] rowf_scale (tile 0: rowf[m]), as float32: the fma is
    one fp32 rounding of an exact float64 sum, inv is a power of two, rf one fp32 product, then ONE rounded product."""
    M, N = hi.shape
    v = ((hi.double() + lo.double() / 2048.0).float().double() * inv_of(bound)).float()
    if rowf is None:
        return v
    rf = rowf.float() * torch.tensor(rowf_scale, dtype=F32)
    tile = (torch.arange(N) // rowf_tile) if rowf_tile > 0 else torch.zeros(N, dtype=torch.long)
    fac = rf.view(-1)[tile[None, :] * M + torch.arange(M)[:, None]]
    return (v.double() * fac.double()).float()


def ratio(x, ref, tol):
    return float(((x - ref).abs() / (tol + 1e-300)).max())
