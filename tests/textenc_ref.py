"""Float64 torch restatement of the CUB text encoder's stages (mvk_txt_*, csrc/textenc.hip) and of the whole encoder
(kernels.TextEncoderFn), written from the formulas; plus the kernels' case table, seeded inputs and error model.  CPU only: no GPU, no
libmvk.so; nothing here reads the reference project or multivae_amd.

Encoder.  tokens [B,S], E columns, nh heads of hd = E / nh columns, F feed-forward units, V vocabulary rows.
h0 = drop(emb[tokens] sqrt(E) + pe[:S]); per layer (post-norm, ReLU): qkv = h Win^T + bin, per (sentence, head)
P = softmax((q / sqrt(hd)) k^T, keys with mask 0 at -inf), ctx = drop(P) v, a = ctx Wo^T + bo, y1 = LN1(h + drop(a)),
f = W2 drop(relu(W1 y1 + b1)) + b2, h = LN2(y1 + drop(f)).  LN: biased variance, rstd = 1 / sqrt(var + eps).  Dropout: an element
is kept iff u >= p and scaled by 1 / (1 - p), u from ONE flat buffer: pos [B,S,E], then per layer attn [B,nh,S,S], res1 [B,S,E],
ff [B,S,F], res2 [B,S,E].  zero_pads: the last LN2 writes 0 on padded rows (evaluation without autograd).

Every function computes in the dtype of its floating inputs: float64 is the reference, float32 the "same formulas in plain torch fp32
on the CPU" that the constants come from.  Gradients are autograd's of these forwards.

Error model.  u = 2^-24.  `base` of an output entry is u times the value of the stage's formula with every operand replaced by its
magnitude and every sum by the sum of magnitudes (so cancellation cannot shrink it), times the length of the longest chain of additions
behind the entry, plus — where a stage divides by or multiplies with a quantity that itself carries such an error (the softmax
denominator, xh = (z - mean) rstd in the LayerNorm backward) — the first-order effect of that error.  A comparison passes when
|got - ref| <= C_STAGE[stage] * base for EVERY entry.  C_STAGE = 4x the largest |err| / base that the fp32 evaluation shows over the case
table, rounded up (tests/test_textenc_host.py::test_error_constants re-derives it; the HIP kernels have no part in it).

The whole encoder runs five tiled-GEMM sites per layer.  The project's float64 GEMM test pins that engine at 5e-7 sum|a b| per entry
(tests/test_gpu_gemm_dispatch.py C_ENTRY), which is 8.4 u: a chain of GEMMs and LayerNorms cannot be held to a per-stage magnitude
bound, so the whole encoder's base is C_ENTRY * sites * (|ref| + rms(ref)) per entry of an output tensor, sites = the number of stages
between the entry and the farthest input (1 + 8 per layer forward, twice that for a gradient); rms(ref) stands for the error a
LayerNorm spreads over its row.  C_WHOLE is again 4x the fp32 evaluation's largest ratio, rounded up.

`mut` names deliberate mistakes of the REFERENCE, used only to show that the bounds reject them (MUTATIONS)."""
import math
from dataclasses import dataclass

import torch

F64 = torch.float64
U = 2.0 ** -24
TINY = 2.0 ** -126
C_ENTRY = 5e-7  # tests/test_gpu_gemm_dispatch.py: the tiled engine's entrywise bound, in units of sum|a b|

# 4x the value measured by tests/test_textenc_host.py::test_error_constants, rounded up
C_STAGE = {"embed": 6.0, "dE": 3.0, "P": 1.2, "ctx": 0.9, "dqkv": 3.0, "y": 0.6, "y_zero": 0.6, "mean": 0.7, "rstd": 0.4, "dx": 0.25,
           "dt": 0.25, "dgamma": 0.15, "dbeta": 0.16,
           # keep * scale * x is ONE rounding (none at p = 0.5: the fp32 evaluation is exact over the table): one u |result|
           "drop": 1.0}
C_WHOLE = {"out": 2.0, "grad": 9.0}

MUTATIONS = ("no_qscale", "no_keymask", "no_dropscale", "no_sqrtE", "no_pos", "no_eps", "no_zero_pads")

EN = ((8, 2), (64, 4), (512, 4), (96, 3))  # (96, 3): head_dim 32
SS = (1, 5, 32, 64)
BS = (1, 3)
FS = (16, 1024)
VS = (7, 1590)
PADS = ("none", "ragged", "one")
PS = (0.0, 0.5)
NULLS = ((), ("mask",), ("keep",), ("affine",), ("dy2",), ("sums",))
EPS = 1e-5


@dataclass(frozen=True)
class Case:
    name: str
    E: int
    nh: int
    S: int
    B: int
    F: int
    V: int
    pad: str
    p: float
    null: tuple
    seed: int


def _cases():
    out, i = [], 0
    for E, nh in EN:
        for S in SS:
            for B in BS:
                for p in PS:
                    F, V = FS[(i // 2) % 2], VS[(i // 4 + i) % 2]
                    pad, null = PADS[(i + i // 3) % 3], NULLS[(i + i // 6) % len(NULLS)]
                    out.append(Case(f"e{E}-h{nh}-s{S}-b{B}-f{F}-v{V}-{pad}-p{p:g}" + "".join("-null-" + n for n in null), E, nh, S, B, F,
                                    V, pad, p, null, 9100 + i))
                    i += 1
    return out


CASES = _cases()
CASE_BY_NAME = {c.name: c for c in CASES}
# the whole encoder: (case name, layers) — small and default widths, both head sizes, one and two layers, with and without dropout
WHOLE = (("e8-h2-s5-b3", 1), ("e8-h2-s5-b3", 2), ("e64-h4-s32-b3", 2), ("e96-h3-s64-b1", 1), ("e512-h4-s32-b3", 2), ("e512-h4-s1-b3", 1))


def whole_cases():
    out = []
    for prefix, nl in WHOLE:
        for c in CASES:
            if c.name.startswith(prefix + "-"):
                out.append((c, nl))
    return out


def noise_layout(B, S, E, nh, F, n_layers):
    off, layers = B * S * E, []
    for _ in range(n_layers):
        a = off
        r1 = a + B * nh * S * S
        f = r1 + B * S * E
        r2 = f + B * S * F
        off = r2 + B * S * E
        layers.append((a, r1, f, r2))
    return off, 0, layers


def positions(S, E):
    """pe [S,E] fp32: pe[t, 2i] = sin(t w_i), pe[t, 2i + 1] = cos(t w_i), w_i = 10000^(-2i / E)."""
    t = torch.arange(S, dtype=torch.float32).unsqueeze(1)
    w = torch.exp(torch.arange(0, E, 2, dtype=torch.float32) * (-math.log(10000.0) / E))
    pe = torch.zeros(S, E)
    pe[:, 0::2] = torch.sin(t * w)
    pe[:, 1::2] = torch.cos(t * w)[:, : E // 2]
    return pe


def make_noise(n, p, g):
    """U[0,1) fp32 with entries equal to p exactly (kept) and one ulp below it (dropped)."""
    u = torch.rand(n, generator=g)
    if p > 0:
        u[0::7] = p
        u[3::7] = float(torch.nextafter(torch.tensor(p, dtype=torch.float32), torch.tensor(0.0)))
    return u


def make_inputs(case, n_layers=1):
    """Seeded fp32 inputs of every stage and of the whole encoder."""
    g = torch.Generator().manual_seed(case.seed)
    E, nh, S, B, F, V, p = case.E, case.nh, case.S, case.B, case.F, case.V, case.p
    rn = lambda *s: torch.randn(*s, generator=g)
    if V == 7:  # ids 0..5 in turn (every id repeated once B S >= 12), shuffled; id 6 is never used
        tok = (torch.arange(B * S) % 6)[torch.randperm(B * S, generator=g)].reshape(B, S)
    else:
        tok = torch.randint(0, V, (B, S), generator=g)
        tok[0, 0] = V - 1
    mask = torch.ones(B, S, dtype=torch.int32)
    if case.pad == "ragged":
        for b in range(B):
            mask[b, max(1, (S * (b + 1)) // (B + 1)):] = 0
    elif case.pad == "one":
        mask[0, 1:] = 0
    I = dict(tok=tok, mask=mask, emb=(torch.rand(V, E, generator=g) - 0.5) * 0.2, pe=positions(S, E))
    total, pos_off, offs = noise_layout(B, S, E, nh, F, n_layers)
    I["noise"] = make_noise(total, p, g)
    I["layout"] = (total, pos_off, offs)
    # stage inputs
    I["qkv"] = rn(B, S, 3 * E) * (1.0 + 0.5 * (case.seed % 3))
    I["dctx"] = rn(B, S, E)
    I["x"], I["t"] = rn(B, S, E), rn(B, S, E) * 0.7 + 0.3
    I["gamma"], I["beta"] = 1.0 + 0.3 * rn(E), 0.2 * rn(E)
    I["dy"], I["dy2"] = rn(B, S, E), rn(B, S, E) * 0.5
    I["g"], I["g2"] = rn(B, S, E), rn(B, S, E) * 0.5
    I["ff"] = rn(B, S, F)
    layers = []
    for _ in range(n_layers):
        k = lambda n, m: (torch.rand(n, m, generator=g) * 2 - 1) / math.sqrt(m)
        layers += [k(3 * E, E) * 1.5, 0.1 * rn(3 * E), k(E, E), 0.1 * rn(E), k(F, E), 0.1 * rn(F), k(E, F), 0.1 * rn(E),
                   1.0 + 0.2 * rn(E), 0.1 * rn(E), 1.0 + 0.2 * rn(E), 0.1 * rn(E)]
    I["params"] = layers
    I["dout"] = rn(B, S, E)
    return I


# ---- the stages --------------------------------------------------------------------------------------------------------------------
def _drop(x, u, p, mut=()):
    if u is None or p == 0:
        return x
    scale = 1.0 if "no_dropscale" in mut else 1.0 / (1.0 - p)
    return torch.where(u.reshape(x.shape) >= torch.tensor(p, dtype=torch.float32), x * scale, torch.zeros_like(x))


def embed_fwd(tok, emb, pe, u, p, mut=()):
    E = emb.shape[1]
    h = emb[tok] * (1.0 if "no_sqrtE" in mut else math.sqrt(E))
    if "no_pos" not in mut:
        h = h + pe[: tok.shape[1]].to(emb.dtype)
    return _drop(h, u, p, mut)


def attn_fwd(qkv, mask, u, p, nh, mut=()):
    """-> (ctx [B,S,E], P [B,nh,S,S] before dropout)"""
    B, S, E3 = qkv.shape
    E = E3 // 3
    hd = E // nh
    q, k, v = [t.reshape(B, S, nh, hd).transpose(1, 2) for t in qkv.split(E, dim=-1)]
    if "no_qscale" not in mut:
        q = q / math.sqrt(hd)
    s = q @ k.transpose(-1, -2)
    if mask is not None and "no_keymask" not in mut:
        s = s.masked_fill((mask == 0)[:, None, None, :], -math.inf)
    P = torch.softmax(s, dim=-1)
    ctx = _drop(P, u, p, mut) @ v
    return ctx.transpose(1, 2).reshape(B, S, E), P


def add_ln_fwd(x, t, u, p, gamma, beta, eps, rowmask=None, zero_pads=False, mut=()):
    """-> (y, z, mean, rstd)"""
    z = x + _drop(t, u, p, mut)
    mean = z.mean(-1, keepdim=True)
    var = ((z - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + (0.0 if "no_eps" in mut else eps))
    y = (z - mean) * rstd
    if gamma is not None:
        y = y * gamma + beta
    if zero_pads and rowmask is not None and "no_zero_pads" not in mut:
        y = y * (rowmask != 0).to(y.dtype).reshape(*y.shape[:-1], 1)
    return y, z, mean.squeeze(-1), rstd.squeeze(-1)


def encoder(tok, mask, emb, pe, params, u, p, nh, eps, layout, zero_pads=False, mut=()):
    """The whole encoder -> [B,S,E].  params: 12 per layer (in_proj w, b; out_proj w, b; linear1 w, b; linear2 w, b; norm1 w, b;
    norm2 w, b); layout = noise_layout(...)."""
    B, S = tok.shape
    E = emb.shape[1]
    _, pos_off, offs = layout
    site = lambda off, n: None if u is None or p == 0 else u[off:off + n]
    h = embed_fwd(tok, emb, pe, site(pos_off, B * S * E), p, mut)
    n_layers = len(params) // 12
    for l in range(n_layers):
        w_in, b_in, w_o, b_o, w1, b1, w2, b2, g1, be1, g2, be2 = params[12 * l:12 * l + 12]
        F = w1.shape[0]
        oa, or1, of, or2 = offs[l]
        ctx, _ = attn_fwd(h @ w_in.t() + b_in, mask, site(oa, B * nh * S * S), p, nh, mut)
        y1 = add_ln_fwd(h, ctx @ w_o.t() + b_o, site(or1, B * S * E), p, g1, be1, eps, mut=mut)[0]
        f = _drop(torch.relu(y1 @ w1.t() + b1), site(of, B * S * F), p, mut) @ w2.t() + b2
        last = l == n_layers - 1
        h = add_ln_fwd(y1, f, site(or2, B * S * E), p, g2, be2, eps, mask if last else None, zero_pads and last, mut)[0]
    return h


# ---- per-stage references with their bases -----------------------------------------------------------------------------------------
def _keepscale(u, p, shape, dt=F64):
    if u is None or p == 0:
        return torch.ones(shape, dtype=dt)
    return (u.reshape(shape) >= torch.tensor(p, dtype=torch.float32)).to(dt) / (1.0 - p)


def _cast(I, dt):
    return {k: (v.to(dt) if torch.is_tensor(v) and v.is_floating_point() and k != "noise" else v) for k, v in I.items()}


def stage_outputs(case, I, dt=F64, mut=()):
    """{stage: tensor} of every per-stage output for the case's inputs, computed in dtype dt."""
    J = _cast(I, dt)
    E, nh, S, B, F, V, p = case.E, case.nh, case.S, case.B, case.F, case.V, case.p
    null = case.null
    _, pos_off, offs = I["layout"]
    u = I["noise"]
    site = lambda off, n: None if p == 0 else u[off:off + n]
    mask = None if "mask" in null else I["mask"]
    affine = "affine" not in null
    out = {}
    # embedding and its gradient
    emb = J["emb"].clone().requires_grad_(True)
    h0 = embed_fwd(I["tok"], emb, J["pe"], site(pos_off, B * S * E), p, mut)
    out["embed"] = h0.detach()
    g = J["g"] + (0 if "dy2" in null else J["g2"])
    out["dE"] = torch.autograd.grad(h0, emb, g)[0]
    # attention
    qkv = J["qkv"].clone().requires_grad_(True)
    ctx, P = attn_fwd(qkv, mask, site(offs[0][0], B * nh * S * S), p, nh, mut)
    out["ctx"], out["P"] = ctx.detach(), P.detach()
    out["dqkv"] = torch.autograd.grad(ctx, qkv, J["dctx"])[0]
    # residual + LayerNorm
    x, t = J["x"].clone().requires_grad_(True), J["t"].clone().requires_grad_(True)
    gamma = J["gamma"].clone().requires_grad_(True) if affine else None
    beta = J["beta"].clone().requires_grad_(True) if affine else None
    y, z, mean, rstd = add_ln_fwd(x, t, site(offs[0][1], B * S * E), p, gamma, beta, EPS, mut=mut)
    out["y"], out["mean"], out["rstd"] = y.detach(), mean.detach(), rstd.detach()
    dy = J["dy"] + (0 if "dy2" in null else J["dy2"])
    gr = torch.autograd.grad(y, [x, t] + ([gamma, beta] if affine else []), dy)
    out["dx"], out["dt"] = gr[0], gr[1]
    if affine:
        out["dgamma"], out["dbeta"] = gr[2], gr[3]
    else:  # the sums are still the kernel's: with gamma = 1, beta = 0
        xh = ((z - mean.unsqueeze(-1)) * rstd.unsqueeze(-1)).detach()
        out["dgamma"], out["dbeta"] = (dy * xh).sum((0, 1)), dy.sum((0, 1))
    out["y_zero"] = add_ln_fwd(x, t, site(offs[0][1], B * S * E), p, gamma, beta, EPS, I["mask"], True, mut)[0].detach()
    out["drop"] = _drop(J["ff"], site(offs[0][2], B * S * F), p, mut)
    return out


def stage_bases(case, I):
    """{stage: base} in float64 (module docstring)."""
    J = _cast(I, F64)
    E, nh, S, B, F, V, p = case.E, case.nh, case.S, case.B, case.F, case.V, case.p
    null = case.null
    hd = E // nh
    _, pos_off, offs = I["layout"]
    u = I["noise"]
    tok = I["tok"]
    base = {}
    D = _keepscale(u[pos_off:pos_off + B * S * E], p, (B, S, E))
    base["embed"] = U * 2 * D * (J["emb"][tok].abs() * math.sqrt(E) + J["pe"][:S].abs())
    g = J["g"].abs() + (0 if "dy2" in null else J["g2"].abs())
    A = torch.zeros(V, E, dtype=F64).index_add_(0, tok.reshape(-1), (D * g).reshape(-1, E)) * math.sqrt(E)
    cnt = torch.bincount(tok.reshape(-1), minlength=V).to(F64).unsqueeze(1)
    base["dE"] = U * (cnt + 3) * A
    # attention
    mask = None if "mask" in null else I["mask"]
    q, k, v = [t.reshape(B, S, nh, hd).transpose(1, 2) for t in J["qkv"].split(E, dim=-1)]
    ctx, P = attn_fwd(J["qkv"], mask, None, 0.0, nh)
    Da = _keepscale(u[offs[0][0]:offs[0][0] + B * nh * S * S], p, (B, nh, S, S))
    As = (q.abs() @ k.abs().transpose(-1, -2)) / math.sqrt(hd)
    if mask is not None:
        As = As.masked_fill((mask == 0)[:, None, None, :], 0.0)
    eP = U * P * ((hd + 2) * (As + (P * As).sum(-1, keepdim=True)) + S + 8)
    base["P"] = eP
    bc = (eP * Da) @ v.abs() + U * (S + 2) * ((P * Da) @ v.abs())
    base["ctx"] = bc.transpose(1, 2).reshape(B, S, E)
    dc = J["dctx"].reshape(B, S, nh, hd).transpose(1, 2).abs()
    n = hd + S + 8
    PD = P * Da
    dV = PD.transpose(-1, -2) @ dc
    dP = (dc @ v.abs().transpose(-1, -2)) * Da
    dS = P * (dP + (dP * P).sum(-1, keepdim=True))
    dQ = dS @ k.abs() / math.sqrt(hd)
    dK = dS.transpose(-1, -2) @ q.abs() / math.sqrt(hd)
    pack = lambda t: t.transpose(1, 2).reshape(B, S, E)
    base["dqkv"] = U * n * torch.cat([pack(dQ), pack(dK), pack(dV)], dim=-1)
    # residual + LayerNorm
    affine = "affine" not in null
    gam = J["gamma"].abs() if affine else torch.ones(E, dtype=F64)
    bet = J["beta"].abs() if affine else torch.zeros(E, dtype=F64)
    Dr = _keepscale(u[offs[0][1]:offs[0][1] + B * S * E], p, (B, S, E))
    y, z, mean, rstd = add_ln_fwd(J["x"], J["t"], u[offs[0][1]:offs[0][1] + B * S * E] if p else None, p,
                                  J["gamma"] if affine else None, J["beta"] if affine else None, EPS)
    za = J["x"].abs() + Dr * J["t"].abs()
    zm = za.mean(-1, keepdim=True)
    depth = E / 64.0 + 12
    rs, mu = rstd.unsqueeze(-1), mean.unsqueeze(-1)
    zc = (z - mu).abs()
    var = (zc ** 2).mean(-1, keepdim=True)
    rel_rstd = U * depth * (1 + (zc * (za + zm)).mean(-1, keepdim=True) / (var + EPS))  # relative error of rstd
    ex = U * depth * rs * (za + zm) + zc * rs * rel_rstd                                 # error of xh = (z - mean) rstd
    base["mean"] = (U * depth * zm).squeeze(-1)
    base["rstd"] = (rs * rel_rstd).squeeze(-1)
    base["y"] = ex * gam + U * 2 * (y.abs() + bet)
    base["y_zero"] = base["y"]
    dya = J["dy"].abs() + (0 if "dy2" in null else J["dy2"].abs())
    ga = dya * gam
    xh = zc * rs
    m2 = (ga * xh).mean(-1, keepdim=True)
    bdx = U * depth * rs * (ga + ga.mean(-1, keepdim=True) + xh * m2) + rs * (ex * m2 + xh * (ga * ex).mean(-1, keepdim=True)) \
        + rel_rstd * rs * (ga + ga.mean(-1, keepdim=True) + xh * m2)
    base["dx"] = bdx
    base["dt"] = bdx * Dr
    rows = B * S
    cd = rows / 64.0 + 66
    base["dgamma"] = U * cd * (dya * xh).sum((0, 1)) + (dya * ex).sum((0, 1))
    base["dbeta"] = U * cd * dya.sum((0, 1))
    Df = _keepscale(u[offs[0][2]:offs[0][2] + B * S * F], p, (B, S, F))
    base["drop"] = U * Df * J["ff"].abs()
    return {k: b + TINY for k, b in base.items()}


def worst_ratio(got, ref, base):
    """max |got - ref| / base over the entries where the reference is finite; a NaN / inf mismatch counts as inf."""
    got, ref = got.to(F64), ref.to(F64)
    fin = torch.isfinite(ref)
    if not bool(torch.isfinite(got[fin]).all()):
        return math.inf
    if not bool(fin.any()):
        return 0.0
    return float(((got - ref).abs()[fin] / base.expand_as(ref)[fin]).max())


def whole_reference(case, n_layers, dt=F64, mut=(), zero_pads=False, grad=True):
    """-> (out, {name: gradient}) of the whole encoder for upstream dout; gradient names: "emb" and "l{layer}.{index}"."""
    I = make_inputs(case, n_layers)
    p = case.p
    emb = I["emb"].to(dt).requires_grad_(grad)
    params = [t.to(dt).requires_grad_(grad) for t in I["params"]]
    out = encoder(I["tok"], I["mask"], emb, I["pe"].to(dt), params, I["noise"] if p else None, p, case.nh, EPS, I["layout"],
                  zero_pads=zero_pads, mut=mut)
    if not grad:
        return out.detach(), {}
    gr = torch.autograd.grad(out, [emb] + params, I["dout"].to(dt))
    names = ["emb"] + [f"l{i // 12}.{i % 12}" for i in range(len(params))]
    return out.detach(), dict(zip(names, gr))


def whole_base(ref, n_layers, grad):
    sites = (1 + 8 * n_layers) * (2 if grad else 1)
    ref = ref.to(F64)
    fin = torch.where(torch.isfinite(ref), ref, torch.zeros_like(ref))
    return C_ENTRY * sites * (fin.abs() + fin.pow(2).mean().sqrt()) + TINY
