"""Float64 torch reference of the MMVAE / MMVAE+ importance-weight kernels (csrc/mmvae.hip), one function per kernel, written
from the formulas; plus the case table, the seeded inputs and the error model of tests/test_gpu_mmvae_kernels.py.  CPU only.
tests/test_mmvae_ref_host.py pins the composition of these stages to oracle.elbo.mmvae_forward / mmvaeplus_forward.

With M modalities, K samples, B rows, L latent dims of which the first Ls are shared (MMVAE: Ls = L), n_b = the number of
modalities present in row b, a_m[b] in {0, 1} the mask of modality m:
    t(n) = n (normal) | -sign(n) log1p(-|n|) (laplace, n ~ U(-1, 1));   z_c[k,b,:] = mu_c[b,:] + sd_c[b,:] t(noise_c[k,b,:])
    log N(z; m, s) = -(z-m)^2 / (2 s^2) - log s - log(2 pi)/2;         log Lap(z; m, s) = -log(2 s) - |z-m| / s
    lpz_c[k,b]      = sum_{l < L} log p(z_c; prior_mean_l, prior_sd_l)
    lq_all_c[m,k,b] = sum_{l < Ls} log q_m(z_c; mu_m[b,l], sd_m[b,l])                 (-inf where a_m[b] = 0)
    lqz_c[k,b]      = logsumexp_m lq_all_c[m,k,b] - log n_b;   lqw_c[k,b] = sum_{l >= Ls} log q_c(z_c)   (MMVAE+ only)
    lw_c[k,b]       = a_c[b] (sum_r -rows_cr[k,b] a_r[b] + beta (lpz_c - lqz_c - lqw_c))
    w_c[k,b]        = exp(lw_c[k,b] - logsumexp_k lw_c[:,b]);   rowcoef_c = -w_c a_c / n_b  (= d loss / d lw_c, both losses)
    loss            = -sum_c sum_b obj_c[b] / n_b;   obj = logsumexp_k lw - log K (IWAE) | sum_k stopgrad(w) lw (DReG)
DReG also detaches the q parameters inside lq_all / lqw and multiplies every gradient that reaches z_c by w_c (a hook).
    std(lv) = exp(lv / 2) | softmax(lv) L + 1e-6 | softplus(lv; threshold 20) + 1e-6
    cross latent: zc[r,:Ls] = z[r,:Ls];  zc[r,Ls+j] = prior_sd[j] t(noise[r,j])

Every function takes the arrays its kernel takes and returns what the kernel writes; `dtype` selects float64 (the reference) or
float32 (the same formulas in plain torch fp32: what the error constants are measured on).  `mut` names deliberate mistakes,
used only to show that the tolerances reject them.

Error model.  u = 2^-24.  Every output has a `base` of the same shape: base = u S + A, S the float64 sum of the absolute values
of the terms that are added up for that entry, A the argument-rounding terms of expf / logf and the error handed down from an
input the stage recomputes (w from lw, the responsibilities from lq_all).  A comparison passes when |got - ref| <= C * base
for EVERY entry, with one constant C per stage (C_STAGE below: 4x the largest |err| / base that plain torch fp32 shows on the
CPU over the whole case table, rounded up; tests/test_mmvae_ref_host.py re-derives it)."""
import math
from dataclasses import dataclass

import torch
import torch.nn.functional as F

U = 2.0 ** -24
TINY = 2.0 ** -126  # smallest normal fp32: an exp that underflows may be flushed
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
ONE_MINUS = 1.0 - 2.0 ** -24  # largest fp32 below 1
F64 = torch.float64

# one constant per stage: 4x the value measured by tests/test_mmvae_ref_host.py::test_error_constants (recorded there), rounded up
C_STAGE = dict(std=6.0, std_bwd=6.0, z=6.0, lpz=14.0, lq_all=23.0, lqz=6.0, lqw=7.0, lw=13.0, w=4.0, rowcoef=4.0, loss=2.0,
               dmu=8.0, dsd=8.0, dprior=9.0, cross=4.0, cross_bwd=1.0)


def f32(x):
    """A Python float rounded to fp32 (what a `float` argument of the C ABI carries)."""
    return float(torch.tensor(float(x), dtype=torch.float32))


def _l(ts, dtype):
    return None if ts is None else [None if t is None else t.to(dtype) for t in ts]


def t_of(family, noise):
    if family == "normal":
        return noise
    return -noise.sign() * torch.log1p(-noise.abs())


def logp(family, z, loc, sd):
    if family == "normal":
        return -((z - loc) ** 2) / (2 * sd * sd) - torch.log(sd) - HALF_LOG_2PI
    return -torch.log(2 * sd) - (z - loc).abs() / sd


def logp_abs(family, z, loc, sd):
    """Sum of the absolute values of the terms of logp."""
    if family == "normal":
        return ((z - loc) ** 2) / (2 * sd * sd) + torch.log(sd).abs() + HALF_LOG_2PI
    return torch.log(2 * sd).abs() + (z - loc).abs() / sd


def logp_terms(family, z, loc, sd):
    """logp as its two terms (distance, normaliser): their derivatives w.r.t. sd cancel, so magnitudes keep them apart."""
    if family == "normal":
        return -((z - loc) ** 2) / (2 * sd * sd), -torch.log(sd) - HALF_LOG_2PI + 0 * z
    return -(z - loc).abs() / sd, -torch.log(2 * sd) + 0 * z


def avail_of(masks, M, B):
    """-> avail [M,B] bool, n_avail [B] (float64)."""
    if masks is None:
        av = torch.ones(M, B, dtype=torch.bool)
    else:
        av = torch.stack([torch.ones(B, dtype=torch.bool) if m is None else m.bool() for m in masks])
    return av, av.sum(0).to(F64)


# ---- std -------------------------------------------------------------------------------------------------------------------
def std(lv, family, dtype=F64):
    lv = lv.to(dtype)
    if family == "laplace_with_softmax":
        return F.softmax(lv, dim=-1) * lv.shape[-1] + 1e-6
    if family == "normal_with_softplus":
        return F.softplus(lv, threshold=20) + 1e-6
    return torch.exp(0.5 * lv)


def std_base(lv, family):
    """base of std: one exp / log1p chain per entry; the softmax argument lv - max is rounded before the exp."""
    lv = lv.to(F64)
    sd = std(lv, family)
    if family == "laplace_with_softmax":
        return U * sd * (2 + (lv - lv.amax(-1, keepdim=True)).abs())
    return U * sd * 2


def std_vjp(lv, dsd, family, dtype=F64):
    x = lv.to(dtype).clone().requires_grad_()
    (std(x, family, dtype) * dsd.to(dtype)).sum().backward()
    return x.grad


def std_vjp_base(lv, dsd, family):
    lv, dsd = lv.to(F64), dsd.to(F64)
    if family == "laplace_with_softmax":  # d lv_i = L p_i (dsd_i - sum_j dsd_j p_j)
        p = F.softmax(lv, dim=-1)
        S = lv.shape[-1] * p * (dsd.abs() + (dsd.abs() * p).sum(-1, keepdim=True))
        return U * S * (2 + (lv - lv.amax(-1, keepdim=True)).abs())
    if family == "normal_with_softplus":
        return U * 2 * (dsd * torch.sigmoid(lv)).abs() + TINY
    return U * 2 * (dsd * 0.5 * torch.exp(0.5 * lv)).abs() + TINY


# ---- latent forward ----------------------------------------------------------------------------------------------------------
def sample(mus, sds, noises, family, dtype=F64):
    mus, sds, noises = _l(mus, dtype), _l(sds, dtype), _l(noises, dtype)
    return [mus[c] + sds[c] * t_of(family, noises[c]) for c in range(len(mus))]


def sample_base(mus, sds, noises, family):
    mus, sds, noises = _l(mus, F64), _l(sds, F64), _l(noises, F64)
    return [U * (mus[c].abs() + 2 * (sds[c] * t_of(family, noises[c])).abs()) for c in range(len(mus))]


def densities(family, zs, q, masks, prior_mean, prior_sd, Ls, mut=(), want_base=False):
    """The density half of latent_fwd on given (differentiable) z: q[m] = (mu_m, sd_m) [B,L]; prior_sd [L] or [B,L]."""
    M = len(zs)
    K, B, L = zs[0].shape
    av, nav = avail_of(masks, M, B)
    nav = nav.to(zs[0].dtype)
    out = dict(lpz=[], lqz=[], lq_all=[], lqw=[], b_lpz=[], b_lq_all=[], b_lqz=[], b_lqw=[])
    for c in range(M):
        z = zs[c]
        ps = prior_sd
        if "prior_shift" in mut and Ls < L:  # (f) prior_sd indexed by l - Ls in the private dims
            ps = torch.cat([prior_sd[..., :Ls], prior_sd[..., : L - Ls]], dim=-1)
        Lq = L if "private_mixture" in mut else Ls  # (e) private dims scored by the mixture
        lq = [logp(family, z[..., :Lq], q[m][0][:, :Lq], q[m][1][:, :Lq]).sum(-1) for m in range(M)]
        lq_all = torch.stack([torch.where(av[m][None, :], lq[m], torch.full_like(lq[m], -math.inf)) for m in range(M)])
        n = torch.full_like(nav, float(M)) if "logM" in mut else nav  # (a)
        lse = torch.logsumexp(lq_all, dim=0)
        lqz = lse - torch.log(n)
        if "resp_shift" in mut and M > 1:  # (g) every responsibility taken from the next modality (values unchanged)
            r = torch.roll(torch.softmax(lq_all.detach(), dim=0), -1, 0)
            fin = torch.stack([torch.where(av[m][None, :], lq[m], torch.zeros_like(lq[m])) for m in range(M)])
            lqz = lqz.detach() + (r * (fin - fin.detach())).sum(0)
        if Ls < L and "private_mixture" not in mut:
            lqw = logp(family, z[..., Ls:], q[c][0][:, Ls:], q[c][1][:, Ls:]).sum(-1)
        else:
            lqw = torch.zeros_like(lqz)
        out["lpz"].append(logp(family, z, prior_mean, ps).sum(-1))
        out["lqz"].append(lqz)
        out["lq_all"].append(lq_all)
        out["lqw"].append(lqw)
        if want_base:
            with torch.no_grad():
                out["b_lpz"].append(U * logp_abs(family, z, prior_mean, ps).sum(-1))
                b_lq = torch.stack([U * logp_abs(family, z[..., :Ls], q[m][0][:, :Ls], q[m][1][:, :Ls]).sum(-1)
                                    for m in range(M)])
                out["b_lq_all"].append(b_lq)
                worst = torch.where(av[:, None, :].expand_as(b_lq), b_lq, torch.zeros_like(b_lq)).amax(0)
                out["b_lqz"].append(worst + U * (lse.abs() + torch.log(n).abs() + lqz.abs() + M + 2))
                out["b_lqw"].append(U * logp_abs(family, z[..., Ls:], q[c][0][:, Ls:], q[c][1][:, Ls:]).sum(-1)
                                    if Ls < L else torch.zeros_like(lqz))
    return out


def latent_fwd(mus, sds, noises, masks, prior_mean, prior_sd, family, Ls, zs=None, dtype=F64, mut=(), want_base=False):
    """mvk_mmvae_latent_fwd.  zs: the z the densities are evaluated at (the kernel's own fp32 z in the staged comparison;
    None = the samples computed here).  -> dict z, lpz, lqz, lqw [M][K,B], lq_all [M][M,K,B] (+ b_* bases)."""
    mus, sds = _l(mus, dtype), _l(sds, dtype)
    z = sample(mus, sds, noises, family, dtype)
    out = densities(family, z if zs is None else _l(zs, dtype), list(zip(mus, sds)), masks, prior_mean.to(dtype),
                    prior_sd.to(dtype), Ls, mut, want_base)
    out["z"] = z
    return out


# ---- objective ---------------------------------------------------------------------------------------------------------------
def objective(rows, lpz, lqz, lqw, masks, beta, dreg, dtype=F64, mut=(), want_base=False):
    """mvk_mmvae_objective_fwd.  rows[c][r], lpz[c], lqz[c], lqw[c] (or None): [K,B].  -> lw, w, rowcoef [M][K,B], loss."""
    M = len(lpz)
    K, B = lpz[0].shape
    av, nav = avail_of(masks, M, B)
    nav = nav.to(dtype)
    beta = f32(beta)
    out = dict(lw=[], w=[], rowcoef=[], b_lw=[], b_w=[], b_rowcoef=[])
    loss, b_loss, S_loss = 0.0, 0.0, 0.0
    for c in range(M):
        mc = av[c].to(dtype)
        lpx, S = 0.0, 0.0
        for r in range(M):
            lpx = lpx - rows[c][r].to(dtype) * av[r].to(dtype)
            S = S + rows[c][r].to(F64).abs() * av[r].to(F64)
        lat = lpz[c].to(dtype) - lqz[c].to(dtype) - (lqw[c].to(dtype) if lqw is not None else 0.0)
        lw = ((beta * lpx if "beta_lpx" in mut else lpx) + beta * lat) * mc  # (b)
        lse = torch.logsumexp(lw, dim=0)
        w = torch.exp(lw - lse).detach()
        obj = (w * lw).sum(0) if dreg else lse - math.log(K)
        loss = loss - (obj / nav).sum()
        out["lw"].append(lw)
        out["w"].append(w)
        out["rowcoef"].append(-w * mc / nav)
        if want_base:
            with torch.no_grad():
                S = (S + beta * (lpz[c].to(F64).abs() + lqz[c].to(F64).abs()
                                 + (lqw[c].to(F64).abs() if lqw is not None else 0.0))) * av[c].to(F64)
                b_lw = U * S
                lw64, lse64, w64 = lw.to(F64), lse.to(F64), w.to(F64)
                e_col = 2 * b_lw.amax(0) + U * (lw64.abs().amax(0) + lse64.abs() + K + 2)  # relative error of w[:, b]
                b_w = w64 * e_col + TINY
                out["b_lw"].append(b_lw)
                out["b_w"].append(b_w)
                out["b_rowcoef"].append(b_w / nav.to(F64) + U * (w64 / nav.to(F64)))
                if dreg:
                    b_obj = (b_w * lw64.abs() + w64 * b_lw).sum(0) + U * (w64 * lw64).abs().sum(0)
                else:
                    b_obj = b_lw.amax(0) + U * (lse64.abs() + math.log(K) + obj.to(F64).abs() + K + 2)
                b_loss = b_loss + (b_obj / nav.to(F64)).sum()
                S_loss = S_loss + (obj.to(F64).abs() / nav.to(F64)).sum()
    out["loss"] = loss
    if want_base:
        out["S_loss"] = S_loss
        out["b_loss"] = b_loss + U * S_loss
    return out


def loss_from_lw(lw, masks, dreg, w=None):
    """The loss from given lw (float64): -sum_c sum_b obj / n_avail; -> loss, S = sum |obj| / n_avail."""
    M = len(lw)
    K, B = lw[0].shape
    _, nav = avail_of(masks, M, B)
    loss, S = 0.0, 0.0
    for c in range(M):
        x = lw[c].to(F64)
        lse = torch.logsumexp(x, dim=0)
        wc = torch.exp(x - lse) if w is None else w[c].to(F64)
        obj = (wc * x).sum(0) if dreg else lse - math.log(K)
        loss = loss - (obj / nav).sum()
        S = S + (obj.abs() / nav).sum()
    return loss, S


# ---- latent backward -----------------------------------------------------------------------------------------------------------
def latent_bwd(mus, sds, noises, masks, prior_mean, prior_sd, family, Ls, beta, dreg, dz_dec, gloss, w=None, rows=None,
               zs=None, dtype=F64, mut=()):
    """mvk_mmvae_latent_bwd by autograd through latent_fwd + objective.  dz_dec[c] [K,B,L]: the gradient reaching z_c through
    the decoders (already scaled by gloss, as mvk_recon_nll_bwd + mvk_scale_by_device_scalar leave it); gloss: the seed of the
    loss.  w given (the array the kernel consumes): the objective enters through its exact derivative d loss / d lw_c =
    -w_c a_c / n (both losses), i.e. the surrogate -sum w lw a_c / n; w None: rows[c][r] are needed and the whole objective is
    differentiated (tests/test_mmvae_ref_host.py shows the two agree).  zs: evaluate at these z values (the kernel's fp32 z)
    while the gradient still flows through mu + sd t(noise).  -> dmu [M][B,L], dsd [M][B,L], dprior_rows [B,L]."""
    M = len(mus)
    K, B, L = noises[0].shape
    mu = [t.to(dtype).clone().requires_grad_() for t in mus]
    sd = [t.to(dtype).clone().requires_grad_() for t in sds]
    ps = prior_sd.to(dtype).reshape(1, L).expand(B, L).clone().requires_grad_()  # one copy per row: per-row terms
    z = sample(mu, sd, noises, family, dtype)
    if zs is not None:
        z = [zs[c].to(dtype) + (z[c] - z[c].detach()) for c in range(M)]
    detach_q = dreg or "iwae_detached_q" in mut  # (d)
    q = [(m_.detach(), s_.detach()) if detach_q else (m_, s_) for m_, s_ in zip(mu, sd)]
    d = densities(family, z, q, masks, prior_mean.to(dtype), ps, Ls, mut)
    av, nav = avail_of(masks, M, B)
    nav = nav.to(dtype)
    gloss = float(gloss)
    if w is None:
        o = objective(rows, d["lpz"], d["lqz"], d["lqw"] if Ls < L else None, masks, beta, dreg, dtype, mut)
        total, wk = gloss * o["loss"], o["w"]
    else:
        wk = [t.to(dtype) for t in w]
        b32 = f32(beta)
        total = 0.0
        for c in range(M):
            lw = b32 * (d["lpz"][c] - d["lqz"][c] - d["lqw"][c]) * av[c].to(dtype)
            total = total - gloss * (wk[c] * lw * av[c].to(dtype) / nav).sum()
    for c in range(M):
        total = total + (dz_dec[c].to(dtype) * z[c]).sum()
        if dreg and "no_hook" not in mut:  # (c)
            z[c].register_hook(lambda g, w_=wk[c].detach(): w_.unsqueeze(-1) * g)
    total.backward()
    zero = torch.zeros(B, L, dtype=dtype)
    return ([t.grad if t.grad is not None else zero for t in mu], [t.grad if t.grad is not None else zero for t in sd],
            ps.grad if ps.grad is not None else zero)


def latent_bwd_base(mus, sds, noises, masks, prior_mean, prior_sd, family, Ls, beta, dreg, dz_dec, gloss, w, zs, b_lq_all,
                    lqz):
    """base of dmu / dsd / dprior_rows: u * (sum over (c, k) and over the terms of lw — prior, own private posterior, each
    mixture component, decoder — of |contribution|, the sampling path (through z) and the parameter path kept apart) plus the
    mixture contributions times the relative error of their responsibility, exp(lq_all - lse) recomputed from fp32 lq_all
    (error b_lq_all) and an fp32 lse."""
    M = len(mus)
    K, B, L = noises[0].shape
    av, nav = avail_of(masks, M, B)
    mus, sds, noises, zs, w = _l(mus, F64), _l(sds, F64), _l(noises, F64), _l(zs, F64), _l(w, F64)
    pm, b32, gloss = prior_mean.to(F64), f32(beta), float(gloss)
    def acc():
        return ([torch.zeros(B, L, dtype=F64) for _ in range(M)], [torch.zeros(B, L, dtype=F64) for _ in range(M)],
                torch.zeros(B, L, dtype=F64))

    (S_mu, S_sd, S_ps), (E_mu, E_sd, E_ps) = acc(), acc()

    def run(c, part, coef, into):
        A_mu, A_sd, A_ps = into
        mz, sz = mus[c].expand(K, B, L).clone().requires_grad_(), sds[c].expand(K, B, L).clone().requires_grad_()
        mq = [t.expand(K, B, L).clone().requires_grad_() for t in mus]
        sq = [t.expand(K, B, L).clone().requires_grad_() for t in sds]
        ps = prior_sd.to(F64).reshape(1, 1, L).expand(K, B, L).clone().requires_grad_()
        z = mz + sz * t_of(family, noises[c])
        z = zs[c] + (z - z.detach())
        if dreg:
            z.register_hook(lambda g: w[c].unsqueeze(-1) * g)
        qm = [(a.detach(), b.detach()) if dreg else (a, b) for a, b in zip(mq, sq)]
        val = part(z, qm, ps)
        tot = (val if coef is None else coef * val).sum()
        if not tot.requires_grad:
            return
        tot.backward()
        for t, A, m in ([(mz, A_mu, c), (sz, A_sd, c)] + [(mq[m], A_mu, m) for m in range(M)]
                        + [(sq[m], A_sd, m) for m in range(M)]):
            if t.grad is not None:
                A[m] += t.grad.abs().sum(0)
        if ps.grad is not None:
            A_ps += ps.grad.abs().sum(0)

    S_all, E_all = (S_mu, S_sd, S_ps), (E_mu, E_sd, E_ps)
    for c in range(M):
        coef = -gloss * w[c] * av[c].to(F64) / nav * b32  # [K,B]
        lse = lqz[c].to(F64) + torch.log(nav)
        lq = torch.stack([torch.where(av[m][None, :], logp(family, zs[c][..., :Ls], mus[m][:, :Ls], sds[m][:, :Ls]).sum(-1),
                                      torch.full((K, B), -math.inf, dtype=F64)) for m in range(M)])
        r = torch.softmax(lq, dim=0)
        b_lq = torch.where(av[:, None, :].expand_as(b_lq_all[c]), b_lq_all[c], torch.zeros_like(b_lq_all[c]))
        e_r = 2 * b_lq.amax(0) + U * (2 * lse.abs() + M + 4)  # [K,B]: relative error of the responsibilities
        run(c, lambda z, q, ps: (dz_dec[c].to(F64) * z).sum(-1), None, S_all)
        for i in (0, 1):  # the distance term and the normaliser of every density
            run(c, lambda z, q, ps: logp_terms(family, z, pm, ps)[i].sum(-1), coef, S_all)
            if Ls < L:
                run(c, lambda z, q, ps: -logp_terms(family, z[..., Ls:], q[c][0][..., Ls:], q[c][1][..., Ls:])[i].sum(-1),
                    coef, S_all)
            for m in range(M):
                if not bool(av[m].any()):
                    continue

                def part(z, q, ps, m=m):
                    return -(r[m] * logp_terms(family, z[..., :Ls], q[m][0][..., :Ls], q[m][1][..., :Ls])[i].sum(-1))

                run(c, part, coef, S_all)
                run(c, part, coef * e_r / U, E_all)  # the same contributions times e_r (in units of u)
    b_mu = [U * (S_mu[i] * 2 + E_mu[i]) + TINY for i in range(M)]
    b_sd = [U * (S_sd[i] * 2 + E_sd[i]) + TINY for i in range(M)]
    return b_mu, b_sd, U * 2 * S_ps + TINY


def compose_loss(mus, sds, noises, masks, prior_mean, prior_sd, family, Ls, beta, dreg, decode, dtype=F64):
    """The stages chained into a whole loss, differentiable in mus / sds / prior_sd and whatever `decode` closes over:
    decode(c, z_c [K,B,L]) -> [rows_c0, ..] (NLL rows [K,B] of every modality reconstructed from z_c)."""
    M = len(mus)
    L = noises[0].shape[-1]
    z = sample(mus, sds, noises, family, dtype)
    q = [(m_.detach(), s_.detach()) if dreg else (m_, s_) for m_, s_ in zip(mus, sds)]
    d = densities(family, z, q, masks, prior_mean, prior_sd, Ls)
    rows = [decode(c, z[c]) for c in range(M)]
    o = objective(rows, d["lpz"], d["lqz"], d["lqw"] if Ls < L else None, masks, beta, dreg, dtype)
    if dreg:
        for c in range(M):
            if z[c].requires_grad:
                z[c].register_hook(lambda g, w_=o["w"][c]: w_.unsqueeze(-1) * g)
    return o["loss"], o, d, z


# ---- MMVAE+ cross-modal decoder input ----------------------------------------------------------------------------------------------
def cross_latent(z, prior_sd, noise, Ls, family, dtype=F64):
    z, prior_sd, noise = z.to(dtype), prior_sd.to(dtype).reshape(-1), noise.to(dtype)
    return torch.cat([z[..., :Ls], prior_sd * t_of(family, noise)], dim=-1)


def cross_latent_vjp(dzc, z, prior_sd, noise, Ls, family, dtype=F64):
    """-> dz, dprior_sd [D - Ls], and the base of dprior_sd (u * 2 * sum_rows |dzc t(noise)|)."""
    zz = z.to(dtype).clone().requires_grad_()
    ps = prior_sd.to(dtype).reshape(-1).clone().requires_grad_()
    (cross_latent(zz, ps, noise, Ls, family, dtype) * dzc.to(dtype)).sum().backward()
    S = (dzc.to(F64)[..., Ls:] * t_of(family, noise.to(F64))).abs().reshape(-1, ps.numel()).sum(0)
    return zz.grad, ps.grad, U * 2 * S + TINY


# ---- the case table ------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    M: int
    K: int
    B: int
    L: int
    family: str = "normal"
    dreg: bool = False
    Ls: int = 0            # 0: MMVAE (Ls = L)
    mask: str = "none"     # none | random (first modality always present) | mixed (random + a row where only the LAST modality
    #                        is present: the conditioning modality is absent for every other c; + a row with only the first)
    beta: float = 1.0
    gloss: float = 1.0     # 0: 1 / B
    prior: str = "unit"    # unit | learned
    big: bool = False      # rows ~ 3e3 instead of U(0, 50)
    why: str = ""

    @property
    def shared(self):
        return self.Ls or self.L


N, LAP = "normal", "laplace_with_softmax"
CASES = [
    Case("m1-k1-b1-l1-normal-iwae", 1, 1, 1, 1, why="smallest launch: one wave, one lane, K = 1 (w == 1)"),
    Case("m2-k2-b3-l5-laplace-dreg", 2, 2, 3, 5, LAP, True, why="small Laplace DReG, M*K*B = 12"),
    Case("m3-k10-b5-l20-normal-dreg-random-g1B", 3, 10, 5, 20, N, True, mask="random", gloss=0, why="B not a multiple of 4"),
    Case("m5-k2-b5-l64-laplace-iwae-mixed", 5, 2, 5, 64, LAP, False, mask="mixed", why="L = one full wave trip; M = 5"),
    Case("m8-k2-b3-l65-normal-iwae-mixed-learned", 8, 2, 3, 65, N, False, mask="mixed", prior="learned",
         why="M = MVK_MAX_MODALITIES; L one past a wave trip"),
    Case("m8-k1-b160-l20-laplace-dreg-random", 8, 1, 160, 20, LAP, True, mask="random",
         why="M * B = 1280 > 1024 at M = 8: objective_kernel loops"),
    Case("m3-k2-b400-l5-normal-iwae-g1B", 3, 2, 400, 5, N, False, gloss=0, why="M * B = 1200 > 1024 at M = 3"),
    Case("m2-k10-b512-l64-laplace-dreg-learned", 2, 10, 512, 64, LAP, True, prior="learned",
         why="headline size: M * B = 1024 exactly"),
    Case("m2-k33-b64-l70-normal-dreg", 2, 33, 64, 70, N, True, why="K = 33, L = 70: second wave trip of 6 lanes"),
    Case("m3-k33-b3-l130-laplace-iwae-random", 3, 33, 3, 130, LAP, False, mask="random",
         why="L = 130: three wave trips; M*K*B = 297 not a multiple of 4"),
    Case("m2-k2-b5-l130-normal-dreg-learned", 2, 2, 5, 130, N, True, prior="learned", why="wide L, learned prior, DReG"),
    Case("m5-k10-b1-l20-laplace-iwae", 5, 10, 1, 20, LAP, False, why="B = 1"),
    Case("m3-k1-b64-l1-normal-dreg-mixed", 3, 1, 64, 1, N, True, mask="mixed", why="L = 1 with masks; K = 1 under DReG"),
    Case("m2-k2-b3-l64-normal-iwae-random-b2.5", 2, 2, 3, 64, N, False, mask="random", beta=2.5,
         why="beta != 1 without a private part"),
    Case("m3-k10-b5-l65-laplace-dreg-mixed-b0.5-learned", 3, 10, 5, 65, LAP, True, mask="mixed", beta=0.5, prior="learned",
         why="Laplace x masked x DReG x learned prior x beta < 1"),
    Case("p-m2-k2-b5-l20-ls12-normal-iwae-b2.5", 2, 2, 5, 20, N, False, Ls=12, beta=2.5, why="MMVAE+: Ls < L <= 64"),
    Case("p-m3-k10-b5-l70-ls64-laplace-dreg-mixed-b0.5", 3, 10, 5, 70, LAP, True, Ls=64, mask="mixed", beta=0.5,
         why="MMVAE+: Ls = 64 < L, the private part is exactly the second wave trip"),
    Case("p-m2-k2-b3-l100-ls70-normal-dreg-learned-b2.5", 2, 2, 3, 100, N, True, Ls=70, prior="learned", beta=2.5,
         why="MMVAE+: split beyond the first wave trip; per-column prior scales (teeth e, f)"),
    Case("p-m3-k2-b64-l100-ls70-laplace-iwae-random-b2.5-g1B", 3, 2, 64, 100, LAP, False, Ls=70, mask="random", beta=2.5,
         gloss=0, prior="learned", why="MMVAE+ Laplace IWAE masked, non-unit seed"),
    Case("p-m8-k1-b3-l65-ls64-normal-iwae-mixed", 8, 1, 3, 65, N, False, Ls=64, mask="mixed", why="MMVAE+ at M = 8, one private dim"),
    Case("p-m5-k33-b1-l5-ls1-laplace-dreg", 5, 33, 1, 5, LAP, True, Ls=1, why="MMVAE+: one shared dim"),
    Case("p-m2-k10-b512-l130-ls64-normal-dreg-b0.5", 2, 10, 512, 130, N, True, Ls=64, beta=0.5,
         why="MMVAE+ at the headline batch, L = 130"),
    Case("p-m1-k2-b3-l20-ls5-normal-iwae", 1, 2, 3, 20, N, False, Ls=5, why="MMVAE+ with a single modality"),
    Case("big-m2-k10-b64-l20-laplace-dreg", 2, 10, 64, 20, LAP, True, big=True, why="rows ~ 3e3: weights noisy in fp32"),
    Case("big-m8-k2-b512-l5-normal-iwae", 8, 2, 512, 5, N, False, big=True,
         why="M * B = 4096, rows ~ 3e3: the loss accumulates over four trips (suspect 2; teeth h)"),
    Case("big-m8-k2-b512-l5-normal-dreg-random", 8, 2, 512, 5, N, True, big=True, mask="random", why="the same under DReG, masked"),
    Case("big-m3-k33-b5-l64-normal-dreg-mixed-g1B", 3, 33, 5, 64, N, True, big=True, mask="mixed", gloss=0, why="K = 33, rows ~ 3e3"),
    Case("big-p-m2-k10-b5-l70-ls64-laplace-iwae-b2.5", 2, 10, 5, 70, LAP, False, Ls=64, big=True, beta=2.5,
         why="MMVAE+ IWAE, rows ~ 3e3"),
    Case("big-m3-k2-b400-l20-laplace-iwae-mixed", 3, 2, 400, 20, LAP, False, big=True, mask="mixed", why="M * B = 1200, rows ~ 3e3"),
    Case("m5-k2-b64-l70-laplace-dreg-random-g1B", 5, 2, 64, 70, LAP, True, mask="random", gloss=0, why="M = 5, L = 70, Laplace DReG"),
    Case("m2-k1-b512-l5-normal-iwae-mixed", 2, 1, 512, 5, N, False, mask="mixed", why="K = 1 at B = 512 (the one large golden shape)"),
    Case("m8-k10-b5-l130-normal-dreg-b2.5", 8, 10, 5, 130, N, True, beta=2.5, why="M = 8 at L = 130"),
]
CASE_BY_NAME = {c.name: c for c in CASES}


TEETH = [  # (mutation of the REFERENCE, the stages where it must show, the cases named for it)
    ("logM", ("lqz",), ["m3-k10-b5-l20-normal-dreg-random-g1B", "m5-k2-b5-l64-laplace-iwae-mixed"]),
    ("beta_lpx", ("lw",), ["m2-k2-b3-l64-normal-iwae-random-b2.5", "p-m3-k10-b5-l70-ls64-laplace-dreg-mixed-b0.5"]),
    ("no_hook", ("dmu", "dsd"), ["m2-k2-b3-l5-laplace-dreg", "m2-k33-b64-l70-normal-dreg"]),
    ("iwae_detached_q", ("dmu", "dsd"), ["m5-k2-b5-l64-laplace-iwae-mixed", "p-m2-k2-b5-l20-ls12-normal-iwae-b2.5"]),
    ("private_mixture", ("lq_all", "lqw"), ["p-m2-k2-b3-l100-ls70-normal-dreg-learned-b2.5",
                                            "p-m3-k10-b5-l70-ls64-laplace-dreg-mixed-b0.5"]),
    ("prior_shift", ("lpz",), ["p-m2-k2-b3-l100-ls70-normal-dreg-learned-b2.5",
                               "p-m3-k2-b64-l100-ls70-laplace-iwae-random-b2.5-g1B"]),
    ("resp_shift", ("dmu", "dsd"), ["m3-k10-b5-l20-normal-dreg-random-g1B", "m5-k2-b5-l64-laplace-iwae-mixed"]),
    ("two_piece", ("lw",), ["big-m8-k2-b512-l5-normal-iwae", "big-m2-k10-b64-l20-laplace-dreg"]),
]



def make_masks(case, gen):
    M, B = case.M, case.B
    if case.mask == "none":
        return None
    mk = [torch.rand(B, generator=gen) > 0.4 for _ in range(M)]
    mk[0][:] = True
    if case.mask == "mixed":
        for m in range(M):
            mk[m][0] = m == M - 1          # row 0: only the last modality
            if B > 1:
                mk[m][1] = m == 0          # row 1: only the first
        if B > 2 and M > 1:
            mk[1][2] = False               # row 2: the second modality absent, the first present
    return mk


def make_inputs(case):
    """Seeded fp32 inputs of one case: asymmetric (per-row scales on mu, sd in [0.05, 3], per-column prior scales)."""
    import zlib

    gen = torch.Generator().manual_seed(zlib.crc32(case.name.encode()))
    M, K, B, L = case.M, case.K, case.B, case.L
    lap = case.family == LAP
    mus, sds, noises = [], [], []
    for m in range(M):
        mus.append((torch.randn(B, L, generator=gen) * (0.25 + 1.75 * torch.rand(B, 1, generator=gen))
                    + 0.3 * torch.randn(1, L, generator=gen)).float())
        sd = 0.05 + 2.95 * torch.rand(B, L, generator=gen) ** 2 * (0.1 + 0.9 * torch.rand(B, 1, generator=gen))
        sds.append(sd.clamp(0.05, 3.0).float())
        if lap:
            n = (torch.rand(K, B, L, generator=gen) * 2 - 1).float().clamp(-ONE_MINUS, ONE_MINUS)
            flat = n.view(-1)
            flat[0] = 0.0  # Laplace edge values: sign(0) = 0 and the two ends of the open interval
            if flat.numel() > 2:
                flat[1], flat[2] = ONE_MINUS, -ONE_MINUS
        else:
            n = torch.randn(K, B, L, generator=gen).float()
        noises.append(n)
    if case.prior == "learned":
        pm = (0.5 * torch.randn(L, generator=gen)).float()
        ps = (0.5 + 1.5 * torch.rand(L, generator=gen)).float()
    else:
        pm, ps = torch.zeros(L), torch.ones(L)
    masks = make_masks(case, gen)
    if case.big:
        rows = [[(3000.0 * (0.8 + 0.4 * torch.rand(K, B, generator=gen))).float() for _ in range(M)] for _ in range(M)]
    else:
        rows = [[(50.0 * torch.rand(K, B, generator=gen)).float() for _ in range(M)] for _ in range(M)]
    dz_unit = [torch.randn(K, B, L, generator=gen).float() * (0.5 + torch.rand(1, 1, L, generator=gen)) for _ in range(M)]
    gloss = case.gloss or 1.0 / B
    return dict(mus=mus, sds=sds, noises=noises, pm=pm, ps=ps, masks=masks, rows=rows, dz_unit=dz_unit, gloss=f32(gloss))


def dz_dec_from(inp, rowcoef):
    """The decoder-side gradient of the staged backward: gloss * rowcoef_c[k,b] * (a seeded direction), fp32 — the scale
    mvk_recon_nll_bwd gives it, and exactly zero where the conditioning modality is absent (rowcoef == 0 there)."""
    return [(inp["gloss"] * rowcoef[c].float().unsqueeze(-1) * inp["dz_unit"][c] * 3.0).float() for c in range(len(rowcoef))]


def two_piece(x):
    """x rounded to hi + mid of a bf16 split (16 significant bits), in float64."""
    hi = x.float().bfloat16()
    mid = (x.float() - hi.float()).bfloat16()
    return hi.double() + mid.double()


def worst_ratio(got, ref, base):
    """max over EVERY entry of |got - ref| / base (matching infinities count as equal; a NaN or a lone infinity is inf)."""
    got, ref, base = got.detach().to(F64), ref.detach().to(F64), torch.as_tensor(base, dtype=F64)
    if got.numel() == 0:
        return 0.0
    same = (got == ref)
    err = torch.where(same, torch.zeros_like(ref), (got - ref).abs())
    ratio = torch.where(same, torch.zeros_like(ref), err / base.expand_as(ref))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
    return float(ratio.max())


# ---- staged comparison of one implementation (the HIP kernels, or the same formulas in torch fp32) ------------------------------
def run_torch32(case, inp):
    """The three stages in plain torch fp32 on the CPU, chained the way the kernels are (each stage reads the fp32 arrays the
    previous one wrote): the implementation the error constants are measured on."""
    f = torch.float32
    Ls, L = case.shared, case.L
    fw = latent_fwd(inp["mus"], inp["sds"], inp["noises"], inp["masks"], inp["pm"], inp["ps"], case.family, Ls, dtype=f)
    got = {k: [t.detach() for t in fw[k]] for k in ("z", "lpz", "lqz", "lq_all", "lqw")}
    ob = objective(inp["rows"], got["lpz"], got["lqz"], got["lqw"] if Ls < L else None, inp["masks"], case.beta, case.dreg, f)
    got.update(lw=ob["lw"], w=ob["w"], rowcoef=ob["rowcoef"], loss=ob["loss"])
    got["dz_dec"] = dz_dec_from(inp, got["rowcoef"])
    got["dmu"], got["dsd"], got["dprior_rows"] = latent_bwd(
        inp["mus"], inp["sds"], inp["noises"], inp["masks"], inp["pm"], inp["ps"], case.family, Ls, case.beta, case.dreg,
        got["dz_dec"], inp["gloss"], w=got["w"], zs=got["z"], dtype=f)
    return got


def staged_ratios(case, inp, got, mut=(), two_piece_rows=False):
    """max |got - ref| / base per stage, the float64 reference of every stage consuming the fp32 arrays `got` holds for the
    stage before it.  No entry is left out of any comparison.  -> {stage: ratio}; divide by C_STAGE[stage] to judge."""
    Ls, L, M = case.shared, case.L, case.M
    fam, masks = case.family, inp["masks"]
    out = {}
    zr = sample(inp["mus"], inp["sds"], inp["noises"], fam)
    zb = sample_base(inp["mus"], inp["sds"], inp["noises"], fam)
    out["z"] = max(worst_ratio(got["z"][c], zr[c], zb[c]) for c in range(M))
    fw = latent_fwd(inp["mus"], inp["sds"], inp["noises"], masks, inp["pm"], inp["ps"], fam, Ls, zs=got["z"], mut=mut,
                    want_base=True)
    for k in ("lpz", "lq_all", "lqz") + (("lqw",) if Ls < L else ()):
        out[k] = max(worst_ratio(got[k][c], fw[k][c], fw["b_" + k][c]) for c in range(M))
    rows = inp["rows"]
    ins = [got["lpz"], got["lqz"], got["lqw"] if Ls < L else None]
    if two_piece_rows:  # (h) operands at 16 significant bits
        rows = [[two_piece(t) for t in rr] for rr in rows]
        ins = [None if x is None else [two_piece(t) for t in x] for x in ins]
    ob = objective(rows, ins[0], ins[1], ins[2], masks, case.beta, case.dreg, mut=mut, want_base=True)
    for k in ("lw", "w", "rowcoef"):
        out[k] = max(worst_ratio(got[k][c], ob[k][c], ob["b_" + k][c]) for c in range(M))
    out["loss"] = worst_ratio(torch.as_tensor(got["loss"]), ob["loss"], ob["b_loss"])
    args = (inp["mus"], inp["sds"], inp["noises"], masks, inp["pm"], inp["ps"], fam, Ls, case.beta, case.dreg,
            got["dz_dec"], inp["gloss"])
    dmu, dsd, dpr = latent_bwd(*args, w=got["w"], zs=got["z"], mut=mut)
    b_mu, b_sd, b_pr = latent_bwd_base(*args, got["w"], got["z"], fw["b_lq_all"], got["lqz"])
    out["dmu"] = max(worst_ratio(got["dmu"][m], dmu[m], b_mu[m]) for m in range(M))
    out["dsd"] = max(worst_ratio(got["dsd"][m], dsd[m], b_sd[m]) for m in range(M))
    out["dprior"] = worst_ratio(got["dprior_rows"], dpr, b_pr)
    return out
