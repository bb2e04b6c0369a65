"""Float64 torch reference of the CMVAE latent kernels (mvk_cmvae_latent_fwd / _bwd, mvk_cmvae_assign; csrc/cmvae.hip), written
from the formulas; plus the kernels' case table, seeded inputs and error model, and the procedural inputs of the CMVAE golden
cases (tests/golden/cmvae_*.npz).  CPU only: no GPU, no libmvk.so; nothing here reads the reference project.

Latent stage.  Per conditioning modality c: mu_c, sd_c [B,D], noise_c [K,B,D], D = Ls + S;  z_c = mu_c + sd_c t(noise_c) = [u, w];
    lq_all[c][m] = sum_{l<Ls} log q_m(u_l)  (-inf where mask_m is 0),   lqz[c] = logsumexp_m lq_all[c][m] - log n_avail,
    lqw[c] = sum_{l>=Ls} log q_c(w_l),   a_j = log pi_j + sum_{l<Ls} log p(u_l; mean_jl, sd_jl),   pi = softmax(logits),
    lpz[c] = MIX(a) + sum_{l>=Ls} log p(w_l; 0, wsd_l),   resp[c] = softmax_j a_j.
MIX in the LITERAL form of the reference (`reference`): q = softmax_j(a_j) + 1e-20, a loop over the clusters adding
q_j (a_j - log q_j);  in the CLOSED form (`closed_form`, what the kernel evaluates): logsumexp_j a_j.  A logit of -inf: the
literal form is run WITHOUT that cluster (with it, 1e-20 * -inf = -inf), its responsibility and gradients are 0.
Backward (float64 autograd) of  sum_c sum_{k,b} g_c (lpz[c] - lqz[c] - lqw[c]) + sum_c <z_c, dz_dec_c>  over the rows where mask_c
is set, g_c[k,b] = -gscale w_c[k,b] beta / n_avail[b] a constant; DReG: the posterior parameters inside log q are detached and
the gradient reaching z_c is multiplied by w_c (the hook on the sample).  Outputs dmu, dsd per modality, dmeans [C,Ls], dlogits [C].

Assignment.  z [R,Ls]: lpc = log(pi + 1e-20), pc_z = softmax_j(lpc_j + log p(z|j)) [C,R], argmax, norm_llik =
sum_j pc_j (log p(z|j) + lpc_j - log pc_j) / Ls with 0 log 0 = 0.

Error model.  A comparison passes when |got - ref| <= C_STAGE[stage] * base for EVERY entry.  base = 2^-23 times the sum of the
absolute values of the terms added to form the entry, evaluated in float64, each with the error handed down from its operands
(a difference z - loc carries |z| + |loc|, an exp(a - lse) carries 1 + sum |terms of a| + sum |terms of lse|), plus 2^-23 times
its own magnitude, plus 2^-126 (an fp32 exp below the smallest normal may be flushed).  The literal form's own 1e-20 is kept out
of the base: a cluster whose responsibility underflows to 0 keeps a weight of 1e-20 there, so its dmeans / dlogits entries are up
to 1e-20 sum |g d log p| instead of 0; that amount (bases()["literal_1e-20"]), which no rounding produces and no constant
multiplies, is taken off |got - ref| before the comparison.  C_STAGE = 4x the largest |err| / base
that the CLOSED form in plain torch fp32 on the CPU (backward: fp32 autograd) shows over the case table, rounded up
(tests/test_cmvae_host.py::test_error_constants re-derives it; the HIP kernel has no part in it).
The Laplace log-density has a kink at z == loc: make_inputs moves every draw whose sample would come within 1e-4 of a location it
is scored against (cluster means, posterior means, 0), so no entry sits on a kink and none is exempt from comparison.
`mut` names deliberate mistakes of the REFERENCE, used only to show that the bounds reject them (TEETH)."""
import math
import os
import sys
from collections import OrderedDict
from dataclasses import dataclass

import numpy as np
import torch

from mmvae_ref import F64, HALF_LOG_2PI, TINY, logp, logp_abs, t_of, worst_ratio  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import procedural as P  # noqa: E402

from multivae_amd import _lib as MVK  # noqa: E402  (constants only: the library itself is not loaded here)

U2 = 2.0 ** -23
KINK_MARGIN = 1e-4

# one constant per output: 4x the value measured by tests/test_cmvae_host.py::test_error_constants, rounded up
C_STAGE = {"z": 3.0, "lpz": 3.0, "lqz": 2.0, "lqw": 2.0, "resp": 4.0, "dmu": 3.0, "dsd": 4.0, "dmeans": 2.0, "dlogits": 23.0,
           "pc_z": 4.0, "norm_llik": 5.0}
STAGES = tuple(C_STAGE)
FWD_STAGES = ("z", "lpz", "lqz", "lqw", "resp")
BWD_STAGES = ("dmu", "dsd", "dmeans", "dlogits")
ASSIGN_STAGES = ("pc_z", "norm_llik")

# ---- the case table -------------------------------------------------------------------------------------------------------------------
LS = (1, 5, 64, 70)     # one lane, a few, a full wave, past one wave of lanes
SS = (1, 3, 32)
CS = (1, 2, 10, 65)     # 65: the second cluster of a lane
MS = (1, 2, 3)
KS = (1, 4)
BS = (1, 3, 5, 260)     # partial workgroups, more than one workgroup per modality
FAMILIES = ("normal", "laplace")
SPREADS = (1.0, 6.0)    # 6: responsibilities underflow to exact zero in fp32
N_CASES = 48


@dataclass(frozen=True)
class Case:
    name: str
    Ls: int
    S: int
    C: int
    M: int
    K: int
    B: int
    family: str
    dreg: int
    masked: bool
    pruned: bool
    spread: float
    beta: float
    seed: int

    @property
    def D(self):
        return self.Ls + self.S


def _cases():
    out = []
    for i in range(N_CASES):  # the options are cycled with different periods, not multiplied out
        Ls, S, C = LS[i % 4], SS[i % 3], CS[(i // 4 + i) % 4]
        M, K, B = MS[(i // 2 + i // 12) % 3], KS[(i // 3) % 2], BS[(i // 4 + i // 16 + 2 * (i % 2)) % 4]
        family, dreg = FAMILIES[(i + i // 8) % 2], (i // 2 + i // 16) % 2
        masked = M >= 2 and (i // 3 + i // 24) % 2 == 0
        pruned = C >= 2 and (i // 5) % 2 == 0
        spread, beta = SPREADS[(i // 2 + i // 6) % 2], (1.0, 2.5)[(i // 7) % 2]
        name = (f"{i:02d}-l{Ls}-s{S}-c{C}-m{M}-k{K}-b{B}-{family}-{'dreg' if dreg else 'iwae'}" + ("-masked" if masked else "")
                + ("-pruned" if pruned else "") + f"-sp{int(spread)}")
        out.append(Case(name, Ls, S, C, M, K, B, family, dreg, masked, pruned, spread, beta, 7000 + i))
    return out


CASES = _cases()
FAMILY_CODE = {"normal": MVK.FAMILY["normal"], "laplace": MVK.FAMILY["laplace_with_softmax"]}  # the kernels' family argument
for _c in CASES:  # every case fits the kernels' cluster table (include/mvk.h)
    assert _c.C <= MVK.CMVAE_MAX_CLUSTERS and _c.C * (2 * (_c.Ls | 1) + 1) + 4 * _c.Ls <= MVK.CMVAE_MAX_LDS_FLOATS, _c.name
CASE_BY_NAME = {c.name: c for c in CASES}


def _uniform_noise(shape, g):
    lo = float(torch.finfo(torch.float32).eps) - 1.0
    return torch.rand(shape, generator=g) * (1.0 - lo) + lo


def _sample(I, c):
    """fp32 inputs -> float64 z_c [K,B,D]."""
    return I["mu"][c].to(F64) + I["sd"][c].to(F64) * t_of(I["family"], I["noise"][c].to(F64))


def kink_distance(case, I):
    """Smallest |sample - location| over every (sample, location) pair that a log-density scores, float64."""
    Ls, best = case.Ls, math.inf
    for c in range(case.M):
        z = _sample(I, c)
        u, w = z[..., :Ls], z[..., Ls:]
        best = min(best, float((u.unsqueeze(-2) - I["cmean"].to(F64)).abs().min()), float(w.abs().min()))
        for m in range(case.M):
            lim = Ls if m != c else case.D
            best = min(best, float((z[..., :lim] - I["mu"][m].to(F64)[:, :lim]).abs().min()))
    return best


def make_inputs(case):
    """Seeded fp32 inputs.  Cluster stds graded over [0.3, 3]; posterior means spread `spread` around the means of randomly chosen
    clusters; weights w_c a softmax over K; one logit at -inf when pruned; masks leave row 0 with modality 0 alone."""
    g = torch.Generator().manual_seed(case.seed)
    Ls, S, C, M, K, B, D = case.Ls, case.S, case.C, case.M, case.K, case.B, case.D
    cmean = 2.0 * (2.0 * torch.rand(C, Ls, generator=g) - 1.0)
    ramp = torch.arange(C * Ls, dtype=torch.float32).reshape(C, Ls) / max(C * Ls - 1, 1)
    csd = 0.3 * torch.exp(math.log(10.0) * ramp) * (1.0 + 0.05 * torch.rand(C, Ls, generator=g))
    csd = csd.clamp(0.3, 3.0)[torch.randperm(C, generator=g)]
    logits = torch.randn(C, generator=g)
    if case.pruned:
        logits[case.seed % C] = -math.inf
    wsd = 0.5 + torch.rand(S, generator=g)
    mu, sd, noise, w, dz = [], [], [], [], []
    for _ in range(M):
        idx = torch.randint(C, (B,), generator=g)
        mu_u = cmean[idx] + case.spread * torch.randn(B, Ls, generator=g)
        mu.append(torch.cat([mu_u, torch.randn(B, S, generator=g)], dim=1))
        sd.append(0.3 + torch.rand(B, D, generator=g))
        noise.append(torch.randn(K, B, D, generator=g) if case.family == "normal" else _uniform_noise((K, B, D), g))
        w.append(torch.softmax(2.0 * torch.randn(K, B, generator=g), dim=0))
        dz.append(torch.randn(K, B, D, generator=g))
    masks = None
    if case.masked:
        masks = [torch.rand(B, generator=g) > 0.4 for _ in range(M)]
        masks[0][:] |= ~torch.stack(masks).any(0)  # every row keeps a modality
        masks[0][0] = True
        for m in range(1, M):
            masks[m][0] = False
    idx = torch.randint(C, (B,), generator=g)
    assign_z = cmean[idx] + case.spread * torch.randn(B, Ls, generator=g)
    I = dict(family=case.family, mu=mu, sd=sd, noise=noise, w=w, dz=dz, masks=masks, cmean=cmean, csd=csd, logits=logits, wsd=wsd,
             assign_z=assign_z, gscale=0.75, beta=case.beta)
    # keep every sample off the kinks of the Laplace density (and their fp32 neighbourhood): move the offending draws
    for _ in range(8):
        moved = False
        for c in range(M):
            z = _sample(I, c)
            near = (z[..., :Ls].unsqueeze(-2) - cmean.to(F64)).abs().min(-2)[0] < KINK_MARGIN
            near = torch.cat([near, z[..., Ls:].abs() < KINK_MARGIN], dim=-1)
            for m in range(M):
                lim = Ls if m != c else D
                near[..., :lim] |= (z[..., :lim] - mu[m].to(F64)[:, :lim]).abs() < KINK_MARGIN
            if bool(near.any()):
                moved = True
                step = 3e-3 if case.family == "normal" else -3e-3 * noise[c].sign()
                noise[c] = torch.where(near, noise[c] + step, noise[c])
        if not moved:
            break
    near = (assign_z.unsqueeze(-2) - cmean).abs().min(-2)[0] < KINK_MARGIN
    I["assign_z"] = torch.where(near, assign_z + 3e-3, assign_z)
    return I


# ---- formulas -------------------------------------------------------------------------------------------------------------------------
MUTATIONS = ["no_logpi", "unweighted_means", "no_pi_dlogits"]
# (mutation, the stages where it must show, the cases named for it)
_TEETH_CASES = [c.name for c in CASES if c.C >= 10 and not c.pruned and c.spread == 1.0][:2]  # several live clusters sharing the mass
TEETH = [
    ("no_logpi", ("lpz", "resp"), _TEETH_CASES),
    ("unweighted_means", ("dmeans",), _TEETH_CASES),
    ("no_pi_dlogits", ("dlogits",), _TEETH_CASES),
]


def avail_of(case, I):
    if I["masks"] is None:
        av = torch.ones(case.M, case.B, dtype=torch.bool)
    else:
        av = torch.stack([m.bool() for m in I["masks"]])
    return av, av.sum(0).to(F64)


def mixture(a, literal):
    """a [..., C] -> MIX(a) [...]: the explicit expectation under softmax(a) + 1e-20 (cluster loop), or logsumexp."""
    if not literal:
        return torch.logsumexp(a, dim=-1)
    q = torch.softmax(a, dim=-1) + 1e-20
    total = 0
    for j in range(a.shape[-1]):
        total = total + q[..., j] * (a[..., j] - q[..., j].log())
    return total


def evaluate(case, I, dtype, literal=False, mut=()):
    """Forward and autograd backward in `dtype` on the fp32 inputs -> dict of per-stage lists / tensors (keys of STAGES without the
    assignment ones, plus lq_all).  A cluster with a logit of -inf is left out of the computation; its entries are 0."""
    Ls, M, K, B, C, fam = case.Ls, case.M, case.K, case.B, case.C, case.family
    av, nav = avail_of(case, I)
    nav = nav.to(dtype)
    kept = torch.nonzero(torch.isfinite(I["logits"])).reshape(-1)
    mus = [t.to(dtype).requires_grad_(True) for t in I["mu"]]
    sds = [t.to(dtype).requires_grad_(True) for t in I["sd"]]
    cmean = I["cmean"].to(dtype)[kept].requires_grad_(True)
    csd = I["csd"].to(dtype)[kept]
    logits = I["logits"].to(dtype)[kept].requires_grad_(True)
    wsd = I["wsd"].to(dtype)
    beta, gs = I["beta"], I["gscale"]
    qmu = [t.detach() for t in mus] if case.dreg else mus
    qsd = [t.detach() for t in sds] if case.dreg else sds
    lpc = torch.log_softmax(logits, dim=0)
    if "no_logpi" in mut:
        lpc = torch.zeros_like(lpc)
    if "no_pi_dlogits" in mut:
        lpc = logits
    out = {k: [] for k in ("z", "lpz", "lqz", "lqw", "resp", "lq_all", "a")}
    total = 0
    for c in range(M):
        z = mus[c] + sds[c] * t_of(fam, I["noise"][c].to(dtype))
        out["z"].append(z.detach())
        if case.dreg:
            z.register_hook(lambda gr, wc=I["w"][c].to(dtype): gr * wc.unsqueeze(-1))
        u, wv = z[..., :Ls], z[..., Ls:]
        lq = torch.stack([torch.where(av[m], logp(fam, u, qmu[m][:, :Ls], qsd[m][:, :Ls]).sum(-1),
                                      torch.full((), -math.inf, dtype=dtype)) for m in range(M)])
        lqz = torch.logsumexp(lq, dim=0) - torch.log(nav)
        lqw = logp(fam, wv, qmu[c][:, Ls:], qsd[c][:, Ls:]).sum(-1)
        a = lpc + logp(fam, u.unsqueeze(-2), cmean, csd).sum(-1)  # [K,B,C']
        mix = a.sum(-1) if "unweighted_means" in mut else mixture(a, literal)
        lpz = mix + logp(fam, wv, torch.zeros_like(wsd), wsd).sum(-1)
        resp = torch.zeros(K, B, C, dtype=dtype)
        resp[..., kept] = torch.softmax(a, dim=-1).detach()
        afull = torch.full((K, B, C), -math.inf, dtype=dtype)
        afull[..., kept] = a.detach()
        for k, v in (("lpz", lpz), ("lqz", lqz), ("lqw", lqw), ("lq_all", lq)):
            out[k].append(v.detach())
        out["resp"].append(resp)
        out["a"].append(afull)
        g = -(gs / nav) * I["w"][c].to(dtype) * beta * av[c].to(dtype)
        total = total + (g * (lpz - lqz - lqw)).sum() + (z * I["dz"][c].to(dtype) * av[c].to(dtype).unsqueeze(-1)).sum()
    grads = torch.autograd.grad(total, mus + sds + [cmean, logits], allow_unused=True)
    grads = [torch.zeros_like(t) if gr is None else gr for gr, t in zip(grads, mus + sds + [cmean, logits])]
    out["dmu"], out["dsd"] = grads[:M], grads[M : 2 * M]
    out["dmeans"] = torch.zeros(C, Ls, dtype=dtype)
    out["dmeans"][kept] = grads[2 * M]
    out["dlogits"] = torch.zeros(C, dtype=dtype)
    out["dlogits"][kept] = grads[2 * M + 1]
    return out


def reference(case, I, mut=()):
    """The reference's literal form in float64."""
    return evaluate(case, I, F64, literal=True, mut=mut)


def closed_form(case, I, dtype=F64):
    return evaluate(case, I, dtype, literal=False)


def assign(case, I, dtype=F64):
    """-> dict(pc_z [C,R], argmax [R], norm_llik [R], a [R,C])."""
    z = I["assign_z"].to(dtype)
    lpc = torch.log(torch.softmax(I["logits"].to(dtype), dim=0) + 1e-20)
    lpz = logp(case.family, z.unsqueeze(-2), I["cmean"].to(dtype), I["csd"].to(dtype)).sum(-1)  # [R,C]
    a = lpc + lpz
    pc = torch.softmax(a, dim=-1)
    norm = ((pc * a).sum(-1) - torch.special.xlogy(pc, pc).sum(-1)) / case.Ls
    return dict(pc_z=pc.t().contiguous(), argmax=pc.argmax(-1), norm_llik=norm, a=a)


# ---- error model ----------------------------------------------------------------------------------------------------------------------
def _lp_abs(fam, z, loc, sd, zerr):
    """|terms of logp| plus |d logp / dz| times the error (in units of 2^-23) handed down in z - loc."""
    return logp_abs(fam, z, loc, sd) + _dz_abs(fam, z, loc, sd, 0 * zerr) * zerr


def _dz_abs(fam, z, loc, sd, zerr):
    if fam == "normal":
        return ((z - loc).abs() + zerr) / (sd * sd)
    return 1.0 / sd + 0 * (z - loc)


def _dsd_abs(fam, z, loc, sd, zerr):
    d = (z - loc).abs()
    if fam == "normal":
        return (d * d + 2 * d * zerr) / sd ** 3 + 1.0 / sd
    return 1.0 / sd + (d + zerr) / (sd * sd)


def bases(case, I, ref=None):
    """The error model's base of every latent-stage output, float64, shaped like `reference`."""
    ref = reference(case, I) if ref is None else ref
    Ls, M, fam = case.Ls, case.M, case.family
    av, nav = avail_of(case, I)
    beta, gs = I["beta"], I["gscale"]
    cmean, csd, wsd = I["cmean"].to(F64), I["csd"].to(F64), I["wsd"].to(F64)
    lpc_abs = torch.log_softmax(I["logits"].to(F64), 0).abs()
    lpc_abs = torch.where(torch.isfinite(lpc_abs), lpc_abs, torch.zeros_like(lpc_abs))  # an absent cluster adds no term
    pi = torch.softmax(I["logits"].to(F64), 0)
    out = {k: [] for k in FWD_STAGES}
    dmu_abs = [torch.zeros_like(t, dtype=F64) for t in I["mu"]]
    dsd_abs = [torch.zeros_like(t, dtype=F64) for t in I["mu"]]
    dmeans_abs, dlogits_abs = torch.zeros(case.C, Ls, dtype=F64), torch.zeros(case.C, dtype=F64)
    dmeans_lit, dlogits_lit = torch.zeros(case.C, Ls, dtype=F64), torch.zeros(case.C, dtype=F64)  # the literal form's 1e-20
    with torch.no_grad():
        for c in range(M):
            mu_c, sd_c = I["mu"][c].to(F64), I["sd"][c].to(F64)
            tn = t_of(fam, I["noise"][c].to(F64))
            z = ref["z"][c]
            zerr = mu_c.abs() + (sd_c * tn).abs()  # rounding of z, in units of 2^-23 (also the magnitude of its two addends)
            out["z"].append(U2 * (zerr + z.abs()) + TINY)
            u, wv, uerr, werr = z[..., :Ls], z[..., Ls:], zerr[..., :Ls], zerr[..., Ls:]
            # cluster scores and their mixture
            a_abs = lpc_abs + _lp_abs(fam, u.unsqueeze(-2), cmean, csd, uerr.unsqueeze(-2) + cmean.abs()).sum(-1)  # [K,B,C]
            resp = ref["resp"][c]
            mix_abs = (resp * a_abs).sum(-1)
            lpw_abs = _lp_abs(fam, wv, torch.zeros_like(wsd), wsd, werr).sum(-1)
            out["lpz"].append(U2 * (mix_abs + lpw_abs + ref["lpz"][c].abs()) + TINY)
            resp_rel = 1 + a_abs + mix_abs.unsqueeze(-1)
            out["resp"].append(U2 * resp * resp_rel + TINY)
            # mixture of experts
            lq = ref["lq_all"][c]
            lse = ref["lqz"][c] + torch.log(nav)
            lq_abs = torch.stack([_lp_abs(fam, u, I["mu"][m].to(F64)[:, :Ls], I["sd"][m].to(F64)[:, :Ls],
                                          uerr + I["mu"][m].to(F64)[:, :Ls].abs()).sum(-1) for m in range(M)])
            r = torch.exp(lq - lse)  # 0 for absent modalities
            lse_abs = (r * lq_abs).sum(0)
            out["lqz"].append(U2 * (lse_abs + torch.log(nav) + ref["lqz"][c].abs()) + TINY)
            out["lqw"].append(U2 * (_lp_abs(fam, wv, mu_c[:, Ls:], sd_c[:, Ls:], werr + mu_c[:, Ls:].abs()).sum(-1)
                                    + ref["lqw"][c].abs()) + TINY)
            # backward
            wk = I["w"][c].to(F64)
            g = (gs / nav) * wk * beta * av[c].to(F64)  # [K,B]
            dclu = _dz_abs(fam, u.unsqueeze(-2), cmean, csd, uerr.unsqueeze(-2) + cmean.abs())  # [K,B,C,Ls]
            reff = (resp * resp_rel).unsqueeze(-1)
            gz = torch.zeros_like(z)
            gz[..., :Ls] = g.unsqueeze(-1) * (reff * dclu).sum(-2)
            gz[..., Ls:] = g.unsqueeze(-1) * _dz_abs(fam, wv, torch.zeros_like(wsd), wsd, werr)
            dmeans_abs += (g[..., None, None] * reff * dclu).sum((0, 1))
            dlogits_abs += (g.unsqueeze(-1) * (resp * resp_rel + pi * (1 + lpc_abs))).sum((0, 1))
            dmeans_lit += 1e-20 * (g[..., None, None] * dclu).sum((0, 1))
            dlogits_lit += 1e-20 * g.sum() * (1 + a_abs.amax((0, 1)))
            for m in range(M):
                lim = Ls if m != c else case.D
                mu_m, sd_m = I["mu"][m].to(F64), I["sd"][m].to(F64)
                e = zerr + mu_m.abs()
                rm = (r[m] * (1 + lq_abs[m] + lse_abs)).unsqueeze(-1) * torch.ones_like(z)
                rm[..., Ls:] = 1.0 if m == c else 0.0
                gq = g.unsqueeze(-1) * rm * _dz_abs(fam, z, mu_m, sd_m, e)
                gq[..., lim:] = 0
                gz += gq
                if not case.dreg:
                    dmu_abs[m] += gq.sum(0)
                    gs_ = g.unsqueeze(-1) * rm * _dsd_abs(fam, z, mu_m, sd_m, e)
                    gs_[..., lim:] = 0
                    dsd_abs[m] += gs_.sum(0)
            gt = gz + I["dz"][c].to(F64).abs() * av[c].to(F64).unsqueeze(-1)
            if case.dreg:
                gt = gt * wk.unsqueeze(-1)
            dmu_abs[c] += gt.sum(0)
            dsd_abs[c] += (gt * tn.abs()).sum(0)
    out["dmu"] = [U2 * (dmu_abs[m] + ref["dmu"][m].abs()) + TINY for m in range(M)]
    out["dsd"] = [U2 * (dsd_abs[m] + ref["dsd"][m].abs()) + TINY for m in range(M)]
    out["dmeans"] = U2 * (dmeans_abs + ref["dmeans"].abs()) + TINY
    out["dlogits"] = U2 * (dlogits_abs + ref["dlogits"].abs()) + TINY
    out["literal_1e-20"] = dict(dmeans=dmeans_lit, dlogits=dlogits_lit)  # not rounding, not part of a base: see `ratios`
    return out


def assign_bases(case, I, ref=None):
    ref = assign(case, I) if ref is None else ref
    z, cmean, csd = I["assign_z"].to(F64), I["cmean"].to(F64), I["csd"].to(F64)
    lpc = torch.log(torch.softmax(I["logits"].to(F64), 0) + 1e-20).abs()
    a_abs = lpc + _lp_abs(case.family, z.unsqueeze(-2), cmean, csd, z.abs().unsqueeze(-2) + cmean.abs()).sum(-1)  # [R,C]
    pc = ref["pc_z"].t()
    lse_abs = (pc * a_abs).sum(-1)
    return dict(pc_z=(U2 * pc * (1 + a_abs + lse_abs.unsqueeze(-1)) + TINY).t().contiguous(),
                norm_llik=U2 * (lse_abs / case.Ls + ref["norm_llik"].abs()) + TINY)


def ratios(got, ref, base, stages):
    """max |got - ref| / base per stage over EVERY entry -> {stage: ratio}; list-valued stages (one tensor per modality) pooled.
    Where base["literal_1e-20"] names the stage, 1.01x that amount is taken off |got - ref| first (the literal form's 1e-20)."""
    out = {}
    for k in stages:
        g, r, b = got[k], ref[k], base[k]
        slack = base.get("literal_1e-20", {}).get(k)
        if slack is not None:
            d = g.detach().to(F64) - r.detach().to(F64)
            g = r.detach().to(F64) + torch.sign(d) * (d.abs() - 1.01 * slack).clamp(min=0) + 0 * d  # 0 * d: a NaN stays a NaN
        if not isinstance(g, (list, tuple)):
            g, r, b = [g], [r], [b]
        assert len(g) == len(r) == len(b), k
        worst = 0.0
        for gi, ri, bi in zip(g, r, b):
            assert tuple(gi.shape) == tuple(ri.shape) == tuple(bi.shape), (k, gi.shape, ri.shape, bi.shape)
            worst = max(worst, worst_ratio(gi, ri, bi))
        out[k] = worst
    return out


# ---- the CMVAE golden cases: procedural inputs ----------------------------------------------------------------------------------------
TINY_DIMS = OrderedDict(mod1=(2,), mod2=(3,), mod3=(4,), mod4=(4,))
MNIST_SVHN_DIMS = OrderedDict(mnist=(1, 28, 28), svhn=(3, 32, 32))
TINY_L = 5
CMVAE_CASES = ["cmvae_tiny_normal_iwae", "cmvae_tiny_laplace_dreg", "cmvae_tiny_softplus_dreg", "cmvae_tiny_laplace_iwae_masked",
               "cmvae_tiny_normal_dreg_beta_rescale", "cmvae_mnistsvhn_mlp_k2"]
CASE_CONFIGS = {
    "cmvae_tiny_normal_iwae": dict(arch="tiny", B=6, K=3, S=3, C=4, family="normal", loss="iwae_looser", beta=1.0, rescaling=False,
                                   masked=False, seed=801),
    "cmvae_tiny_laplace_dreg": dict(arch="tiny", B=6, K=3, S=3, C=10, family="laplace_with_softmax", loss="dreg_looser", beta=1.0,
                                    rescaling=False, masked=False, seed=802),
    "cmvae_tiny_softplus_dreg": dict(arch="tiny", B=7, K=3, S=2, C=3, family="normal_with_softplus", loss="dreg_looser", beta=1.0,
                                     rescaling=False, masked=False, seed=803),
    "cmvae_tiny_laplace_iwae_masked": dict(arch="tiny", B=6, K=2, S=4, C=5, family="laplace_with_softmax", loss="iwae_looser",
                                           beta=1.0, rescaling=False, masked=True, seed=804),
    "cmvae_tiny_normal_dreg_beta_rescale": dict(arch="tiny", B=5, K=4, S=2, C=6, family="normal", loss="dreg_looser", beta=2.5,
                                                rescaling=True, masked=False, seed=805),
    "cmvae_mnistsvhn_mlp_k2": dict(arch="mnistsvhn", B=8, K=2, S=8, C=10, family="laplace_with_softmax", loss="dreg_looser",
                                   beta=1.0, rescaling=False, masked=False, seed=806),
    "cmvae_predict_prune": dict(arch="tiny", B=12, K=1, S=3, C=4, family="normal", loss="dreg_looser", beta=1.0, rescaling=False,
                                masked=False, seed=807, batch_size=6),
    "cmvae_joint_nll": dict(arch="tiny", B=4, K=1, S=3, C=4, family="laplace_with_softmax", loss="dreg_looser", beta=2.5,
                            rescaling=True, masked=False, seed=808, nll_K=12),
}


def case_dims(cfg):
    return TINY_DIMS if cfg["arch"] == "tiny" else MNIST_SVHN_DIMS


def case_latent_dim(cfg):
    return TINY_L if cfg["arch"] == "tiny" else 20


def case_inputs(cfg):
    """-> dims, data {m: np [B, *dim]}, masks {m: np bool [B]} | None (procedural, bit-exact)."""
    dims, B, seed = case_dims(cfg), cfg["B"], cfg["seed"]
    data = {m: P.uniform((B,) + d, seed + i) for i, (m, d) in enumerate(dims.items())}
    masks = None
    if cfg["masked"]:
        masks = {m: P.hash_uniform(B, seed + 50 + i) > 0.4 for i, m in enumerate(dims)}
        masks["mod1"][:] = True
        for m in ("mod2", "mod3", "mod4"):
            masks[m][0] = False  # sample 0 has a single modality
    return dims, data, masks


def case_state_dict(cfg):
    """Procedural weights of the default multi-latent MLP encoders / decoders and of the CMVAE's own parameters, under the
    reference's parameter names."""
    dims, L, S, C, seed = case_dims(cfg), case_latent_dim(cfg), cfg["S"], cfg["C"], cfg["seed"]
    sd = P.make_state_dict(P.mmvaeplus_mlp_shapes(dims, L, S), seed)
    for i, m in enumerate(dims):
        sd[f"r_mean_priors.{m}"] = np.zeros((1, S), np.float32)
        sd[f"r_logvars_priors.{m}"] = P.uniform((1, S), seed + 900 + i, -0.3, 0.3)
    sd["w_mean_prior"] = np.zeros((1, S), np.float32)
    sd["w_logvar_prior"] = P.uniform((1, S), seed + 950, -0.3, 0.3)
    sd["_pc_params"] = P.uniform((C,), seed + 960, -0.5, 0.5)
    for j in range(C):
        sd[f"mean_clusters.{j}"] = P.uniform((1, L), seed + 1000 + j, -1.0, 1.0)
        sd[f"logvar_clusters.{j}"] = P.uniform((1, L), seed + 2000 + j, -0.3, 0.3)
    return sd
