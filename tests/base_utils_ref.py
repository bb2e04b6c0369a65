"""Float64 torch reference of the public helper kernels of csrc/utils.hip (mvk_poe_fwd/bwd in both modes, mvk_kl_gauss_fwd/bwd,
mvk_logprob_fwd/bwd with the four distributions), written from the formulas of oracle.elbo (poe, stable_poe, kl_divergence,
recon_log_prob); plus the case table, the seeded inputs and the error model of tests/test_gpu_base_utils.py.  CPU only: no GPU,
no libmvk.so.  tests/test_base_utils_ref_host.py pins the reference to oracle.elbo evaluated in float64.

    poe   (mode 0)  T_e = 1 / (exp(lv_e) + eps);  mu = sum_e mu_e T_e / sum_e T_e;  lv = log(1 / sum_e T_e)      eps = float32(1e-8)
    spoe  (mode 1)  lv = -logsumexp_e(-lv_e);  mu = sum_e exp(-lv_e) mu_e * exp(lv);  E == 1: the expert itself;  lv_e = +inf:
                    weight exactly 0 and gradient exactly 0
          backward: the float64 autograd gradient of sum(mu gmu + lv glv)  (gmu / glv NULL = 0)
    kl    rows of sum_l 1/2 (plv - lv + exp(lv - plv) + (mean - pmean)^2 / exp(plv) - 1); every operand indexed modulo its own
          element count (trailing-dimension broadcasting); backward: the full-shape [rows, L] partial derivatives times g[row]
    logprob  oracle.elbo.recon_log_prob element-wise, the target indexed modulo its count (broadcast over leading dimensions);
          categorical: x * log_softmax(r + eps) over rows of C classes; backward: g * d lp / d recon (categorical: the vector-
          Jacobian product over the class row)

Error model (the form of tests/elbo_ref.py): |got - ref| <= C_STAGE[stage] * base for EVERY entry, base computed in float64 from
the inputs as u times the sum of the absolute values of what is added or cancelled (with the argument-rounding terms of expf /
logf: an exponential of argument a carries u |a| of relative error) plus u times the entry's own magnitude, plus TINY for a
flushed subnormal.  The formulas are in the *_base functions below.  C_STAGE is 4x the largest |err| / base that oracle.elbo in
plain torch fp32 on the CPU (backward: fp32 autograd) shows over the case table, rounded up;
tests/test_base_utils_ref_host.py::test_error_constants re-derives it.  `mut` names deliberate mistakes of the REFERENCE, used
only to show that the bounds reject them (TEETH).

Every stable-PoE case keeps lv >= -80: below about -88 the oracle's own exp(-lv) * mu overflows in float32, which is the
reference's defined behaviour and not a kernel fault (tests/elbo_ref.py says the same of the MVAE cases)."""
import math
import zlib
from dataclasses import dataclass

import torch

from elbo_ref import EPS32, acc
from mmvae_ref import TINY, U, f32, worst_ratio  # noqa: F401  (re-exported to the tests)
from oracle import elbo

F64 = torch.float64
XENT_EPS = f32(1e-6)
DISTS = ("normal", "laplace", "bernoulli", "categorical")

# one constant per stage: 4x the value measured by tests/test_base_utils_ref_host.py::test_error_constants, rounded up
C_STAGE = {
    "poe.mu": 2.0, "poe.lv": 2.0, "poe.dmu": 2.0, "poe.dlv": 2.0,
    "spoe.mu": 2.0, "spoe.lv": 2.0, "spoe.dmu": 3.0, "spoe.dlv": 4.0,
    "kl.fwd": 3.0, "kl.dmean": 3.0, "kl.dlv": 3.0, "kl.dpmean": 3.0, "kl.dplv": 4.0,
    "logprob.normal.fwd": 3.0, "logprob.normal.bwd": 6.0, "logprob.laplace.fwd": 3.0, "logprob.laplace.bwd": 3.0,
    "logprob.bernoulli.fwd": 4.0, "logprob.bernoulli.bwd": 4.0, "logprob.categorical.fwd": 3.0, "logprob.categorical.bwd": 4.0,
}


@dataclass(frozen=True)
class Case:
    name: str
    fam: str                # poe | spoe | kl | logprob
    why: str = ""
    # poe / spoe
    E: int = 0
    n: int = 0
    regime: str = "benign"  # poe: benign | wide | eps (exp(lv) ~ 1e-8); spoe: benign | wide | inf (lv = +inf experts)
    null: tuple = ()        # optional pointers passed as NULL (gmu, glv)
    # kl: the shape is [K,B,L], rows = K * B; sizes[j] in full | bl | l | one for mean, lv, pmean, plv
    K: int = 1
    B: int = 1
    L: int = 1
    sizes: tuple = ("full",) * 4
    # logprob: recon [K * nx], target [nx]; categorical: rows of C classes
    dist: str = ""
    nx: int = 0
    C: int = 0
    scale: float = 1.0


def _poe_cases():
    out = []
    for fam in ("poe", "spoe"):
        special = "eps" if fam == "poe" else "inf"
        rows = [
            (1, 1, "benign", (), "one element, one expert" + (": returned bit for bit" if fam == "spoe" else "")),
            (2, 255, "wide", (), "one short of a workgroup; lv on [-12, 6]"),
            (3, 256, special, (), "exactly one workgroup; " + ("exp(lv) ~ eps decides" if fam == "poe" else "+inf experts")),
            (8, 257, "benign", ("glv",), "a second workgroup with one live thread; E = 8; glv NULL"),
            (3, 1300, "wide", ("gmu",), "six workgroups, the last partial; gmu NULL"),
            (2, 1300, special, (), "the special regime across workgroups"),
            (1, 257, "wide", (), "E = 1 across two workgroups"),
        ]
        for E, n, regime, null, why in rows:
            nm = f"{fam}-e{E}-n{n}-{regime}" + "".join(f"-no{x}" for x in null)
            out.append(Case(nm, fam, why, E=E, n=n, regime=regime, null=null))
    return out


def _kl_cases():
    kinds = ("full", "bl", "l", "one")
    out = []
    shapes = [(3, 85, 5, range(4), "rows = 255, K = 3: [B,L] differs from the full size"),
              (3, 85, 130, range(4), "rows = 255, L = 130: 130 workgroups in the backward"),
              (1, 257, 5, (0, 2), "rows = 257: a second workgroup of the forward with one live thread"),
              (1, 257, 130, (1,), "rows = 257, L = 130"),
              (1, 1, 1, (0,), "one row, one column"),
              (3, 85, 1, (3,), "L = 1: a row is an element"),
              (1, 1, 130, (2,), "a single long row")]
    for K, B, L, pats, why in shapes:
        for p in pats:
            sizes = tuple(kinds[(p + j) % 4] for j in range(4))
            nm = f"kl-k{K}-b{B}-l{L}-" + "-".join(sizes)
            out.append(Case(nm, "kl", why + "; operand sizes rotated by " + str(p), K=K, B=B, L=L, sizes=sizes))
    out.append(Case("kl-k3-b85-l5-allfull", "kl", "no broadcasting at all", K=3, B=85, L=5))
    return out


def _logprob_cases():
    out = []
    for dist, scale in (("normal", 1.0), ("normal", 0.75), ("laplace", 0.75), ("bernoulli", 1.0)):
        for K, nx, why in ((1, 1, "one element"), (1, 255, "one short of a workgroup"), (1, 257, "one past a workgroup"),
                           (4, 325, "n = 1300 with n_target = n / 4: the modulo wraps three times"),
                           (1, 1300, "n = 1300, n_target = n")):
            if dist == "normal" and scale == 0.75 and nx not in (257, 325):
                continue
            out.append(Case(f"logprob-{dist}{scale:g}-k{K}-nx{nx}", "logprob", why, dist=dist, K=K, nx=nx, scale=f32(scale)))
    for C, K, rx, why in ((1, 1, 1, "C = 1, one row: three idle waves"), (64, 3, 1, "three rows from one target row"),
                          (65, 1, 5, "five rows: a partial second block of four"), (130, 3, 3, "nine rows, target rows wrap"),
                          (64, 1, 9, "nine rows, n_target = n"), (65, 5, 1, "five rows, one target row"),
                          (130, 1, 3, "three rows, three trips")):
        out.append(Case(f"logprob-categorical-c{C}-k{K}-rows{rx}", "logprob", why, dist="categorical", K=K, nx=rx * C, C=C))
    return out


CASES = _poe_cases() + _kl_cases() + _logprob_cases()
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)

TEETH = [  # (mutation of the REFERENCE, the stages where it must show, the cases named for it)
    ("no_eps", ("poe.lv", "poe.mu"), ["poe-e3-n256-eps", "poe-e2-n1300-eps"]),
    ("mean_not_poe", ("poe.mu", "spoe.mu"), ["poe-e2-n255-wide", "spoe-e2-n255-wide"]),
    ("dlnT_no_eps", ("poe.dlv",), ["poe-e3-n256-eps", "poe-e2-n1300-eps"]),
    ("kl_no_half", ("kl.fwd", "kl.dlv"), ["kl-k3-b85-l5-full-bl-l-one", "kl-k1-b1-l1-full-bl-l-one"]),
    ("kl_wrap_rows", ("kl.fwd", "kl.dmean"), ["kl-k3-b85-l5-bl-l-one-full", "kl-k3-b85-l130-full-bl-l-one"]),
    ("kl_dplv_no_sq", ("kl.dplv",), ["kl-k3-b85-l5-full-bl-l-one", "kl-k1-b257-l130-bl-l-one-full"]),
    ("target_no_wrap", ("logprob.normal.fwd", "logprob.categorical.bwd"), ["logprob-normal1-k4-nx325",
                                                                          "logprob-categorical-c130-k3-rows3"]),
    ("laplace_half", ("logprob.laplace.fwd",), ["logprob-laplace0.75-k1-nx257"]),
    ("xent_no_gx", ("logprob.categorical.bwd",), ["logprob-categorical-c65-k1-rows5"]),
]


# ---- seeded inputs ---------------------------------------------------------------------------------------------------------------------
def kl_shape(case, kind):
    K, B, L = case.K, case.B, case.L
    return {"full": (K, B, L), "bl": (B, L), "l": (L,), "one": (1,)}[kind]


def make_inputs(case):
    gen = torch.Generator().manual_seed(zlib.crc32(case.name.encode()))
    rn = lambda *s: torch.randn(*s, generator=gen)
    ru = lambda *s: torch.rand(*s, generator=gen)
    if case.fam in ("poe", "spoe"):
        E, n = case.E, case.n
        mu, lv = rn(E, n), 0.5 * rn(E, n)
        if case.regime == "wide":
            mu, lv = 10.0 * rn(E, n), 18.0 * ru(E, n) - 12.0
        elif case.regime == "eps":  # the first and the last expert have exp(lv) ~ 1e-8
            lv[0], lv[-1] = -20.0 + 4.0 * ru(n), -20.0 + 4.0 * ru(n)
        elif case.regime == "inf":  # a missing modality: +inf, never on every expert of an element
            gone = ru(E, n) < 0.4
            gone[0] = False
            gone[1, 0] = True
            lv = torch.where(gone, torch.full_like(lv, math.inf), lv)
        g = 10.0 ** (6 * ru(n) - 3)
        return dict(mu=mu.float(), lv=lv.float(), gmu=None if "gmu" in case.null else (rn(n) * g).float(),
                    glv=None if "glv" in case.null else (rn(n) * g).float())
    if case.fam == "kl":
        ops = []
        for j, kind in enumerate(case.sizes):
            s = kl_shape(case, kind)
            ops.append((rn(*s) if j % 2 == 0 else 6.0 * ru(*s) - 4.0).float())  # log-variances on [-4, 2]
        rows = case.K * case.B
        return dict(ops=ops, g=(rn(rows) * 10.0 ** (6 * ru(rows) - 3)).float())
    K, nx, C = case.K, case.nx, case.C
    if case.dist == "categorical":
        r = 2.0 * rn(K, nx // C, C)
        r = torch.where(ru(K, nx // C, C) < 0.1, 80.0 * ru(K, nx // C, C) - 40.0, r)
        x = torch.softmax(rn(nx // C, C), -1) if (nx // C) % 2 else \
            torch.nn.functional.one_hot(torch.randint(0, C, (nx // C,), generator=gen), C).float()
        r, x = r.reshape(K, nx), x.reshape(nx)
    elif case.dist == "bernoulli":
        r = torch.where(ru(K, nx) < 0.1, 180.0 * ru(K, nx) - 90.0, 3.0 * rn(K, nx))
        r.view(-1)[0], r.view(-1)[-1] = -90.0, 90.0
        x = ru(nx)
        x = torch.where(ru(nx) < 0.5, (x > 0.5).float(), x)  # hard and soft targets
    else:
        r, x = rn(K, nx), ru(nx)
        if case.dist == "laplace":
            tie = ru(K, nx) < 0.05
            tie[0, 0] = True
            r = torch.where(tie, x.expand(K, nx), r)
    return dict(r=r.float().contiguous(), x=x.float().contiguous(), g=(rn(K, nx) * 10.0 ** (6 * ru(K, nx) - 3)).float())


# ---- the float64 reference -----------------------------------------------------------------------------------------------------------
def _poe_fwd(case, mu, lv, mut=()):
    if case.fam == "poe":
        lnT = -torch.log(torch.exp(lv) + (0.0 if "no_eps" in mut else EPS32))
        if "dlnT_no_eps" in mut:  # the backward's d ln T / d lv taken as -1 (its value without eps) instead of -exp(lv) T
            lnT = lnT.detach() + (lv.detach() - lv)
        T = torch.exp(lnT)
        if "mean_not_poe" in mut:
            return mu.mean(0), torch.log(1.0 / T.sum(0))
        return (mu * T).sum(0) / T.sum(0), torch.log(1.0 / T.sum(0))
    if case.E == 1:
        return mu[0], lv[0]
    lnv = -torch.logsumexp(-lv, 0)
    if "mean_not_poe" in mut:
        return mu.mean(0), lnv
    return (torch.exp(-lv) * mu).sum(0) * torch.exp(lnv), lnv


def _kl_elem(a, b, c, d, mut=()):
    h = 1.0 if "kl_no_half" in mut else 0.5
    q = (a - c) ** 2 / torch.exp(d)
    if "kl_dplv_no_sq" in mut:  # d / d plv without the (mean - pmean)^2 / exp(plv) term (values unchanged)
        q = (a - c) ** 2 / torch.exp(d.detach())
    return h * (d - b + torch.exp(b - d) + q - 1.0)


def _lp(case, r, x, mut=()):
    """Element-wise log-probability [K, nx]."""
    K, nx, C, s = case.K, case.nx, case.C, case.scale
    if "target_no_wrap" in mut and K > 1:  # the target read at i instead of i mod n_target (clamped to its last entry)
        idx = torch.arange(K * nx).clamp(max=nx - 1).reshape(K, nx)
        xx = x[idx]
    else:
        xx = x.expand(K, nx)
    if case.dist == "normal":
        return -((xx - r) ** 2) / (2.0 * s * s) - math.log(s) - 0.5 * math.log(2.0 * math.pi)
    if case.dist == "laplace":
        return -math.log((1.0 if "laplace_half" in mut else 2.0) * s) - (xx - r).abs() / s
    if case.dist == "bernoulli":
        ls = torch.nn.functional.logsigmoid
        return xx * ls(r) + (1.0 - xx) * ls(-r)
    v = r.reshape(K, nx // C, C) + XENT_EPS
    lsm = v - torch.logsumexp(v, -1, keepdim=True)
    if "xent_no_gx" in mut:  # the softmax term of the backward left out (values unchanged)
        lsm = v - torch.logsumexp(v, -1, keepdim=True).detach()
    return (xx.reshape(K, nx // C, C) * lsm).reshape(K, nx)


def expand_ops(case, ops, dtype):
    """The four KL operands expanded to the full [K,B,L] shape as autograd leaves (their gradients are the full-shape partials)."""
    full = kl_shape(case, "full")
    return [t.to(dtype).expand(full).clone().requires_grad_() for t in ops]


def reference(case, inp, mut=(), dtype=F64):
    """Every array the forward and the backward entry point of the case's family write, in `dtype`."""
    if case.fam in ("poe", "spoe"):
        mu, lv = inp["mu"].to(dtype).clone().requires_grad_(), inp["lv"].to(dtype).clone().requires_grad_()
        om, ol = _poe_fwd(case, mu, lv, mut)
        tot = 0.0
        if inp["gmu"] is not None:
            tot = tot + (om * inp["gmu"].to(dtype)).sum()
        if inp["glv"] is not None:
            tot = tot + (ol * inp["glv"].to(dtype)).sum()
        dmu, dlv = torch.autograd.grad(tot, [mu, lv], allow_unused=True)
        dmu = torch.zeros_like(mu) if dmu is None else dmu
        dlv = torch.zeros_like(lv) if dlv is None else dlv
        return dict(mu=om.detach(), lv=ol.detach(), dmu=dmu, dlv=dlv.nan_to_num(0.0) if case.regime == "inf" else dlv)
    if case.fam == "kl":
        leaves = expand_ops(case, inp["ops"], dtype)
        a, b, c, d = leaves
        if "kl_wrap_rows" in mut:  # a [B,L] operand read at row r instead of r mod B (clamped to its last row)
            row = torch.arange(case.K * case.B).clamp(max=case.B - 1)
            a, b, c, d = (t if kind != "bl" else t.reshape(-1, case.L)[row].reshape(t.shape)
                          for t, kind in zip(leaves, case.sizes))
        kl = _kl_elem(a, b, c, d, mut).sum(-1)
        gs = torch.autograd.grad((kl * inp["g"].to(dtype).reshape(kl.shape)).sum(), leaves)
        return dict(fwd=kl.detach().reshape(-1), dmean=gs[0], dlv=gs[1], dpmean=gs[2], dplv=gs[3])
    r = inp["r"].to(dtype).clone().requires_grad_()
    lp = _lp(case, r, inp["x"].to(dtype), mut)
    (dr,) = torch.autograd.grad((lp * inp["g"].to(dtype)).sum(), r)
    return dict(fwd=lp.detach(), bwd=dr)


def oracle_eval(case, inp, dtype):
    """The same arrays by oracle.elbo's own functions in `dtype`, gradients by autograd."""
    if case.fam in ("poe", "spoe"):
        mu, lv = inp["mu"].to(dtype).clone().requires_grad_(), inp["lv"].to(dtype).clone().requires_grad_()
        om, ol = elbo.poe(mu, lv, EPS32) if case.fam == "poe" else elbo.stable_poe(mu, lv)
        tot = 0.0
        if inp["gmu"] is not None:
            tot = tot + (om * inp["gmu"].to(dtype)).sum()
        if inp["glv"] is not None:
            tot = tot + (ol * inp["glv"].to(dtype)).sum()
        dmu, dlv = torch.autograd.grad(tot, [mu, lv], allow_unused=True)
        dmu = torch.zeros_like(mu) if dmu is None else dmu
        dlv = torch.zeros_like(lv) if dlv is None else dlv
        return dict(mu=om.detach(), lv=ol.detach(), dmu=dmu, dlv=dlv.nan_to_num(0.0) if case.regime == "inf" else dlv)
    if case.fam == "kl":
        ops = expand_ops(case, inp["ops"], dtype)
        kl = elbo.kl_divergence(*ops)
        gs = torch.autograd.grad((kl * inp["g"].to(dtype).reshape(kl.shape)).sum(), ops)
        return dict(fwd=kl.detach().reshape(-1), dmean=gs[0], dlv=gs[1], dpmean=gs[2], dplv=gs[3])
    K, nx, C = case.K, case.nx, case.C
    r = inp["r"].to(dtype).clone().requires_grad_()
    x = inp["x"].to(dtype)
    if case.dist == "categorical":
        lp = elbo.recon_log_prob("categorical", r.reshape(K, nx // C, C), x.reshape(nx // C, C)).reshape(K, nx)
    else:
        lp = elbo.recon_log_prob(case.dist, r, x, case.scale)
    (dr,) = torch.autograd.grad((lp * inp["g"].to(dtype)).sum(), r)
    return dict(fwd=lp.detach(), bwd=dr)


def run_torch32(case, inp):
    return oracle_eval(case, inp, torch.float32)


# ---- the error model -------------------------------------------------------------------------------------------------------------------
def _poe_base(case, inp):
    mu, lv = inp["mu"].to(F64), inp["lv"].to(F64)
    gm = 0.0 if inp["gmu"] is None else inp["gmu"].to(F64).abs()
    gl = 0.0 if inp["glv"] is None else inp["glv"].to(F64).abs()
    ref = reference(case, inp)
    with torch.no_grad():
        if case.fam == "poe":
            lnT = -torch.log(torch.exp(lv) + EPS32)
            dln = torch.exp(lv) * torch.exp(lnT)  # |d ln T / d lv|
        else:
            lnT, dln = -lv, torch.ones_like(lv)
        mx = lnT.amax(0)
        w = torch.exp(lnT - torch.logsumexp(lnT, 0))  # T_e / sum T
        Fe = 3 + lv.abs().nan_to_num(posinf=0.0) + lnT.abs().nan_to_num(posinf=0.0) + (lnT - mx).abs().nan_to_num(posinf=0.0)
        Fb = (w * Fe).sum(0)  # the error of the normalisation, in units of u
        pm, pl = ref["mu"], ref["lv"]
        EM = (w * mu.abs() * (Fe + Fb)).sum(0) + pm.abs()
        EL = acc(case.E) + Fb + mx.abs() + pl.abs()
        if case.fam == "spoe" and case.E == 1:
            EM, EL = torch.zeros_like(pm), torch.zeros_like(pl)  # returned bit for bit
        dmu = U * (gm * w * (Fe + Fb) + ref["dmu"].abs()) + TINY
        dlv = U * (w * dln * (gm * (mu.abs() * (Fe + Fb) + EM) + gl * (Fe + Fb)) + ref["dlv"].abs()) + TINY
        dlv = torch.where(w == 0, torch.zeros_like(dlv), dlv)  # a +inf expert: exactly 0
        return dict(mu=U * EM + TINY, lv=U * EL + TINY, dmu=dmu, dlv=dlv)


def _kl_base(case, inp):
    ref = reference(case, inp)
    with torch.no_grad():
        a, b, c, d = (t.detach() for t in expand_ops(case, inp["ops"], F64))
        L = case.L
        g = inp["g"].to(F64).abs().reshape(case.K, case.B, 1)
        inv, e1, df = torch.exp(-d), torch.exp(b - d), (a - c).abs()
        q = df * df * inv
        cancel = df * (a.abs() + c.abs()) * inv  # the rounding of mean - pmean, carried into its square
        E1 = e1 * (2 + (b - d).abs() + b.abs() + d.abs())
        Q = q * (3 + d.abs()) + 2 * cancel
        eb = 0.5 * (d.abs() + b.abs() + E1 + Q + 1)
        t = _kl_elem(a, b, c, d).abs()
        fwd = U * (eb.sum(-1) + acc(L) * t.sum(-1) + ref["fwd"].abs().reshape(case.K, case.B)) + TINY
        dm = U * g * inv * ((a.abs() + c.abs()) + df * (3 + d.abs())) + TINY
        dlv = U * (g * 0.5 * (E1 + 1) + ref["dlv"].abs()) + TINY
        dplv = U * (g * 0.5 * (1 + E1 + Q) + ref["dplv"].abs()) + TINY
        return dict(fwd=fwd.reshape(-1), dmean=dm, dlv=dlv, dpmean=dm, dplv=dplv)


def _lp_base(case, inp):
    ref = reference(case, inp)
    with torch.no_grad():
        K, nx, C, s = case.K, case.nx, case.C, case.scale
        r, x, g = inp["r"].to(F64), inp["x"].to(F64).expand(K, nx), inp["g"].to(F64).abs()
        own_f, own_b = ref["fwd"].abs(), ref["bwd"].abs()
        if case.dist == "normal":
            d = (x - r).abs()
            fwd = (x.abs() + r.abs()) * d / (s * s) + d * d / (2 * s * s) + abs(math.log(s)) + 0.919
            bwd = g * (x.abs() + r.abs()) / (s * s)
        elif case.dist == "laplace":
            fwd = abs(math.log(2 * s)) + (x.abs() + r.abs()) / s + (x - r).abs() / s
            bwd = torch.zeros_like(r)
        elif case.dist == "bernoulli":
            l1p = torch.log1p(torch.exp(-r.abs()))
            # the fp32 oracle is -BCE-with-logits = -((1 - x) r + max(-r, 0) + log(1 + exp(-|r|))): (1 - x) r cancels against
            # max(-r, 0) for r < 0 and the log is taken of 1 + exp(-|r|), so a saturated entry has an absolute error of
            # u (|r| + 1) where the kernel's min(a, 0) - log1pf(..) form has a relative one; the base follows the oracle's form
            fwd = (1 + 2 * x.abs()) * (r.abs() + l1p + 1)
            bwd = g * (x.abs() + torch.sigmoid(r))
        else:
            v = r.reshape(K, -1, C) + XENT_EPS
            xx, gg = x.reshape(K, -1, C), g.reshape(K, -1, C)
            mx, lse = v.amax(-1, keepdim=True), torch.logsumexp(v, -1, keepdim=True)
            p = torch.exp(v - lse)
            EL = lse.abs() + mx.abs() + acc(C) + 2 + (p * ((v - mx).abs() + v.abs())).sum(-1, keepdim=True)
            fwd = (xx.abs() * (v.abs() + lse.abs() + EL)).reshape(K, nx)
            sgx = (gg * xx.abs()).sum(-1, keepdim=True)
            bwd = (gg * xx.abs() + p * sgx * (2 + acc(C) + v.abs() + lse.abs() + EL)).reshape(K, nx)
        return dict(fwd=U * (fwd + own_f) + TINY, bwd=U * (bwd + own_b) + TINY * (1 + g))


def bases(case, inp):
    return {"poe": _poe_base, "spoe": _poe_base, "kl": _kl_base, "logprob": _lp_base}[case.fam](case, inp)


def stage_of(case, key):
    return f"logprob.{case.dist}.{key}" if case.fam == "logprob" else f"{case.fam}.{key}"


def ratios(case, got, ref, base):
    """max |got - ref| / base over EVERY entry, per stage -> {stage: ratio} (None: the array was not written)."""
    out = {}
    for k, gv in got.items():
        if gv is not None and k in ref:
            assert gv.shape == ref[k].shape == base[k].shape, (k, gv.shape, ref[k].shape, base[k].shape)
            out[stage_of(case, k)] = worst_ratio(gv, ref[k], base[k])
    return out
