"""Float64 torch reference of the MHVAE level kernel (mvk_mhvae_level_fwd/bwd, csrc/mhvae.hip) and of the MHVAE training loss, with
the kernel's case table, seeded inputs, error model and the architectures / procedural inputs of the MHVAE golden cases
(tests/golden/mhvae_*.npz).  CPU only: no GPU, no libmvk.so; nothing here reads the reference project.

Literal form (`literal`): what the reference executes per subset, subset_encode :119-184 with poe (base_utils.py:122-130) and
kl_divergence (:111-119): the log-variance of a masked-out expert is index-put to +inf, the prior is appended, the experts are
stacked, var = exp(lv) + 1e-8, T = 1 / var, jmu = sum(mu T) / sum(T), jlv = log(1 / sum(T)), z = jmu + exp(jlv / 2) eps,
kl = 1/2 (plv - jlv + exp(jlv - plv) + (jmu - pmu)^2 / exp(plv) - 1) summed over the row.  Its backward is torch autograd.  It is
parameterised by dtype: float64 is the reference of every test, float32 is what the error constants are measured on.

Error model.  u = 2^-24.  The `base` of an output entry is a running first-order rounding-error bound of the SAME operation sequence
evaluated once in fp32: every quantity carries (value, absolute error in units of u); an input is exact; a sum, difference, product
or quotient hands its operands' errors down (|a| e_b + |b| e_a for a product, ...) and adds |result| for its own rounding; exp
multiplies the argument's absolute error into a relative one, log divides it; a row sum of n addends adds
(ceil(log2 n) + 1) sum |addend|.  The forward runs the literal sequence above, the backward the formulas of include/mvk.h (`EV`,
`formulas`; their float64 values are also checked against autograd of the literal form, test_mhvae_host.py).  A comparison passes
when |got - ref| <= C_STAGE[stage] * u * base for EVERY entry.  C_STAGE = 2 x the largest |err| / base that the literal form in plain
torch fp32 on the CPU (backward: fp32 autograd) reaches against float64 over the case table, rounded up to one decimal: the
margin of 2 is there because the kernel adds the experts and the rows in another order than torch.  The measured ratios are in
profiles/NOTES_mhvae.md and re-derived by test_mhvae_host.py::test_error_constants; the HIP kernel has no part in them.
`mut` names deliberate mistakes of the REFERENCE, used only to show that the bounds reject them (TEETH)."""
import math
import os
import sys
from collections import OrderedDict
from dataclasses import dataclass
from itertools import combinations

import numpy as np
import torch

from mmvae_ref import TINY, U, worst_ratio  # noqa: F401  (re-exported to the tests)

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import procedural as P  # noqa: E402

F64 = torch.float64
POE_EPS = 1e-8

# one constant per output of the kernel: 2x the value measured by tests/test_mhvae_host.py::test_error_constants, rounded up
C_STAGE = {"z": 1.2, "kl": 0.6, "dmu": 1.0, "dlv": 1.0, "dpmu": 1.2, "dplv": 1.0}
STAGES = tuple(C_STAGE)


def acc(n):
    """Accumulation term of a sum of n addends (a tree or a short sequential run), in units of u sum |addend|."""
    return math.ceil(math.log2(max(n, 1))) + 1


def all_subsets(E):
    """Bitmasks of every non-empty subset of E experts in the model's order: by size, then lexicographic."""
    return [sum(1 << e for e in c) for r in range(1, E + 1) for c in combinations(range(E), r)]


# ---- the kernel's case table ---------------------------------------------------------------------------------------------------------
# (B, F): partial and several workgroups; one lane, a full wave, past a wave, 2 x 2 x 2 (16-byte accesses), past one workgroup's row
# (1030: scalar, 1032: 16-byte accesses with four waves on a row)
SHAPES = ((1, 1), (3, 5), (5, 64), (3, 70), (260, 8), (3, 1030), (5, 8), (260, 5))
EXPERTS = ((1, "all"), (2, "all"), (3, "all"), (5, "all"), (3, "one"), (2, "one"))  # "one": S = 1, the full subset
MASKS = ("none", "some", "row")  # "row": row 0 has every expert masked out
NULLS = ((), ("dz",), ("gkl",), ())


@dataclass(frozen=True)
class Case:
    name: str
    B: int
    F: int
    E: int
    subsets: str
    shared: bool
    masks: str
    eps: bool
    spread: bool
    null: tuple
    seed: int

    @property
    def member(self):
        return all_subsets(self.E) if self.subsets == "all" else [(1 << self.E) - 1]


def _name(B, F, E, subsets, shared, masks, eps, spread, null):
    return (f"b{B}-f{F}-e{E}-{subsets}-{'shared' if shared else 'own'}-m{masks}" + ("" if eps else "-mean")
            + ("-spread" if spread else "") + "".join("-null-" + n for n in null))


def _cases():
    out = []
    for i, (B, F) in enumerate(SHAPES):
        for j, (E, subsets) in enumerate(EXPERTS):
            k = i * len(EXPERTS) + j
            shared = (i + j) % 2 == 0
            masks = MASKS[(i + 2 * j) % 3]
            eps = k % 5 != 3
            null = NULLS[(i + j // 2) % 4]
            out.append(Case(_name(B, F, E, subsets, shared, masks, eps, False, null), B, F, E, subsets, shared, masks, eps, False,
                            null, 7000 + k))
    extra = [(5, 70, 3, "all", True, "some", True, True, ()), (5, 70, 3, "all", False, "some", True, True, ()),
             (3, 1032, 2, "all", True, "row", True, False, ()), (3, 1032, 3, "all", False, "some", True, False, ())]
    for k, a in enumerate(extra):
        out.append(Case(_name(*a), *a, 7100 + k))
    return out


CASES = _cases()
CASE_BY_NAME = {c.name: c for c in CASES}
GROUPS = sorted({(c.B, c.F) for c in CASES})  # one GPU test item per shape


def group_cases(B, F):
    return [c for c in CASES if (c.B, c.F) == (B, F)]


def make_inputs(case):
    """Seeded fp32 inputs.  Log-variances uniform over [-6, 4] ([-20, 20] in the spread cases, where exp(lv) passes 1e-8)."""
    g = torch.Generator().manual_seed(case.seed)
    B, F, E = case.B, case.F, case.E
    member = case.member
    S = len(member)
    lo, hi = (-20.0, 20.0) if case.spread else (-6.0, 4.0)

    def logvar(*shape):
        return lo + (hi - lo) * torch.rand(*shape, generator=g)

    mus, lvs = [], []
    for e in range(E):
        lead = (B, F) if case.shared else (sum(1 for m in member if m >> e & 1), B, F)
        mus.append(1.5 * torch.randn(*lead, generator=g))
        lvs.append(logvar(*lead))
    pmu = plv = None
    if not case.shared:
        pmu, plv = torch.randn(S, B, F, generator=g), logvar(S, B, F)
    masks = None
    if case.masks != "none":
        masks = [torch.rand(B, generator=g) < 0.6 for _ in range(E)]
        if case.masks == "row":
            for m in masks:
                m[0] = False
    eps = torch.randn(S, B, F, generator=g) if case.eps else None
    dz = None if "dz" in case.null else torch.randn(S, B, F, generator=g)
    gkl = None if "gkl" in case.null else torch.randn(S, B, generator=g)
    return dict(mus=mus, lvs=lvs, pmu=pmu, plv=plv, masks=masks, eps=eps, dz=dz, gkl=gkl, member=member)


def ranks(member, E):
    """rank[s][e] = the block of subset s inside expert e in the per-subset layout."""
    count, out = [0] * E, []
    for m in member:
        out.append(list(count))
        for e in range(E):
            count[e] += m >> e & 1
    return out


# ---- the literal form ----------------------------------------------------------------------------------------------------------------
def poe(mus, logvars, eps=POE_EPS):
    var = torch.exp(logvars) + eps
    T = 1.0 / var
    pd_mu = torch.sum(mus * T, dim=0) / torch.sum(T, dim=0)
    pd_var = 1.0 / torch.sum(T, dim=0)
    return pd_mu, torch.log(pd_var)


def kl_divergence(mean, log_var, prior_mean, prior_log_var, eps=0.0):
    kl = 0.5 * (prior_log_var - log_var + torch.exp(log_var - prior_log_var)
                + ((mean - prior_mean) ** 2) / (torch.exp(prior_log_var) + eps) - 1)
    return kl.sum(dim=-1)


def literal(mus, lvs, pmu, plv, masks, eps, member, shared, mut=()):
    """-> z [S,B,F], kl [S,B] in the dtype of the inputs.  pmu = plv = None: the N(0, I) prior."""
    E = len(mus)
    rk = ranks(member, E)
    zs, kls = [], []
    for s, m in enumerate(member):
        list_mu, list_lv = [], []
        for e in range(E):
            if m >> e & 1:
                mu_e, lv_e = (mus[e], lvs[e]) if shared else (mus[e][rk[s][e]], lvs[e][rk[s][e]])
                lv_e = lv_e.clone()
                if masks is not None and "count_masked" not in mut:
                    lv_e[~masks[e]] = torch.inf
                list_mu.append(mu_e)
                list_lv.append(lv_e)
        p_mu = torch.zeros_like(list_mu[0]) if pmu is None else pmu[s]
        p_lv = torch.zeros_like(list_lv[0]) if plv is None else plv[s]
        if "no_prior" not in mut:
            list_mu.append(p_mu)
            list_lv.append(p_lv.detach() if "dplv_no_expert" in mut else p_lv)
        jmu, jlv = poe(torch.stack(list_mu), torch.stack(list_lv), 0.0 if "no_eps" in mut else POE_EPS)
        zs.append(jmu if eps is None else jmu + torch.exp(0.5 * jlv) * eps[s])
        kls.append(kl_divergence(jmu, jlv, p_mu, p_lv, POE_EPS if "kl_eps" in mut else 0.0))
    return torch.stack(zs), torch.stack(kls)


def evaluate(case, I, dtype, mut=()):
    """Forward and autograd backward in `dtype` on the fp32 inputs -> dict(z, kl, dmu [E], dlv [E], dpmu, dplv); dpmu / dplv are
    None without a prior.  dz / gkl None = no upstream gradient (0)."""
    mus = [t.to(dtype).requires_grad_(True) for t in I["mus"]]
    lvs = [t.to(dtype).requires_grad_(True) for t in I["lvs"]]
    pmu = plv = None
    if I["pmu"] is not None:
        pmu, plv = I["pmu"].to(dtype).requires_grad_(True), I["plv"].to(dtype).requires_grad_(True)
    eps = None if I["eps"] is None else I["eps"].to(dtype)
    z, kl = literal(mus, lvs, pmu, plv, I["masks"], eps, I["member"], case.shared, mut)
    total = z.sum() * 0
    if I["dz"] is not None:
        total = total + (z * I["dz"].to(dtype)).sum()
    if I["gkl"] is not None:
        total = total + (kl * I["gkl"].to(dtype)).sum()
    leaves = mus + lvs + ([pmu, plv] if pmu is not None else [])
    grads = torch.autograd.grad(total, leaves, allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, leaves)]
    E = len(mus)
    out = dict(z=z.detach(), kl=kl.detach(), dmu=grads[:E], dlv=grads[E:2 * E], dpmu=None, dplv=None)
    if pmu is not None:
        out.update(dpmu=grads[2 * E], dplv=grads[2 * E + 1])
    return out


def reference(case, I, mut=()):
    return evaluate(case, I, F64, mut)


def run_torch32(case, I):
    return evaluate(case, I, torch.float32)


# ---- running error analysis ------------------------------------------------------------------------------------------------------------
class EV:
    """A float64 value with a first-order bound of the absolute rounding error its fp32 evaluation carries, in units of u."""

    def __init__(self, v, e=None):
        self.v = v
        self.e = torch.zeros_like(v) if e is None else e

    @staticmethod
    def of(x, like=None):
        if isinstance(x, EV):
            return x
        return EV(torch.full_like(like.v, float(x)))

    def __add__(self, o):
        o = EV.of(o, self)
        v = self.v + o.v
        return EV(v, self.e + o.e + v.abs())

    def __sub__(self, o):
        o = EV.of(o, self)
        v = self.v - o.v
        return EV(v, self.e + o.e + v.abs())

    def __mul__(self, o):
        o = EV.of(o, self)
        v = self.v * o.v
        return EV(v, self.v.abs() * o.e + o.v.abs() * self.e + v.abs())

    def __truediv__(self, o):
        o = EV.of(o, self)
        v = self.v / o.v
        return EV(v, (self.e + v.abs() * o.e) / o.v.abs() + v.abs())

    def scale(self, c):
        """Times a power of two, or a sign: exact."""
        return EV(self.v * c, self.e * abs(c))

    def exp(self):
        v = torch.exp(self.v)
        return EV(v, v * (self.e + 1))

    def log(self):
        v = torch.log(self.v)
        return EV(v, self.e / self.v.abs() + v.abs())

    def where(self, cond):
        """The value where cond holds, an exact zero elsewhere."""
        return EV(torch.where(cond, self.v, torch.zeros_like(self.v)), torch.where(cond, self.e, torch.zeros_like(self.e)))


def _row_sum(x, n):
    return EV(x.v.sum(-1), x.e.sum(-1) + acc(n) * x.v.abs().sum(-1) + x.v.sum(-1).abs())


def formulas(case, I):
    """The forward in the literal operation sequence and the backward by the formulas of include/mvk.h, in float64, every output with
    its error base -> (values, bases), both dicts shaped like `reference`."""
    with torch.no_grad():
        E, member, shared = case.E, I["member"], case.shared
        S, B, F = len(member), case.B, case.F
        rk = ranks(member, E)
        ev = lambda t: EV(t.to(F64))
        one = torch.ones(B, F, dtype=F64)
        avail = [torch.ones(B, F, dtype=torch.bool) if I["masks"] is None else I["masks"][e].unsqueeze(-1).expand(B, F)
                 for e in range(E)]
        zs, kls, zb, klb = [], [], [], []
        zero = lambda: EV(torch.zeros(B, F, dtype=F64))
        g_mu = [[zero() for _ in range(1 if shared else sum(1 for m in member if m >> e & 1))] for e in range(E)]
        g_lv = [[zero() for _ in range(len(g_mu[e]))] for e in range(E)]
        g_pmu, g_plv = [], []
        for s, m in enumerate(member):
            ex, T, mu = {}, {}, {}
            for e in range(E):
                if m >> e & 1:
                    k = 0 if shared else rk[s][e]
                    mu[e] = ev(I["mus"][e] if shared else I["mus"][e][k])
                    ex[e] = ev(I["lvs"][e] if shared else I["lvs"][e][k]).exp()
                    T[e] = (EV.of(1.0, ex[e]) / (ex[e] + POE_EPS)).where(avail[e])
            pm = zero() if I["pmu"] is None else ev(I["pmu"][s])
            pl = zero() if I["plv"] is None else ev(I["plv"][s])
            vp = pl.exp()
            Tp = EV.of(1.0, vp) / (vp + POE_EPS)
            Psum, Nsum = None, None
            for e in T:
                Psum = T[e] if Psum is None else Psum + T[e]
                Nsum = mu[e] * T[e] if Nsum is None else Nsum + mu[e] * T[e]
            Psum, Nsum = Psum + Tp, Nsum + pm * Tp
            jmu = Nsum / Psum
            var = EV.of(1.0, Psum) / Psum
            jlv = var.log()
            eps = None if I["eps"] is None else ev(I["eps"][s])
            z = jmu if eps is None else jmu + jlv.scale(0.5).exp() * eps
            d = jmu - pm
            r = (jlv - pl).exp()
            q = d * d / vp
            kl = _row_sum((pl - jlv + r + q - 1.0).scale(0.5), F)
            zs.append(z.v), zb.append(z.e), kls.append(kl.v), klb.append(kl.e)
            # backward (include/mvk.h)
            dz = zero() if I["dz"] is None else ev(I["dz"][s])
            gk = EV(torch.zeros(B, F, dtype=F64) if I["gkl"] is None else I["gkl"][s].to(F64).unsqueeze(-1).expand(B, F).clone())
            a = gk * d / vp
            Gmu = dz + a
            GP = (gk * (var - var * r)).scale(0.5)
            if eps is not None:
                GP = GP - (dz * eps * var * jlv.scale(0.5).exp()).scale(0.5)
            for e in T:
                k = 0 if shared else rk[s][e]
                dT = Gmu * (mu[e] - jmu) * var + GP
                gm = (Gmu * T[e] * var).where(avail[e])
                gl = (dT * ex[e] * T[e] * T[e]).scale(-1.0).where(avail[e])
                g_mu[e][k] = g_mu[e][k] + gm if shared else gm
                g_lv[e][k] = g_lv[e][k] + gl if shared else gl
            if I["pmu"] is not None:
                dTp = Gmu * (pm - jmu) * var + GP
                g_pmu.append(Gmu * Tp * var - a)
                g_plv.append((dTp * vp * Tp * Tp).scale(-1.0) + (gk * (EV.of(1.0, r) - r - q)).scale(0.5))
        pack = lambda xs, f: [(f(x[0]) if shared else torch.stack([f(t) for t in x])) for x in xs]
        val = dict(z=torch.stack(zs), kl=torch.stack(kls), dmu=pack(g_mu, lambda t: t.v), dlv=pack(g_lv, lambda t: t.v),
                   dpmu=None, dplv=None)
        base = dict(z=torch.stack(zb) + TINY / U, kl=torch.stack(klb) + TINY / U, dmu=pack(g_mu, lambda t: t.e + TINY / U),
                    dlv=pack(g_lv, lambda t: t.e + TINY / U), dpmu=None, dplv=None)
        if I["pmu"] is not None:
            val.update(dpmu=torch.stack([t.v for t in g_pmu]), dplv=torch.stack([t.v for t in g_plv]))
            base.update(dpmu=torch.stack([t.e for t in g_pmu]) + TINY / U, dplv=torch.stack([t.e for t in g_plv]) + TINY / U)
        return val, base


def bases(case, I):
    """The error model's base of every output in units of u, float64, shaped like `reference`."""
    return formulas(case, I)[1]


def _pairs(got, ref, base, k):
    if got.get(k) is None or ref.get(k) is None:
        return []
    if isinstance(ref[k], (list, tuple)):
        return list(zip(got[k], ref[k], base[k]))
    return [(got[k], ref[k], base[k])]


def ratios(case, I, got, mut=(), ref=None, base=None):
    """max |got - ref| / (u base) per stage over EVERY entry (`got[k]` None: not written) -> {stage: ratio}."""
    ref = reference(case, I, mut) if ref is None else ref
    base = bases(case, I) if base is None else base
    out = {}
    for k in STAGES:
        for g, r, b in _pairs(got, ref, base, k):
            assert g.shape == r.shape == b.shape, (k, g.shape, r.shape, b.shape)
            out[k] = max(out.get(k, 0.0), worst_ratio(g, r, U * b))
    return out


# (mutation, the stages where it must show, the cases named for it)
TEETH = [
    ("no_prior", ("z", "kl"), ["b260-f8-e2-all-own-mnone", "b5-f64-e3-all-shared-mnone"]),
    ("no_eps", ("z", "kl"), ["b5-f70-e3-all-shared-msome-spread", "b5-f70-e3-all-own-msome-spread"]),
    ("kl_eps", ("kl",), ["b5-f70-e3-all-own-msome-spread"]),
    ("count_masked", ("z", "kl"), ["b3-f70-e3-all-own-msome", "b5-f64-e3-one-shared-msome", "b260-f5-e3-all-own-mrow"]),
    ("dplv_no_expert", ("dplv",), ["b3-f70-e3-all-own-msome", "b5-f64-e5-all-own-mrow", "b3-f1032-e3-all-own-msome"]),
]


# ---- the MHVAE golden cases: architectures of Linear, SiLU, sigmoid and reshapes; procedural inputs ----------------------------------
MHVAE_CASES = ["mhvae_tiny_complete", "mhvae_tiny_masked", "mhvae_tiny_own_posteriors", "mhvae_tiny_two_levels",
               "mhvae_tiny_beta_rescale", "mhvae_tiny_spatial"]
_DIMS3 = [["m1", [6]], ["m2", [5]], ["m3", [2, 3]]]
CASE_CONFIGS = {
    "mhvae_tiny_complete": dict(dims=_DIMS3, n_latent=3, beta=1.0, masked=False, share=True, rescale=False, B=5, seed=3301,
                                shapes=[[4], [6], [3]]),
    "mhvae_tiny_masked": dict(dims=_DIMS3, n_latent=3, beta=1.0, masked=True, share=True, rescale=False, B=7, seed=3302,
                              shapes=[[4], [6], [3]]),
    "mhvae_tiny_own_posteriors": dict(dims=_DIMS3, n_latent=3, beta=1.0, masked=False, share=False, rescale=False, B=5, seed=3303,
                                      shapes=[[4], [6], [3]]),
    "mhvae_tiny_two_levels": dict(dims=_DIMS3, n_latent=2, beta=1.0, masked=True, share=True, rescale=False, B=6, seed=3304,
                                  shapes=[[5], [3]]),
    "mhvae_tiny_beta_rescale": dict(dims=_DIMS3, n_latent=3, beta=2.5, masked=False, share=True, rescale=True, B=5, seed=3305,
                                    shapes=[[4], [6], [3]]),
    "mhvae_tiny_spatial": dict(dims=[["img", [1, 3, 3]], ["vec", [4]]], n_latent=3, beta=0.5, masked=False, share=True,
                               rescale=False, B=4, seed=3306, shapes=[[4, 3, 3], [2, 2, 2], [3]]),
}
# shapes[l - 1] = the shape of z_l and of the l-th bottom-up result (channels first); the top-down result h_l has the shape of z_l


def case_dims(cfg):
    return OrderedDict((m, tuple(d)) for m, d in cfg["dims"])


def case_inputs(cfg):
    """-> dims, data {m: np [B, *dim]}, masks {m: np bool [B]} or None (procedural, bit-exact)."""
    dims = case_dims(cfg)
    data = {m: P.uniform((cfg["B"],) + d, cfg["seed"] + i) for i, (m, d) in enumerate(dims.items())}
    masks = None
    if cfg["masked"]:
        names = list(dims)
        masks = {m: P.hash_uniform(cfg["B"], cfg["seed"] + 50 + i) > 0.4 for i, m in enumerate(names)}
        masks[names[0]][:] = True
        masks[names[-1]][0] = False
    return dims, data, masks


def build_blocks(cfg, nn_mod, BaseEncoder, BaseDecoder, ModelOutput):
    """The architectures of a golden case from the given base classes (the package's or the reference's): Linear, SiLU, sigmoid and
    reshapes only; a level latent [B, C, H, W] is a view, concatenation is on dim 1.
    -> dict(encoders, decoders, bottom_up_blocks, top_down_blocks, posterior_blocks, prior_blocks)."""
    nn = nn_mod
    dims, shapes, L = case_dims(cfg), [tuple(s) for s in cfg["shapes"]], cfg["n_latent"]
    size = lambda s: int(np.prod(s))

    class Enc(BaseEncoder):  # x -> embedding of shape `out`
        def __init__(self, n_in, out):
            BaseEncoder.__init__(self)
            self.out, self.fc = out, nn.Linear(n_in, size(out))

        def forward(self, x):
            h = torch.nn.functional.silu(self.fc(x.reshape(x.shape[0], -1)))
            return ModelOutput(embedding=h.reshape(-1, *self.out))

    class Up(nn.Module):  # a bottom-up block between two levels
        def __init__(self, inp, out):
            nn.Module.__init__(self)
            self.out, self.fc = out, nn.Linear(size(inp), size(out))

        def forward(self, x):
            return torch.nn.functional.silu(self.fc(x.reshape(x.shape[0], -1))).reshape(-1, *self.out)

    class Gauss(BaseEncoder):  # x (any shape) -> embedding, log_covariance of shape `out`
        def __init__(self, n_in, out):
            BaseEncoder.__init__(self)
            self.out, self.mu, self.lv = out, nn.Linear(n_in, size(out)), nn.Linear(n_in, size(out))

        def forward(self, x):
            h = x.reshape(x.shape[0], -1)
            return ModelOutput(embedding=self.mu(h).reshape(-1, *self.out), log_covariance=self.lv(h).reshape(-1, *self.out))

    class Dec(BaseDecoder):
        def __init__(self, inp, out):
            BaseDecoder.__init__(self)
            self.out, self.fc = out, nn.Linear(size(inp), size(out))

        def forward(self, z):
            return ModelOutput(reconstruction=torch.sigmoid(self.fc(z.reshape(z.shape[0], -1))).reshape(-1, *self.out))

    def posterior(i):  # input: cat([h_(i+1), d_(i+1)], dim=1), both of shape shapes[i]
        return Gauss(2 * size(shapes[i]), shapes[i])

    encoders = {m: Enc(size(d), shapes[0]) for m, d in dims.items()}
    decoders = {m: Dec(shapes[0], d) for m, d in dims.items()}
    bottom_up = {m: [Up(shapes[i], shapes[i + 1]) for i in range(L - 2)] + [Gauss(size(shapes[L - 2]), shapes[L - 1])] for m in dims}
    top_down = [Up(shapes[i + 1], shapes[i]) for i in range(L - 1)]
    prior = [Gauss(size(shapes[i]), shapes[i]) for i in range(L - 1)]
    post = [posterior(i) for i in range(L - 1)] if cfg["share"] else {m: [posterior(i) for i in range(L - 1)] for m in dims}
    return dict(encoders=encoders, decoders=decoders, bottom_up_blocks=bottom_up, top_down_blocks=top_down,
                posterior_blocks=post, prior_blocks=prior)


def config_kwargs(cfg):
    dims = case_dims(cfg)
    return dict(n_modalities=len(dims), latent_dim=int(np.prod(cfg["shapes"][-1])), input_dims=dict(dims), n_latent=cfg["n_latent"],
                beta=cfg["beta"], uses_likelihood_rescaling=cfg["rescale"], decoders_dist={m: "normal" for m in dims})


def case_state_dict(cfg):
    """The procedural weights, in the parameter order recorded from the reference."""
    shapes = OrderedDict((k, tuple(s)) for k, s in cfg["sd_shapes"])
    return P.make_state_dict(shapes, cfg["seed"])


def subsets_of(names):
    out = []
    for r in range(1, len(names) + 1):
        out += combinations(names, r)
    return out


def repack_draws(cfg, draws):
    """The reference draws subset-major, level L down to 1 inside a subset -> {"z_l": [S, B, *shape_l]}."""
    L, S = cfg["n_latent"], len(subsets_of([m for m, _ in cfg["dims"]]))
    assert len(draws) == S * L, (len(draws), S, L)
    return {f"z_{L - j}": np.stack([np.asarray(draws[s * L + j]) for s in range(S)]) for j in range(L)}


def mhvae_loss(model, data, masks, noise, batched, dtype=F64):
    """The MHVAE loss from a model's blocks in torch only (any device-less module set built by `build_blocks`), the subsets either
    walked one by one as the reference does (batched=False) or as a batch axis, the way the package's forward runs (batched=True).
    model: an object with encoders, decoders, bottom_up_blocks, top_down_blocks, prior_blocks, _get_posterior_block, n_latent, beta,
    rescale_factors.  noise {"z_l": [S, B, *shape]} -> dict(loss, metrics, z {"z_l": [S, B, *shape]})."""
    names = list(model.encoders.keys())
    L = model.n_latent
    subsets = subsets_of(names)
    S = len(subsets)
    top, skips = {}, {}
    for m in names:
        z = model.encoders[m](data[m]).embedding
        skips[m] = [z]
        for i in range(L - 2):
            z = model.bottom_up_blocks[m][i](z)
            skips[m].append(z)
        top[m] = model.bottom_up_blocks[m][-1](z)
    B = data[names[0]].shape[0]
    mk = None if masks is None else [masks[m] for m in names]
    member = [sum(1 << k for k, m in enumerate(names) if m in s) for s in subsets]
    groups = [list(range(S))] if batched else [[s] for s in range(S)]
    zs = {f"z_{l}": [None] * S for l in range(1, L + 1)}
    kls = {l: [None] * S for l in range(1, L + 1)}
    recon = [None] * S
    for grp in groups:
        n = len(grp)
        mem = [member[s] for s in grp]
        shape = top[names[0]].embedding.shape[1:]
        flat = lambda t, k: t.reshape(k, B, -1)
        used = [k for k in range(len(names)) if any(mm >> k & 1 for mm in mem)]
        sub = [sum(1 << j for j, k in enumerate(used) if mm >> k & 1) for mm in mem]
        umk = None if mk is None else [mk[k] for k in used]
        z, kl = literal([flat(top[names[k]].embedding, 1)[0] for k in used], [flat(top[names[k]].log_covariance, 1)[0] for k in used],
                        None, None, umk, flat(noise[f"z_{L}"][grp], n), sub, True)
        for j, s in enumerate(grp):
            zs[f"z_{L}"][s], kls[L][s] = z[j].reshape(B, *shape), kl[j]
        cur = z.reshape(n * B, *shape)
        for i in range(L - 1, 0, -1):
            h = model.top_down_blocks[i - 1](cur)
            prior = model.prior_blocks[i - 1](h)
            shape = prior.embedding.shape[1:]
            hv = h.reshape(n, B, *h.shape[1:])
            mus, lvs = [], []
            for j, k in enumerate(used):
                rows = [r for r in range(n) if sub[r] >> j & 1]
                hm = torch.cat([hv[r] for r in rows])
                d = skips[names[k]][i - 1].repeat(len(rows), *([1] * (hv.dim() - 2)))
                out = model._get_posterior_block(names[k], i - 1)(torch.cat([hm, d], dim=1))
                mus.append(flat(out.embedding, len(rows)))
                lvs.append(flat(out.log_covariance, len(rows)))
            z, kl = literal(mus, lvs, flat(prior.embedding, n), flat(prior.log_covariance, n), umk, flat(noise[f"z_{i}"][grp], n),
                            sub, False)
            for j, s in enumerate(grp):
                zs[f"z_{i}"][s], kls[i][s] = z[j].reshape(B, *shape), kl[j]
            cur = z.reshape(n * B, *shape)
        for j, s in enumerate(grp):
            recon[s] = {m: model.decoders[m](cur.reshape(n, B, *shape)[j]).reconstruction for m in names}
    losses = []
    for s in range(S):
        rec = 0
        for m in names:
            nll = (0.5 * (recon[s][m] - data[m]) ** 2 + 0.5 * math.log(2 * math.pi)) * float(model.rescale_factors[m])
            nll = nll.reshape(B, -1).sum(-1)
            if masks is not None:
                nll = nll * masks[m]
            rec = rec + nll.sum()
        losses.append(rec + model.beta * sum(kls[l][s].sum() for l in range(1, L + 1)))
    loss = torch.stack(losses).mean()
    metrics = {f"kl_{l}": kls[l][S - 1].sum() for l in range(1, L + 1)}
    return dict(loss=loss, metrics=metrics, z={k: torch.stack(v) for k, v in zs.items()})
