"""Float64 torch reference of the fused posterior kernels of csrc/elbo.hip (mvk_mopoe_posterior_*, mvk_mvtcae_posterior_*,
mvk_mvae_posterior_*, mvk_jmvae_posterior_*, mvk_gauss_sample_kl_*), one forward function per family written from the formulas
of oracle/elbo.py (poe, stable_poe, rsample, mopoe_inference / mopoe_joint_divergence, the MVTCAE / MVAE / JMVAE forward code),
the backward by float64 autograd of that forward; plus the case table, the seeded inputs and the error model of
tests/test_gpu_elbo_posterior.py.  CPU only: no GPU, no libmvk.so.  tests/test_elbo_ref_host.py pins these functions to
oracle.elbo evaluated in float64.

With M experts (mu_m, lv_m) [B,L], eps = float32(1e-8) (the value the kernel and the fp32 oracle add), a missing modality taken
as lv_m = +inf exactly as the oracle does it:
    poe:        T_m = 1 / (exp(lv_m) + eps);  D = sum_m T_m (+ 1 / (1 + eps): the N(0,I) expert);  mu = sum_m mu_m T_m / D;
                lv = log(1 / D)
    stable_poe: lv = -logsumexp_m(-lv_m, 0);  mu = sum_m exp(-lv_m) mu_m * exp(lv)        (the 0: the N(0,I) expert, always)
    rsample:    z[k] = mu + exp(lv / 2) eps[k];          KL(mu, lv) = -1/2 sum_l (1 - exp(lv) - mu^2 + lv)
    MoPoE:      poe per subset (prior expert on the full subset only), z from subset sel[b], kld[b] = sum_s w[s,b] KL_s[b]
    MVTCAE:     poe of all experts without prior; joint KL; cond_m = -1/2 sum_l (1 - e^lv / e^lv_m - (mu - mu_m)^2 / e^lv_m
                + lv - lv_m), 0 where m is missing
    MVAE:       stable_poe per subset of the subset's present experts; one sample per subset, copied into every member's slab
    JMVAE:      z, KL of the joint encoder's (mu, lv); ljm = sum_l sum_m 1/2 (lv_m - lv + (e^lv + (mu - mu_m)^2) / e^lv_m - 1)
    gauss:      rsample and KL of one diagonal Gaussian
Every MVAE case keeps lv >= -80 (the regimes here stay above -20): below about -88 the oracle's own exp(-lv) * mu overflows in
float32, which is the reference's defined behaviour and not a kernel fault.

Error model.  u = 2^-24.  Every output has a `base` of its own shape, computed in float64 from the inputs: u times the sum of
the absolute values of the terms that are added or cancelled to form the entry (with the error handed down from the values the
entry is formed from: EM, the error of a product-of-experts mean in units of u, = sum_m |mu_m| T_m / D + |mu|, and EL, that of
its log-variance, = 1 + |lv|) plus u times its own magnitude; row sums: the sum of the per-element bases plus
(ceil(log2 n) + 1) u sum |addend| for n addends.  A comparison passes when |got - ref| <= C * base for EVERY entry, with one
constant per family and output (C_STAGE: 4x the largest |err| / base that oracle.elbo in plain torch fp32 on the CPU, backward
by fp32 autograd, shows over the whole case table, rounded up; tests/test_elbo_ref_host.py re-derives it).  Where a base is 0
(gradients of a missing modality's rows) the entry must be exactly the reference's 0.
`mut` names deliberate mistakes of the REFERENCE, used only to show that the tolerances reject them (TEETH)."""
import math
import zlib
from dataclasses import dataclass

import torch

from mmvae_ref import TINY, U, worst_ratio  # noqa: F401  (U, TINY: re-exported to the tests)
from oracle import elbo

F64 = torch.float64
EPS32 = float(torch.tensor(1e-8, dtype=torch.float32))  # the PoE epsilon as the kernel and the fp32 oracle hold it
MAX_SUBSETS = 32  # MVK_MVAE_MAX_SUBSETS

# one constant per family and output: 4x the value measured by tests/test_elbo_ref_host.py::test_error_constants, rounded up
C_STAGE = {
    "mopoe.z": 6.0, "mopoe.kld": 1.0, "mopoe.mu": 15.0, "mopoe.lv": 9.0, "mopoe.dmu": 21.0, "mopoe.dlv": 15.0,
    "mvtcae.z": 8.0, "mvtcae.jkl": 1.0, "mvtcae.ckl": 2.0, "mvtcae.mu": 12.0, "mvtcae.lv": 10.0, "mvtcae.dmu": 13.0,
    "mvtcae.dlv": 11.0,
    "mvae.z": 3.0, "mvae.kld": 1.0, "mvae.mu": 2.0, "mvae.lv": 3.0, "mvae.dmu": 4.0, "mvae.dlv": 4.0,
    "jmvae.z": 3.0, "jmvae.kld": 2.0, "jmvae.ljm": 2.0, "jmvae.djmu": 10.0, "jmvae.djlv": 11.0, "jmvae.dmu": 5.0,
    "jmvae.dlv": 9.0,
    "gauss.z": 3.0, "gauss.kl": 2.0, "gauss.dmu": 10.0, "gauss.dlv": 11.0,
}
_KEY = dict(mus_out="mu", lvs_out="lv", joint_mu="mu", joint_lv="lv", sub_mu="mu", sub_lv="lv", zm="z", w="z")


def stage_of(fam, key):
    return f"{fam}.{_KEY.get(key, key)}"


def acc(n):
    """Accumulation term of a sum of n addends (a tree or a short sequential run), in units of u sum |addend|."""
    return math.ceil(math.log2(max(n, 1))) + 1


# ---- the case table ------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    fam: str               # mopoe | mvtcae | mvae | jmvae | gauss
    M: int
    K: int                 # samples (MVAE draws one per subset: K is unused there)
    B: int
    L: int
    regime: str = "benign"  # benign | wide | eps | agree | dominated (see make_experts)
    mask: str = "none"     # none | random (0.3 missing, modality 0 present) | one (row b keeps modality b % M only) | tail (the only
    #                        missing rows are in the last, partial workgroup of four rows) | empty (MVAE: rows where every modality
    #                        but the first is missing, so that the unimodal subsets of the others have nothing present)
    graded: bool = False   # upstream gradient rows scaled by 10^U(-3, 3)
    sub: str = ""          # MoPoE: power | routed (power set, weights given, sel = b mod S) | chosen (M = 8 list);
    #                        MVAE: joint | sub (joint + unimodal) | rand (+ 3 random subsets) | max (32 subsets)
    null: tuple = ()       # optional pointers of the C ABI passed as NULL
    why: str = ""


def _common(fam):
    """The shape edges, input regimes and masks every family gets (B in {1, 3, 4, 5, 9, 260}, L in {1, 5, 63, 64, 65, 130},
    K in {1, 4, 5, 7, 11}, M in {1, 2, 3, 8}); the masked ones only where the entry point takes masks or weights."""
    masked = fam in ("mopoe", "mvtcae", "mvae")
    rows = [
        ("m1-k1-b1-l1", 1, 1, 1, 1, "benign", "none", False, "smallest launch: one wave, one lane, one expert"),
        ("m2-k4-b3-l5-wide", 2, 4, 3, 5, "wide", "none", False, "lv on [-12, 6], |mu| ~ 10; K = 4: tail loop only"),
        ("m3-k7-b5-l63-random", 3, 7, 5, 63, "benign", "random", False,
         "K = 7: one group of five and a tail of two; L one short of a wave trip; B = 5: partial second workgroup"),
        ("m3-k11-b9-l64-eps-graded", 3, 11, 9, 64, "eps", "none", True,
         "lv on [-20, -16]: POE_EPS decides; K = 11: two groups and a tail; L = one full wave trip; graded upstream rows"),
        ("m3-k5-b4-l65-agree", 3, 5, 4, 65, "agree", "none", False,
         "experts agree at |mu| ~ 30: g_mu (mu_m - mu_s) cancels; K = 5: groups only; L one past a trip; B * L = 260"),
        ("m8-k4-b5-l130-dominated-random", 8, 4, 5, 130, "dominated", "random", False,
         "M = MVK_MAX_MODALITIES; one expert at lv = -10, the rest +4: the conditional KL cancels; L = three trips"),
        ("m3-k4-b9-l5-one", 3, 4, 9, 5, "benign", "one", False, "every row keeps exactly one modality"),
        ("m2-k5-b9-l20-tail-graded", 2, 5, 9, 20, "benign", "tail", True, "the only missing row is row 8, alone in the last workgroup"),
        ("m2-k1-b260-l130-wide-graded", 2, 1, 260, 130, "wide", "none", True, "largest shape: 65 workgroups, three trips, K = 1"),
        ("m2-k4-b260-l5-random", 2, 4, 260, 5, "benign", "random", False, "masks across 65 workgroups"),
    ]
    out = []
    for name, M, K, B, L, regime, mask, graded, why in rows:
        if mask != "none" and not masked:
            mask, name = "none", name.replace("-random", "").replace("-one", "").replace("-tail", "")
        if fam == "gauss":
            M, name = 1, "-".join(name.split("-")[1:])
        if fam == "mvae":
            name = "-".join(p for p in name.split("-") if not (p[0] == "k" and p[1:].isdigit()))
        sub = {"mopoe": "chosen" if M == 8 else "power", "mvae": "sub"}.get(fam, "")
        c = Case(f"{fam}-{name}", fam, M, K, B, L, regime, mask, graded, sub, (), why)
        if c.name not in [o.name for o in out]:
            out.append(c)
    return out


CASES = sum((_common(f) for f in ("mopoe", "mvtcae", "mvae", "jmvae", "gauss")), []) + [
    # MoPoE
    Case("mopoe-m2-k1-b3-l5-power", "mopoe", 2, 1, 3, 5, sub="power", why="M = 2 power set, weights NULL, sel by row bounds with B = S"),
    Case("mopoe-m3-k4-b9-l20-routed", "mopoe", 3, 4, 9, 20, sub="routed", why="weights given (uniform); sel walks all 7 subsets"),
    Case("mopoe-m5-k1-b260-l5-routed-graded", "mopoe", 5, 1, 260, 5, graded=True, sub="routed",
         why="M = 5: 31 subsets, rows routed to every one of them through sel"),
    Case("mopoe-m8-k7-b4-l64-chosen-eps", "mopoe", 8, 7, 4, 64, "eps", sub="chosen",
         why="M = 8 caller-chosen list with the full set (prior expert, bits == full) and singletons, POE_EPS regime"),
    Case("mopoe-m3-k11-b5-l5-dominated-random-graded", "mopoe", 3, 11, 5, 5, "dominated", "random", True, "power",
         why="masked weights (0 and 1 / n_avail) with graded rows"),
    Case("mopoe-m3-k7-b5-l20-null-outs", "mopoe", 3, 7, 5, 20, sub="power", null=("mus_out", "joint"),
         why="mus_out / lvs_out and joint_mu / joint_lv NULL"),
    Case("mopoe-m3-k7-b5-l20-null-gkld", "mopoe", 3, 7, 5, 20, "wide", sub="routed", null=("gkld",), why="gkld_rows NULL"),
    Case("mopoe-m3-k5-b9-l63-agree-random-graded", "mopoe", 3, 5, 9, 63, "agree", "random", True, "power",
         why="agreeing experts under masked weights"),
    # MVTCAE
    Case("mvtcae-m2-k7-b5-l20-null-joint", "mvtcae", 2, 7, 5, 20, null=("joint",), why="joint_mu / joint_lv NULL"),
    Case("mvtcae-m3-k7-b5-l20-null-gjoint", "mvtcae", 3, 7, 5, 20, "wide", "random", null=("gjoint",), why="gjoint_rows NULL"),
    Case("mvtcae-m3-k7-b5-l20-null-gcond", "mvtcae", 3, 7, 5, 20, "wide", "random", null=("gcond",), why="gcond_rows NULL"),
    Case("mvtcae-m3-k4-b9-l64-dominated-one-graded", "mvtcae", 3, 4, 9, 64, "dominated", "one", True,
         why="a single present modality: the conditional KL is ~ 0 while its terms are O(|lv|)"),
    Case("mvtcae-m8-k1-b3-l65-eps", "mvtcae", 8, 1, 3, 65, "eps", why="M = 8 without masks, POE_EPS regime"),
    Case("mvtcae-m3-k11-b4-l5-agree-graded", "mvtcae", 3, 11, 4, 5, "agree", "none", True, why="agreeing experts, graded rows, K = 11"),
    # MVAE
    Case("mvae-m3-b5-l20-joint", "mvae", 3, 1, 5, 20, sub="joint", why="mvae_subsets without subsampling: the joint subset alone"),
    Case("mvae-m3-b9-l64-rand-eps-graded", "mvae", 3, 1, 9, 64, "eps", "random", True, "rand",
         why="joint + unimodal + 3 random subsets: a modality in up to five subsets (five slots)"),
    Case("mvae-m5-b3-l5-max", "mvae", 5, 1, 3, 5, "wide", sub="max", why="S = MVK_MVAE_MAX_SUBSETS = 32"),
    Case("mvae-m3-b9-l20-empty-graded", "mvae", 3, 1, 9, 20, "benign", "empty", True, "sub",
         why="subsets none of whose members is present for some rows: posterior = prior, KL = 0, z = eps"),
    Case("mvae-m3-b5-l20-null-sub", "mvae", 3, 1, 5, 20, sub="sub", null=("sub",), why="sub_mu / sub_lv NULL"),
    Case("mvae-m3-b5-l20-null-gkld", "mvae", 3, 1, 5, 20, "wide", "random", sub="sub", null=("gkld",), why="gkld_rows NULL"),
    Case("mvae-m3-b5-l65-null-dzm1", "mvae", 3, 1, 5, 65, "dominated", "random", sub="rand", null=("dzm1",),
         why="dzm of modality 1 NULL: its decoder returned no gradient"),
    Case("mvae-m8-b4-l130-agree-one", "mvae", 8, 1, 4, 130, "agree", "one", sub="sub", why="M = 8, S = 9, one modality per row"),
    # JMVAE
    Case("jmvae-m2-k7-b5-l20-null-dz", "jmvae", 2, 7, 5, 20, null=("dz",), why="dz NULL"),
    Case("jmvae-m2-k7-b5-l20-null-gkld", "jmvae", 2, 7, 5, 20, "wide", null=("gkld",), why="gkld_rows NULL"),
    Case("jmvae-m2-k7-b5-l20-null-gljm", "jmvae", 2, 7, 5, 20, "wide", null=("gljm",), why="gljm_rows NULL"),
    Case("jmvae-m3-k1-b4-l64", "jmvae", 3, 1, 4, 64, why="B * L = 256: exactly one block of the flat backward"),
    # style-latent Gaussian
    Case("gauss-k7-b5-l20-null-dw", "gauss", 1, 7, 5, 20, null=("dw",), why="dw NULL"),
    Case("gauss-k7-b5-l20-null-gkl-graded", "gauss", 1, 7, 5, 20, "wide", graded=True, null=("gkl",), why="gkl NULL"),
    Case("gauss-k1-b4-l64", "gauss", 1, 1, 4, 64, why="B * L = 256: exactly one block of the flat backward"),
]
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)

TEETH = [  # (mutation of the REFERENCE, the stages where it must show, the cases named for it)
    ("no_prior_full", ("mopoe.mu", "mopoe.lv", "mopoe.kld"), ["mopoe-m3-k5-b4-l65-agree", "mopoe-m2-k1-b3-l5-power"]),
    ("prior_everywhere", ("mopoe.mu", "mopoe.lv", "mopoe.kld"), ["mopoe-m3-k7-b5-l63-random", "mopoe-m8-k7-b4-l64-chosen-eps"]),
    ("no_eps", ("mopoe.lv", "mvtcae.lv"), ["mopoe-m3-k11-b9-l64-eps-graded", "mvtcae-m8-k1-b3-l65-eps"]),
    ("uniform_w", ("mopoe.kld", "mopoe.dmu"), ["mopoe-m3-k7-b5-l63-random", "mopoe-m3-k11-b5-l5-dominated-random-graded"]),
    ("sel_off", ("mopoe.z", "mopoe.mu"), ["mopoe-m3-k4-b9-l20-routed", "mopoe-m5-k1-b260-l5-routed-graded"]),
    ("lv0_missing", ("mvtcae.z", "mvtcae.mu", "mvtcae.lv"), ["mvtcae-m3-k7-b5-l63-random", "mvtcae-m3-k4-b9-l5-one"]),
    ("mvae_no_prior", ("mvae.mu", "mvae.lv", "mvae.kld"), ["mvae-m3-b5-l20-joint", "mvae-m2-b260-l130-wide-graded"]),
    ("sd_no_half", ("mopoe.dlv", "mvtcae.dlv", "mvae.dlv", "jmvae.djlv", "gauss.dlv"),
     ["mopoe-m3-k7-b5-l63-random", "mvtcae-m2-k4-b3-l5-wide", "mvae-m3-b5-l63-random", "jmvae-m3-k7-b5-l63", "gauss-k7-b5-l63"]),
    ("drop_tail", ("mopoe.dmu", "mvtcae.dmu", "jmvae.djmu", "gauss.dmu"),
     ["mopoe-m3-k7-b5-l63-random", "mopoe-m3-k11-b9-l64-eps-graded", "mvtcae-m3-k7-b5-l63-random", "jmvae-m3-k7-b5-l63",
      "gauss-k7-b5-l63"]),
]


# ---- seeded inputs ---------------------------------------------------------------------------------------------------------------------
def make_experts(case, gen, n):
    """n experts (mu, lv) [B,L] fp32 of one regime:
    benign     mu ~ N(0,1), lv ~ 0.5 N(0,1)
    wide       lv uniform on [-12, 6], mu ~ 10 N(0,1)
    eps        benign, but the first and the last expert have lv uniform on [-20, -16]: exp(lv) ~ POE_EPS
    agree      every mu within 1e-3 of a common value of magnitude 24 .. 36, lv uniform on [-4, 0]
    dominated  in row b expert b mod n has lv = -10, the others +4; mu ~ N(0,1)"""
    B, L = case.B, case.L
    r = case.regime
    rn = lambda *s: torch.randn(*s, generator=gen)
    ru = lambda *s: torch.rand(*s, generator=gen)
    mus, lvs = [], []
    common = (ru(B, L) > 0.5).float().mul(2).sub(1) * 30.0 * (0.8 + 0.4 * ru(B, L))
    for i in range(n):
        if r == "wide":
            mu, lv = 10.0 * rn(B, L), ru(B, L) * 18.0 - 12.0
        elif r == "agree":
            mu, lv = common + 1e-3 * (2 * ru(B, L) - 1), -4.0 * ru(B, L)
        elif r == "dominated":
            mu = rn(B, L)
            lv = torch.where((torch.arange(B) % n == i).unsqueeze(1), torch.full((B, L), -10.0), torch.full((B, L), 4.0))
        else:
            mu, lv = rn(B, L), 0.5 * rn(B, L)
            if r == "eps" and i in (0, n - 1):
                lv = -20.0 + 4.0 * ru(B, L)
        mus.append(mu.float().contiguous())
        lvs.append(lv.float().contiguous())
    return mus, lvs


def make_masks(case, gen):
    M, B = case.M, case.B
    if case.mask == "none":
        return None
    if case.mask == "one":
        return [torch.arange(B) % M == m for m in range(M)]
    if case.mask == "tail":
        mk = [torch.ones(B, dtype=torch.bool) for _ in range(M)]
        for m in range(1, M):
            mk[m][4 * ((B - 1) // 4):] = False
        return mk
    mk = [torch.rand(B, generator=gen) > 0.3 for _ in range(M)]
    mk[0][:] = True
    if case.mask == "empty":
        for m in range(1, M):
            mk[m][torch.arange(B) % 3 == 1] = False
    return mk


def bits_of(case, gen):
    """The subset list of a MoPoE / MVAE case as bit masks (bit m = modality m; names m0 .. m7 sort in index order)."""
    M = case.M
    names = [f"m{i}" for i in range(M)]
    pos = {n: i for i, n in enumerate(names)}
    if case.fam == "mopoe":
        if case.sub == "chosen":  # M = 8: the full set first and last but one, singletons, pairs, halves
            assert M == 8
            return [255, 1, 128, 6, 0x0F, 0xAA, 255, 64]
        return [sum(1 << pos[m] for m in mods) for _, mods in elbo.mopoe_subsets(names)]
    rand = []
    if case.sub in ("rand", "max"):
        n = 3 if case.sub == "rand" else MAX_SUBSETS - 1 - M
        for _ in range(n):
            size = int(torch.randint(1, M + 1, (1,), generator=gen))
            rand.append([names[int(i)] for i in torch.randperm(M, generator=gen)[:size]])
    subs = elbo.mvae_subsets(names, use_subsampling=case.sub != "joint", random_subsets=rand)
    return [sum(1 << pos[m] for m in s) for s in subs]


def make_inputs(case):
    """Seeded fp32 inputs of one case (CPU tensors; None where the case passes NULL)."""
    gen = torch.Generator().manual_seed(zlib.crc32(case.name.encode()))
    fam, M, K, B, L = case.fam, case.M, case.K, case.B, case.L
    I = dict(masks=None)
    if fam == "jmvae":
        mus, lvs = make_experts(case, gen, M + 1)
        I.update(jmu=mus[0], jlv=lvs[0], mus=mus[1:], lvs=lvs[1:])
    else:
        mus, lvs = make_experts(case, gen, M)
        I.update(mus=mus, lvs=lvs)
    if fam in ("mopoe", "mvtcae", "mvae"):
        I["masks"] = make_masks(case, gen)
    g = 10.0 ** (6 * torch.rand(B, generator=gen) - 3) if case.graded else torch.ones(B)
    rn = lambda *s: torch.randn(*s, generator=gen)
    if fam == "mvae":
        bits = bits_of(case, gen)
        S = len(bits)
        I.update(bits=bits, eps=rn(S, B, L).float())
        I["dzm"] = [(rn(sum((b >> m) & 1 for b in bits), B, L) * g[None, :, None]).float() for m in range(M)]
        for m in range(M):
            if f"dzm{m}" in case.null or I["dzm"][m].shape[0] == 0:
                I["dzm"][m] = None
        I["gk"] = None if "gkld" in case.null else (rn(S, B) * g).float()
        return I
    I["eps"] = rn(K, B, L).float()
    dz = (rn(K, B, L) * g[None, :, None]).float()
    if fam == "mopoe":
        bits = bits_of(case, gen)
        S = len(bits)
        given = case.mask != "none" or case.sub == "routed"
        if given:
            mk = I["masks"] or [torch.ones(B, dtype=torch.bool)] * M
            av = torch.stack([torch.stack([mk[m] for m in range(M) if (bt >> m) & 1]).all(0) for bt in bits])  # [S,B]
            a = av.float()
            I["weights"] = (a / a.sum(0)).contiguous()
            sel = torch.zeros(B, dtype=torch.int32)
            for b in range(B):
                ok = [s for s in range(S) if av[s, b]]
                sel[b] = ok[(b * 7 + 3) % len(ok)] if case.mask != "none" else b % S
        else:
            I["weights"] = None
            bnd = elbo.mopoe_row_bounds(B, S)
            sel = torch.zeros(B, dtype=torch.int32)
            for k in range(S):
                sel[bnd[k]:bnd[k + 1]] = k
        I.update(bits=bits, sel=sel, dz=dz, gk=None if "gkld" in case.null else (rn(B) * g).float())
    elif fam == "mvtcae":
        I.update(dz=dz, gj=None if "gjoint" in case.null else (rn(B) * g).float(),
                 gc=None if "gcond" in case.null else (rn(M, B) * g).float())
    elif fam == "jmvae":
        I.update(dz=None if "dz" in case.null else dz, gk=None if "gkld" in case.null else (rn(B) * g).float(),
                 gl=None if "gljm" in case.null else (rn(B) * g).float())
    else:
        I.update(dz=None if "dw" in case.null else dz, gk=None if "gkl" in case.null else (rn(B) * g).float())
    return I


# ---- the forward reference, one function per family ----------------------------------------------------------------------------------------
def _poe(mu, lv, prior, eps):
    """oracle.elbo.poe over dim 0 (+ the N(0,I) expert: mu 0, var exp(0) + eps)."""
    T = 1.0 / (torch.exp(lv) + eps)
    D, N = T.sum(0), (mu * T).sum(0)
    if prior:
        D = D + 1.0 / (1.0 + eps)
    return N / D, torch.log(1.0 / D)


def _kl(mu, lv):
    return -0.5 * (1 - lv.exp() - mu.pow(2) + lv).sum(-1)


def _sample(mu, lv, eps, mut):
    sd = torch.exp(0.5 * lv)
    if "sd_no_half" in mut:  # d sd / d lv = sd instead of sd / 2 (values unchanged)
        sd = sd.detach() + 2.0 * (sd - sd.detach())
    return mu + sd * eps


def _missing(lv, mask, fill=math.inf):
    return lv if mask is None else torch.where(mask.unsqueeze(-1), lv, torch.full_like(lv, fill))


def mopoe_fwd(P, I, mut=()):
    mus, lvs, bits, M = P["mus"], P["lvs"], I["bits"], len(P["mus"])
    S, B = len(bits), mus[0].shape[0]
    dt = mus[0].dtype
    full = (1 << M) - 1
    eps = 0.0 if "no_eps" in mut else EPS32
    smu, slv = [], []
    for bt in bits:
        idx = [m for m in range(M) if (bt >> m) & 1]
        prior = (bt == full and "no_prior_full" not in mut) or "prior_everywhere" in mut
        a, b = _poe(torch.stack([mus[m] for m in idx]), torch.stack([lvs[m] for m in idx]), prior, eps)
        smu.append(a)
        slv.append(b)
    smu, slv = torch.stack(smu), torch.stack(slv)
    if I["weights"] is None or "uniform_w" in mut:
        w = torch.full((S, B), 1.0 / S, dtype=dt)
    else:
        w = I["weights"].to(dt)
    sel = I["sel"].long()
    if "sel_off" in mut:
        sel = (sel + 1) % S
    jm, jl = smu[sel, torch.arange(B)], slv[sel, torch.arange(B)]
    return dict(z=_sample(jm, jl, I["eps"].to(dt), mut), kld=(w * _kl(smu, slv)).sum(0), mus_out=smu, lvs_out=slv,
                joint_mu=jm, joint_lv=jl)


def mvtcae_fwd(P, I, mut=()):
    mus, lvs, mk, M = P["mus"], P["lvs"], I["masks"], len(P["mus"])
    dt = mus[0].dtype
    le = [_missing(lvs[m], None if mk is None else mk[m]) for m in range(M)]
    lp = [_missing(lvs[m], None if mk is None else mk[m], 0.0) for m in range(M)] if "lv0_missing" in mut else le
    jmu, jlv = _poe(torch.stack(mus), torch.stack(lp), False, 0.0 if "no_eps" in mut else EPS32)
    ckl = []
    for m in range(M):
        k = -0.5 * (1 - jlv.exp() / le[m].exp() - (jmu - mus[m]).pow(2) / le[m].exp() + jlv - le[m]).sum(-1)
        ckl.append(k if mk is None else torch.where(mk[m], k, torch.zeros_like(k)))
    return dict(z=_sample(jmu, jlv, I["eps"].to(dt), mut), jkl=_kl(jmu, jlv), ckl=torch.stack(ckl), joint_mu=jmu, joint_lv=jlv)


def mvae_fwd(P, I, mut=()):
    mus, lvs, mk, bits, M = P["mus"], P["lvs"], I["masks"], I["bits"], len(P["mus"])
    dt = mus[0].dtype
    zs, kld, smu, slv = [], [], [], []
    for s, bt in enumerate(bits):
        idx = [m for m in range(M) if (bt >> m) & 1]
        ln_inv = [-_missing(lvs[m], None if mk is None else mk[m]) for m in idx]
        ms = [mus[m] for m in idx]
        if "mvae_no_prior" not in mut:
            ln_inv.append(torch.zeros_like(mus[0]))
            ms.append(torch.zeros_like(mus[0]))
        ln_inv, ms = torch.stack(ln_inv), torch.stack(ms)
        lv = -torch.logsumexp(ln_inv, dim=0)
        mu = (torch.exp(ln_inv) * ms).sum(0) * torch.exp(lv)
        zs.append(_sample(mu, lv, I["eps"][s].to(dt), mut))
        kld.append(-0.5 * (1 + lv - mu.pow(2) - lv.exp()).sum(-1))
        smu.append(mu)
        slv.append(lv)
    zm = []
    for m in range(M):
        mine = [zs[s] for s, bt in enumerate(bits) if (bt >> m) & 1]
        zm.append(torch.stack(mine) if mine else None)
    return dict(zm=zm, kld=torch.stack(kld), sub_mu=torch.stack(smu), sub_lv=torch.stack(slv))


def jmvae_fwd(P, I, mut=()):
    mu, lv = P["jmu"], P["jlv"]
    ljm = 0
    for um, ul in zip(P["mus"], P["lvs"]):
        ljm = ljm + 0.5 * (ul - lv + (torch.exp(lv) + (mu - um) ** 2) / torch.exp(ul) - 1)
    return dict(z=_sample(mu, lv, I["eps"].to(mu.dtype), mut), kld=-0.5 * (1 + lv - mu.pow(2) - lv.exp()).sum(-1),
                ljm=ljm.sum(-1))


def gauss_fwd(P, I, mut=()):
    mu, lv = P["mus"][0], P["lvs"][0]
    return dict(w=_sample(mu, lv, I["eps"].to(mu.dtype), mut), kl=_kl(mu, lv))


FWD = dict(mopoe=mopoe_fwd, mvtcae=mvtcae_fwd, mvae=mvae_fwd, jmvae=jmvae_fwd, gauss=gauss_fwd)


# ---- backward: autograd of sum(output * upstream gradient) ---------------------------------------------------------------------------------
def leaves(case, I, dtype):
    P = dict(mus=[t.to(dtype).clone().requires_grad_() for t in I["mus"]],
             lvs=[t.to(dtype).clone().requires_grad_() for t in I["lvs"]])
    if case.fam == "jmvae":
        P.update(jmu=I["jmu"].to(dtype).clone().requires_grad_(), jlv=I["jlv"].to(dtype).clone().requires_grad_())
    return P


def seeded_total(case, I, out, mut=()):
    """sum over the outputs of output * its upstream gradient (NULL = 0): what the backward entry point differentiates."""
    fam = case.fam
    dt = (out["zm"][0] if fam == "mvae" else out["w" if fam == "gauss" else "z"]).dtype

    def dot(o, g):
        if g is None:
            return 0.0
        g = g.to(dt)
        if "drop_tail" in mut and g.dim() == 3 and g.shape[0] > 1:  # the last sample is left out of the sum over K
            g = torch.cat([g[:-1], torch.zeros_like(g[-1:])])
        return (o * g).sum()

    if fam == "mopoe":
        return dot(out["z"], I["dz"]) + dot(out["kld"], I["gk"])
    if fam == "mvtcae":
        return dot(out["z"], I["dz"]) + dot(out["jkl"], I["gj"]) + dot(out["ckl"], I["gc"])
    if fam == "mvae":
        t = dot(out["kld"], I["gk"])
        for m, z in enumerate(out["zm"]):
            if z is not None and I["dzm"][m] is not None:
                t = t + (z * I["dzm"][m].to(dt)).sum()
        return t
    if fam == "jmvae":
        return dot(out["z"], I["dz"]) + dot(out["kld"], I["gk"]) + dot(out["ljm"], I["gl"])
    return dot(out["w"], I["dz"]) + dot(out["kl"], I["gk"])


def with_grads(case, P, out, total):
    """-> every output detached, plus dmu / dlv (and djmu / djlv) by autograd of `total`."""
    flat = P["mus"] + P["lvs"] + ([P["jmu"], P["jlv"]] if case.fam == "jmvae" else [])
    if torch.is_tensor(total) and total.requires_grad:
        gs = torch.autograd.grad(total, flat, allow_unused=True)
    else:
        gs = [None] * len(flat)
    gs = [torch.zeros_like(p) if g is None else g for g, p in zip(gs, flat)]
    M = len(P["mus"])
    res = {k: ([None if t is None else t.detach() for t in v] if isinstance(v, list) else v.detach()) for k, v in out.items()}
    res.update(dmu=gs[:M], dlv=gs[M:2 * M])
    if case.fam == "jmvae":
        res.update(djmu=gs[2 * M], djlv=gs[2 * M + 1])
    return res


def reference(case, I, mut=(), dtype=F64):
    """Every array the forward and the backward entry point of the case's family write, in float64."""
    P = leaves(case, I, dtype)
    out = FWD[case.fam](P, I, mut)
    return with_grads(case, P, out, seeded_total(case, I, out, mut))


# ---- oracle.elbo evaluated in a given precision (float64: pins the reference; float32: what the constants are measured on) -----------------
def _with_poe_eps(fn):
    """oracle.elbo.poe adds the Python float 1e-8; in float32 that is EPS32.  The float64 evaluation has to add the same value."""
    old = elbo.poe
    elbo.poe = lambda mus, logvars, eps=EPS32: old(mus, logvars, eps)
    try:
        return fn()
    finally:
        elbo.poe = old


def oracle_eval(case, I, dtype):
    """The same arrays as `reference`, computed by oracle.elbo's own functions in `dtype`, gradients by autograd."""
    return _with_poe_eps(lambda: _oracle_eval(case, I, dtype))


def _oracle_eval(case, I, dtype):
    fam, M, B, L = case.fam, case.M, case.B, case.L
    P = leaves(case, I, dtype)
    names = [f"m{i}" for i in range(M)]
    eps = I["eps"].to(dtype)
    mk = I["masks"]
    zero = {n: (lambda z: z * 0) for n in names}
    if fam == "mopoe":
        enc = {n: (P["mus"][i], P["lvs"][i]) for i, n in enumerate(names)}
        subs = [("_".join(mods), mods) for mods in ([names[m] for m in range(M) if (bt >> m) & 1] for bt in I["bits"])]
        S = len(subs)
        if I["weights"] is None:
            inf = elbo.mopoe_inference(enc, names, subsets=subs)
            w = inf["weights"]
        else:
            masks = {n: (torch.ones(B, dtype=torch.bool) if mk is None else mk[i]) for i, n in enumerate(names)}
            inf = elbo.mopoe_inference(enc, names, masks=masks, choice=torch.eye(S)[I["sel"].long()], subsets=subs)
            assert torch.allclose(inf["weights"].float(), I["weights"])
            w = I["weights"].to(dtype)  # the array the entry point is given (fp32 values)
        _, klds = elbo.mopoe_joint_divergence(inf["mus"], inf["logvars"], w)
        out = dict(z=elbo.rsample(inf["joint_mu"], inf["joint_logvar"], eps), kld=(w * klds).sum(0), mus_out=inf["mus"],
                   lvs_out=inf["logvars"], joint_mu=inf["joint_mu"], joint_lv=inf["joint_logvar"])
    elif fam == "mvtcae":
        enc = {n: (P["mus"][i], P["lvs"][i]) for i, n in enumerate(names)}
        data = {n: torch.zeros(B, L, dtype=dtype) for n in names}
        masks = None if mk is None else {n: mk[i] for i, n in enumerate(names)}
        o = elbo.mvtcae_forward(enc, data, zero, eps, names=names, masks=masks)
        jkl, ckl = [], [[] for _ in names]
        for b in range(B):  # the oracle reports batch sums: one call per row gives the rows
            r = slice(b, b + 1)
            ob = elbo.mvtcae_forward({n: (enc[n][0][r], enc[n][1][r]) for n in names}, {n: data[n][r] for n in names}, zero,
                                     eps[:, r], names=names, masks=None if masks is None else {n: masks[n][r] for n in names})
            jkl.append(ob["metrics"]["joint_divergence"])
            for i, n in enumerate(names):
                ckl[i].append(ob["metrics"]["kld_" + n])
        out = dict(z=o["z"], jkl=torch.stack(jkl), ckl=torch.stack([torch.stack(c) for c in ckl]), joint_mu=o["joint_mu"],
                   joint_lv=o["joint_logvar"])
    elif fam == "mvae":
        zs, kld, smu, slv = [], [], [], []
        for s, bt in enumerate(I["bits"]):
            idx = [m for m in range(M) if (bt >> m) & 1]
            ls = [_missing(P["lvs"][m], None if mk is None else mk[m]) for m in idx] + [torch.zeros(B, L, dtype=dtype)]
            ms = [P["mus"][m] for m in idx] + [torch.zeros(B, L, dtype=dtype)]
            mu, lv = elbo.stable_poe(torch.stack(ms), torch.stack(ls))
            zs.append(elbo.rsample(mu, lv, eps[s]))
            kld.append(-0.5 * torch.sum(1 + lv - mu.pow(2) - lv.exp(), dim=-1))  # mvae_forward's KLD, per row
            smu.append(mu)
            slv.append(lv)
        zm = []
        for m in range(M):
            mine = [zs[s] for s, bt in enumerate(I["bits"]) if (bt >> m) & 1]
            zm.append(torch.stack(mine) if mine else None)
        out = dict(zm=zm, kld=torch.stack(kld), sub_mu=torch.stack(smu), sub_lv=torch.stack(slv))
    elif fam == "jmvae":
        enc = {n: (P["mus"][i], P["lvs"][i]) for i, n in enumerate(names)}
        data = {n: torch.zeros(B, L, dtype=dtype) for n in names}
        # Laplace(recon = 0, scale 1/2) at x = 0 has log-probability exactly 0: loss_sum = beta * kld + alpha * ljm
        kw = dict(names=names, warmup=1, epoch=1, dists={n: "laplace" for n in names}, dist_scales={n: 0.5 for n in names})
        z = elbo.jmvae_forward((P["jmu"], P["jlv"]), enc, data, zero, eps, **kw)["z"]
        kld, ljm = [], []
        for b in range(B):
            r = slice(b, b + 1)
            args = ((P["jmu"][r], P["jlv"][r]), {n: (enc[n][0][r], enc[n][1][r]) for n in names}, {n: data[n][r] for n in names},
                    zero, eps[:, r])
            kld.append(elbo.jmvae_forward(*args, alpha=0.0, beta=1.0, **kw)["loss_sum"])
            ljm.append(elbo.jmvae_forward(*args, alpha=1.0, beta=0.0, **kw)["loss_sum"])
        out = dict(z=z, kld=torch.stack(kld), ljm=torch.stack(ljm))
    else:
        mu, lv = P["mus"][0], P["lvs"][0]
        _, klds = elbo.mopoe_joint_divergence(mu[None], lv[None], torch.ones(1, B, dtype=dtype))  # the style KL's formula
        out = dict(w=elbo.rsample(mu, lv, eps), kl=klds[0])
    return with_grads(case, P, out, seeded_total(case, I, out))


# ---- the error model -----------------------------------------------------------------------------------------------------------------
def _poe_stats(mu, lv, prior):
    """float64 product of experts over dim 0 with EM, EL: the error of mu / lv in units of u."""
    ev = torch.exp(lv)
    T = 1.0 / (ev + EPS32)
    D = T.sum(0) + (1.0 / (1.0 + EPS32) if prior else 0.0)
    m = (mu * T).sum(0) / D
    l = -torch.log(D)
    return dict(T=T, ev=ev, D=D, mu=m, lv=l, EM=(mu.abs() * T).sum(0) / D + m.abs(), EL=1.0 + l.abs())


def _kl_row_base(mu, lv, EM, EL):
    """KL(mu, lv) rows: the terms 1, e^lv, mu^2, lv with the errors of mu and lv, summed over L."""
    e = 0.5 * (1 + lv.exp() * (1 + EL) + mu * mu + 2 * mu.abs() * EM + lv.abs() + EL)
    kl = (-0.5 * (1 - lv.exp() - mu * mu + lv)).abs()
    return U * (e.sum(-1) + acc(mu.shape[-1]) * kl.sum(-1)), kl.sum(-1)


def _z_base(mu, lv, EM, EL, eps):
    se = (torch.exp(0.5 * lv) * eps).abs()
    return U * (EM + se * (0.5 * EL + 2) + (mu + torch.exp(0.5 * lv) * eps).abs())


def _abs_k(dz, eps=None):
    """sum_k |dz_k| or sum_k |dz_k eps_k| (0 for a NULL dz)."""
    if dz is None:
        return 0.0
    return (dz.abs() if eps is None else (dz * eps).abs()).sum(0)


def _d(ts):
    return [None if t is None else t.to(F64) for t in ts]


def _a(t):
    return 0.0 if t is None else t.to(F64).abs()


def mopoe_base(case, I):
    mus, lvs, eps, dz = _d(I["mus"]), _d(I["lvs"]), I["eps"].to(F64), I["dz"].to(F64)
    bits, M = I["bits"], case.M
    S, B, L = len(bits), case.B, case.L
    st = []
    for bt in bits:
        idx = [m for m in range(M) if (bt >> m) & 1]
        s = _poe_stats(torch.stack([mus[m] for m in idx]), torch.stack([lvs[m] for m in idx]), bt == (1 << M) - 1)
        s["idx"] = idx
        st.append(s)
    w = torch.full((S, B), 1.0 / S, dtype=F64) if I["weights"] is None else I["weights"].to(F64)
    sel = I["sel"].long()
    rows = torch.arange(B)
    pick = lambda k: torch.stack([s[k] for s in st])[sel, rows]
    b_row = torch.stack([_kl_row_base(s["mu"], s["lv"], s["EM"], s["EL"])[0] for s in st])
    kl = torch.stack([_kl_row_base(s["mu"], s["lv"], s["EM"], s["EL"])[1] for s in st])
    out = dict(mus_out=U * torch.stack([s["EM"] for s in st]), lvs_out=U * torch.stack([s["EL"] for s in st]),
               kld=(w * b_row).sum(0) + U * (acc(S) + 1) * (w * kl).sum(0))
    out.update(joint_mu=U * pick("EM"), joint_lv=U * pick("EL"), z=_z_base(pick("mu"), pick("lv"), pick("EM"), pick("EL"), eps))
    dmu = [torch.zeros(B, L, dtype=F64) for _ in range(M)]
    dlv = [torch.zeros(B, L, dtype=F64) for _ in range(M)]
    for si, s in enumerate(st):
        c = (_a(I["gk"]) * w[si]).unsqueeze(-1) if I["gk"] is not None else torch.zeros(B, 1, dtype=F64)
        on = (sel == si).to(F64).unsqueeze(-1)
        A_mu = c * s["EM"] + on * _abs_k(dz)
        A_lv = c * 0.5 * (s["lv"].exp() * (1 + s["EL"]) + 1) + on * 0.5 * torch.exp(0.5 * s["lv"]) * _abs_k(dz, eps) * (2 + 0.5 * s["EL"])
        for j, m in enumerate(s["idx"]):
            share = s["T"][j] / s["D"]
            dmu[m] += A_mu * share
            dlv[m] += share * (s["T"][j] * s["ev"][j]) * (A_mu * (mus[m].abs() + s["EM"]) + A_lv)
    out.update(dmu=[U * t + TINY for t in dmu], dlv=[U * t + TINY for t in dlv])
    return out


def mvtcae_base(case, I):
    mus, lvs, eps, dz = _d(I["mus"]), _d(I["lvs"]), I["eps"].to(F64), I["dz"].to(F64)
    M, B, L = case.M, case.B, case.L
    av = [torch.ones(B, dtype=torch.bool) if I["masks"] is None else I["masks"][m] for m in range(M)]
    s = _poe_stats(torch.stack(mus), torch.stack([_missing(lvs[m], av[m]) for m in range(M)]), False)
    jmu, jlv, EM, EL = s["mu"], s["lv"], s["EM"], s["EL"]
    out = dict(joint_mu=U * EM, joint_lv=U * EL, z=_z_base(jmu, jlv, EM, EL, eps), jkl=_kl_row_base(jmu, jlv, EM, EL)[0])
    jc = _a(I["gj"]).unsqueeze(-1) if I["gj"] is not None else torch.zeros(B, 1, dtype=F64)
    A_mu = _abs_k(dz) + jc * EM
    A_lv = 0.5 * torch.exp(0.5 * jlv) * _abs_k(dz, eps) * (2 + 0.5 * EL) + jc * 0.5 * (jlv.exp() * (1 + EL) + 1)
    ckl, own_mu, own_lv = [], [], []
    for m in range(M):
        a = av[m].to(F64).unsqueeze(-1)
        iv, dm = torch.exp(-lvs[m]), (jmu - mus[m]).abs()
        DM = dm + EM  # the error of jmu - mu_m: jmu's own
        r, q = torch.exp(jlv - lvs[m]), dm * dm * iv
        e = 0.5 * (1 + r * (3 + EL) + q + 2 * dm * DM * iv + jlv.abs() + EL + lvs[m].abs())
        k = (-0.5 * (1 - r - q + jlv - lvs[m])).abs()
        ckl.append(U * (e.sum(-1) + acc(L) * k.sum(-1)) * av[m].to(F64))
        cc = (_a(I["gc"][m]).unsqueeze(-1) if I["gc"] is not None else torch.zeros(B, 1, dtype=F64)) * a
        A_mu = A_mu + cc * iv * DM
        A_lv = A_lv + cc * 0.5 * (r * (3 + EL) + 1)
        own_mu.append(cc * iv * DM)
        own_lv.append(cc * 0.5 * (r * (3 + EL) + q + 2 * dm * DM * iv + 1))
    out["ckl"] = torch.stack(ckl)
    dmu, dlv = [], []
    for m in range(M):
        a = av[m].to(F64).unsqueeze(-1)
        share = s["T"][m] / s["D"]
        dmu.append(U * a * (A_mu * share + own_mu[m]))
        dlv.append(U * a * (share * (s["T"][m] * s["ev"][m]).nan_to_num(0.0) * (A_mu * (mus[m].abs() + EM) + A_lv) + own_lv[m]))
    out.update(dmu=dmu, dlv=dlv)  # base 0 on a missing modality's rows: the gradient there is exactly 0
    return out


def mvae_base(case, I):
    mus, lvs, eps = _d(I["mus"]), _d(I["lvs"]), I["eps"].to(F64)
    bits, M, B, L = I["bits"], case.M, case.B, case.L
    mk = I["masks"]
    dmu = [torch.zeros(B, L, dtype=F64) for _ in range(M)]
    dlv = [torch.zeros(B, L, dtype=F64) for _ in range(M)]
    b_z, b_kld, b_mu, b_lv = [], [], [], []
    slot = [0] * M
    for s, bt in enumerate(bits):
        idx = [m for m in range(M) if (bt >> m) & 1]
        A = torch.stack([-_missing(lvs[m], None if mk is None else mk[m]) for m in idx] + [torch.zeros(B, L, dtype=F64)])
        ms = torch.stack([mus[m] for m in idx] + [torch.zeros(B, L, dtype=F64)])
        lse = torch.logsumexp(A, dim=0)
        wgt = torch.exp(A - lse)  # the precision weights: softmax of -lv over the present experts and the prior
        lnv, mu = -lse, (wgt * ms).sum(0)
        EL = 3 + A.amax(0).abs() + lnv.abs()  # logsumexp: the maximum, log of the sum, the sum of shifted exponentials
        EM = (wgt * ms.abs()).sum(0) * (3 + EL) + mu.abs()
        e = 0.5 * (1 + lnv.abs() + EL + mu * mu + 2 * mu.abs() * EM + lnv.exp() * (1 + EL))
        kl = (-0.5 * (1 + lnv - mu * mu - lnv.exp())).abs()
        b_kld.append(U * (e.sum(-1) + acc(L) * kl.sum(-1)))
        b_mu.append(U * EM)
        b_lv.append(U * EL)
        b_z.append(_z_base(mu, lnv, EM, EL, eps[s]))
        dza, gk = 0.0, (_a(I["gk"][s]).unsqueeze(-1) if I["gk"] is not None else torch.zeros(B, 1, dtype=F64))
        for m in idx:
            if I["dzm"][m] is not None:
                dza = dza + I["dzm"][m][slot[m]].to(F64).abs()
            slot[m] += 1
        A_mu = dza + gk * EM
        A_lv = dza * 0.5 * (torch.exp(0.5 * lnv) * eps[s]).abs() * (2 + 0.5 * EL) + 0.5 * gk * (1 + lnv.exp() * (1 + EL))
        for j, m in enumerate(idx):
            dmu[m] += wgt[j] * (1 + EL) * A_mu
            dlv[m] += wgt[j] * (1 + EL) * (A_lv + A_mu * (mus[m].abs() + EM))
    zm = []
    for m in range(M):
        mine = [b_z[s] for s, bt in enumerate(bits) if (bt >> m) & 1]
        zm.append(torch.stack(mine) if mine else None)
    return dict(zm=zm, kld=torch.stack(b_kld), sub_mu=torch.stack(b_mu), sub_lv=torch.stack(b_lv),
                dmu=[U * t for t in dmu], dlv=[U * t for t in dlv])  # weight 0 (a missing modality's rows): exactly 0


def jmvae_base(case, I):
    mu, lv, eps = I["jmu"].to(F64), I["jlv"].to(F64), I["eps"].to(F64)
    mus, lvs = _d(I["mus"]), _d(I["lvs"])
    L = case.L
    dz = None if I["dz"] is None else I["dz"].to(F64)
    ev, sd = lv.exp(), torch.exp(0.5 * lv)
    gk, gl = (_a(I[k]).unsqueeze(-1) if I[k] is not None else 0.0 for k in ("gk", "gl"))
    out = dict(z=U * (mu.abs() + 2 * (sd * eps).abs() + (mu + sd * eps).abs()))
    kl = 0.5 * (1 + lv.abs() + 2 * mu * mu + ev)
    out["kld"] = U * (kl.sum(-1) + acc(L) * (-0.5 * (1 + lv - mu * mu - ev)).abs().sum(-1))
    A_mu = gk * mu.abs() + _abs_k(dz)
    A_lv = gk * 0.5 * (1 + ev) + _abs_k(dz, eps) * sd
    e, t, dmu, dlv = 0.0, 0.0, [], []
    for um, ul in zip(mus, lvs):
        iv, d = torch.exp(-ul), (mu - um).abs()
        e = e + 0.5 * (ul.abs() + lv.abs() + 3 * (ev + d * d) * iv + 1)
        t = t + 0.5 * (ul - lv + (ev + d * d) * iv - 1)
        A_mu = A_mu + 3 * gl * d * iv
        A_lv = A_lv + gl * 0.5 * (3 * ev * iv + 1)
        dmu.append(U * 3 * gl * d * iv + TINY)
        dlv.append(U * gl * 0.5 * (1 + 3 * (ev + d * d) * iv) + TINY)
    out["ljm"] = U * (e.sum(-1) + acc(L * case.M) * t.abs().sum(-1))
    out.update(djmu=U * A_mu + TINY, djlv=U * A_lv + TINY, dmu=dmu, dlv=dlv)
    return out


def gauss_base(case, I):
    mu, lv, eps = I["mus"][0].to(F64), I["lvs"][0].to(F64), I["eps"].to(F64)
    dz = None if I["dz"] is None else I["dz"].to(F64)
    gk = _a(I["gk"]).unsqueeze(-1) if I["gk"] is not None else 0.0
    ev, sd = lv.exp(), torch.exp(0.5 * lv)
    kl = 0.5 * (1 + ev + 2 * mu * mu + lv.abs())
    return dict(w=U * (mu.abs() + 2 * (sd * eps).abs() + (mu + sd * eps).abs()),
                kl=U * (kl.sum(-1) + acc(case.L) * (-0.5 * (1 - ev - mu * mu + lv)).abs().sum(-1)),
                dmu=[U * (_abs_k(dz) + gk * mu.abs()) + TINY], dlv=[U * (_abs_k(dz, eps) * sd + gk * 0.5 * (ev + 1)) + TINY])


BASE = dict(mopoe=mopoe_base, mvtcae=mvtcae_base, mvae=mvae_base, jmvae=jmvae_base, gauss=gauss_base)


def bases(case, I):
    with torch.no_grad():
        return BASE[case.fam](case, I)


# ---- comparison of one implementation (the HIP kernels, or oracle.elbo in torch fp32) ----------------------------------------------------------
def run_torch32(case, I):
    return oracle_eval(case, I, torch.float32)


def ratios(case, I, got, mut=(), ref=None, base=None):
    """max |got - ref| / base per stage over EVERY entry of every array `got` holds (None: the array was not written: the
    NULL form of an optional output).  -> {stage: (ratio, array name)}; compare with C_STAGE[stage]."""
    ref = reference(case, I, mut) if ref is None else ref
    base = bases(case, I) if base is None else base
    out = {}
    for k, g in got.items():
        if g is None:
            continue
        gl, rl, bl = (g, ref[k], base[k]) if isinstance(g, list) else ([g], [ref[k]], [base[k]])
        r = 0.0
        for x, y, b in zip(gl, rl, bl):
            if x is not None:
                assert x.shape == y.shape == b.shape, (k, x.shape, y.shape, b.shape)
                r = max(r, worst_ratio(x, y, b))
        st = stage_of(case.fam, k)
        if r >= out.get(st, (-1.0, ""))[0]:
            out[st] = (r, k)
    return out
