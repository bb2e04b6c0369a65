"""Float64 torch reference of the conditional-latent kernel (mvk_cond_latent_fwd/bwd, csrc/elbo.hip) and of the CVAE training loss,
written from the formulas; plus the kernel's case table, seeded inputs and error model, and the procedural inputs of the CVAE
golden cases (tests/golden/cvae_*.npz).  CPU only: no GPU, no libmvk.so; nothing here reads the reference project.

Kernel.  mu, lv, pmu, plv [B,L] (a NULL prior is pmu = plv = 0), eps [K,B,L], conditioning pieces [B, C_j], C = sum C_j:
    zc[k,b,:L] = mu[b] + exp(lv[b] / 2) eps[k,b];      zc[k,b,L+off_j : L+off_j+C_j] = piece_j[b]   (copied: bit-exact)
    kl[b] = 1/2 sum_l (plv - lv + exp(lv - plv) + (mu - pmu)^2 / exp(plv) - 1)
backward (float64 autograd of the above) for upstream dzc [K,B,L+C] (its last C columns unused) and gkl [B].

Model.  mu, lv = encoder(x, c);  pmu, plv = prior_network(c) or 0, 0;  z = mu + exp(lv / 2) eps;  r = decoder([z, c]);
    recon_loss = sum_b nll(x_b | r_b) / B;   kl = mean_b kl[b];   loss = recon_loss + beta kl.

Error model (the form of tests/elbo_ref.py).  u = 2^-24.  Every output entry has a `base`, computed in float64 from the inputs: u
times the sum of the absolute values of the terms added or cancelled to form it, each with the error handed down from its
operands (an exp carries 1 + |argument|, a difference of two inputs their magnitudes), plus u times its own magnitude; the KL row
sum: the per-element bases plus (ceil(log2 L) + 1) u sum |addend|.  A comparison passes when |got - ref| <= C_STAGE[stage] * base
for EVERY entry; C_STAGE = 4x the largest |err| / base that the same formulas in plain torch fp32 on the CPU (backward: fp32
autograd) show over the case table, rounded up (tests/test_cvae_host.py::test_error_constants re-derives it; the HIP kernel has
no part in it).  The copied conditioning columns have no tolerance: they are compared bit for bit.
`mut` names deliberate mistakes of the REFERENCE, used only to show that the bounds reject them (MUTATIONS)."""
import math
import os
import sys
from collections import OrderedDict
from dataclasses import dataclass

import numpy as np
import torch

from mmvae_ref import TINY, U, worst_ratio  # noqa: F401  (re-exported to the tests)

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import procedural as P  # noqa: E402

F64 = torch.float64
LOG_2PI = math.log(2.0 * math.pi)

# one constant per output of the kernel: 4x the value measured by tests/test_cvae_host.py::test_error_constants, rounded up
C_STAGE = {"z": 4.0, "kl": 2.0, "dmu": 3.0, "dlv": 4.0, "dpmu": 3.0, "dplv": 4.0}
STAGES = tuple(C_STAGE)


def acc(n):
    """Accumulation term of a sum of n addends (a tree or a short sequential run), in units of u sum |addend|."""
    return math.ceil(math.log2(max(n, 1))) + 1


# ---- the kernel's case table ---------------------------------------------------------------------------------------------------------
LS = (5, 64, 130)          # less than a wave, exactly a wave, the lane loop
BS = (1, 3, 5, 260)        # partial and full last workgroups
KS = (1, 4)
PIECES = ((), (3,), (7, 1), (130,), (1024,))  # n_cond = 0, odd L + C, two pieces, the spread copy (16-byte form where L % 4 == 0)
NULLS = ((), ("dzc",), ("gkl",), ("kl_rows",))  # the optional pointers, cycled over the grid


@dataclass(frozen=True)
class Case:
    name: str
    L: int
    B: int
    K: int
    pieces: tuple
    prior: bool
    null: tuple
    seed: int


def _cases():
    out, i = [], 0
    for L in LS:
        for pieces in PIECES:
            for B in BS:
                for K in KS:
                    for prior in (False, True):
                        j = i // 2  # the shape's index; the cycle below meets every K, B, L, piece list and both priors
                        null = NULLS[(j + j // 2 + j // 8 + 2 * int(prior)) % len(NULLS)]
                        tag = "x".join(str(c) for c in pieces) or "none"
                        name = f"l{L}-b{B}-k{K}-c{tag}-{'prior' if prior else 'std'}" + "".join("-null-" + n for n in null)
                        out.append(Case(name, L, B, K, pieces, prior, null, 4000 + i))
                        i += 1
    return out


CASES = _cases()
CASE_BY_NAME = {c.name: c for c in CASES}
GROUPS = [(L, pieces) for L in LS for pieces in PIECES]  # one GPU test item per group


def group_cases(L, pieces):
    return [c for c in CASES if c.L == L and c.pieces == pieces]


def make_inputs(case):
    """Seeded fp32 inputs.  lv is graded over [-12, 6] and plv over [-6, 6] along the flattened [B, L] index (with a seeded
    jitter), so exp(lv - plv) spans e^-18 ... e^12 inside every case that has a prior."""
    g = torch.Generator().manual_seed(case.seed)
    B, L, K = case.B, case.L, case.K
    n = B * L
    ramp = torch.arange(n, dtype=torch.float32).reshape(B, L) / max(n - 1, 1)
    mu = 1.5 * torch.randn(B, L, generator=g)
    lv = -12.0 + 18.0 * ramp + 0.3 * torch.randn(B, L, generator=g)
    pmu = plv = None
    if case.prior:
        pmu = mu + torch.randn(B, L, generator=g) * torch.exp(2.0 * torch.randn(B, L, generator=g)).clamp(max=8.0)
        plv = 6.0 - 12.0 * ramp.flip(1) + 0.3 * torch.randn(B, L, generator=g)
        plv = plv[torch.randperm(B, generator=g)]
    eps = torch.randn(K, B, L, generator=g)
    pieces = [torch.randn(B, c, generator=g) for c in case.pieces]
    C = sum(case.pieces)
    dzc = None if "dzc" in case.null else torch.randn(K, B, L + C, generator=g)
    gkl = None if "gkl" in case.null else torch.randn(B, generator=g)
    return dict(mu=mu, lv=lv, pmu=pmu, plv=plv, eps=eps, pieces=pieces, dzc=dzc, gkl=gkl)


# ---- forward formulas --------------------------------------------------------------------------------------------------------------------
MUTATIONS = ["no_prior", "sd_no_half", "dpmu_sign", "drop_tail", "swap_pieces"]
# (mutation, the stages where it must show, the cases named for it)
TEETH = [
    ("no_prior", ("kl",), ["l5-b3-k4-c7x1-prior", "l64-b3-k4-c3-prior"]),
    ("sd_no_half", ("z", "dlv"), ["l5-b5-k4-c3-std", "l130-b3-k4-cnone-prior"]),
    ("dpmu_sign", ("dpmu",), ["l5-b3-k4-c7x1-prior", "l64-b5-k4-c7x1-prior"]),
    ("drop_tail", ("dmu", "dlv"), ["l5-b5-k4-c3-std", "l130-b3-k4-cnone-prior"]),
    ("swap_pieces", ("cond",), ["l5-b3-k4-c7x1-prior", "l130-b3-k4-c7x1-std"]),
]


def kl_rows(mu, lv, pmu, plv):
    return (0.5 * (plv - lv + torch.exp(lv - plv) + (mu - pmu) ** 2 / torch.exp(plv) - 1)).sum(-1)


def cond_latent(mu, lv, pmu, plv, eps, pieces, mut=()):
    """-> zc [K,B,L+C], kl [B] in the dtype of the inputs (pmu = plv = None: the N(0, I) prior)."""
    if pmu is None:
        pmu, plv = torch.zeros_like(mu), torch.zeros_like(lv)
    sd = torch.exp(lv) if "sd_no_half" in mut else torch.exp(0.5 * lv)
    z = mu + sd * eps
    kl = kl_rows(mu, lv, torch.zeros_like(mu), torch.zeros_like(lv)) if "no_prior" in mut else kl_rows(mu, lv, pmu, plv)
    ps = list(reversed(pieces)) if "swap_pieces" in mut else list(pieces)
    K, B = eps.shape[0], eps.shape[1]
    zc = torch.cat([z] + [p.unsqueeze(0).expand(K, B, p.shape[1]) for p in ps], dim=-1)
    return zc, kl


def evaluate(case, I, dtype, mut=()):
    """Forward and autograd backward in `dtype` on the fp32 inputs -> dict(z, cond, kl, dmu, dlv, dpmu, dplv); dpmu / dplv are
    None without a prior, cond is None without pieces.  dzc / gkl None = no upstream gradient (0)."""
    L = case.L
    mu, lv = I["mu"].to(dtype).requires_grad_(True), I["lv"].to(dtype).requires_grad_(True)
    pmu = plv = None
    if I["pmu"] is not None:
        pmu, plv = I["pmu"].to(dtype).requires_grad_(True), I["plv"].to(dtype).requires_grad_(True)
    eps = I["eps"].to(dtype)
    zc, kl = cond_latent(mu, lv, pmu, plv, eps, [p.to(dtype) for p in I["pieces"]], mut)
    total = zc.sum() * 0
    if I["dzc"] is not None:
        dz = I["dzc"].to(dtype)
        if "drop_tail" in mut:
            dz = dz.clone()
            dz[-1] = 0
        total = total + (zc * dz).sum()
    if I["gkl"] is not None:
        total = total + (kl * I["gkl"].to(dtype)).sum()
    leaves = [mu, lv] + ([pmu, plv] if pmu is not None else [])
    grads = torch.autograd.grad(total, leaves, allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, leaves)]
    if "dpmu_sign" in mut and pmu is not None:
        grads[2] = -grads[2]
    out = dict(z=zc[..., :L].detach(), cond=zc[..., L:].detach() if case.pieces else None, kl=kl.detach(), dmu=grads[0],
               dlv=grads[1], dpmu=None, dplv=None)
    if pmu is not None:
        out.update(dpmu=grads[2], dplv=grads[3])
    return out


def reference(case, I, mut=()):
    return evaluate(case, I, F64, mut)


def run_torch32(case, I):
    return evaluate(case, I, torch.float32)


def bases(case, I, ref=None):
    """The error model's base of every output, float64, same shapes as `reference` (cond has none: it is exact)."""
    ref = reference(case, I) if ref is None else ref
    with torch.no_grad():
        mu, lv, eps = I["mu"].to(F64), I["lv"].to(F64), I["eps"].to(F64)
        pmu = torch.zeros_like(mu) if I["pmu"] is None else I["pmu"].to(F64)
        plv = torch.zeros_like(lv) if I["plv"] is None else I["plv"].to(F64)
        L = case.L
        sd, d, ip, r = torch.exp(0.5 * lv), mu - pmu, torch.exp(-plv), torch.exp(lv - plv)
        q = ip * (d * d * (3 + plv.abs()) + 2 * d.abs() * (mu.abs() + pmu.abs()))  # error of (mu - pmu)^2 exp(-plv), in u
        re = r * (2 + (lv - plv).abs())                                            # error of exp(lv - plv), in u
        z = mu + sd * eps
        term = 0.5 * (plv - lv + r + d * d * ip - 1)
        kl_elem = 0.5 * (plv.abs() + lv.abs() + re + q + 1)
        out = dict(z=U * (mu.abs() + (sd * eps).abs() * (2 + 0.5 * lv.abs()) + z.abs()),
                   kl=U * (kl_elem.sum(-1) + acc(L) * term.abs().sum(-1) + term.sum(-1).abs()))
        if I["dzc"] is not None:
            dz = I["dzc"].to(F64)[..., :L]
            sa, sae = dz.abs().sum(0), (dz * eps).abs().sum(0)
        else:
            sa = sae = torch.zeros_like(mu)
        gk = torch.zeros(case.B, 1, dtype=F64) if I["gkl"] is None else I["gkl"].to(F64).abs().unsqueeze(-1)
        a = gk * ip * (d.abs() * (3 + plv.abs()) + mu.abs() + pmu.abs())
        ak = acc(case.K)
        out["dmu"] = U * (ak * sa + a + ref["dmu"].abs()) + TINY
        out["dlv"] = U * (sd * sae * (ak + 2 + 0.5 * lv.abs()) + 0.5 * gk * (re + 1) + ref["dlv"].abs()) + TINY
        if I["pmu"] is not None:
            out["dpmu"] = U * (a + ref["dpmu"].abs()) + TINY
            out["dplv"] = U * (0.5 * gk * (1 + re + q) + ref["dplv"].abs()) + TINY
        return out


def ratios(case, I, got, mut=(), ref=None, base=None):
    """max |got - ref| / base per stage over EVERY entry (`got[k]` None: not written) -> {stage: ratio}.  The stage "cond" is
    exact: 0.0 when the copied columns equal the reference's bit for bit, inf otherwise."""
    ref = reference(case, I, mut) if ref is None else ref
    base = bases(case, I) if base is None else base
    out = {}
    for k in STAGES:
        if got.get(k) is not None and ref.get(k) is not None:
            assert got[k].shape == ref[k].shape == base[k].shape, (k, got[k].shape, ref[k].shape)
            out[k] = worst_ratio(got[k], ref[k], base[k])
    if got.get("cond") is not None:
        same = torch.equal(got["cond"].to(torch.float32).view(torch.int32), ref["cond"].to(torch.float32).view(torch.int32))
        out["cond"] = 0.0 if same else math.inf
    return out


# ---- the CVAE golden cases: procedural inputs, float64 loss ------------------------------------------------------------------------------
CVAE_CASES = ["cvae_tiny_stdprior", "cvae_tiny_prior_two_cond", "cvae_tiny_bernoulli_prior", "cvae_mnist_label"]
CASE_CONFIGS = {
    "cvae_tiny_stdprior": dict(dims=[["x", [7]], ["c", [3]]], main="x", cond=["c"], L=5, beta=1.0, dist="normal", prior=False,
                               B=7, seed=2201),
    "cvae_tiny_prior_two_cond": dict(dims=[["x", [6]], ["c1", [5]], ["c2", [3, 2]]], main="x", cond=["c1", "c2"], L=4, beta=2.5,
                                     dist="laplace", prior=True, B=9, seed=2202),
    "cvae_tiny_bernoulli_prior": dict(dims=[["x", [2, 4]], ["c", [3]]], main="x", cond=["c"], L=3, beta=1.0, dist="bernoulli",
                                      prior=True, B=5, seed=2203),
    "cvae_mnist_label": dict(dims=[["mnist", [1, 28, 28]], ["label", [10]]], main="mnist", cond=["label"], L=16, beta=1.0,
                             dist="normal", prior=True, B=8, seed=2204),
}


def case_dims(cfg):
    return OrderedDict((m, tuple(d)) for m, d in cfg["dims"])


def case_inputs(cfg):
    """-> dims, data {m: np [B, *dim]} (procedural, bit-exact)."""
    dims = case_dims(cfg)
    data = {m: P.uniform((cfg["B"],) + d, cfg["seed"] + i) for i, (m, d) in enumerate(dims.items())}
    if cfg["dist"] == "bernoulli":
        data[cfg["main"]] = (data[cfg["main"]] > 0.5).astype(np.float32)
    return dims, data


def case_state_dict(cfg):
    """The procedural weights, in the parameter order recorded from the reference."""
    shapes = OrderedDict((k, tuple(s)) for k, s in cfg["sd_shapes"])
    return P.make_state_dict(shapes, cfg["seed"])


def _mlp_encoder(sd, prefix, x):
    h = x.reshape(x.shape[0], -1)
    i = 0
    while f"{prefix}layers.{i}.0.weight" in sd:
        h = torch.relu(h @ sd[f"{prefix}layers.{i}.0.weight"].T + sd[f"{prefix}layers.{i}.0.bias"])
        i += 1
    return h @ sd[prefix + "embedding.weight"].T + sd[prefix + "embedding.bias"]


def joint_encoder(sd, prefix, data, names):
    """MultipleHeadJointEncoder over default MLP encoders: their means concatenated, [Linear + ReLU] layers, two heads."""
    h = torch.cat([_mlp_encoder(sd, f"{prefix}encoders.{m}.", data[m]) for m in names], dim=1)
    i = 0
    while f"{prefix}enc.{i}.0.weight" in sd:
        h = torch.relu(h @ sd[f"{prefix}enc.{i}.0.weight"].T + sd[f"{prefix}enc.{i}.0.bias"])
        i += 1
    return h @ sd[prefix + "fc1.weight"].T + sd[prefix + "fc1.bias"], h @ sd[prefix + "fc2.weight"].T + sd[prefix + "fc2.bias"]


def decoder(sd, z, cond):
    zc = torch.cat([z] + [c.reshape(z.shape[0], -1) for c in cond], dim=1)
    h = torch.relu(zc @ sd["decoder.network.layers.0.0.weight"].T + sd["decoder.network.layers.0.0.bias"])
    return torch.sigmoid(h @ sd["decoder.network.layers.1.0.weight"].T + sd["decoder.network.layers.1.0.bias"])


def nll_rows(dist, r, x):
    x = x.reshape(x.shape[0], -1)
    if dist == "normal":
        e = 0.5 * (x - r) ** 2 + 0.5 * LOG_2PI
    elif dist == "laplace":
        e = (x - r).abs() + math.log(2.0)
    elif dist == "bernoulli":  # the decoder output is taken as logits
        e = torch.nn.functional.softplus(r) - x * r
    else:
        raise ValueError(dist)
    return e.sum(-1)


def cvae_loss(cfg, sd, data, eps):
    """sd: name -> tensor; data {m: tensor}; eps [B, L] -> dict(loss, metrics={kl, recon_loss}, mu, recon)."""
    names = [m for m, _ in cfg["dims"]]
    mu, lv = joint_encoder(sd, "encoder.", data, names)
    if cfg["prior"]:
        pmu, plv = joint_encoder(sd, "prior_network.", data, cfg["cond"])
    else:
        pmu, plv = torch.zeros_like(mu), torch.zeros_like(lv)
    z = mu + torch.exp(0.5 * lv) * eps
    r = decoder(sd, z, [data[m] for m in cfg["cond"]])
    recon = nll_rows(cfg["dist"], r, data[cfg["main"]]).sum() / mu.shape[0]
    kl = kl_rows(mu, lv, pmu, plv).mean()
    return dict(loss=recon + cfg["beta"] * kl, metrics=dict(kl=kl, recon_loss=recon), mu=mu, recon=r)


def case_tensors(cfg, arrays, dtype=F64):
    _, data = case_inputs(cfg)
    return {m: torch.from_numpy(v).to(dtype) for m, v in data.items()}, torch.from_numpy(arrays["eps"]).to(dtype)


def reference_grads(cfg, arrays):
    """-> (result dict, {name: float64 gradient}) of the float64 loss at the golden case's recorded draw."""
    sd = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in case_state_dict(cfg).items()}
    data, eps = case_tensors(cfg, arrays)
    out = cvae_loss(cfg, sd, data, eps)
    out["loss"].backward()
    return out, {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in sd.items()}
