"""Float64 torch reference of TELBO's stage-two latent kernel (mvk_telbo_latent_fwd/bwd, csrc/telbo.hip) and of both stages of the
TELBO training loss, written from the formulas; plus the kernel's case table, seeded inputs and error model, and the procedural
inputs of the TELBO golden cases (tests/golden/telbo_*.npz).  CPU only: no GPU, no libmvk.so; nothing here reads the reference
project.

Kernel.  joint_lv [B,L]; mu, lv, eps [M,B,L] (M modalities):
    z[m,b,l] = mu_m + exp(lv_m / 2) eps[m,b,l];      kld[m,b] = -1/2 sum_l (1 + joint_lv[b,l] - mu_m^2 - exp(lv_m))
(the JOINT log-variance inside the unimodal "KL": the reference's formula).  Backward: float64 autograd of the above for upstream
dz [M,B,L] and gkld [M,B] -> dmu, dlv [M,B,L], djoint_lv [B,L].

Model.  Stage one (epoch <= warmup): z = mu_J + exp(lv_J / 2) eps, recon = sum_m lambda_m sum_b nll(x_m | dec_m(z)),
KLD = -1/2 sum (1 + lv_J - mu_J^2 - exp(lv_J)), loss = (recon + KLD) / B.  Stage two: per modality z_m from the unimodal encoder,
elbo_m = gamma_m sum_b nll(x_m | dec_m(z_m)) + sum_b kld[m,b], loss = sum_m elbo_m / B, loss_sum = sum_m elbo_m.

Error model (the form of tests/cvae_ref.py).  u = 2^-24.  Every output entry has a `base`, computed in float64 from the inputs: u
times the sum of the absolute values of the terms added or cancelled to form it, each with the error handed down from its
operands (an exp carries 1 + |argument|), plus u times its own magnitude; a sum of n addends: the addends' bases plus
(ceil(log2 n) + 1) u sum |addend|.  A comparison passes when |got - ref| <= C_STAGE[stage] * base for EVERY entry; C_STAGE = 4x the
largest |err| / base that the same formulas in plain torch fp32 on the CPU (backward: fp32 autograd) show over the case table,
rounded up (tests/test_telbo_host.py::test_error_constants re-derives it; the HIP kernel has no part in it).
`mut` names deliberate mistakes of the REFERENCE, used only to show that the bounds reject them (MUTATIONS)."""
import math
import os
import sys
from collections import OrderedDict
from dataclasses import dataclass

import numpy as np
import torch

from cvae_ref import LOG_2PI, acc, joint_encoder
from mmvae_ref import TINY, U, worst_ratio  # noqa: F401  (re-exported to the tests)

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import procedural as P  # noqa: E402

F64 = torch.float64

# one constant per output of the kernel: 4x the value measured by tests/test_telbo_host.py::test_error_constants, rounded up
C_STAGE = {"z": 4.0, "kld": 2.0, "dmu": 3.0, "dlv": 3.0, "djoint_lv": 2.0}
STAGES = tuple(C_STAGE)

# ---- the kernel's case table ---------------------------------------------------------------------------------------------------------
LS = (1, 5, 64, 130)       # one element, less than a wave, exactly a wave, the lane loop (all but 64 odd or not a multiple of 4)
BS = (1, 3, 260)           # partial and full last workgroups of the forward's four rows
MS = (1, 2, 5)
NULLS = ((), ("dz",), ("gkld",), ("djoint_lv",))  # the optional pointers, cycled over the grid


@dataclass(frozen=True)
class Case:
    name: str
    L: int
    B: int
    M: int
    null: tuple
    seed: int


def _cases():
    out, i = [], 0
    for L in LS:
        for B in BS:
            for M in MS:
                null = NULLS[(i + i // 3 + i // 9) % len(NULLS)]
                out.append(Case(f"l{L}-b{B}-m{M}" + "".join("-null-" + n for n in null), L, B, M, null, 5000 + i))
                i += 1
    return out


CASES = _cases()
CASE_BY_NAME = {c.name: c for c in CASES}


def make_inputs(case):
    """Seeded fp32 inputs.  lv is graded over [-12, 6] and joint_lv over [-6, 6] along the flattened index (with a seeded jitter)."""
    g = torch.Generator().manual_seed(case.seed)
    M, B, L = case.M, case.B, case.L
    n = M * B * L
    ramp = torch.arange(n, dtype=torch.float32).reshape(M, B, L) / max(n - 1, 1)
    jramp = torch.arange(B * L, dtype=torch.float32).reshape(B, L) / max(B * L - 1, 1)
    mu = 1.5 * torch.randn(M, B, L, generator=g)
    lv = -12.0 + 18.0 * ramp + 0.3 * torch.randn(M, B, L, generator=g)
    jlv = 6.0 - 12.0 * jramp + 0.3 * torch.randn(B, L, generator=g)
    eps = torch.randn(M, B, L, generator=g)
    dz = None if "dz" in case.null else torch.randn(M, B, L, generator=g)
    gkld = None if "gkld" in case.null else torch.randn(M, B, generator=g)
    return dict(mu=mu, lv=lv, jlv=jlv, eps=eps, dz=dz, gkld=gkld)


# ---- formulas ----------------------------------------------------------------------------------------------------------------------------
MUTATIONS = ["kl_own_lv", "sd_no_half", "dlv_kl_sign", "swap_modalities", "djoint_drop_m"]
# (mutation, the stages where it must show, the cases named for it)
TEETH = [
    ("kl_own_lv", ("kld",), ["l5-b3-m2-null-gkld", "l130-b1-m5-null-dz"]),
    ("sd_no_half", ("z", "dlv"), ["l5-b3-m2-null-gkld", "l64-b260-m5"]),
    ("dlv_kl_sign", ("dlv",), ["l130-b3-m2", "l5-b3-m5-null-djoint_lv"]),
    ("swap_modalities", ("z",), ["l5-b3-m2-null-gkld", "l64-b260-m5"]),
    ("djoint_drop_m", ("djoint_lv",), ["l130-b3-m2", "l1-b3-m2-null-dz"]),
]


def telbo_latent(mu, lv, jlv, eps, mut=()):
    """-> z [M,B,L], kld [M,B] in the dtype of the inputs."""
    sd = torch.exp(lv) if "sd_no_half" in mut else torch.exp(0.5 * lv)
    e = eps
    if "swap_modalities" in mut and eps.shape[0] > 1:
        e = eps.clone()
        e[0] = eps[1]
    z = mu + sd * e
    inner = lv if "kl_own_lv" in mut else jlv
    kld = (-0.5 * (1 + inner - mu.pow(2) - lv.exp())).sum(-1)
    return z, kld


def evaluate(case, I, dtype, mut=()):
    """Forward and autograd backward in `dtype` on the fp32 inputs -> dict(z, kld, dmu, dlv, djoint_lv).  dz / gkld None = no
    upstream gradient (0)."""
    mu, lv = I["mu"].to(dtype).requires_grad_(True), I["lv"].to(dtype).requires_grad_(True)
    jlv = I["jlv"].to(dtype).requires_grad_(True)
    eps = I["eps"].to(dtype)
    z, kld = telbo_latent(mu, lv, jlv, eps, mut)
    total = z.sum() * 0 + jlv.sum() * 0
    if I["dz"] is not None:
        total = total + (z * I["dz"].to(dtype)).sum()
    if I["gkld"] is not None:
        gk = I["gkld"].to(dtype)
        total = total + (kld * gk).sum()
    dmu, dlv, djlv = torch.autograd.grad(total, [mu, lv, jlv])
    if I["gkld"] is not None:
        gk = I["gkld"].to(dtype).unsqueeze(-1)
        if "dlv_kl_sign" in mut:
            dlv = dlv - gk * lv.detach().exp()  # 1/2 gk exp(lv) with the other sign
        if "djoint_drop_m" in mut:
            djlv = djlv + 0.5 * gk[-1].expand_as(djlv)  # the sum over the first M - 1 modalities only
    return dict(z=z.detach(), kld=kld.detach(), dmu=dmu, dlv=dlv, djoint_lv=djlv)


def reference(case, I, mut=()):
    return evaluate(case, I, F64, mut)


def run_torch32(case, I):
    return evaluate(case, I, torch.float32)


def bases(case, I, ref=None):
    """The error model's base of every output, float64, same shapes as `reference`."""
    ref = reference(case, I) if ref is None else ref
    with torch.no_grad():
        mu, lv, jlv, eps = I["mu"].to(F64), I["lv"].to(F64), I["jlv"].to(F64), I["eps"].to(F64)
        M, B, L = mu.shape
        sd, ev = torch.exp(0.5 * lv), torch.exp(lv)
        z = mu + sd * eps
        term = -0.5 * (1 + jlv - mu * mu - ev)
        # three additions at the magnitude of what they combine, the square, the exp
        elem = 0.5 * (3 * (1 + jlv.abs() + mu * mu + ev) + mu * mu + ev * (1 + lv.abs()))
        out = dict(z=U * (mu.abs() + (sd * eps).abs() * (2 + 0.5 * lv.abs()) + z.abs()),
                   kld=U * (elem.sum(-1) + acc(L) * term.abs().sum(-1) + term.sum(-1).abs()))
        dz = torch.zeros_like(mu) if I["dz"] is None else I["dz"].to(F64)
        gk = torch.zeros(M, B, 1, dtype=F64) if I["gkld"] is None else I["gkld"].to(F64).unsqueeze(-1)
        out["dmu"] = U * (dz.abs() + 2 * (gk * mu).abs() + ref["dmu"].abs()) + TINY
        out["dlv"] = U * (0.5 * (sd * eps * dz).abs() * (3 + 0.5 * lv.abs()) + 0.5 * gk.abs() * ev * (2 + lv.abs())
                          + ref["dlv"].abs()) + TINY
        out["djoint_lv"] = (U * (acc(M) * 0.5 * gk.abs().sum(0) + ref["djoint_lv"].abs()) + TINY).expand(B, L)
        return out


def ratios(case, I, got, mut=(), ref=None, base=None):
    """max |got - ref| / base per stage over EVERY entry (`got[k]` None: not written) -> {stage: ratio}."""
    ref = reference(case, I, mut) if ref is None else ref
    base = bases(case, I) if base is None else base
    out = {}
    for k in STAGES:
        if got.get(k) is not None:
            assert got[k].shape == ref[k].shape == base[k].shape, (k, got[k].shape, ref[k].shape, base[k].shape)
            out[k] = worst_ratio(got[k], ref[k], base[k])
    return out


# ---- the TELBO golden cases: procedural inputs, float64 loss ---------------------------------------------------------------------------
TINY_DIMS = [["m1", [2]], ["m2", [3]], ["m3", [4]]]
TINY_DISTS = dict(m1="normal", m2="laplace", m3="bernoulli")
TELBO_CASES = ["telbo_tiny_stage1", "telbo_tiny_boundary", "telbo_tiny_stage2", "telbo_tiny_stage2_factors",
               "telbo_mnistsvhn_mlp_stage2"]
CASE_CONFIGS = {
    "telbo_tiny_stage1": dict(dims=TINY_DIMS, L=5, B=6, seed=3301, warmup=2, epoch=1, dists=TINY_DISTS, rescaling=True,
                              lambda_factors=None, gamma_factors=None, scale=None),
    "telbo_tiny_boundary": dict(dims=TINY_DIMS, L=5, B=7, seed=3302, warmup=2, epoch=2, dists=TINY_DISTS, rescaling=True,
                                lambda_factors=None, gamma_factors=None, scale=None),
    "telbo_tiny_stage2": dict(dims=TINY_DIMS, L=5, B=6, seed=3303, warmup=2, epoch=3, dists=TINY_DISTS, rescaling=True,
                              lambda_factors=None, gamma_factors=None, scale=None),
    "telbo_tiny_stage2_factors": dict(dims=TINY_DIMS, L=5, B=5, seed=3304, warmup=2, epoch=3, dists=TINY_DISTS, rescaling=False,
                                      lambda_factors=dict(m1=0.5, m2=2.0, m3=1.5), gamma_factors=dict(m1=1.25, m2=0.75, m3=3.0),
                                      scale=0.75),
    "telbo_mnistsvhn_mlp_stage2": dict(dims=[["mnist", [1, 28, 28]], ["svhn", [3, 32, 32]]], L=20, B=8, seed=3305, warmup=2,
                                       epoch=3, dists=None, rescaling=True, lambda_factors=None, gamma_factors=None, scale=None),
}
FOLDER = "telbo_reference_folder"
FOLDER_CONFIG = dict(dims=TINY_DIMS, L=3, warmup=4)


def case_dims(cfg):
    return OrderedDict((m, tuple(d)) for m, d in cfg["dims"])


def case_dists(cfg):
    return {m: (cfg["dists"] or {}).get(m, "normal") for m, _ in cfg["dims"]}


def config_kwargs(cfg):
    """Keyword arguments of TELBOConfig (this package's and the reference's) for a golden case."""
    dims = case_dims(cfg)
    kw = dict(n_modalities=len(dims), latent_dim=cfg["L"], input_dims=dict(dims), warmup=cfg["warmup"],
              uses_likelihood_rescaling=cfg["rescaling"], lambda_factors=cfg["lambda_factors"], gamma_factors=cfg["gamma_factors"])
    if cfg["dists"]:
        kw["decoders_dist"] = dict(cfg["dists"])
    if cfg["scale"] is not None:
        kw["decoder_dist_params"] = {m: {"scale": cfg["scale"]} for m, d in case_dists(cfg).items() if d in ("normal", "laplace")}
    return kw


def case_inputs(cfg):
    """-> dims, data {m: np [B, *dim]} (procedural, bit-exact)."""
    dims = case_dims(cfg)
    dists = case_dists(cfg)
    data = {m: P.uniform((cfg["B"],) + d, cfg["seed"] + i) for i, (m, d) in enumerate(dims.items())}
    for m in dims:
        if dists[m] == "bernoulli":
            data[m] = (data[m] > 0.5).astype(np.float32)
    return dims, data


def case_state_dict(cfg):
    """The procedural weights (default MLP encoders / decoders, MultipleHeadJointEncoder: the layout of JMVAE)."""
    return P.make_state_dict(P.jmvae_mlp_shapes(case_dims(cfg), cfg["L"]), cfg["seed"])


def factors(cfg, which):
    """lambda (stage one) / gamma (stage two) factors: the explicit ones, else the rescale factors (ones without rescaling)."""
    given = cfg["lambda_factors" if which == "lambda" else "gamma_factors"]
    if given is not None:
        return {m: float(v) for m, v in given.items()}
    dims = case_dims(cfg)
    if not cfg["rescaling"]:
        return {m: 1.0 for m in dims}
    mx = max(int(np.prod(d)) for d in dims.values())
    return {m: mx / int(np.prod(d)) for m, d in dims.items()}


def mlp_encoder(sd, prefix, x):
    h = x.reshape(x.shape[0], -1)
    i = 0
    while f"{prefix}layers.{i}.0.weight" in sd:
        h = torch.relu(h @ sd[f"{prefix}layers.{i}.0.weight"].T + sd[f"{prefix}layers.{i}.0.bias"])
        i += 1
    return (h @ sd[prefix + "embedding.weight"].T + sd[prefix + "embedding.bias"],
            h @ sd[prefix + "log_var.weight"].T + sd[prefix + "log_var.bias"])


def mlp_decoder(sd, prefix, z):
    h = torch.relu(z @ sd[prefix + "layers.0.0.weight"].T + sd[prefix + "layers.0.0.bias"])
    return torch.sigmoid(h @ sd[prefix + "layers.1.0.weight"].T + sd[prefix + "layers.1.0.bias"])


def nll_rows(dist, r, x, scale=1.0):
    x = x.reshape(x.shape[0], -1)
    if dist == "normal":
        e = 0.5 * ((x - r) / scale) ** 2 + math.log(scale) + 0.5 * LOG_2PI
    elif dist == "laplace":
        e = (x - r).abs() / scale + math.log(2.0 * scale)
    elif dist == "bernoulli":  # the decoder output is taken as logits
        e = torch.nn.functional.softplus(r) - x * r
    else:
        raise ValueError(dist)
    return e.sum(-1)


def telbo_loss(cfg, sd, data, eps):
    """sd: name -> tensor; data {m: tensor}; eps [B,L] (stage one) or [M,B,L] (stage two) -> the ModelOutput's entries as a dict."""
    names = [m for m, _ in cfg["dims"]]
    dists = case_dists(cfg)
    scale = 1.0 if cfg["scale"] is None else cfg["scale"]
    jmu, jlv = joint_encoder(sd, "joint_encoder.", data, names)
    B = jmu.shape[0]
    if cfg["epoch"] <= cfg["warmup"]:
        lam = factors(cfg, "lambda")
        z = jmu + torch.exp(0.5 * jlv) * eps
        recon = sum(lam[m] * nll_rows(dists[m], mlp_decoder(sd, f"decoders.{m}.", z), data[m], scale).sum() for m in names)
        kld = -0.5 * torch.sum(1 + jlv - jmu.pow(2) - jlv.exp())
        return dict(recon_loss=recon / B, KLD=kld / B, loss=(recon + kld) / B, metrics=dict(kld_joint=kld, recon_joint=recon / B))
    gam = factors(cfg, "gamma")
    jlv = jlv.detach()
    elbos = {}
    for i, m in enumerate(names):
        mu, lv = mlp_encoder(sd, f"encoders.{m}.", data[m])
        z = mu + torch.exp(0.5 * lv) * eps[i]
        rec = gam[m] * nll_rows(dists[m], mlp_decoder(sd, f"decoders.{m}.", z), data[m], scale).sum()
        elbos[m] = rec + -0.5 * torch.sum(1 + jlv - mu.pow(2) - lv.exp())
    total = sum(elbos.values())
    return dict(loss=total / B, loss_sum=total, metrics=elbos)


def case_tensors(cfg, arrays, dtype=F64):
    _, data = case_inputs(cfg)
    return {m: torch.from_numpy(v).to(dtype) for m, v in data.items()}, torch.from_numpy(arrays["eps"]).to(dtype)


def reference_grads(cfg, arrays):
    """-> (result dict, {name: float64 gradient or None}) of the float64 loss at the golden case's recorded draw.  In stage two
    the decoders are frozen: their weights take part without a gradient."""
    sd = {k: torch.from_numpy(v).double() for k, v in case_state_dict(cfg).items()}
    stage2 = cfg["epoch"] > cfg["warmup"]
    for k, v in sd.items():
        v.requires_grad_(k.startswith("encoders.") if stage2 else True)
    data, eps = case_tensors(cfg, arrays)
    out = telbo_loss(cfg, sd, data, eps)
    out["loss"].backward()
    return out, {k: v.grad for k, v in sd.items()}
