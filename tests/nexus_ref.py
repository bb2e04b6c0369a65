"""Float64 torch reference of the Nexus training loss (Vasco et al. 2022), written from the model's formulas, plus the
procedural inputs of the Nexus golden cases (tests/golden/nexus_*.npz).  CPU only; nothing here reads the reference project.

Per row b, with annealing a = min(epoch / warmup, 1) and every draw given (eps_m, eps_joint, keep):
    z_m = mu_m + exp(lv_m / 2) eps_m                         (bottom encoders, default MLPs)
    bottom_b = sum_m mask_m [ rescale_m nll_m(x_m | dec_m(z_m)) + beta_m a KL(q_m || N(0, I)) ]
    msg_m = top_enc_m(stopgrad z_m).mu;  agg = sum_m keep_m msg_m / sum_m keep_m
    z_s = mu_s + exp(lv_s / 2) eps_joint                      (joint encoder on agg)
    top_b = sum_m gamma_m mask_m sum_d -ln N(stopgrad z_m | top_dec_m(z_s), s_m) + top_beta a KL(q_s || N(0, I))
    s_m = 1, or sqrt(mean over the whole [B, D_m] block of (z_m - top_dec_m(z_s))^2) (adapted, NOT detached)
loss = mean_b (bottom_b + top_b), loss_sum = sum_b (bottom_b + top_b)."""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import procedural as P  # noqa: E402

NEXUS_CASES = ["nexus_tiny_complete", "nexus_tiny_masked", "nexus_tiny_m4_drop_all", "nexus_mnistsvhn"]
TINY_DIMS = dict(mod1=(2,), mod2=(3,), mod3=(4,), mod4=(4,))
MNIST_SVHN_DIMS = dict(mnist=(1, 28, 28), svhn=(3, 32, 32))
LOG_2PI = math.log(2.0 * math.pi)


def case_dims(cfg):
    if cfg["arch"] == "tiny":
        return {m: TINY_DIMS[m] for m in cfg["names"]}
    return dict(MNIST_SVHN_DIMS)


def case_inputs(cfg):
    """-> dims, data {m: np [B, *dim]}, masks {m: bool np [B]} | None (procedural, bit-exact)."""
    B, seed = cfg["B"], cfg["seed"]
    dims = case_dims(cfg)
    data = {m: P.uniform((B,) + tuple(d), seed + i) for i, (m, d) in enumerate(dims.items())}
    for m, d in (cfg.get("dists") or {}).items():
        if d == "bernoulli":
            data[m] = (data[m] > 0.5).astype(np.float32)
    masks = None
    if cfg["masked"]:
        masks = {m: P.hash_uniform(B, seed + 50 + i) > 0.4 for i, m in enumerate(dims)}
        first = list(dims)[0]
        masks[first][:] = True  # every row keeps at least one modality
        masks[list(dims)[-1]][0] = False
    return dims, data, masks


def case_state_dict(cfg):
    """The procedural weights, in the parameter order recorded from the reference."""
    from collections import OrderedDict

    shapes = OrderedDict((k, tuple(s)) for k, s in cfg["sd_shapes"])
    return P.make_state_dict(shapes, cfg["seed"])


def _encoder(sd, prefix, x):
    h = x.reshape(x.shape[0], -1)
    i = 0
    while f"{prefix}layers.{i}.0.weight" in sd:
        h = torch.relu(h @ sd[f"{prefix}layers.{i}.0.weight"].T + sd[f"{prefix}layers.{i}.0.bias"])
        i += 1
    mu = h @ sd[prefix + "embedding.weight"].T + sd[prefix + "embedding.bias"]
    lv = h @ sd[prefix + "log_var.weight"].T + sd[prefix + "log_var.bias"]
    return mu, lv


def _decoder(sd, prefix, z):
    h = torch.relu(z @ sd[prefix + "layers.0.0.weight"].T + sd[prefix + "layers.0.0.bias"])
    return torch.sigmoid(h @ sd[prefix + "layers.1.0.weight"].T + sd[prefix + "layers.1.0.bias"])


def _nll_rows(dist, scale, r, x):
    x = x.reshape(x.shape[0], -1)
    if dist == "normal":
        e = 0.5 * ((x - r) / scale) ** 2 + math.log(scale) + 0.5 * LOG_2PI
    elif dist == "laplace":
        e = (x - r).abs() / scale + math.log(2.0 * scale)
    elif dist == "bernoulli":  # the decoder output is taken as logits (the reference's Bernoulli(logits=...))
        e = torch.nn.functional.softplus(r) - x * r
    else:
        raise ValueError(dist)
    return e.sum(-1)


def _kl_rows(mu, lv):
    return -0.5 * (1 + lv - mu ** 2 - lv.exp()).sum(-1)


def nexus_loss(cfg, sd, data, masks, eps, eps_joint, keep, epoch):
    """sd: name -> float64 tensor; data, masks, eps: {m: tensor}; keep [B, M] (ignored with masks).  -> dict(loss, loss_sum,
    metrics) of float64 tensors (the metrics of the reference, same names and meanings)."""
    names = cfg["names"]
    dims = case_dims(cfg)
    B = next(iter(data.values())).shape[0]
    a = min(epoch / cfg["warmup"], 1.0)
    dists = cfg.get("dists") or {}
    if cfg["rescaling"]:
        mx = max(int(np.prod(d)) for d in dims.values())
        resc = {m: mx / int(np.prod(dims[m])) for m in names}
    else:
        resc = {m: 1.0 for m in names}
    mk = {m: (masks[m].double() if masks is not None else torch.ones(B, dtype=torch.float64)) for m in names}
    metrics, zd, msgs = {}, {}, []
    bottom = torch.zeros(B, dtype=torch.float64)
    for m in names:
        mu, lv = _encoder(sd, f"encoders.{m}.", data[m])
        z = mu + torch.exp(0.5 * lv) * eps[m]
        r = _decoder(sd, f"decoders.{m}.", z)
        nll = resc[m] * _nll_rows(dists.get(m, "normal"), 1.0, r, data[m])
        kl = _kl_rows(mu, lv)
        bottom = bottom + (nll + kl * cfg["bottom_betas"][m] * a) * mk[m]
        zd[m] = z.detach()
        msgs.append(_encoder(sd, f"top_encoders.{m}.", zd[m])[0])
        metrics["recon_loss_" + m] = nll.mean()
        metrics["kl_" + m] = kl.mean()
    kp = torch.stack([mk[m] for m in names], 1) if masks is not None else keep.double()
    agg = sum(kp[:, i:i + 1] * msgs[i] for i in range(len(names))) / kp.sum(1, keepdim=True)
    mu_j, lv_j = _encoder(sd, "joint_encoder.", agg)
    zj = mu_j + torch.exp(0.5 * lv_j) * eps_joint
    top = torch.zeros(B, dtype=torch.float64)
    for m in names:
        r = _decoder(sd, f"top_decoders.{m}.", zj)
        D = r.shape[1]
        s2 = ((zd[m] - r) ** 2).mean() if m in (cfg["adapt"] or []) else torch.tensor(1.0, dtype=torch.float64)
        row = (((zd[m] - r) ** 2).sum(-1) / (2 * s2) + 0.5 * D * torch.log(s2) + 0.5 * D * LOG_2PI) * cfg["gammas"][m] * mk[m]
        top = top + row
        metrics["recon_z_" + m] = row.mean()
    jkl = _kl_rows(mu_j, lv_j)
    top = top + cfg["top_beta"] * jkl * a
    total = top + bottom
    metrics.update(annealing=a, bottom_loss=bottom.mean(), top_loss=top.mean(), joint_KLD=jkl.mean())
    return dict(loss=total.mean(), loss_sum=total.sum(), metrics=metrics)


def case_tensors(cfg, arrays, dtype=torch.float64):
    """The inputs and recorded draws of a golden case as CPU tensors: data, masks, eps {m}, eps_joint, keep."""
    _, data, masks = case_inputs(cfg)
    data = {m: torch.from_numpy(v).to(dtype) for m, v in data.items()}
    masks = None if masks is None else {m: torch.from_numpy(v) for m, v in masks.items()}
    eps = {m: torch.from_numpy(arrays["eps/" + m]).to(dtype) for m in cfg["names"]}
    eps_joint = torch.from_numpy(arrays["eps_joint"]).to(dtype)
    keep = torch.from_numpy(arrays["keep"]).to(dtype)
    return data, masks, eps, eps_joint, keep


def reference_grads(cfg, arrays):
    """-> (result dict, {name: float64 gradient}) of the float64 loss at the golden case's recorded draws."""
    sd = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in case_state_dict(cfg).items()}
    data, masks, eps, eps_joint, keep = case_tensors(cfg, arrays)
    out = nexus_loss(cfg, sd, data, masks, eps, eps_joint, keep, cfg["epoch"])
    out["loss"].backward()
    return out, {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in sd.items()}
