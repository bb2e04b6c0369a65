"""Generate tests/golden/convmmnist_*.npz by running the REAL reference classes EncoderConvMMNIST, EncoderConvMMNIST_adapted,
EncoderConvMMNIST_multilatents and DecoderConvMMNIST (multivae/models/nn/mmnist.py:36-206).  Runs only where the reference is
readable (tests/golden/_reference_import.py), like make_golden.py, whose helpers it imports:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_convmmnist_golden.py

For every case: procedural weights (procedural.make_state_dict over convmmnist_ref.shapes) loaded through load_state_dict, seeded
images [B, 3, 28, 28] and latents ([B, L] and [K, B, L]), a fixed random projection loss, forward + backward in fp32.  Stored:
the outputs, dz, the grad_stats of every parameter gradient with the gradient's largest magnitude, the reference's state-dict
keys and shapes, the output shapes at n = 1 (the reference's squeezes), and the distance of the reference's fp32 results from
the float64 evaluation of tests/convmmnist_ref.py (relative to each tensor's largest magnitude).

Seeds: the case's seed is the first one from seed0 at which, in the float64 evaluation, every ReLU pre-activation lies further from
zero than its own entry bound C_ENTRY * op(|a|, |b|) (convmmnist_ref.Margin).  The script asserts it and stores the smallest margin:
the fixture's ReLU masks are then those of any evaluation within the entry bound, and gradients compare entry by entry.
The fixtures hold arrays and JSON settings only.
"""
import sys

sys.dont_write_bytecode = True
import os
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np
import torch

import make_golden as MG  # installs the reference import
import procedural as P

import convmmnist_ref as CR

t = MG.t
KINDS = ("conv", "adapted", "multi")
OUT_NAMES = ("mu", "lv", "smu", "slv")


inputs, state_dicts = CR.golden_inputs, CR.golden_state_dicts


def sd64(sd_np, grad=True):
    return {k: t(v).double().requires_grad_(grad) for k, v in sd_np.items()}


def rel(a, b):
    """max |a - b| / max |b|."""
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-300))


def margin_of(seed, B, K, L, S):
    x, z2, z3, *_ = inputs(seed, B, K, L, S)
    sds = state_dicts(seed, L, S)
    m = CR.Margin()
    with torch.no_grad():
        for k in KINDS:
            CR.encoder64(k, sd64(sds[k], False), t(x).double(), m)
        CR.decoder64(sd64(sds["dec"], False), t(z2).double(), m)
        CR.decoder64(sd64(sds["dec"], False), t(z3).double(), m)
    return m


def case(name, *, B, K, L, S, seed0):
    from multivae.models.nn.mmnist import DecoderConvMMNIST, EncoderConvMMNIST, EncoderConvMMNIST_adapted, EncoderConvMMNIST_multilatents

    print(name)
    for seed in range(seed0, seed0 + 64):
        m = margin_of(seed, B, K, L, S)
        if m.margin > 0:
            break
    else:
        raise AssertionError("no seed keeps every ReLU unit outside its entry bound")
    print(f"  seed {seed}: {m.units} ReLU units, smallest |pre| - C_ENTRY * bound = {m.margin:.3e}")
    cfgo = types.SimpleNamespace(latent_dim=L, style_dim=S)
    classes = dict(conv=EncoderConvMMNIST, adapted=EncoderConvMMNIST_adapted, multi=EncoderConvMMNIST_multilatents, dec=DecoderConvMMNIST)
    x, z2, z3, pe, pd2, pd3 = inputs(seed, B, K, L, S)
    sds = state_dicts(seed, L, S)
    arrays, dist, keys, n1 = {}, {}, {}, {}
    for k in KINDS:
        model = classes[k](cfgo)
        keys[k] = [[n_, list(v.shape)] for n_, v in model.state_dict().items()]
        assert keys[k] == [[n_, list(s)] for n_, s in CR.shapes(k, L, S).items()], k
        model.load_state_dict({n_: t(v) for n_, v in sds[k].items()})
        o = model(t(x))
        outs = [o[n_] for n_ in ("embedding", "log_covariance", "style_embedding", "style_log_covariance") if n_ in o]
        sum((a * t(p)).sum() for a, p in zip(outs, pe)).backward()
        with torch.no_grad():
            n1[k] = [list(v.shape) for v in model(t(x[:1])).values()]
        s64 = sd64(sds[k])
        o64 = CR.encoder64(k, s64, t(x).double())
        sum((a * t(p).double()).sum() for a, p in zip(o64, pe)).backward()
        for a, a64, nme in zip(outs, o64, OUT_NAMES):
            arrays[f"{k}.{nme}"] = a.detach()
            dist[f"{k}.{nme}"] = rel(a.detach(), a64.detach())
        grads = {f"{k}.{n_}": p.grad for n_, p in model.named_parameters()}
        for n_, p in model.named_parameters():
            dist[f"{k}.{n_}"] = rel(p.grad, s64[n_].grad)
            arrays[f"gmax/{k}.{n_}"] = np.array([float(p.grad.abs().max())])
        arrays.update(MG.grad_stats(grads))
    dec = classes["dec"](cfgo)
    keys["dec"] = [[n_, list(v.shape)] for n_, v in dec.state_dict().items()]
    assert keys["dec"] == [[n_, list(s)] for n_, s in CR.shapes("dec", L, S).items()]
    dec.load_state_dict({n_: t(v) for n_, v in sds["dec"].items()})
    for tag, z_np, pd in (("dec2", z2, pd2), ("dec3", z3, pd3)):
        dec.zero_grad()
        z = t(z_np).requires_grad_(True)
        rec = dec(z).reconstruction
        assert tuple(rec.shape) == tuple(z.shape[:-1]) + (3, 28, 28)
        (rec * t(pd)).sum().backward()
        s64 = sd64(sds["dec"])
        z64 = t(z_np).double().requires_grad_(True)
        r64 = CR.decoder64(s64, z64)
        (r64 * t(pd).double()).sum().backward()
        r = rec.detach()
        arrays[f"{tag}.recon_sample"] = r.reshape(-1)[P.hash_indices(r.numel(), 512, 77)]
        arrays[f"{tag}.recon_sum"] = np.array([float(r.double().sum()), float(r.double().abs().sum()), float(r.abs().max())])
        arrays[f"{tag}.dz"] = z.grad.detach()
        dist[f"{tag}.recon"], dist[f"{tag}.dz"] = rel(r, r64.detach()), rel(z.grad, z64.grad)
        for n_, p in dec.named_parameters():
            dist[f"{tag}.{n_}"] = rel(p.grad, s64[n_].grad)
            arrays[f"gmax/{tag}.{n_}"] = np.array([float(p.grad.abs().max())])
        arrays.update(MG.grad_stats({f"{tag}.{n_}": p.grad.clone() for n_, p in dec.named_parameters()}))
    print(f"  largest fp32-to-float64 distance: {max(dist.values()):.3e}")
    MG.save(name, dict(model="ConvMMNIST", B=B, K=K, L=L, S=S, seed=seed, relu_margin=m.margin, relu_units=m.units, keys=keys,
                       shapes_n1=n1, dist=dist), arrays)


def main():
    case("convmmnist_L5_S3", B=3, K=2, L=5, S=3, seed0=4100)
    case("convmmnist_L64_S0", B=2, K=2, L=64, S=0, seed0=4200)
    case("convmmnist_L512_S0", B=2, K=1, L=512, S=0, seed0=4300)


if __name__ == "__main__":
    main()
