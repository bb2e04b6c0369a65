"""Time the CUB text encoder on the GPU, the fused path (kernels.TextEncoderFn: csrc/textenc.hip + the tiled GEMM engine) beside the
same module's torch path (profiles/NOTES_textenc.md):

    1. a training step's forward + backward of CubTextEncoder on B sentences (dropout p, every parameter's gradient);
    2. the evaluation forward (eval mode, no autograd: padded rows zeroed);
    3. with --stages: each stage of csrc/textenc.hip alone at the same shape.

    python tools/textenc_probe.py [--B 64 128] [--S 32] [--E 512] [--nhead 4] [--F 1024] [--layers 4] [--V 1590] [--p 0.5]
                                  [--reps 30] [--inner 10] [--stages]

Each item: `reps` rounds that alternate the two forms; in a round each form runs `inner` times between two device events (after a
warm-up of both); per form the median over the rounds of the time per call and the 10th / 90th percentile.  Both forms hold the same
parameters; at p = 0 their outputs and gradients are compared first (largest difference relative to the largest entry).  One JSON
line per item.  No GPU: an error, not a fallback."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multivae_amd import kernels  # noqa: E402
from multivae_amd.models.nn.cub import CubTextEncoder  # noqa: E402


def alternate(forms, reps, inner):
    """forms: {name: callable} -> {name: (median, p10, p90)} in microseconds per call."""
    for f in forms.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(reps):
        for k, f in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                f()
            e1.record()
            e1.synchronize()
            times[k].append(1e3 * e0.elapsed_time(e1) / inner)
    out = {}
    for k, v in times.items():
        v = sorted(v)
        out[k] = (v[len(v) // 2], v[len(v) // 10], v[(9 * len(v)) // 10])
    return out


def rel(a, b):
    a, b = a.detach(), b.detach()
    return float((a - b).abs().max() / b.abs().max())


def us(t):
    return {k: [round(x, 1) for x in v] for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--S", type=int, default=32)
    ap.add_argument("--E", type=int, default=512)
    ap.add_argument("--nhead", type=int, default=4)
    ap.add_argument("--F", type=int, default=1024)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--V", type=int, default=1590)
    ap.add_argument("--p", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--stages", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("textenc_probe needs the GPU")
    dev = torch.device("cuda:0")
    for B in a.B:
        torch.manual_seed(0)
        enc = CubTextEncoder(64, a.S, a.V, a.E, a.nhead, a.F, a.layers, a.p).to(dev)
        tok = torch.randint(0, a.V, (B, a.S), device=dev)
        pm = (torch.arange(a.S, device=dev)[None, :] < torch.randint(1, a.S + 1, (B, 1), device=dev)).float()
        x = dict(tokens=tok, padding_mask=pm)
        params = list(enc.parameters())
        shape = dict(B=B, S=a.S, E=a.E, nhead=a.nhead, F=a.F, layers=a.layers, V=a.V, p=a.p)

        def step(fused):
            enc.use_fused = "always" if fused else False
            for q in params:
                q.grad = None
            o = enc(x)
            (o.embedding.sum() + o.log_covariance.sum()).backward()
            return o

        diff = None
        for m in enc.modules():  # the comparison runs without dropout
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
        for l in enc.transformer_encoder.layers:
            l.self_attn.dropout = 0.0
        enc.train()
        o1 = step(True)
        g1 = [q.grad.clone() for q in params]
        o2 = step(False)
        diff = max([rel(o1.transformer_output, o2.transformer_output)] + [rel(g, q.grad) for g, q in zip(g1, params)])
        for m in enc.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = a.p
        for l in enc.transformer_encoder.layers:
            l.self_attn.dropout = a.p
        t = alternate(dict(fused=lambda: step(True), torch=lambda: step(False)), a.reps, a.inner)
        print(json.dumps(dict(item="encoder fwd+bwd", **shape, max_rel_diff_p0=diff, us=us(t))), flush=True)

        enc.eval()

        def ev(fused):
            enc.use_fused = "always" if fused else False
            with torch.no_grad():
                return enc(x).embedding

        t = alternate(dict(fused=lambda: ev(True), torch=lambda: ev(False)), a.reps, a.inner)
        print(json.dumps(dict(item="encoder eval forward", **shape, us=us(t))), flush=True)

        if a.stages:
            M, E, F, nh, S = B * a.S, a.E, a.F, a.nhead, a.S
            u = torch.rand(max(M * F, B * nh * S * S), device=dev)
            qkv, h, g = torch.randn(B, S, 3 * E, device=dev), torch.randn(B, S, E, device=dev), torch.randn(B, S, E, device=dev)
            km = pm.to(torch.int32)
            ctx, P = kernels.txt_attn_fwd(qkv, nh, km, u, a.p)
            y, z, mean, rstd = kernels.txt_add_ln_fwd(h, g, None, None, 1e-5, u, a.p)
            gam, dg, db = torch.ones(E, device=dev), torch.zeros(E, device=dev), torch.zeros(E, device=dev)
            emb, pe, ff = enc.token_embedding.weight.detach(), enc.pos_encoder.pe[0], torch.randn(M, F, device=dev)
            forms = {
                "embed_fwd": lambda: kernels.txt_embed_fwd(tok, emb, pe, u, a.p),
                "embed_bwd": lambda: kernels.txt_embed_bwd(tok, g, a.V, None, u, a.p),
                "attn_fwd": lambda: kernels.txt_attn_fwd(qkv, nh, km, u, a.p),
                "attn_bwd": lambda: kernels.txt_attn_bwd(qkv, P, g, nh, u, a.p),
                "add_ln_fwd": lambda: kernels.txt_add_ln_fwd(h, g, gam, gam, 1e-5, u, a.p),
                "add_ln_bwd": lambda: kernels.txt_add_ln_bwd(g, z, mean, rstd, gam, None, u, a.p, dgamma=dg, dbeta=db),
                "drop": lambda: kernels.txt_drop(ff, u, a.p),
            }
            t = alternate(forms, a.reps, a.inner)
            print(json.dumps(dict(item="stages", **shape, us=us(t))), flush=True)


if __name__ == "__main__":
    main()
