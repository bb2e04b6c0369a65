"""Describe TELBO's two training steps on the GPU (profiles/NOTES_telbo.md): the MnistSvhn-shaped model with the default MLP
encoders / decoders and joint encoder (mnist 1x28x28, svhn 3x32x32, latent 20) at B = 256, zero_grad + forward + backward + the
fused Adam over the stage's flat buffers, as MultistageTrainer runs it eagerly.

    python tools/telbo_probe.py --stage 1|2 [--steps N] [--warmup W]      the steps alone, one JSON line with the wall time per step
                                                                        (a host clock around work that ends in a device
                                                                        synchronise); run it under a kernel-trace profiler
                                                                        (`rocprofv3 --kernel-trace --stats -d DIR -- python
                                                                        tools/telbo_probe.py ...`) for launches and kernel time
    python tools/telbo_probe.py --count                                 torch.profiler's kernel list of ONE step per stage, and of
                                                                        the fused latent step (TELBOLatentFn, forward + backward)
                                                                        beside the composition it replaces: M x GaussSampleKLFn
                                                                        plus the torch arithmetic of the joint-log-variance KL
Both are this package's code: a description, not a comparison against a baseline."""
import argparse
import collections
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multivae_amd import kernels, schedule  # noqa: E402
from multivae_amd.data.datasets.base import DatasetOutput  # noqa: E402
from multivae_amd.models import TELBO, TELBOConfig  # noqa: E402
from multivae_amd.trainers import FlatParams, FusedAdam  # noqa: E402

DIMS = dict(mnist=(1, 28, 28), svhn=(3, 32, 32))
L, B, WARMUP_EPOCHS = 20, 256, 2


def build(stage):
    torch.manual_seed(0)
    model = TELBO(TELBOConfig(n_modalities=2, latent_dim=L, input_dims=dict(DIMS), warmup=WARMUP_EPOCHS)).cuda().train()
    epoch = WARMUP_EPOCHS if stage == 1 else WARMUP_EPOCHS + 1
    flat = FlatParams(model, params=model.stage_parameters(epoch))
    opt = FusedAdam(flat, lr=1e-3, zero_grad_in_step=True)
    inputs = DatasetOutput(data={m: torch.rand(B, *d, device="cuda") for m, d in DIMS.items()})
    return model, flat, opt, inputs, epoch


def step(model, flat, opt, inputs, epoch):
    flat.zero_grad()
    with schedule.deferred_reductions(flat):
        out = model(inputs, epoch=epoch)
        out.loss.backward(gradient=kernels.unit_seed(out.loss))
    opt.step()
    return out


def kernel_names(fn):
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def latent_fused(eps, jlv, mus, lvs, gz, gk):
    out = kernels.TELBOLatentFn.apply(eps, jlv, *mus, *lvs)
    torch.autograd.backward(list(out), [gk] + list(gz))


def latent_composed(eps, jlv, mus, lvs, gz, gk):
    """What the fused launch replaces: one sample launch per modality (GaussSampleKLFn, its own KL unused) and the reference's
    arithmetic for the KL with the joint log-variance, in torch."""
    outs, grads = [], []
    for m in range(len(mus)):
        z, _ = kernels.GaussSampleKLFn.apply(eps[m:m + 1], mus[m], lvs[m])
        kld = (-0.5 * (1 + jlv - mus[m].pow(2) - lvs[m].exp())).sum(-1)
        outs += [z, kld]
        grads += [gz[m].unsqueeze(0), gk[m]]
    torch.autograd.backward(outs, grads)


def count():
    rec = dict(B=B, L=L, dims={m: list(d) for m, d in DIMS.items()})
    for stage in (1, 2):
        model, flat, opt, inputs, epoch = build(stage)
        for _ in range(5):
            step(model, flat, opt, inputs, epoch)
        names = kernel_names(lambda: step(model, flat, opt, inputs, epoch))
        rec[f"stage{stage}"] = dict(kernels_per_step=len(names), kernels_by_name=dict(collections.Counter(names).most_common()))
    M = len(DIMS)
    mk = lambda *s: torch.randn(*s, device="cuda")
    eps, jlv, gz, gk = mk(M, B, L), mk(B, L), mk(M, B, L), mk(M, B)
    for tag, fn in (("latent_fused", latent_fused), ("latent_composed", latent_composed)):
        mus, lvs = [mk(B, L).requires_grad_(True) for _ in range(M)], [mk(B, L).requires_grad_(True) for _ in range(M)]
        for _ in range(3):
            fn(eps, jlv, mus, lvs, gz, gk)
        names = kernel_names(lambda: fn(eps, jlv, mus, lvs, gz, gk))
        rec[tag] = dict(kernels=len(names), kernels_by_name=dict(collections.Counter(names).most_common()))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stage", type=int, choices=(1, 2), default=2)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--count", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a GPU"
    if a.count:
        rec = count()
    else:
        model, flat, opt, inputs, epoch = build(a.stage)
        for _ in range(a.warmup):
            step(model, flat, opt, inputs, epoch)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            out = step(model, flat, opt, inputs, epoch)
        torch.cuda.synchronize()
        rec = dict(stage=a.stage, B=B, L=L, steps=a.steps, warmup=a.warmup, step_ms=(time.perf_counter() - t0) * 1e3 / a.steps,
                   loss=float(out.loss.detach()), trained_floats=int(flat.numel))
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
