"""Per-step time of a Nexus training step (forward, backward, fused Adam) on MnistSvhn-shaped synthetic batches.

    python tools/nexus_step.py [--batch 512] [--steps 50] [--warmup 10]

Prints ONE JSON line: for dropout_rate in {0, 0.2} x adapt_top_decoder_variance off / on ("svhn"), the eager step and the
hipGraph-replayed step (GraphedStep, Adam behind the replay), each as ms per step (median of per-step device events) and
samples / s.  Default MLP architectures (the reference's defaults), latent 20, first-level latents 16 / 20, msg_dim 10."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def measure(step, steps, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    marks[0].record()
    for i in range(steps):
        out = step()
        marks[i + 1].record()
    torch.cuda.synchronize()
    ms = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(steps))
    loss = float(out.loss.detach())
    if loss != loss:
        raise ArithmeticError("NaN loss")
    return ms[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    from multivae_amd import kernels
    from multivae_amd.data.datasets.base import DatasetOutput
    from multivae_amd.models import Nexus, NexusConfig
    from multivae_amd.trainers import FlatParams, FusedAdam, GraphedStep

    d = torch.device("cuda:0")
    B = args.batch
    g = torch.Generator().manual_seed(0)
    inputs = DatasetOutput(data=dict(mnist=torch.rand(B, 1, 28, 28, generator=g).to(d),
                                     svhn=torch.rand(B, 3, 32, 32, generator=g).to(d)))
    res = dict(metric="nexus_train_step", batch=B, device=torch.cuda.get_device_name(d), configs=[])
    for dropout in (0.0, 0.2):
        for adapt in (None, ["svhn"]):
            torch.manual_seed(0)
            model = Nexus(NexusConfig(n_modalities=2, latent_dim=20, input_dims=dict(mnist=(1, 28, 28), svhn=(3, 32, 32)),
                                      modalities_specific_dim=dict(mnist=16, svhn=20), dropout_rate=dropout,
                                      adapt_top_decoder_variance=adapt)).to(d).train()
            flat = FlatParams(model)
            opt = FusedAdam(flat, lr=1e-4)

            def eager():
                opt.zero_grad()
                out = model(inputs, epoch=25)
                out.loss.backward(gradient=kernels.unit_seed(out.loss))
                opt.step()
                return out

            t_eager = measure(eager, args.steps, args.warmup)
            gs = GraphedStep(model, flat, inputs, epoch=25)

            def graphed():
                out = gs(inputs)
                opt.step()
                return out

            t_graph = measure(graphed, args.steps, args.warmup)
            res["configs"].append(dict(dropout_rate=dropout, adapt=bool(adapt), eager_ms=round(t_eager, 4),
                                       eager_samples_per_s=round(B / t_eager * 1e3, 1), graph_ms=round(t_graph, 4),
                                       graph_samples_per_s=round(B / t_graph * 1e3, 1)))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
