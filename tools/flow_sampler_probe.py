"""Time the flow samplers' two hot paths on the GPU, the fused kernels beside the plain torch flow modules
(profiles/NOTES_flow_samplers.md), for a MAF and an IAF:

    1. one fit step of samplers/flow_fit.py on B codes: forward with the NLL rows, backward and Adam (fused: mvk_maf_fwd/bwd or
       mvk_iaf_fwd/bwd and one mvk_adam_step_fused launch over the flat buffer; modules: the flow under autograd and
       torch.optim.Adam);
    2. the flow's inverse on R rows, what `sample` runs (kernels.maf_inverse / iaf_inverse against `flow.inverse`).

    python tools/flow_sampler_probe.py [--B 64] [--D 20] [--H 128] [--rows 1000] [--reps 15] [--inner 5]

Each item: `reps` rounds that alternate the two forms; in a round each form runs `inner` times between two device events (after a
warm-up of both); per form the median over the rounds of the time per call and the 10th / 90th percentile.  Both forms start from
the same seeded parameters and codes, and their first step's loss (inverse: their outputs) is compared first.  One JSON line per
item.  No GPU: an error, not a fallback."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multivae_amd import kernels  # noqa: E402
from multivae_amd.models.nn.flows import IAF, MAF, IAFConfig, MAFConfig  # noqa: E402
from multivae_amd.samplers import flow_fit  # noqa: E402
from multivae_amd.trainers import BaseTrainerConfig  # noqa: E402


def alternate(forms, reps, inner):
    """forms: {name: callable} -> {name: (median, p10, p90)} in microseconds per call."""
    for f in forms.values():
        for _ in range(3):
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
    return float((a - b).abs().max() / b.abs().max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--D", type=int, default=20)
    ap.add_argument("--H", type=int, default=128)
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("flow_sampler_probe needs the GPU")
    dev = torch.device("cuda:0")
    cfg = BaseTrainerConfig(learning_rate=1e-4)
    for name, Flow, Config in (("MAF", MAF, MAFConfig), ("IAF", IAF, IAFConfig)):
        flows = []
        for _ in range(2):
            torch.manual_seed(0)
            flows.append(Flow(Config(input_dim=(a.D,), hidden_size=a.H)).to(dev))
        x = torch.randn(a.B, a.D, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 0.8
        fused = flow_fit._Fused(flows[0], *flow_fit.flow_dims(flows[0]), cfg)
        module = flow_fit._Module(flows[1], cfg)
        diff = rel(fused.step(x).sum(), module.step(x).sum())
        t = alternate(dict(fused=lambda: fused.step(x), modules=lambda: module.step(x)), a.reps, a.inner)
        print(json.dumps(dict(item=f"{name} fit step", B=a.B, D=a.D, H=a.H, first_loss_rel_diff=diff,
                              us={k: [round(v, 1) for v in w] for k, w in t.items()})), flush=True)
        y = torch.randn(a.rows, a.D, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
        dims, Ws, bs = flow_fit.flow_dims(flows[0])
        Ws, bs = [w.detach() for w in Ws], [b.detach() for b in bs]
        inverse = kernels.maf_inverse if Flow is MAF else kernels.iaf_inverse

        def inv_fused():
            return inverse(y, dims, Ws, bs)[0]

        def inv_modules():
            with torch.no_grad():
                return flows[0].inverse(y).out

        diff = rel(inv_fused(), inv_modules())
        t = alternate(dict(fused=inv_fused, modules=inv_modules), a.reps, a.inner)
        print(json.dumps(dict(item=f"{name} inverse", rows=a.rows, D=a.D, H=a.H, max_rel_diff=diff,
                              us={k: [round(v, 1) for v in w] for k, w in t.items()})), flush=True)


if __name__ == "__main__":
    main()
