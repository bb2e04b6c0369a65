"""One CMVAE (or MMVAE+) training step at the same MnistSvhn-like shape, repeated, for a kernel trace:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o NAME -- python tools/cmvae_probe.py cmvae
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o NAME -- python tools/cmvae_probe.py mmvaeplus
    python tools/cmvae_probe.py summary OUT/.../NAME_kernel_stats.csv [STEPS]    # launch list: calls per step, average ns

Default multi-latent MLPs, mnist (1, 28, 28) + svhn (3, 32, 32), B = 128, K = 10, latent_dim = 20, modalities_specific_dim = 8, CMVAE
with 10 clusters, Laplace / DReG (the defaults of both configurations); eager forward + backward, no optimiser, STEPS = 20 steps after
3 warm-up steps (the warm-up steps are in the trace as well: divide by STEPS + 3).  Also runs predict_clusters once per step for
CMVAE so that mvk_cmvae_assign's launch is in the trace.  Results: profiles/NOTES_cmvae.md."""
import csv
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
STEPS, WARMUP = 20, 3


def summary(path, steps):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: -float(r["TotalDurationNs"]))
    print(f"{'kernel':70s} {'calls/step':>10s} {'avg us':>8s} {'us/step':>8s}")
    total = 0.0
    for r in rows:
        calls, tot = int(r["Calls"]), float(r["TotalDurationNs"])
        total += tot / steps / 1e3
        print(f"{r['Name'][:70]:70s} {calls / steps:10.2f} {tot / calls / 1e3:8.2f} {tot / steps / 1e3:8.1f}")
    print(f"launches per step {sum(int(r['Calls']) for r in rows) / steps:.1f}, device time per step {total:.1f} us")


def main():
    if sys.argv[1] == "summary":
        return summary(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else STEPS + WARMUP)
    import torch

    from multivae_amd.data.datasets.base import DatasetOutput
    from multivae_amd.models import CMVAE, CMVAEConfig, MMVAEPlus, MMVAEPlusConfig

    d = torch.device("cuda:0")
    torch.manual_seed(0)
    dims = dict(mnist=(1, 28, 28), svhn=(3, 32, 32))
    kw = dict(n_modalities=2, latent_dim=20, input_dims=dims, K=10, modalities_specific_dim=8)
    model = (CMVAE(CMVAEConfig(number_of_clusters=10, **kw)) if sys.argv[1] == "cmvae" else MMVAEPlus(MMVAEPlusConfig(**kw))).to(d).train()
    inputs = DatasetOutput(data={m: torch.rand(128, *s, device=d) for m, s in dims.items()})
    for _ in range(WARMUP + STEPS):
        model.zero_grad(set_to_none=True)
        out = model(inputs)
        out.loss.backward()
        if sys.argv[1] == "cmvae":
            model.predict_clusters(inputs, compute_lliks=True)
    torch.cuda.synchronize()
    print(sys.argv[1], "loss", float(out.loss.detach()))


if __name__ == "__main__":
    main()
