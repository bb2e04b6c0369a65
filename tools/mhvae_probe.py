"""Describe one MHVAE training step on the GPU with subset batching on and off (profiles/NOTES_mhvae.md): a 3-modality, 3-level
hierarchy of Linear + SiLU blocks at B = 256 (inputs 784 / 784 / 256, latents 128 / 64 / 32), zero_grad + forward + backward + Adam.

Three sources: (1) a host clock around `steps` steps that end in a device synchronise, after a warm-up, the two settings alternated
over `rounds` rounds (the spread between rounds is printed with the medians); (2) torch.profiler's kernel list of ONE step per
setting: the launch counts by kernel name; (3) the profiler's device durations of the two level kernels over `prof_steps` steps, and
HIP events around back-to-back MHVAELevelFn calls at the model's level shapes (these include the launch overhead).  Both settings
are this package's code: a description, not a comparison against a baseline.  Prints one JSON line.

    python tools/mhvae_probe.py [--out FILE]"""
import argparse
import collections
import json
import os
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multivae_amd import kernels  # noqa: E402
from multivae_amd.data.datasets.base import DatasetOutput  # noqa: E402
from multivae_amd.models import MHVAE, MHVAEConfig  # noqa: E402
from multivae_amd.models.base.base_utils import ModelOutput  # noqa: E402
from multivae_amd.models.nn.base_architectures import BaseDecoder, BaseEncoder  # noqa: E402

DIMS = dict(m1=(784,), m2=(784,), m3=(256,))
LEVELS = (128, 64, 32)  # sizes of z_1, z_2, z_3


class Enc(BaseEncoder):
    def __init__(self, n_in, n_out):
        BaseEncoder.__init__(self)
        self.fc = nn.Linear(n_in, n_out)

    def forward(self, x):
        return ModelOutput(embedding=nn.functional.silu(self.fc(x.reshape(x.shape[0], -1))))


class Up(nn.Module):
    def __init__(self, n_in, n_out):
        nn.Module.__init__(self)
        self.fc = nn.Linear(n_in, n_out)

    def forward(self, x):
        return nn.functional.silu(self.fc(x))


class Gauss(BaseEncoder):
    def __init__(self, n_in, n_out):
        BaseEncoder.__init__(self)
        self.mu, self.lv = nn.Linear(n_in, n_out), nn.Linear(n_in, n_out)

    def forward(self, x):
        return ModelOutput(embedding=self.mu(x), log_covariance=self.lv(x))


class Dec(BaseDecoder):
    def __init__(self, n_in, shape):
        BaseDecoder.__init__(self)
        self.shape, self.fc = shape, nn.Linear(n_in, int(torch.Size(shape).numel()))

    def forward(self, z):
        return ModelOutput(reconstruction=torch.sigmoid(self.fc(z)).reshape(-1, *self.shape))


def build():
    n = lambda d: int(torch.Size(d).numel())
    L = len(LEVELS)
    cfg = MHVAEConfig(n_modalities=len(DIMS), latent_dim=LEVELS[-1], input_dims=dict(DIMS), n_latent=L)
    return MHVAE(cfg, encoders={m: Enc(n(d), LEVELS[0]) for m, d in DIMS.items()},
                 decoders={m: Dec(LEVELS[0], d) for m, d in DIMS.items()},
                 bottom_up_blocks={m: [Up(LEVELS[i], LEVELS[i + 1]) for i in range(L - 2)] + [Gauss(LEVELS[L - 2], LEVELS[L - 1])]
                                   for m in DIMS},
                 top_down_blocks=[Up(LEVELS[i + 1], LEVELS[i]) for i in range(L - 1)],
                 posterior_blocks=[Gauss(2 * LEVELS[i], LEVELS[i]) for i in range(L - 1)],
                 prior_blocks=[Gauss(LEVELS[i], LEVELS[i]) for i in range(L - 1)])


def step(model, opt, inputs):
    opt.zero_grad(set_to_none=True)
    out = model(inputs)
    out.loss.backward()
    opt.step()
    return out


def wall_ms(model, opt, inputs, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step(model, opt, inputs)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def kernel_list(model, opt, inputs, steps=1):
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        for _ in range(steps):
            step(model, opt, inputs)
        torch.cuda.synchronize()
    return [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def level_events(S, B, F, shared, reps):
    E = 3
    member = [1, 2, 4, 3, 5, 6, 7][:S]
    mk = lambda *s: torch.randn(*s, device="cuda")
    count = lambda e: 1 if shared else sum(1 for m in member if m >> e & 1)
    leaves = [mk(count(e // 2), B, F).requires_grad_(True) for e in range(2 * E)]
    prior = [None, None] if shared else [mk(S, B, F).requires_grad_(True), mk(S, B, F).requires_grad_(True)]
    eps, gz, gk = mk(S, B, F), mk(S, B, F), mk(S, B)
    res = {}
    for backward in (False, True):
        def once():
            z, kl = kernels.MHVAELevelFn.apply(eps, member, shared, None, B, F, *prior, *leaves)
            if backward:
                torch.autograd.backward([z, kl], [gz, gk])
                for t in leaves + [p for p in prior if p is not None]:
                    t.grad = None

        for _ in range(20):
            once()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            once()
        e1.record()
        torch.cuda.synchronize()
        res["fwd_bwd_us" if backward else "fwd_us"] = e0.elapsed_time(e1) * 1e3 / reps
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--prof-steps", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a GPU"
    torch.manual_seed(0)
    B = 256
    model = build().cuda().train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    inputs = DatasetOutput(data={m: torch.rand(B, *d, device="cuda") for m, d in DIMS.items()})
    rec = dict(B=B, dims={m: list(d) for m, d in DIMS.items()}, levels=list(LEVELS), steps=a.steps, rounds=a.rounds)
    wall = {True: [], False: []}
    for on in (True, False):  # warm every shape of both settings
        model.subset_batching = on
        wall_ms(model, opt, inputs, 20)
    for _ in range(a.rounds):
        for on in (True, False):
            model.subset_batching = on
            wall[on].append(wall_ms(model, opt, inputs, a.steps))
    for on in (True, False):
        model.subset_batching = on
        key = "batched" if on else "per_subset"
        ev = kernel_list(model, opt, inputs)
        names = collections.Counter(e.name for e in ev)
        many = kernel_list(model, opt, inputs, a.prof_steps)
        lvl = {}
        for tag in ("mhvae_level_fwd_kernel", "mhvae_level_bwd_kernel"):
            d = sorted(e.device_time for e in many if tag in e.name)
            lvl[tag] = dict(launches_per_step=len(d) / a.prof_steps, median_us=d[len(d) // 2] if d else None,
                            sum_per_step_us=sum(d) / a.prof_steps)
        rec[key] = dict(step_ms_rounds=wall[on], step_ms_median=sorted(wall[on])[len(wall[on]) // 2], kernels_per_step=len(ev),
                        kernels_by_name=dict(names.most_common()), level_kernels_profiler=lvl)
    rec["level_launch_events"] = {"top_shared_S7_B256_F32": level_events(7, B, LEVELS[2], True, 500),
                                  "own_S7_B256_F64": level_events(7, B, LEVELS[1], False, 500),
                                  "own_S7_B256_F128": level_events(7, B, LEVELS[0], False, 500)}
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
