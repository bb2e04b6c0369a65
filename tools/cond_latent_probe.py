"""Time CVAE's fused latent step (mvk_cond_latent_fwd / mvk_cond_latent_bwd, one launch each way) against the composition it
replaces, built from entry points that predate it: GaussSampleKLFn (sample + KL to N(0, I)), base_utils.kl_divergence against the
prior, torch.stack + reshape + torch.cat for the decoder input.  B = 512, L = 20, C = 784, K in {1, 10}.

Two sources, both on the GPU: (1) the library's device-timestamp profiler (mvk_prof_enable): first workgroup in -> last
workgroup out of the two new launches (the composition's launches carry no profiler record); (2) HIP events around `reps`
back-to-back repetitions of each side, forward and forward + backward, after a warm-up: launch overheads included, the same for
both sides.  Launch counts come from torch.profiler's kernel list of one repetition.  Prints one JSON line per K.

    python tools/cond_latent_probe.py [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multivae_amd import _lib, kernels  # noqa: E402
from multivae_amd.models.base.base_utils import kl_divergence  # noqa: E402


def fused(eps, mu, lv, pmu, plv, cond):
    return kernels.CondLatentFn.apply(eps, mu, lv, pmu, plv, True, cond)


def composed(eps, mu, lv, pmu, plv, cond):
    K, B, L = eps.shape
    z, _ = kernels.GaussSampleKLFn.apply(eps, mu, lv)
    kl = kl_divergence(mu, lv, pmu, plv)
    c = torch.stack([cond] * K).reshape(K * B, -1)
    return torch.cat([z.reshape(K * B, L), c], dim=1).reshape(K, B, -1), kl


def timed(fn, args, gz, gk, backward, reps):
    def once():
        zc, kl = fn(*args)
        if backward:
            torch.autograd.backward([zc, kl], [gz, gk])
            for t in args[1:5]:
                t.grad = None

    for _ in range(10):
        once()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        once()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps  # microseconds per repetition


def launches(fn, args, gz, gk):
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        zc, kl = fn(*args)
        torch.cuda.synchronize()
        nf = None
        torch.autograd.backward([zc, kl], [gz, gk])
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return len(names), names


def device_records(fn, args, gz, gk, reps):
    lib = _lib.load()
    n = 4 * reps + 8
    slots = torch.zeros((n, 520), dtype=torch.int64, device="cuda")
    slots[:, 8:264:8] = -1
    kinds, work = (ctypes.c_int32 * n)(), (ctypes.c_double * n)()
    torch.cuda.synchronize()
    lib.mvk_prof_enable(ctypes.c_void_p(slots.data_ptr()), n, ctypes.cast(kinds, ctypes.c_void_p), ctypes.cast(work, ctypes.c_void_p))
    for _ in range(reps):
        zc, kl = fn(*args)
        torch.autograd.backward([zc, kl], [gz, gk])
    torch.cuda.synchronize()
    cnt = lib.mvk_prof_count()
    lib.mvk_prof_enable(None, 0, None, None)
    khz = lib.mvk_prof_clock_khz()
    s = slots[:cnt, :3].cpu()
    us = [int(s[i, 0]) / (khz * 1e3) * 1e6 for i in range(cnt) if int(s[i, 1])]
    fwd, bwd = sorted(us[0::2]), sorted(us[1::2])
    return dict(fwd_us_median=fwd[len(fwd) // 2], bwd_us_median=bwd[len(bwd) // 2], fwd_bytes=work[0], bwd_bytes=work[1], records=cnt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a GPU"
    torch.manual_seed(0)
    B, L, C = 512, 20, 784
    lines = []
    for K in (1, 10):
        mk = lambda *s: torch.randn(*s, device="cuda")
        leaves = [mk(B, L).requires_grad_(True) for _ in range(4)]
        args = (mk(K, B, L), *leaves, torch.rand(B, C, device="cuda"))
        gz, gk = mk(K, B, L + C), mk(B)
        zf, kf = fused(*args)
        zc, kc = composed(*args)
        assert torch.equal(zf[..., L:], zc[..., L:]) and torch.allclose(zf, zc, rtol=1e-5, atol=1e-6)
        assert torch.allclose(kf, kc, rtol=1e-4, atol=1e-4)
        rec = dict(B=B, L=L, C=C, K=K, reps=a.reps)
        for name, fn in (("fused", fused), ("composed", composed)):
            n, names = launches(fn, args, gz, gk)
            rec[name] = dict(kernels_fwd_bwd=n, kernel_names=names, fwd_us=timed(fn, args, gz, gk, False, a.reps),
                             fwd_bwd_us=timed(fn, args, gz, gk, True, a.reps))
        rec["fused"]["device_timestamps"] = device_records(fused, args, gz, gk, 50)
        lines.append(json.dumps(rec))
        print(lines[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
