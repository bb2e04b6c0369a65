"""Timing of one SSIM evaluation on the fused kernel (csrc/ssim.hip) against the same definition written in torch, on the same GPU.

    python tools/ssim_probe.py [--pairs 10000] [--batch 512] [--shapes 1x28x28,3x32x32] [--reps 30] [--out FILE.json]

An evaluation is what metrics.Reconstruction does for one modality: the image pairs in batches of --batch, per batch the data
range, the per-image SSIM and the accumulation, and ONE host read at the end.  The kernel path is mvk_ssim_range, mvk_ssim_rows and
mvk_ssim_accumulate per batch; the torch path is DESIGN.md's definition as torchmetrics lays it out (a grouped conv2d over the
five-fold concatenation [p, t, pp, tt, pt] and elementwise launches), also without a host read per batch.  The parent commit has
no SSIM, so the torch form is the comparison.  Both paths are warmed up, then timed alternately --reps times with a host clock
around evaluation + synchronise; the median and the spread are reported.  The rows entry alone (tile kernel + per-image finish,
HIP events around back-to-back calls on one batch) gives the bytes it has to read -- both images once -- as a share of the
measured HBM copy rate.  Needs a GPU; prints one JSON line per shape.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HBM_MEASURED = 6.29e12  # bytes / s, float4 copy on an MI355X (8.0e12 is the datasheet value)


def torch_window(C, device):
    i = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-0.5 * (i / 1.5) ** 2)
    g = (g / g.sum()).float()
    return torch.outer(g, g).expand(C, 1, 11, 11).contiguous().to(device)


def torch_evaluation(batches, window):
    """sum of per-image SSIM / images, all on the device; one read at the end."""
    total = torch.zeros((), dtype=torch.float64, device=window.device)
    rows = 0
    for p, t in batches:
        B, C = p.shape[:2]
        R = torch.maximum(p.max() - p.min(), t.max() - t.min())
        c1, c2 = (0.01 * R) ** 2, (0.03 * R) ** 2
        out = F.conv2d(torch.cat([p, t, p * p, t * t, p * t]), window, groups=C)
        mp, mt, pp, tt, pt = out.split(B)
        vp, vt, cv = pp - mp * mp, tt - mt * mt, pt - mp * mt
        ssim = ((2 * mp * mt + c1) * (2 * cv + c2)) / ((mp * mp + mt * mt + c1) * (vp + vt + c2))
        total += ssim.reshape(B, -1).mean(1).double().sum()
        rows += B
    return float(total / rows)


def kernel_evaluation(batches, K, scratch):
    acc = K.ssim_new_acc(batches[0][0].device)
    for p, t in batches:
        ssim, sse = K.ssim_rows(p, t, scratch[p.shape[0]])
        K.ssim_accumulate(acc, sse, ssim)
    a = acc.cpu()
    return float(a[0] / a[2])


def clocked(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    v = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10000)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--shapes", default="1x28x28,3x32x32")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ssim_probe needs a GPU"
    from multivae_amd import kernels as K

    dev = torch.device("cuda:0")
    lines = []
    for spec in a.shapes.split(","):
        C, H, W = (int(v) for v in spec.split("x"))
        g = torch.Generator(device=dev).manual_seed(0)
        target = torch.rand(a.pairs, C, H, W, generator=g, device=dev)
        preds = (target + 0.1 * torch.randn(a.pairs, C, H, W, generator=g, device=dev)).clamp(0, 1)
        batches = [(preds[i:i + a.batch], target[i:i + a.batch]) for i in range(0, a.pairs, a.batch)]
        scratch = {n: K.ssim_scratch(n, C, H, W, dev) for n in {len(p) for p, _ in batches}}
        window = torch_window(C, dev)
        for _ in range(3):
            vk, vt = kernel_evaluation(batches, K, scratch), torch_evaluation(batches, window)
        tk, tt = [], []
        for _ in range(a.reps):  # alternating, so that a drift of the machine hits both
            tk.append(clocked(lambda: kernel_evaluation(batches, K, scratch))[0])
            tt.append(clocked(lambda: torch_evaluation(batches, window))[0])
        # the rows entry alone on one full batch
        p, t = batches[0]
        rng = K.ssim_range(p, t, scratch[len(p)])
        n_calls = 200
        for _ in range(10):
            K.ssim_rows(p, t, scratch[len(p)], data_range=rng)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n_calls):
            K.ssim_rows(p, t, scratch[len(p)], data_range=rng)
        e1.record()
        torch.cuda.synchronize()
        rows_s = e0.elapsed_time(e1) * 1e-3 / n_calls
        nbytes = 2 * p.numel() * 4
        med = statistics.median
        line = dict(shape=[C, H, W], pairs=a.pairs, batch=a.batch, updates=len(batches), reps=a.reps,
                    kernel_eval_ms=dict(median=1e3 * med(tk), min=1e3 * min(tk), max=1e3 * max(tk)),
                    torch_eval_ms=dict(median=1e3 * med(tt), min=1e3 * min(tt), max=1e3 * max(tt)),
                    torch_over_kernel=med(tt) / med(tk), value_kernel=vk, value_torch=vt,
                    rows_entry_us=1e6 * rows_s, rows_entry_bytes=nbytes, rows_entry_bytes_per_s=nbytes / rows_s,
                    rows_entry_share_of_hbm_copy_rate=nbytes / rows_s / HBM_MEASURED)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
