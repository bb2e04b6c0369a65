"""Timing of one picture on the fused launch (csrc/grid.hip) against the plain-torch path of kernels.image_grid, on the same GPU, and the
CPU census of what an fma-contracted quantisation would change.

    python tools/grid_probe.py [--n-data 8] [--n 8] [--mods 5] [--shape 3x28x28] [--reps 30] [--out FILE.json]
    python tools/grid_probe.py --census [--out FILE.json]

A picture is what BaseTrainer.predict makes for `recon_from_all` on PolyMNIST: --mods sources of [n_data, *shape] (the true data)
and --mods of [N n_data, *shape] (the generations), nrow = n_data; the bytes are read back to the host, as for the PNG.  Three
paths, warmed up and then timed alternately --reps times with a host clock around call + host read (which synchronises); median
and spread are reported:
  fused        kernels.image_grid on the contiguous fp32 tensors: one launch, one host read of the uint8 image;
  torch        kernels._image_grid_torch on the same tensors: adapt_shape, cat, the grid from the padded cells, the quantisation;
  tile by tile the reference's form (a copy per tile into a pad-valued grid, then mul / add / clamp / permute / cast).
The launch alone is timed with device events around back-to-back calls, and the bytes it has to move -- every source pixel read at
least once, both outputs written once -- are given as a share of the measured HBM copy rate.  Needs a GPU.

--census needs none: every float32 x in [0, 1] goes through b = trunc(clamp(fl(fl(255 x) + 0.5))) and through the contracted
b' = trunc(clamp(fl(255 x + 0.5))), and the inputs with b != b' are counted.  255 x + 0.5 is exact in float64 for x >= 2^-10 (41
significant bits), so fl() of the float64 value IS the fma; below 2^-10 both forms lie in [0.5, 0.75] and give 0."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HBM_MEASURED = 6.29e12  # bytes / s, float4 copy on an MI355X (8.0e12 is the datasheet value)


def census(chunk=1 << 24):
    one = int(np.float32(1.0).view(np.uint32))
    differ, first, total = 0, [], 0
    for lo in range(0, one + 1, chunk):
        bits = np.arange(lo, min(lo + chunk, one + 1), dtype=np.uint32)
        x = bits.view(np.float32)
        two = (x * np.float32(255.0)).astype(np.float32) + np.float32(0.5)  # numpy rounds every float32 operation
        fused = (x.astype(np.float64) * 255.0 + 0.5).astype(np.float32)
        small = x < np.float32(2.0 ** -10)
        assert not small.any() or (float(two[small].max()) < 0.75 and float(fused[small].max()) < 0.75)
        b2 = np.clip(two, 0, 255).astype(np.uint8)
        b1 = np.clip(fused, 0, 255).astype(np.uint8)
        bad = np.nonzero(b1 != b2)[0]
        differ += len(bad)
        total += len(bits)
        for i in bad[:max(0, 8 - len(first))]:
            first.append(dict(x=float(x[i]), bits=hex(int(bits[i])), two_roundings=int(b2[i]), contracted=int(b1[i])))
    return dict(inputs=total, differing=differ, examples=first)


def tile_by_tile(tensors, nrow, padding=2, pad_value=0.0):
    import torch
    from multivae_amd.data.datasets.utils import adapt_shape

    data, _ = adapt_shape(dict(enumerate(tensors)))
    x = torch.cat(list(data.values()))
    T, _, H, W = x.shape
    xmaps = min(nrow, T)
    ymaps = -(-T // xmaps)
    grid = x.new_full((3, ymaps * (H + padding) + padding, xmaps * (W + padding) + padding), pad_value)
    for k in range(T):
        grid.narrow(1, (k // xmaps) * (H + padding) + padding, H).narrow(2, (k % xmaps) * (W + padding) + padding, W).copy_(x[k])
    return grid.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--census", action="store_true")
    ap.add_argument("--n-data", type=int, default=8)
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--mods", type=int, default=5)
    ap.add_argument("--shape", default="3x28x28")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.census:
        line = census()
    else:
        import torch

        assert torch.cuda.is_available(), "grid_probe needs a GPU (--census does not)"
        from multivae_amd import kernels as K

        dev = torch.device("cuda:0")
        shape = tuple(int(v) for v in a.shape.split("x"))
        g = torch.Generator(device=dev).manual_seed(0)
        tensors = [torch.rand(a.n_data, *shape, generator=g, device=dev) for _ in range(a.mods)]
        tensors += [torch.rand(a.n * a.n_data, *shape, generator=g, device=dev) for _ in range(a.mods)]
        paths = dict(fused=lambda: K.image_grid(tensors, a.n_data, want=("uint8",))[1].cpu(),
                     torch=lambda: K._image_grid_torch(tensors, a.n_data, 2, 0.0, ("uint8",))[1].cpu(),
                     tile_by_tile=lambda: tile_by_tile(tensors, a.n_data))
        outs = {}
        for _ in range(3):
            outs = {k: f() for k, f in paths.items()}
        same = all(torch.equal(outs["fused"], v) for v in outs.values())
        times = {k: [] for k in paths}
        for _ in range(a.reps):  # alternating, so that a drift of the machine hits all
            for k, f in paths.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                times[k].append(time.perf_counter() - t0)
        # the launch alone, both outputs
        grid, image = K.image_grid(tensors, a.n_data)
        n_calls = 200
        for _ in range(10):
            K.image_grid(tensors, a.n_data, grid_out=grid, image_out=image)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n_calls):
            K.image_grid(tensors, a.n_data, grid_out=grid, image_out=image)
        e1.record()
        torch.cuda.synchronize()
        launch_s = e0.elapsed_time(e1) * 1e-3 / n_calls
        nbytes = sum(t.numel() for t in tensors) * 4 + grid.numel() * 4 + image.numel()
        med = statistics.median
        ms = lambda v: dict(median=1e3 * med(v), min=1e3 * min(v), max=1e3 * max(v))
        line = dict(sources=[list(t.shape) for t in tensors], tiles=sum(len(t) for t in tensors), grid=list(grid.shape), reps=a.reps,
                    same_bytes=same, fused_ms=ms(times["fused"]), torch_ms=ms(times["torch"]), tile_by_tile_ms=ms(times["tile_by_tile"]),
                    torch_over_fused=med(times["torch"]) / med(times["fused"]),
                    tile_by_tile_over_fused=med(times["tile_by_tile"]) / med(times["fused"]),
                    launch_us=1e6 * launch_s, launch_bytes=nbytes, launch_bytes_per_s=nbytes / launch_s,
                    launch_share_of_hbm_copy_rate=nbytes / launch_s / HBM_MEASURED)
    print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
