"""Timing of one streaming Fréchet-statistics update (csrc/frechet.hip, mvk_fd_update) at the FIDEvaluator's standard width.

    python tools/fd_probe.py [--dims 2048 64] [--rows 512] [--launches 50] [--out FILE.json]

Per width D, each after a warm-up of the same shape, device events around `--launches` back-to-back launches:
  * update_s: one mvk_fd_update of two streams of `--rows` rows (the per-batch work of FIDEvaluator.get_frechet_distance);
  * state_bytes: what the launch must move at least: the packed upper tiles of both streams' fp64 second moments read and written
    once (the rows themselves, 2 n D fp32, are counted too; they are re-read per tile column from the caches);
  * flop: 2 n T^2 per computed tile and stream (edge tiles are padded, the padding is counted: it is executed);
  * hbm_share = state_bytes / 8 TB/s over update_s and mfma_share = flop / 157.3 TFLOP/s (the f32-input MFMA peak) over update_s;
    bound_share = the larger of the two least times over update_s, `bound` says which;
  * addmm_s, for orientation only: torch.addmm of the same fp32 operands into an fp32 [D, D] accumulator per stream (a full
    matrix, no shift, no fp64: it does not compute what the kernel computes);
  * finish_s: one mvk_fd_finish (mean, full mirrored cov, terms) and distance_s: frechet_distance on its output, host clock
    around a synchronise (once per distance, not per batch).
Needs a GPU; prints one JSON line per width."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 8.0e12
MFMA_F32_FLOP_PER_S = 157.3e12


def events(fn, launches):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs="+", default=[2048, 64])
    ap.add_argument("--rows", type=int, default=512)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "fd_probe needs a GPU: a CPU run measures nothing"
    from multivae_amd import kernels as K
    from multivae_amd.metrics.fids import frechet_distance

    dev = torch.device("cuda:0")
    T, n = K.fd_tile(), a.rows
    results = []
    for D in a.dims:
        g = torch.Generator(device=dev).manual_seed(D)
        x0 = torch.rand(n, D, device=dev, generator=g) + 0.5  # non-negative features away from zero, as pool features are
        x1 = 0.8 * torch.rand(n, D, device=dev, generator=g) + 0.7
        state = K.fd_new_state(D, dev)
        K.fd_begin(state, x0, x1)
        t_update = events(lambda: K.fd_update(state, x0, x1), a.launches)
        nt = -(-D // T)
        tiles = nt * (nt + 1) // 2
        state_bytes = 2 * (2 * tiles * T * T * 8) + 2 * n * D * 4
        flop = 2.0 * n * T * T * tiles * 2
        t_hbm, t_mfma = state_bytes / HBM_BYTES_PER_S, flop / MFMA_F32_FLOP_PER_S
        acc = [torch.zeros(D, D, device=dev), torch.zeros(D, D, device=dev)]

        def addmm():
            acc[0].addmm_(x0.T, x0)
            acc[1].addmm_(x1.T, x1)

        t_addmm = events(addmm, a.launches)
        t_finish = events(lambda: K.fd_finish(state, D), 5)
        mean, cov, _ = K.fd_finish(state, D)
        frechet_distance(mean[0], cov[0], mean[1], cov[1])  # warm-up of the solver
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fd = float(frechet_distance(mean[0], cov[0], mean[1], cov[1]))
        t_distance = time.perf_counter() - t0
        r = dict(D=D, rows=n, tile=T, chunk=K.fd_chunk(), tiles_per_stream=tiles, update_s=t_update, state_bytes=state_bytes, flop=flop,
                 hbm_share=t_hbm / t_update, mfma_share=t_mfma / t_update, bound="hbm" if t_hbm >= t_mfma else "mfma",
                 bound_share=max(t_hbm, t_mfma) / t_update, addmm_s=t_addmm, finish_s=t_finish, distance_s=t_distance, distance=fd)
        print(json.dumps(r), flush=True)
        results.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
