"""Time one CUB batch (B = 256, L = 32, V = 1590, 64x64 pictures, one-hot captions) on a synthetic store, three ways:

  kernels   the two launches of csrc/databatch.hip (kernels.u8_image_batch + kernels.text_batch)
  torch     the same values from torch on the device: index_select + F.one_hot(...).float() + .float().div(255)
  sample    the per-sample path of trainers/base/base_trainer.py::_BatchIterator for a dataset without a device batcher: B
            __getitem__ calls (PIL decode and resize of a PNG, a [32, 1590] one-hot on the host), torch.stack, .to(device)

kernels and torch are timed with device events over windows of --iters batches, alternating, --rounds times; the figure is the
median window.  The kernels' outputs are first compared with the host's picture and the device's caption tensors.  sample is a host clock around whole batches that end in a device
synchronise.  Bytes are the least the batch needs: every output element written once, every picture byte and token read once.
Needs a GPU; prints one JSON line.  See profiles/NOTES_cub_data.md."""
import argparse
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch
import torch.nn.functional as F

PEAK_COPY_TBS = 6.29  # the float4-copy figure of the MI355X micro-architecture notes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sample-batches", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cub_batch_probe: no GPU visible; a time taken elsewhere says nothing")
    from multivae_amd import kernels
    from multivae_amd.data.datasets.base import DatasetOutput
    from multivae_amd.trainers.base.base_trainer import _BatchIterator

    B, L, V, H, W = a.batch, 32, 1590, 64, 64
    n_img, n_cap = a.images, 10 * a.images
    g = torch.Generator().manual_seed(0)
    images = torch.randint(0, 256, (n_img, 3, H, W), generator=g, dtype=torch.uint8)
    tokens = torch.randint(0, V, (n_cap, L), generator=g, dtype=torch.int32)
    lengths = torch.randint(1, L + 1, (n_cap,), generator=g, dtype=torch.int32)
    d_img, d_tok, d_len = images.cuda(), tokens.cuda(), lengths.cuda()
    order = torch.randperm(n_cap, generator=g).cuda()
    nb = n_cap // B
    ar = torch.arange(L, device="cuda")[None, :]

    def by_kernels(j):
        return kernels.u8_image_batch(d_img, j, 10), kernels.text_batch(d_tok, d_len, j, V, want=("one_hot",))

    def by_torch(j):
        tok = d_tok.index_select(0, j).long()
        mask = (ar < d_len.index_select(0, j)[:, None]).float()
        image = d_img.index_select(0, torch.div(j, 10, rounding_mode="floor")).float().div(255)
        return image, dict(one_hot=F.one_hot(tok, V).float(), padding_mask=mask)

    j0 = order[:B]
    (ia, ta), (ib, tb) = by_kernels(j0), by_torch(j0)
    # the definition is the HOST's .float().div(255); torch on the device multiplies by the rounded 1 / 255 instead of dividing,
    # so its picture may differ from both in the last bit: counted, not required
    host_image = images.index_select(0, torch.div(j0.cpu(), 10, rounding_mode="floor")).float().div(255)
    checks = {"image": torch.equal(ia.cpu(), host_image), **{k: torch.equal(ta[k], tb[k]) for k in tb}}
    same = all(checks.values())
    if not same:
        raise SystemExit(f"cub_batch_probe: the kernels disagree with the host's picture or the device's caption tensors: {checks}")
    torch_image_last_bit = int((ib != ia).sum())
    if not torch.allclose(ib, ia, rtol=2e-7, atol=0):
        raise SystemExit("cub_batch_probe: the device torch picture is further than one rounding from the kernel's")

    def window(fn):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for i in range(a.iters):
            fn(order[(i % nb) * B:(i % nb + 1) * B])
        end.record()
        end.synchronize()
        return start.elapsed_time(end) * 1e-3 / a.iters

    for fn in (by_kernels, by_torch):  # warm-up: code objects, the allocator's blocks
        window(fn)
    times = {"kernels": [], "torch": []}
    for _ in range(a.rounds):
        times["kernels"].append(window(by_kernels))
        times["torch"].append(window(by_torch))

    # the per-sample path: PNG bytes in memory, decoded and resized by PIL for every item, a host one-hot per caption
    from PIL import Image

    pngs = []
    for i in range(64):
        buf = io.BytesIO()
        Image.fromarray(np.random.RandomState(i).randint(0, 256, (96, 80, 3), dtype=np.uint8)).save(buf, format="PNG")
        pngs.append(buf.getvalue())

    class PerSample(torch.utils.data.Dataset):
        def __len__(self):
            return n_cap

        def __getitem__(self, i):
            img = Image.open(io.BytesIO(pngs[(i // 10) % len(pngs)])).convert("RGB").resize((W, H), Image.BILINEAR)
            image = torch.from_numpy(np.array(img, dtype=np.uint8)).permute(2, 0, 1).float().div(255)
            mask = torch.zeros(L)
            mask[: int(lengths[i])] = 1
            return DatasetOutput(data=dict(image=image, text=dict(one_hot=F.one_hot(tokens[i].long(), V).float(), padding_mask=mask)))

    sample = []
    it = iter(_BatchIterator(PerSample(), B, True, torch.device("cuda")))
    if a.sample_batches:  # 0: the device paths alone (a kernel-trace run)
        next(it)
        torch.cuda.synchronize()
    for _ in range(a.sample_batches):
        t0 = time.perf_counter()
        next(it)
        torch.cuda.synchronize()
        sample.append(time.perf_counter() - t0)

    need = B * L * V * 4 + B * 3 * H * W * 4 + B * L * 4 + B * 3 * H * W + B * L * 4 + B * 4 + B * 8  # written + read
    out = {"probe": "cub_batch", "B": B, "L": L, "V": V, "image": [3, H, W], "outputs_equal": same, "torch_device_pixels_off_by_a_rounding": torch_image_last_bit,
           "bytes_per_batch": need,
           "peak_copy_TBps": PEAK_COPY_TBS}
    for k, v in times.items():
        t = statistics.median(v)
        out[k] = {"s_per_batch": t, "min": min(v), "max": max(v), "TBps": need / t * 1e-12, "share_of_copy_peak": need / t * 1e-12 / PEAK_COPY_TBS}
    out["torch_over_kernels"] = out["torch"]["s_per_batch"] / out["kernels"]["s_per_batch"]
    if sample:
        out["sample"] = {"s_per_batch": statistics.median(sample), "min": min(sample), "max": max(sample)}
        out["sample_over_kernels"] = out["sample"]["s_per_batch"] / out["kernels"]["s_per_batch"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
