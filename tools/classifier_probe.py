"""Timing of the fused PolyMNIST classifier launch (csrc/clf.hip, mvk_polyclf_fwd) against the torch modules on the same GPU.

    python tools/classifier_probe.py [--rows 8192] [--launches 50] [--rounds 3] [--out FILE.json]

For n = `--rows` generated images [n,3,28,28] and one set of seeded weights, each after a warm-up of the same shape, device events
around `--launches` back-to-back calls, the alternatives taken in turn `--rounds` times (every round is printed; the figure of a row is
the median):
  * fused_logits_s: one launch that writes the logits [n,10] (ClassifierPolyMNIST.forward in eval mode);
  * fused_counts_s: one launch that writes nothing but the counts (what CoherenceEvaluator.coherence_from_subset does per
    generated modality and batch);
  * torch_logits_s: the same weights as the module's nn.Sequential in eval mode under no_grad (the convolutions and the linear
    layers of torch's own libraries);
  * torch_counts_s: that plus ClassCounts.update (argmax, compare, two scatter-adds): what the evaluator did per modality and
    batch before the fused path;
  * flop = 2 n (196 x 10 x 48 + 49 x 20 x 160 + 980 x 128 + 128 x 10), fp32_share = flop / 157.3 TFLOP/s (the fp32 vector and
    f32-input MFMA peak) over the fused time; bytes = n x 9408 read (the weights stay in the caches), hbm_share likewise at 8 TB/s.
    The launch is compute-shaped: fp32_share is its share of peak;
  * max_logit_diff: the largest |fused - torch| logit, and whether the two counts agree.
Needs a GPU; prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 8.0e12
FP32_FLOP_PER_S = 157.3e12
FLOP_PER_IMAGE = 2.0 * (196 * 10 * 48 + 49 * 20 * 160 + 980 * 128 + 128 * 10)


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
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "classifier_probe needs a GPU: a CPU run measures nothing"
    from multivae_amd import kernels as K
    from multivae_amd.metrics import ClassifierPolyMNIST
    from multivae_amd.metrics.coherences.coherences import ClassCounts

    dev = torch.device("cuda:0")
    n = a.rows
    torch.manual_seed(0)
    clf = ClassifierPolyMNIST().to(dev).eval()
    params = [p.detach() for p in clf.kernel_params()]
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand(n, 3, 28, 28, device=dev, generator=g)
    labels = torch.randint(0, 10, (n,), device=dev, generator=g)
    logits = torch.empty(n, 10, device=dev)
    counts = torch.zeros(11, 2, dtype=torch.int64, device=dev)
    cc = ClassCounts(10, dev)

    def fused_logits():
        K.polyclf_forward(x, params, logits=logits)

    def fused_counts():
        K.polyclf_forward(x, params, labels=labels, counts=counts)

    def torch_logits():
        with torch.no_grad():
            return clf.encoder(x)

    def torch_counts():
        cc.update(torch_logits(), labels)

    alts = dict(fused_logits_s=fused_logits, fused_counts_s=fused_counts, torch_logits_s=torch_logits, torch_counts_s=torch_counts)
    rounds = {k: [] for k in alts}
    for _ in range(a.rounds):
        for k, fn in alts.items():
            rounds[k].append(events(fn, a.launches))
            print(k, rounds[k][-1], file=sys.stderr, flush=True)
    r = dict(rows=n, tile=K.polyclf_tile(), launches=a.launches, rounds=rounds)
    for k in alts:
        r[k] = statistics.median(rounds[k])
    flop, nbytes = FLOP_PER_IMAGE * n, 4.0 * 3 * 28 * 28 * n
    r.update(flop=flop, bytes=nbytes)
    for k in ("fused_logits_s", "fused_counts_s"):
        r[k.replace("_s", "_fp32_share")] = flop / FP32_FLOP_PER_S / r[k]
        r[k.replace("_s", "_hbm_share")] = nbytes / HBM_BYTES_PER_S / r[k]
    # the same results: logits to rounding, counts exactly where no argmax sits on a near-tie
    fused_logits()
    ref = torch_logits()
    c0, c1 = torch.zeros_like(counts), ClassCounts(10, dev)
    K.polyclf_forward(x, params, labels=labels, counts=c0)
    c1.update(ref, labels)
    r.update(max_logit_diff=float((logits - ref).abs().max()), max_logit=float(ref.abs().max()),
             counts_equal=bool(torch.equal(c0, c1.counts)), argmax_differs=int((logits.argmax(1) != ref.argmax(1)).sum()))
    print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
