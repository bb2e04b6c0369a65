"""Timing of the PolyMNIST convolutional networks (csrc/polyconv.hip; EncoderConvMMNIST_adapted + DecoderConvMMNIST at latent 512, the
reference benchmark's pair) against the same networks as plain torch modules with the same weights on the same GPU.

    python tools/polyconv_probe.py [--launches 20] [--rounds 3] [--nograd 512,2560] [--train 256,1280] [--out FILE.json]

Each alternative after a warm-up of the same shape, device events around `--launches` back-to-back passes, the alternatives taken in
turn `--rounds` times (every round is printed to stderr; the figure of a row is the median):
  * enc_nograd / dec_nograd at n in --nograd: forward under torch.no_grad() (the fused one-launch trunks + the linear layers);
  * enc_train / dec_train at n in --train: forward + backward of a fixed projection loss, parameter gradients accumulated in place;
  * *_hip_s the package's modules, *_torch_s the torch twins, *_calls the C-ABI entry calls of one HIP pass (mvk_conv3s2_wgrad is two
    kernels: slices and their ordered finish);
  * max_diff: the largest |hip - torch| of each forward output, relative to its largest magnitude.
Where time goes by kernel: run this script once under `rocprofv3 --kernel-trace --stats -- python tools/polyconv_probe.py --rounds 1`.
Needs a GPU; prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import types

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

L = 512


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


class TorchEncoder(nn.Module):
    def __init__(self):
        super().__init__()
        self.shared_encoder = nn.Sequential(nn.Conv2d(3, 32, 3, 2, 1), nn.ReLU(), nn.Conv2d(32, 64, 3, 2, 1), nn.ReLU(),
                                            nn.Conv2d(64, 128, 3, 2, 1), nn.ReLU())
        self.class_mu, self.class_logvar = nn.Conv2d(128, L, 4, 2, 0), nn.Conv2d(128, L, 4, 2, 0)

    def forward(self, x):
        h = self.shared_encoder(x)
        return self.class_mu(h).flatten(1), self.class_logvar(h).flatten(1)


class TorchDecoder(nn.Module):
    def __init__(self):
        super().__init__()
        self.decoder = nn.Sequential(nn.Linear(L, 2048), nn.ReLU(), nn.Unflatten(1, (128, 4, 4)), nn.ConvTranspose2d(128, 64, 3, 2, 1),
                                     nn.ReLU(), nn.ConvTranspose2d(64, 32, 3, 2, 1, output_padding=1), nn.ReLU(),
                                     nn.ConvTranspose2d(32, 3, 3, 2, 1, output_padding=1))

    def forward(self, z):
        return self.decoder(z)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--nograd", default="512,2560")
    ap.add_argument("--train", default="256,1280")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "polyconv_probe needs a GPU: a CPU run measures nothing"
    torch.set_num_threads(min(16, torch.get_num_threads()))
    from multivae_amd import kernels as K
    from multivae_amd.models.nn.mmnist import DecoderConvMMNIST, EncoderConvMMNIST_adapted

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cfg = types.SimpleNamespace(latent_dim=L)
    enc, dec = EncoderConvMMNIST_adapted(cfg).to(dev), DecoderConvMMNIST(cfg).to(dev)
    tenc, tdec = TorchEncoder().to(dev), TorchDecoder().to(dev)
    tenc.load_state_dict(enc.state_dict())
    tdec.load_state_dict(dec.state_dict())
    for m in (enc, dec, tenc, tdec):
        for p in m.parameters():
            p.grad = torch.zeros_like(p)  # gradients accumulate in place, as in the trainer's flat buffer
    g = torch.Generator(device=dev).manual_seed(1)
    calls = [0]
    orig_call = K.call

    def counting(name, *args):
        calls[0] += 1
        return orig_call(name, *args)

    def hip_enc(x):
        o = enc(x)
        return o.embedding, o.log_covariance

    def hip_dec(z):
        return dec(z).reconstruction

    def count(fn):
        K.call = counting
        try:
            calls[0] = 0
            fn()
        finally:
            K.call = orig_call
        return calls[0]

    def rel(x, y):
        return float((x - y).abs().max() / y.abs().max())

    r = dict(latent=L, launches=a.launches, tile=int(K._lib.load().mvk_polyconv_tile()))
    alts = {}
    for n in [int(v) for v in a.nograd.split(",") if v]:
        x = torch.rand(n, 3, 28, 28, device=dev, generator=g)
        z = torch.randn(n, L, device=dev, generator=g)

        def ng(f, inp):
            def run():
                with torch.no_grad():
                    return f(inp)
            return run

        alts[f"enc_nograd_{n}_hip_s"], alts[f"enc_nograd_{n}_torch_s"] = ng(hip_enc, x), ng(tenc, x)
        alts[f"dec_nograd_{n}_hip_s"], alts[f"dec_nograd_{n}_torch_s"] = ng(hip_dec, z), ng(tdec, z)
        r[f"enc_nograd_{n}_calls"], r[f"dec_nograd_{n}_calls"] = count(ng(hip_enc, x)), count(ng(hip_dec, z))
        r[f"enc_nograd_{n}_max_diff"] = max(rel(p, q) for p, q in zip(ng(hip_enc, x)(), ng(tenc, x)()))
        r[f"dec_nograd_{n}_max_diff"] = rel(ng(hip_dec, z)(), ng(tdec, z)())
    for n in [int(v) for v in a.train.split(",") if v]:
        x = torch.rand(n, 3, 28, 28, device=dev, generator=g)
        z = torch.randn(n, L, device=dev, generator=g).requires_grad_(True)  # the latent's gradient is part of a training pass
        pe = torch.randn(n, L, device=dev, generator=g)
        pd = torch.randn(n, 3, 28, 28, device=dev, generator=g)

        def tr_enc(f, x=x, pe=pe):
            def run():
                mu, lv = f(x)
                ((mu + lv) * pe).sum().backward()
            return run

        def tr_dec(f, z=z, pd=pd):
            def run():
                (f(z) * pd).sum().backward()
            return run

        alts[f"enc_train_{n}_hip_s"], alts[f"enc_train_{n}_torch_s"] = tr_enc(hip_enc), tr_enc(tenc)
        alts[f"dec_train_{n}_hip_s"], alts[f"dec_train_{n}_torch_s"] = tr_dec(hip_dec), tr_dec(tdec)
        r[f"enc_train_{n}_calls"], r[f"dec_train_{n}_calls"] = count(tr_enc(hip_enc)), count(tr_dec(hip_dec))
    rounds = {k: [] for k in alts}
    for _ in range(a.rounds):
        for k, fn in alts.items():
            rounds[k].append(events(fn, a.launches))
            print(k, rounds[k][-1], file=sys.stderr, flush=True)
    r["rounds"] = rounds
    for k in alts:
        r[k] = statistics.median(rounds[k])
    print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
