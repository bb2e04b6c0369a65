"""Fixture for the Fréchet distance of the FIDEvaluator: small activation pairs and the values the REFERENCE computes from them.

Build container only (needs the reference checkout):  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_fid_golden.py

For every case of tests/fid_ref.py::GOLDEN_CASES (procedural float32 activations: D = 1, where np.cov returns a 0-d array; a
rank-deficient pair with fewer rows than columns; a pair offset by 500 at unit scale; two ordinary ones) it stores the inputs, the
np.mean / np.cov(rowvar=False) of their float64 copies (what multivae/metrics/fids/fids.py:153-154 takes) and what the reference's
own `FIDEvaluator.calculate_frechet_distance` (fids.py:158-216) returns for them.  Arrays only."""
import sys

sys.dont_write_bytecode = True
import logging
import os
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np

import _reference_import as R

R.install()
# the Inception wrapper subclasses torchvision's blocks at import time; the distance arithmetic does not touch it
_stub = types.ModuleType("multivae.metrics.fids.inception_networks")
_stub.wrapper_inception = None
sys.modules[_stub.__name__] = _stub
import fid_ref as F
from multivae.metrics.fids.fids import FIDEvaluator


def main():
    out = {}
    stub = types.SimpleNamespace(logger=logging.getLogger("make_fid_golden"))
    for name, (D, N, seed, offset) in F.GOLDEN_CASES.items():
        real, gen = F.make_pair(D, N, seed, offset)
        acts = [real.astype(np.float64), gen.astype(np.float64)]
        mus = [np.mean(a, axis=0) for a in acts]
        sigmas = [np.cov(a, rowvar=False) for a in acts]
        fd = FIDEvaluator.calculate_frechet_distance(stub, mus[0], sigmas[0], mus[1], sigmas[1])
        out[name + "/real"], out[name + "/gen"] = real, gen
        out[name + "/mu0"], out[name + "/mu1"] = mus
        out[name + "/s0"], out[name + "/s1"] = sigmas
        out[name + "/fd"] = np.float64(fd)
        print(name, real.shape, sigmas[0].shape, float(fd), "scale", F.scale(mus[0], sigmas[0], mus[1], sigmas[1]))
    np.savez_compressed(F.GOLDEN, **out)
    print(os.path.getsize(F.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
