"""Fixture for ClassifierPolyMNIST: what the REFERENCE class computes, in fp32 on the CPU, for seeded weights and images.

Build container only (needs the reference checkout):  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_classifier_golden.py

The weights and images are those of tests/clf_ref.py::seeded() (regenerated from the seed on both sides, not stored).  Stored: the
reference class's logits for the first clf_ref.GOLDEN_ROWS images in eval mode, and its state-dict key names and shapes.  The
reference's classifier file is loaded by path: under the import stub `import multivae.metrics` fails on the Inception wrapper, and
the file itself needs torch alone.  Arrays only."""
import sys

sys.dont_write_bytecode = True
import importlib.util
import os

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np
import torch

import _reference_import as R
import clf_ref as CR


def main():
    path = os.path.join(R.REFERENCE_SRC, "multivae", "metrics", "classifiers", "mmnist.py")
    spec = importlib.util.spec_from_file_location("reference_mmnist_classifier", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    clf = mod.ClassifierPolyMNIST()
    sd = clf.state_dict()
    keys = list(sd.keys())
    shapes = [tuple(v.shape) for v in sd.values()]
    assert tuple(keys) == CR.KEYS and tuple(shapes) == CR.SHAPES, (keys, shapes)
    weights, x = CR.seeded()
    clf.load_state_dict(CR.state_dict(weights, torch))
    clf.eval()
    torch.set_num_threads(1)
    with torch.no_grad():
        logits = clf(torch.from_numpy(np.array(x[: CR.GOLDEN_ROWS]))).numpy()
    out = {"logits": logits.astype(np.float32), "keys": np.array(keys), "rank": np.array([len(s) for s in shapes], np.int64),
           "shapes": np.array([list(s) + [0] * (4 - len(s)) for s in shapes], np.int64)}
    print("distance from float64:", CR.dist(logits, CR.logits64("seeded")[: CR.GOLDEN_ROWS]))
    np.savez_compressed(CR.GOLDEN, **out)
    print(os.path.getsize(CR.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
