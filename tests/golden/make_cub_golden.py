"""Fixtures for the CUB captions: what the REFERENCE's CUBSentences writes and returns for a small synthetic corpus.

Build container only (needs the reference checkout):  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_cub_golden.py

The reference module's `sent_tokenize` / `word_tokenize` (nltk's, absent here) are replaced by tests/cub_fixtures.py's: "non-empty
lines" and `re.findall(r"\\w+|[^\\w\\s]", s)`.  Written to tests/golden/cub_sentences/ (flat): the corpus (41 train and 10 test
sentences, seeded), the reference-written cub.vocab, cub.train.s8 and cub.test.s8 (JSON), and cub_items.npz with every item of both
splits for both output types.  cub.unique and cub.all are pickles of the reference's classes and are not kept."""
import sys

sys.dont_write_bytecode = True
import importlib
import os
import shutil
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np
import torch

import _reference_import as R
import cub_fixtures as CF

COMMON = "this bird has a white belly and black wings with , .".split()
SOME = "small the long beak yellow crown brown".split()  # around the vocabulary's threshold
RARE = "iridescent speckled tawny mottled russet crested hooked webbed".split()  # mostly excluded: <exc> in the data


def corpus(n, rng):
    lines = []
    for _ in range(n):
        k = int(rng.randint(2, 13))  # 2 .. 12 words: with <eos>, sentences of 7 words and more fill L = 8 and are cut
        pool = COMMON * 6 + SOME * 2 + RARE
        lines.append(" ".join(pool[int(rng.randint(len(pool)))] for _ in range(k)))
    return "\n".join(lines) + "\n"


def main():
    os.makedirs(CF.GOLDEN_DIR, exist_ok=True)
    rng = np.random.RandomState(7)
    texts = {"train": corpus(41, rng), "test": corpus(10, rng)}
    R.install()
    ref = importlib.import_module("multivae.data.datasets.cub")
    ref.sent_tokenize, ref.word_tokenize = CF.sent_tokenize, CF.word_tokenize
    with tempfile.TemporaryDirectory() as root:
        os.makedirs(os.path.join(root, "cub"))
        for split, text in texts.items():
            with open(os.path.join(root, "cub", CF.RAW[split]), "w") as f:
                f.write(text)
        out = {}
        for split in ("train", "test"):  # the train split first: it creates the vocabulary
            for output_type in ("one_hot", "tokens"):
                ds = ref.CUBSentences(root, split, output_type=output_type, max_sequence_length=CF.L)
                items = [ds[i] for i in range(len(ds))]
                out[f"{split}_{output_type}"] = torch.stack([it[output_type] for it in items]).numpy()
                out[f"{split}_{output_type}_padding_mask"] = torch.stack([it["padding_mask"] for it in items]).numpy()
                print(split, output_type, out[f"{split}_{output_type}"].shape, out[f"{split}_{output_type}"].dtype, "V =", ds.vocab_size)
        for split in texts:
            shutil.copy(os.path.join(root, "cub", CF.RAW[split]), os.path.join(CF.GOLDEN_DIR, CF.RAW[split]))
        for name in CF.GENERATED:
            shutil.copy(os.path.join(root, "cub", CF.GEN_DIR, name), os.path.join(CF.GOLDEN_DIR, name))
    np.savez_compressed(os.path.join(CF.GOLDEN_DIR, "cub_items.npz"), **out)
    for name in sorted(os.listdir(CF.GOLDEN_DIR)):
        print(name, os.path.getsize(os.path.join(CF.GOLDEN_DIR, name)), "bytes")


if __name__ == "__main__":
    main()
