"""Shared pieces of the CUB dataset tests: the two tokenisers the golden files were made with, and a tiny `cub/` tree under a
temporary folder (the committed corpus and reference-written caption files of tests/golden/cub_sentences/, a handful of small
PNG / BMP pictures written here with PIL)."""
import os
import re
import shutil

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cub_sentences")
L = 8  # max_sequence_length of the golden files
MIN_OCC = 3
GEN_DIR = f"oc:{MIN_OCC}_msl:{L}"
RAW = {"train": "text_trainvalclasses.txt", "test": "text_testclasses.txt"}
GENERATED = ("cub.vocab", f"cub.train.s{L}", f"cub.test.s{L}")
IM_SIZE = (5, 6)  # (height, width): not square, so a swapped resize shows


def sent_tokenize(text):
    return [line for line in text.split("\n") if line.strip()]


def word_tokenize(sentence):
    return re.findall(r"\w+|[^\w\s]", sentence)


def text_tree(root, generated=True):
    """<root>/cub with the corpus and, when `generated`, the reference-written files in oc:3_msl:8/.  Returns <root> as str."""
    cub = os.path.join(str(root), "cub")
    os.makedirs(cub, exist_ok=True)
    for name in RAW.values():
        shutil.copy(os.path.join(GOLDEN_DIR, name), os.path.join(cub, name))
    if generated:
        os.makedirs(os.path.join(cub, GEN_DIR), exist_ok=True)
        for name in GENERATED:
            shutil.copy(os.path.join(GOLDEN_DIR, name), os.path.join(cub, GEN_DIR, name))
    return str(root)


def _picture(path, h, w, seed):
    from PIL import Image

    rng = np.random.RandomState(seed)
    Image.fromarray(rng.randint(0, 256, size=(h, w, 3), dtype=np.uint8)).save(path)


# (relative path under cub/<split>/, height, width) in the order ImageFolder's rule enumerates them: classes sorted, inside a class
# the folders of os.walk sorted by their path, file names sorted, the extension matched in any letter case
TRAIN_PICTURES = (("001.albatross/a.png", 7, 9), ("001.albatross/b.PNG", 5, 6), ("001.albatross/nested/z.bmp", 6, 6),
                  ("001.albatross/nested/deep/c.png", 12, 4), ("002.auklet/0.png", 3, 11), ("002.auklet/10.png", 9, 9),
                  ("002.auklet/2.png", 8, 5))
TEST_PICTURES = (("150.sparrow/x.png", 10, 10), ("151.wren/y.png", 4, 7))
NOT_PICTURES = ("001.albatross/notes.txt", "002.auklet/nested/readme.md", "001.albatross/a.png.bak")


def image_tree(root, n_train=None, n_test=None):
    """The pictures of the tiny tree (the first n_train / n_test of the lists above) and files that are no pictures."""
    for split, pictures, n in (("train", TRAIN_PICTURES, n_train), ("test", TEST_PICTURES, n_test)):
        base = os.path.join(str(root), "cub", split)
        for k, (rel, h, w) in enumerate(pictures[:n]):
            path = os.path.join(base, rel)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            _picture(path, h, w, seed=100 * (split == "test") + k)
    for rel in NOT_PICTURES:
        path = os.path.join(str(root), "cub", "train", rel)
        if not os.path.isdir(os.path.join(str(root), "cub", "train", rel.split("/")[0])):
            continue  # a class folder without a picture is an error of the enumeration
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write("not a picture\n")
    return str(root)


def cub_tree(root, generated=True, **kw):
    text_tree(root, generated)
    return image_tree(root, **kw)
