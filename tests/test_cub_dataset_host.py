"""CUBSentences and CUB (multivae_amd/data/datasets/cub.py) on the host: the reference's files, items and rules, the picture
enumeration and loading, the train / eval split, and the device batch path on a CPU device and through the trainer's batch iterator.
Everything is compared for exact equality.  The golden files were written by the reference class (tests/golden/make_cub_golden.py)."""
import json
import math
import os

import numpy as np
import pytest
import torch

import cub_fixtures as CF

from multivae_amd.data.datasets import CUB, CUBSentences, DatasetOutput
from multivae_amd.data.datasets import cub as cubmod


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(CF.GOLDEN_DIR, "cub_items.npz")))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return CF.cub_tree(tmp_path_factory.mktemp("cub_tree"))


def _cub(tree, split, output_type="one_hot", **kw):
    return CUB(tree, split, max_words_in_caption=CF.L, im_size=CF.IM_SIZE, output_type=output_type, **kw)


def _parsed(folder, name):
    with open(os.path.join(folder, name), "rb") as f:
        return json.load(f)


# ---- CUBSentences ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", ["train", "test"])
@pytest.mark.parametrize("output_type", ["one_hot", "tokens"])
def test_reference_files_give_the_golden_items(tmp_path, golden, split, output_type):
    root = CF.text_tree(tmp_path)
    ds = CUBSentences(root, split, output_type=output_type, max_sequence_length=CF.L)  # no tokeniser: nothing is created
    want, mask = golden[f"{split}_{output_type}"], golden[f"{split}_{output_type}_padding_mask"]
    assert len(ds) == want.shape[0] and ds.vocab_size == golden["train_one_hot"].shape[2]
    for i in range(len(ds)):
        item = ds[i]
        assert set(item) == {output_type, "padding_mask"}
        assert item[output_type].dtype == (torch.float32 if output_type == "one_hot" else torch.int64)
        assert item["padding_mask"].dtype == torch.float32
        assert np.array_equal(item[output_type].numpy(), want[i]) and np.array_equal(item["padding_mask"].numpy(), mask[i])
    if output_type == "one_hot":  # pad positions are one-hot at <pad>, not zero rows
        assert all(float(ds[i]["one_hot"].sum()) == CF.L for i in range(len(ds)))
        i = next(i for i in range(len(ds)) if ds.data[str(i)]["length"] < CF.L)
        assert int(ds[i]["one_hot"][-1].argmax()) == ds.pad_idx == 1


def test_creation_writes_what_the_reference_wrote(tmp_path):
    root = CF.text_tree(tmp_path, generated=False)
    for split in ("train", "test"):
        ds = CUBSentences(root, split, max_sequence_length=CF.L, sent_tokenize=CF.sent_tokenize, word_tokenize=CF.word_tokenize)
        assert len(ds) == {"train": 41, "test": 10}[split]
    gen = os.path.join(root, "cub", CF.GEN_DIR)
    for name in CF.GENERATED:
        assert _parsed(gen, name) == _parsed(CF.GOLDEN_DIR, name), name
    assert os.path.exists(os.path.join(gen, "cub.unique")) and os.path.exists(os.path.join(gen, "cub.all"))


def test_creation_rules(tmp_path):
    root = CF.text_tree(tmp_path, generated=False)
    ds = CUBSentences(root, "train", max_sequence_length=CF.L, sent_tokenize=CF.sent_tokenize, word_tokenize=CF.word_tokenize)
    assert [ds.w2i[w] for w in ("<exc>", "<pad>", "<eos>")] == [0, 1, 2] and (ds.pad_idx, ds.eos_idx) == (1, 2)
    assert all(isinstance(k, str) for k in ds.i2w) and ds.get_w2i() is ds.w2i and ds.get_i2w() is ds.i2w
    with pytest.raises(KeyError):
        ds.unk_idx
    with open(ds.raw_data_path) as f:
        sentences = [CF.word_tokenize(s) for s in CF.sent_tokenize(f.read())]
    counts = {}
    for s in sentences:
        for w in s:
            counts[w] = counts.get(w, 0) + 1
    assert list(ds.w2i)[3:] == [w for w, c in counts.items() if c > CF.MIN_OCC]  # first-seen order, count > min_occ
    assert any(c <= CF.MIN_OCC for c in counts.values())
    seen_exc = seen_cut = False
    for i, s in enumerate(sentences):
        e = ds.data[str(i)]
        assert e["length"] == min(len(s) + 1, CF.L) and len(e["tok"]) == len(e["idx"]) == CF.L
        assert e["tok"][: e["length"] - 1] == s[: CF.L - 1] and e["tok"][e["length"] - 1] == "<eos>"
        assert e["tok"][e["length"]:] == ["<pad>"] * (CF.L - e["length"])
        assert e["idx"] == [ds.w2i.get(w, 0) for w in e["tok"]]
        seen_exc |= 0 in e["idx"]
        seen_cut |= len(s) > CF.L - 1
    assert seen_exc and seen_cut
    item = ds[0]
    assert ds.one_hot_to_string(item["one_hot"][None].numpy()) == [" ".join(w if w in ds.w2i else "<exc>" for w in ds.data["0"]["tok"])]


def test_sentence_transform_is_applied(tmp_path):
    root = CF.text_tree(tmp_path)
    ds = CUBSentences(root, "test", output_type="tokens", transform=lambda s: s + 100, max_sequence_length=CF.L)
    assert ds[3]["tokens"].tolist() == [t + 100 for t in ds.data["3"]["idx"]]
    ds = CUBSentences(root, "test", output_type="one_hot", transform=lambda s: s * 2, max_sequence_length=CF.L)
    assert float(ds[3]["one_hot"].max()) == 2.0


def test_sentence_refusals(tmp_path, monkeypatch):
    root = CF.text_tree(tmp_path)
    with pytest.raises(Exception, match="Only train or test"):
        CUBSentences(root, "eval", max_sequence_length=CF.L)
    with pytest.raises(AttributeError, match="neither"):
        CUBSentences(root, "train", output_type="text", max_sequence_length=CF.L)[0]
    # creation without tokenisers: other generated files (L = 6) are needed, nltk is absent (or made absent)
    monkeypatch.setattr(cubmod, "_nltk_tokenizers", lambda: (None, None))
    with pytest.raises(ImportError, match="sent_tokenize") as e:
        CUBSentences(root, "train", max_sequence_length=6)
    assert "nltk" in str(e.value)
    with pytest.raises(ImportError):
        CUBSentences(root, "train", max_sequence_length=6, sent_tokenize=CF.sent_tokenize)  # one of the two is not enough
    # a vocabulary can only come from the train split
    with pytest.raises(AssertionError):
        CUBSentences(root, "test", max_sequence_length=5, sent_tokenize=CF.sent_tokenize, word_tokenize=CF.word_tokenize)


# ---- CUB: folders, split, items ------------------------------------------------------------------------------------------------
def test_missing_folder(tmp_path):
    with pytest.raises(AttributeError, match="download is set to False"):
        CUB(str(tmp_path))
    with pytest.raises(NotImplementedError, match="place the extracted data"):
        CUB(str(tmp_path), download=True)
    assert not os.path.exists(os.path.join(str(tmp_path), "cub"))


@pytest.mark.parametrize("n", [2, 3, 9, 10, 11, 19, 20, 30, 37, 41, 100, 1234])
def test_split_is_sklearns(n):
    tr, va = cubmod._split_indices(n)
    try:
        from sklearn.model_selection import train_test_split
    except ImportError:
        perm = np.random.RandomState(0).permutation(n)
        k = int(math.ceil(0.1 * n))
        want_tr, want_va = perm[k:], perm[:k]
    else:
        want_tr, want_va = train_test_split(np.arange(n), test_size=0.1, random_state=0, shuffle=True)
    assert np.array_equal(tr, want_tr) and np.array_equal(va, want_va)


def test_lengths_and_index_arithmetic(tree):
    ds = {s: _cub(tree, s) for s in ("train", "eval", "test")}
    tr, va = cubmod._split_indices(41)
    assert (len(ds["train"]), len(ds["eval"]), len(ds["test"])) == (36, 5, 10) == (len(tr), len(va), 10)
    for s in ds:  # the split is computed for every split name
        assert np.array_equal(ds[s].train_idx, tr if s != "test" else cubmod._split_indices(10)[0])
        assert ds[s].vocab_size == ds[s].text_data.vocab_size == 25
    assert len(ds["train"].image_data) == len(ds["eval"].image_data) == len(CF.TRAIN_PICTURES)
    assert len(ds["test"].image_data) == len(CF.TEST_PICTURES)
    for s, m in (("train", tr), ("eval", va), ("test", np.arange(10))):
        for i in range(len(ds[s])):
            item, j = ds[s][i], int(m[i])
            assert isinstance(item, DatasetOutput) and set(item.data) == {"image", "text"}
            assert torch.equal(item.data["image"], ds[s].image_data[j // 10][0])
            want = ds[s].text_data[j]
            assert set(item.data["text"]) == {"one_hot", "padding_mask"}
            assert all(torch.equal(item.data["text"][k], want[k]) for k in want)
    assert len({int(j) // 10 for j in tr}) >= 4  # several pictures are in play


def test_image_enumeration_order(tree):
    folder = _cub(tree, "train").image_data
    base = os.path.join(tree, "cub", "train")
    assert [os.path.relpath(p, base) for p, _ in folder.samples] == [os.path.normpath(r) for r, _, _ in CF.TRAIN_PICTURES]
    assert [c for _, c in folder.samples] == [0, 0, 0, 0, 1, 1, 1] and folder.classes == ["001.albatross", "002.auklet"]
    x, c = folder[4]
    assert c == 1 and x.shape == (3, *CF.IM_SIZE) and x.dtype == torch.float32


def test_image_loading_is_pil_bilinear_and_a_true_division(tree):
    from PIL import Image

    folder = _cub(tree, "train").image_data
    table = (np.arange(256, dtype=np.float32) / np.float32(255)).astype(np.float32)
    h, w = CF.IM_SIZE
    seen = set()
    for i, (path, _) in enumerate(folder.samples):
        want = np.array(Image.open(path).convert("RGB").resize((w, h), Image.BILINEAR), dtype=np.uint8).transpose(2, 0, 1)
        assert np.array_equal(folder.load_u8(i).numpy(), want)
        assert np.array_equal(folder[i][0].numpy(), table[want])
        seen |= set(want.ravel().tolist())
    assert len(seen) > 100
    assert np.array_equal(torch.arange(256, dtype=torch.uint8).float().div(255).numpy(), table)  # all 256 values
    ds = _cub(tree, "train", img_transform=lambda x: 1 - x)
    assert torch.equal(ds.image_data[2][0], 1 - folder[2][0]) and torch.equal(ds[0].data["image"], 1 - _cub(tree, "train")[0].data["image"])


def test_transform_for_plotting(tree):
    ds = _cub(tree, "test")
    items = [ds[i].data["text"] for i in range(2)]
    one_hot = torch.stack([it["one_hot"] for it in items])
    tokens = one_hot.argmax(-1)
    outs = [ds.transform_for_plotting(one_hot, "text"), ds.transform_for_plotting(dict(one_hot=one_hot), "text"),
            ds.transform_for_plotting(dict(tokens=tokens), "text")]
    for out in outs:
        assert out.shape[:2] == (2, 4) and out.shape[2] > 1 and out.shape[3] > 1 and out.dtype == torch.float32
        assert float(out.min()) >= 0 and float(out.max()) <= 1
        assert torch.equal(out, outs[0])
    assert float(outs[0][:, :3].min()) < 0.5  # something was drawn
    img = torch.rand(2, 3, *CF.IM_SIZE)
    assert ds.transform_for_plotting(img, "image") is img
    with pytest.raises(AttributeError):
        ds.transform_for_plotting(dict(words=tokens), "text")
    with pytest.raises(AttributeError):
        ds.transform_for_plotting([1, 2], "text")


# ---- the device batch path on a CPU device ---------------------------------------------------------------------------------------
def _same(a, b):
    assert set(a.data) == set(b["data"]) == {"image", "text"}
    assert a.data["image"].dtype == b["data"]["image"].dtype and torch.equal(a.data["image"], b["data"]["image"])
    assert set(a.data["text"]) == set(b["data"]["text"])
    for k, v in a.data["text"].items():
        assert v.dtype == b["data"]["text"][k].dtype and torch.equal(v, b["data"]["text"][k]), k


@pytest.mark.parametrize("output_type", ["one_hot", "tokens"])
@pytest.mark.parametrize("split", ["train", "eval", "test"])
def test_cpu_batcher_is_the_stacked_items(tree, split, output_type):
    ds = _cub(tree, split, output_type)
    batcher = ds.device_batcher("cpu")
    assert batcher is not None and ds.device_batcher(torch.device("cpu")) is not None
    idx = torch.arange(len(ds) - 1, -1, -1)
    items = [ds[int(i)] for i in idx]
    want = dict(data=dict(image=torch.stack([it.data["image"] for it in items]),
                          text={k: torch.stack([it.data["text"][k] for it in items]) for k in items[0].data["text"]}))
    _same(batcher(idx), want)
    assert batcher(idx[:0]).data["image"].shape == (0, 3, *CF.IM_SIZE)


def test_no_batcher_with_an_image_transform(tree):
    assert _cub(tree, "train", img_transform=lambda x: x).device_batcher("cpu") is None


def test_store_build_refuses_what_would_fault_later(tmp_path):
    root = CF.cub_tree(tmp_path, n_train=4)  # 41 captions need 5 pictures
    ds = _cub(root, "train")
    with pytest.raises(ValueError, match="pictures"):
        ds.device_batcher("cpu")
    root2 = CF.cub_tree(tmp_path / "second")
    ds = _cub(root2, "test")
    ds.text_data.data["2"]["idx"][1] = ds.vocab_size  # a token id outside the vocabulary
    with pytest.raises(ValueError, match="token ids"):
        ds.device_batcher("cpu")


# ---- through the trainer's batch iterator ------------------------------------------------------------------------------------------
def _batches(dataset, batch_size=4, shuffle=False, seed=3):
    from multivae_amd.trainers.base.base_trainer import _BatchIterator

    it = _BatchIterator(dataset, batch_size, shuffle, torch.device("cpu"))
    torch.manual_seed(seed)
    return it, list(it)


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("output_type", ["one_hot", "tokens"])
def test_batch_iterator_hook_equals_the_generic_path(tree, output_type, shuffle):
    hook, a = _batches(_cub(tree, "train", output_type), shuffle=shuffle)
    generic, b = _batches(_cub(tree, "train", output_type, img_transform=lambda x: x), shuffle=shuffle)
    assert hook.batcher is not None and generic.batcher is None and not hook.fast and not generic.fast
    assert len(a) == len(b) == len(hook) == 9 and a[-1].data["image"].shape[0] == 4
    for x, y in zip(a, b):
        _same(x, y)


def test_batch_iterator_with_a_subset(tree):
    picks = [7, 0, 35, 7, 12, 3]
    hook, a = _batches(torch.utils.data.Subset(_cub(tree, "train", "tokens"), picks), shuffle=True)
    generic, b = _batches(torch.utils.data.Subset(_cub(tree, "train", "tokens", img_transform=lambda x: x), picks), shuffle=True)
    assert hook.batcher is not None and generic.batcher is None and len(a) == len(b) == 2
    for x, y in zip(a, b):
        _same(x, y)
    full = _cub(tree, "train", "tokens")
    _, c = _batches(torch.utils.data.Subset(full, picks), batch_size=6)
    assert torch.equal(c[0].data["text"]["tokens"], torch.stack([full[i].data["text"]["tokens"] for i in picks]))


def test_an_order_out_of_range_is_refused_on_the_host(tree):
    from multivae_amd.trainers.base.base_trainer import _BatchIterator

    ds = _cub(tree, "eval", "tokens")
    it = _BatchIterator(ds, 4, False, torch.device("cpu"))
    it._order = lambda: torch.tensor([0, 1, len(ds)])
    with pytest.raises(IndexError):
        next(iter(it))
    it._order = lambda: torch.tensor([0, -1])
    with pytest.raises(IndexError):
        next(iter(it))
    sub = _BatchIterator(torch.utils.data.Subset(ds, [0, len(ds)]), 4, False, torch.device("cpu"))
    with pytest.raises(IndexError):
        next(iter(sub))


def test_exports():
    import multivae_amd.data.datasets as D

    assert "CUB" in D.__all__ and "CUBSentences" in D.__all__ and issubclass(CUB, D.MultimodalBaseDataset)
