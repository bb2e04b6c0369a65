"""The CUB image-caption dataset with the reference's public surface, on-disk layout and item format
(`multivae/data/datasets/cub.py`), without torchvision, nltk or sklearn, and with a device-resident batch path.

* `CUBSentences` reads and writes the reference's generated files (`<root>/cub/oc:{min_occ}_msl:{L}/cub.{split}.s{L}`,
  `cub.vocab`, `cub.unique`, `cub.all`), so either library loads what the other wrote.  Creating them needs a sentence and a word
  tokeniser: the `sent_tokenize` / `word_tokenize` callables when given, nltk's when nltk imports.  Nothing here reaches the
  network (the reference calls `nltk.download`; the punkt data has to be in place already).
* `CUB` pairs caption j with picture j // 10.  The pictures are enumerated by the documented rule of torchvision's `ImageFolder`
  and loaded as its `Resize([h, w])` + `ToTensor()` on a PIL image are documented to: `convert("RGB")`, `resize((w, h), BILINEAR)`,
  bytes / 255 in CHW float32.  The train / eval split is sklearn's `train_test_split(arange(n), test_size=0.1, random_state=0)`
  restated in numpy.
* `CUB.device_batcher(device)` is the trainer's hook (`trainers/base/base_trainer.py`, `_BatchIterator`): every picture decoded
  once into a uint8 store, the captions as int32 tokens and lengths, all on the device; a batch is the split's index lookup and
  two launches of `csrc/databatch.hip` (`mvk_u8_image_batch`, `mvk_text_batch`).  On a CPU device the same values come from the
  plain torch expressions of `_torch_batch`, which are also what the kernels are tested against."""
import io
import json
import logging
import math
import os
import pickle
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from .base import DatasetOutput, MultimodalBaseDataset

logger = logging.getLogger(__name__)

SPECIAL_TOKENS = ("<exc>", "<pad>", "<eos>")
IMG_EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")
CAPTIONS_PER_IMAGE = 10


def _nltk_tokenizers():
    try:
        from nltk.tokenize import sent_tokenize, word_tokenize
    except ImportError:
        return None, None
    return sent_tokenize, word_tokenize


class CUBSentences(torch.utils.data.Dataset):
    """The CUB captions alone.

    Args:
        root_data_dir (str): the folder that holds `cub/`.
        split (str): "train" (`text_trainvalclasses.txt`) or "test" (`text_testclasses.txt`).
        output_type (str): "one_hot" or "tokens".
        transform (callable): applied to the sentence tensor of an item.  Default: None.
        max_sequence_length (int): words per caption, `<eos>` included.  Default: 32.
        min_occ (int): a word enters the vocabulary when it occurs MORE often than this.  Default: 3.
        sent_tokenize, word_tokenize (callable): text -> sentences, sentence -> words; used when the generated files have to
            be created.  Default: nltk's, when nltk is installed.
    """

    def __init__(self, root_data_dir, split, output_type="one_hot", transform=None, **kwargs):
        super().__init__()
        self.data_dir = os.path.join(root_data_dir, "cub")
        self.split = split
        self.max_sequence_length = kwargs.get("max_sequence_length", 32)
        self.min_occ = kwargs.get("min_occ", 3)
        self.sent_tokenize = kwargs.get("sent_tokenize", None)
        self.word_tokenize = kwargs.get("word_tokenize", None)
        self.transform = transform
        self.output_type = output_type
        self.gen_dir = os.path.join(self.data_dir, "oc:{}_msl:{}".format(self.min_occ, self.max_sequence_length))
        raw = {"train": "text_trainvalclasses.txt", "test": "text_testclasses.txt"}
        if split not in raw:
            raise Exception("Only train or test split is available")
        self.raw_data_path = os.path.join(self.data_dir, raw[split])
        os.makedirs(self.gen_dir, exist_ok=True)
        self.data_file = "cub.{}.s{}".format(split, self.max_sequence_length)
        self.vocab_file = "cub.vocab"
        if os.path.exists(os.path.join(self.gen_dir, self.data_file)):
            self._load_data()
        else:
            logger.info("Data file not found for %s split at %s. Creating new... (this may take a while)", split.upper(),
                        os.path.join(self.gen_dir, self.data_file))
            self._create_data()

    def __len__(self):
        return len(self.data)

    def __getitem__(self, idx):
        entry = self.data[str(idx)]
        L, n = self.max_sequence_length, entry["length"]
        sent = torch.tensor(entry["idx"], dtype=torch.int64)
        padding_mask = torch.zeros(L, dtype=torch.float32)
        padding_mask[:n] = 1.0
        if self.output_type == "one_hot":
            sent = F.one_hot(sent, self.vocab_size).float()
            key = "one_hot"
        elif self.output_type == "tokens":
            key = "tokens"
        else:
            raise AttributeError("The output type should be either 'one_hot' or 'tokens' but is neither.")
        if self.transform is not None:
            sent = self.transform(sent)
        return {key: sent, "padding_mask": padding_mask}

    @property
    def vocab_size(self):
        return len(self.w2i)

    @property
    def pad_idx(self):
        return self.w2i["<pad>"]

    @property
    def eos_idx(self):
        return self.w2i["<eos>"]

    @property
    def unk_idx(self):
        return self.w2i["<unk>"]  # KeyError, as in the reference: the vocabulary's unknown word is <exc>

    def get_w2i(self):
        return self.w2i

    def get_i2w(self):
        return self.i2w

    # -- files -----------------------------------------------------------------------------------------------------------
    def _tokenizers(self):
        """The two tokenisers of a creation; ImportError when neither the callables nor nltk provide them."""
        nltk_sent, nltk_word = _nltk_tokenizers()
        sent, word = self.sent_tokenize or nltk_sent, self.word_tokenize or nltk_word
        if sent is None or word is None:
            raise ImportError(
                f"Creating the CUB caption files in {self.gen_dir} needs a sentence and a word tokeniser. Either pass "
                "sent_tokenize=... and word_tokenize=... (text -> list of sentences, sentence -> list of words), or install "
                "nltk with its punkt data (nothing is downloaded here). Existing generated files load without either.")
        return sent, word

    def _sentences(self):
        sent_tokenize, word_tokenize = self._tokenizers()
        with open(self.raw_data_path, "r") as file:
            return [word_tokenize(line) for line in sent_tokenize(file.read())]

    def _write_json(self, name, obj):
        with io.open(os.path.join(self.gen_dir, name), "wb") as file:
            file.write(json.dumps(obj, ensure_ascii=False).encode("utf8", "replace"))

    def _load_data(self, vocab=True):
        with open(os.path.join(self.gen_dir, self.data_file), "rb") as file:
            self.data = json.load(file)
        if vocab:
            self._load_vocab()

    def _load_vocab(self):
        if not os.path.exists(os.path.join(self.gen_dir, self.vocab_file)):
            self._create_vocab()
        with open(os.path.join(self.gen_dir, self.vocab_file), "r") as file:
            vocab = json.load(file)
        self.w2i, self.i2w = vocab["w2i"], vocab["i2w"]  # i2w's keys are strings after the round trip through JSON

    def _create_data(self):
        self._load_vocab()  # creates it first when it is missing (from the train split only)
        L = self.max_sequence_length
        exc = self.w2i["<exc>"]
        data, whole = {}, 0
        for words in self._sentences():
            tok = list(words[: L - 1]) + ["<eos>"]
            length = len(tok)
            if length < L:
                tok += ["<pad>"] * (L - length)
                whole += 1
            data[len(data)] = dict(tok=tok, idx=[self.w2i.get(w, exc) for w in tok], length=length)
        logger.info("%d out of %d sentences are truncated with max sentence length %d.", len(data) - whole, len(data), L)
        self._write_json(self.data_file, data)
        self._load_data(vocab=False)

    def _create_vocab(self):
        if self.split != "train":
            raise AssertionError("Vocablurary can only be created for training file.")
        counts = OrderedDict()  # first-seen order
        for words in self._sentences():
            for w in words:
                counts[w] = counts.get(w, 0) + 1
        w2i, i2w, excluded = {}, {}, []
        for w in SPECIAL_TOKENS:
            i2w[len(w2i)] = w
            w2i[w] = len(w2i)
        for w, occ in counts.items():
            if occ > self.min_occ and w not in SPECIAL_TOKENS:
                i2w[len(w2i)] = w
                w2i[w] = len(w2i)
            else:
                excluded.append(w)
        logger.info("Vocablurary of %d keys created, %d words are excluded (occurrence <= %d).", len(w2i), len(excluded), self.min_occ)
        self._write_json(self.vocab_file, dict(w2i=w2i, i2w=i2w))
        # the reference's two side files; its cub.all is a pickle of its own counter class, here of a plain OrderedDict
        with open(os.path.join(self.gen_dir, "cub.unique"), "wb") as file:
            pickle.dump(np.array(excluded), file)
        with open(os.path.join(self.gen_dir, "cub.all"), "wb") as file:
            pickle.dump(counts, file)

    # -- strings ---------------------------------------------------------------------------------------------------------
    def one_hot_to_string(self, data):
        return [self._to_string(m) for m in data]

    def _to_string(self, matrix):
        return " ".join(self.i2w[str(int(np.argmax(matrix[i, :])))] for i in range(matrix.shape[0]))

    # -- the device store --------------------------------------------------------------------------------------------------
    def token_store(self):
        """(tokens int32 [n, L], lengths int32 [n]) of every caption, checked: ids in [0, V), lengths in [0, L]."""
        n, L = len(self.data), self.max_sequence_length
        tokens = np.empty((n, L), dtype=np.int64)
        lengths = np.empty(n, dtype=np.int64)
        for i in range(n):
            entry = self.data[str(i)]
            if len(entry["idx"]) != L:
                raise ValueError(f"caption {i} of {self.data_file} has {len(entry['idx'])} tokens, not {L}")
            tokens[i] = entry["idx"]
            lengths[i] = entry["length"]
        if n and (tokens.min() < 0 or tokens.max() >= self.vocab_size):
            raise ValueError(f"{self.data_file} holds token ids outside [0, {self.vocab_size}): it does not belong to this cub.vocab")
        if n and (lengths.min() < 0 or lengths.max() > L):
            raise ValueError(f"{self.data_file} holds lengths outside [0, {L}]")
        return torch.from_numpy(tokens.astype(np.int32)), torch.from_numpy(lengths.astype(np.int32))


class _ImageFolder:
    """The pictures under `root`, enumerated as torchvision's `ImageFolder` documents it: the class directories in sorted order,
    inside each `sorted(os.walk(..., followlinks=True))` with sorted file names, files with a known image extension (any letter
    case).  Item i is `(tensor [3, h, w] float32 in [0, 1], class_index)`: `Resize([h, w])` and `ToTensor()` on the PIL image,
    then `transform`."""

    def __init__(self, root, im_size, transform=None):
        self.root = root
        self.im_size = (int(im_size[0]), int(im_size[1]))
        self.transform = transform
        self.classes = sorted(e.name for e in os.scandir(root) if e.is_dir())
        if not self.classes:
            raise FileNotFoundError(f"Couldn't find any class folder in {root}.")
        self.class_to_idx = {c: i for i, c in enumerate(self.classes)}
        self.samples = []
        for c in self.classes:
            found = 0
            for folder, _, names in sorted(os.walk(os.path.join(root, c), followlinks=True)):
                for name in sorted(names):
                    if name.lower().endswith(IMG_EXTENSIONS):
                        self.samples.append((os.path.join(folder, name), self.class_to_idx[c]))
                        found += 1
            if not found:
                raise FileNotFoundError(f"Found no valid file for the class {c}. Supported extensions are: {', '.join(IMG_EXTENSIONS)}")

    def __len__(self):
        return len(self.samples)

    def load_u8(self, i):
        """Picture i as bytes [3, h, w]: RGB, resized with PIL's BILINEAR."""
        from PIL import Image

        h, w = self.im_size
        with open(self.samples[i][0], "rb") as file:
            img = Image.open(file).convert("RGB")
        img = img.resize((w, h), Image.BILINEAR)
        return torch.from_numpy(np.array(img, dtype=np.uint8)).permute(2, 0, 1).contiguous()

    def __getitem__(self, i):
        x = self.load_u8(i).float().div(255)
        if self.transform is not None:
            x = self.transform(x)
        return x, self.samples[i][1]


def _split_indices(n, test_size=0.1, seed=0):
    """sklearn's `train_test_split(np.arange(n), test_size=test_size, random_state=seed, shuffle=True)`: one permutation of the
    seeded Mersenne Twister, its first ceil(test_size n) entries are the test part, the others the train part."""
    n_test = int(math.ceil(test_size * n))
    if n - n_test < 1:
        raise ValueError(f"With n_samples={n} and test_size={test_size} the resulting train set will be empty.")
    perm = np.random.RandomState(seed).permutation(n)
    return perm[n_test:], perm[:n_test]


def _torch_batch(images, tokens, lengths, j, vocab_size, output_type):
    """The batch of caption indices j from the stores in plain torch: the CPU path of the batcher and the definition the kernels
    of csrc/databatch.hip are tested against."""
    image = images.index_select(0, torch.div(j, CAPTIONS_PER_IMAGE, rounding_mode="floor")).float().div(255)
    tok = tokens.index_select(0, j).long()
    L = tokens.shape[1]
    mask = (torch.arange(L, device=j.device)[None, :] < lengths.index_select(0, j)[:, None]).float()
    if output_type == "one_hot":
        return image, dict(one_hot=F.one_hot(tok, vocab_size).float(), padding_mask=mask)
    return image, dict(tokens=tok, padding_mask=mask)


class CUB(MultimodalBaseDataset):
    """The paired image-caption CUB dataset: item i is `DatasetOutput(data=dict(image=[3, h, w], text=dict(one_hot | tokens,
    padding_mask)))`, ten consecutive captions to a picture.

    Args:
        path (str): the folder that holds `cub/`.
        split (str): "train", "eval" (both from the train files: a seeded 90 / 10 split of the captions) or "test".
        max_words_in_caption (int): words per caption.  Default: 32.
        im_size (tuple): (height, width) of the pictures.  Default: (64, 64).
        img_transform (callable): applied to a picture's tensor.  Default: None.
        output_type (str): "one_hot" or "tokens".
        download (bool): fetching the data is not built; True only changes the error when the data is missing.
    """

    def __init__(self, path, split="train", max_words_in_caption=32, im_size=(64, 64), img_transform=None, output_type="one_hot",
                 download=False):
        self.split = split
        self.check_or_download_data(path, download)
        self.max_words_in_caption = max_words_in_caption
        self.im_size = tuple(im_size)
        self.img_transform = img_transform
        self.output_type = output_type
        files = "train" if split == "eval" else split
        self.text_data = CUBSentences(path, files, output_type=output_type, transform=None, max_sequence_length=max_words_in_caption)
        self.image_data = _ImageFolder(os.path.join(path, "cub", files), self.im_size, transform=img_transform)
        # computed for every split name, as the reference's `== "train" or "eval"` condition does
        self.train_idx, self.val_idx = _split_indices(len(self.text_data))
        self.vocab_size = self.text_data.vocab_size
        self._stores = {}

    def check_or_download_data(self, data_path, download):
        if os.path.exists(os.path.join(data_path, "cub")):
            return
        if download:
            raise NotImplementedError(
                f"Downloading the CUB dataset is not built: place the extracted data (text_trainvalclasses.txt, "
                f"text_testclasses.txt, train/, test/) in {os.path.join(data_path, 'cub')}.")
        raise AttributeError("The CUB dataset is not available at the"
                             " given datapath and download is set to False."
                             "Set download to True or place the dataset"
                             " in the data_path folder.")

    def _index_map(self):
        return {"train": self.train_idx, "eval": self.val_idx}.get(self.split)

    def __getitem__(self, index):
        m = self._index_map()
        if m is not None:
            index = int(m[index])
        image = self.image_data[index // CAPTIONS_PER_IMAGE][0]
        return DatasetOutput(data=dict(image=image, text=self.text_data[index]))

    def __len__(self):
        m = self._index_map()
        return len(self.text_data) if m is None else len(m)

    # -- the device batch path ---------------------------------------------------------------------------------------------
    def _host_stores(self):
        """Every picture decoded and resized once (uint8 [n_images, 3, h, w]), the captions (int32 [n, L]), their lengths and the
        split's index map (int64, None for "test"), checked so that no index of a batch can leave a store."""
        if "host" not in self._stores:
            tokens, lengths = self.text_data.token_store()
            n, n_img = tokens.shape[0], len(self.image_data)
            if n and (n - 1) // CAPTIONS_PER_IMAGE >= n_img:
                raise ValueError(f"{n} captions need {(n - 1) // CAPTIONS_PER_IMAGE + 1} pictures ({CAPTIONS_PER_IMAGE} captions "
                                 f"each) but {self.image_data.root} holds {n_img}")
            h, w = self.im_size
            images = torch.empty(n_img, 3, h, w, dtype=torch.uint8)
            for i in range(n_img):
                images[i] = self.image_data.load_u8(i)
            m = self._index_map()
            self._stores["host"] = (images, tokens, lengths, None if m is None else torch.from_numpy(np.asarray(m, dtype=np.int64)))
        return self._stores["host"]

    def device_batcher(self, device):
        """The trainer's hook: None with an `img_transform` (the per-sample path serves the dataset), else a callable that maps
        a 1-D int64 tensor of dataset indices ON `device` (in [0, len(self)): not checked there) to the batch's DatasetOutput
        on `device`.  The stores are built at the first call and kept."""
        if self.img_transform is not None:
            return None
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._stores:
            self._stores[device] = tuple(None if t is None else t.to(device) for t in self._host_stores())
        images, tokens, lengths, index_map = self._stores[device]
        V, output_type = self.vocab_size, self.output_type
        if output_type not in ("one_hot", "tokens"):
            raise AttributeError("The output type should be either 'one_hot' or 'tokens' but is neither.")

        def batch(index):
            j = index if index_map is None else index_map.index_select(0, index)
            if device.type == "cuda":
                from ... import kernels

                image = kernels.u8_image_batch(images, j, CAPTIONS_PER_IMAGE)
                text = kernels.text_batch(tokens, lengths, j, V, want=(output_type,))
            else:
                image, text = _torch_batch(images, tokens, lengths, j, V, output_type)
            return DatasetOutput(data=dict(image=image, text=text))

        return batch

    # -- plotting ------------------------------------------------------------------------------------------------------------
    def plot_text(self, input_tensor, fig_size=(2, 1.5)):
        """A caption [L, V] drawn as a small picture: [4, H, W] floats in [0, 1] on the tensor's device."""
        from matplotlib.backends.backend_agg import FigureCanvasAgg
        from matplotlib.figure import Figure
        from PIL import Image

        device = input_tensor.device
        sentence = self.text_data._to_string(input_tensor.detach().cpu().numpy())
        words = [w for w in sentence.split() if w != "<eos>"]
        fig = Figure(figsize=fig_size)
        FigureCanvasAgg(fig)
        ax = fig.add_subplot()
        ax.text(x=0.5, y=0.5, s=" ".join(w + "\n" if (n + 1) % 3 == 0 else w for n, w in enumerate(words)), fontsize=7,
                verticalalignment="center_baseline", horizontalalignment="center")
        ax.axis("off")
        fig.tight_layout()
        buf = io.BytesIO()
        fig.savefig(buf, format="png")
        image = np.array(Image.open(buf)).transpose(2, 0, 1) / 255
        return torch.from_numpy(image).float().to(device)

    def transform_for_plotting(self, input, modality):
        """The data of one modality as pictures: `input` has the type `__getitem__` returns for it (a tensor, or the text dict)."""
        if modality == "image":
            return input
        if modality != "text":
            return None
        if isinstance(input, torch.Tensor):
            rows = list(input)
        elif isinstance(input, dict):
            if "one_hot" in input:
                rows = list(input["one_hot"])
            elif "tokens" in input:
                rows = [F.one_hot(x.long(), self.text_data.vocab_size).float() for x in input["tokens"]]
            else:
                raise AttributeError('The text input should be a dictionary with either "one_hot" or "tokens" as a key but it has neither.')
        else:
            raise AttributeError("The input should be either a tensor or a dictionary but is neither")
        return torch.stack([self.plot_text(x) for x in rows])
