"""csrc/databatch.hip (mvk_text_batch, mvk_u8_image_batch) through the C ABI against the plain torch expressions, exactly; the CUB
dataset's device batcher on the GPU against its CPU path; one epoch of MoPoE through BaseTrainer on the tiny CUB tree.

The float outputs are allocated between two guards of 64 sentinel floats and at every 4-byte phase of a 16-byte line, so a store
outside the output shows as a failed comparison."""
import math
from types import SimpleNamespace

import pytest
import torch

import cub_fixtures as CF

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 64, -7.5
EINVAL = -1


def _lib():
    from multivae_amd import _lib

    return _lib, _lib.load()


def _guarded(n, phase=0):
    """(whole buffer, view of n floats) with GUARD sentinel floats on either side; the view begins `phase` floats behind a
    16-byte boundary."""
    buf = torch.full((GUARD + 4 + n + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    lead = (-(buf.data_ptr() // 4) % 4 + phase) % 4  # floats to skip so that the view sits at the wanted phase
    view = buf[GUARD + lead: GUARD + lead + n]
    assert (view.data_ptr() // 4) % 4 == phase
    return buf, view


def _guards_untouched(buf, view):
    first = (view.data_ptr() - buf.data_ptr()) // 4
    host = buf.cpu()
    return bool((host[:first] == SENTINEL).all()) and bool((host[first + view.numel():] == SENTINEL).all())


# ---- mvk_text_batch ----------------------------------------------------------------------------------------------------------------
def _text_store(N, L, V, seed):
    g = torch.Generator().manual_seed(seed)
    tokens = torch.randint(0, V, (N, L), generator=g, dtype=torch.int32)
    lengths = torch.randint(1, L + 1, (N,), generator=g, dtype=torch.int32)
    return tokens, lengths


def _text_oracle(tokens, lengths, index, V):
    tok = tokens.index_select(0, index).long()
    mask = (torch.arange(tokens.shape[1])[None, :] < lengths.index_select(0, index)[:, None]).float()
    return tok, mask, torch.nn.functional.one_hot(tok, V).float()


def _run_text(tokens, lengths, index, V, want_tokens=True, want_one_hot=True, phase=0):
    L_, lib = _lib()
    B, L = index.numel(), tokens.shape[1]
    t, n, i = tokens.cuda(), lengths.cuda(), index.cuda()
    out_tok = torch.full((B, L), -99, dtype=torch.int64, device="cuda") if want_tokens else None
    mbuf, mask = _guarded(B * L, phase)
    obuf, one_hot = _guarded(B * L * V, phase) if want_one_hot else (None, None)
    rc = lib.mvk_text_batch(L_.ptr(t), L_.ptr(n), L_.ptr(i), tokens.shape[0], B, L, V, L_.ptr(out_tok), L_.ptr(mask), L_.ptr(one_hot),
                            L_.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    assert _guards_untouched(mbuf, mask) and (obuf is None or _guards_untouched(obuf, one_hot))
    return (None if out_tok is None else out_tok.cpu(), mask.cpu().view(B, L), None if one_hot is None else one_hot.cpu().view(B, L, V))


def _check_text(tokens, lengths, index, V, **kw):
    tok, mask, one_hot = _text_oracle(tokens, lengths, index, V)
    got = _run_text(tokens, lengths, index, V, **kw)
    assert got[0] is None or (got[0].dtype == torch.int64 and torch.equal(got[0], tok))
    assert torch.equal(got[1], mask)
    assert got[2] is None or torch.equal(got[2], one_hot)
    return got


@pytest.mark.parametrize("phase", [0, 1, 2, 3])
def test_text_batch_small(phase):
    tokens, lengths = _text_store(4, 5, 7, seed=0)
    lengths[1], lengths[2] = 1, 5  # a length of 1 and a length of L
    got = _check_text(tokens, lengths, torch.tensor([2, 1, 2]), 7, phase=phase)  # a repeated index
    assert got[1][1].tolist() == [1, 0, 0, 0, 0] and got[1][0].tolist() == [1] * 5


@pytest.mark.parametrize("phase", [0, 3])
def test_text_batch_cub_shape(phase):
    tokens, lengths = _text_store(6, 32, 1590, seed=1)
    tokens[4, 0], tokens[4, 31], tokens[1, 7], tokens[1, 8] = 0, 1589, 1589, 0  # the first and the last class
    got = _check_text(tokens, lengths, torch.tensor([4, 1]), 1590, phase=phase)
    assert got[2][0, 0, 0] == 1 and got[2][0, 31, 1589] == 1 and float(got[2].sum()) == 2 * 32


def test_text_batch_one_by_one():
    _check_text(torch.zeros(1, 1, dtype=torch.int32), torch.ones(1, dtype=torch.int32), torch.tensor([0]), 1)
    _check_text(torch.zeros(1, 1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), torch.tensor([0]), 1, phase=1)


@pytest.mark.parametrize("phase", [0, 2])
def test_text_batch_optional_outputs(phase):
    tokens, lengths = _text_store(9, 8, 18, seed=2)
    index = torch.tensor([8, 0, 3, 3, 5])
    assert _check_text(tokens, lengths, index, 18, want_one_hot=False, phase=phase)[2] is None
    assert _check_text(tokens, lengths, index, 18, want_tokens=False, phase=phase)[0] is None


def test_text_batch_many_rows_stride_the_grid():
    tokens, lengths = _text_store(50, 32, 5, seed=3)  # 300 x 32 = 9600 rows: more than the 8192 waves of the capped grid
    index = torch.randint(0, 50, (300,), generator=torch.Generator().manual_seed(4))
    _check_text(tokens, lengths, index, 5, phase=1)
    _check_text(tokens, lengths, index.repeat(60), 5, want_one_hot=False)  # 576000 rows > 2048 x 256: the token kernel strides too


def test_text_batch_empty_and_refusals():
    L_, lib = _lib()
    tokens, lengths = _text_store(3, 4, 6, seed=5)
    t, n, i = tokens.cuda(), lengths.cuda(), torch.tensor([0, 2]).cuda()
    tok = torch.full((2, 4), -99, dtype=torch.int64, device="cuda")
    mask, one_hot = torch.full((2, 4), SENTINEL, device="cuda"), torch.full((2, 4, 6), SENTINEL, device="cuda")
    p, s = L_.ptr, L_.stream_ptr()
    assert lib.mvk_text_batch(p(t), p(n), p(i), 3, 0, 4, 6, p(tok), p(mask), p(one_hot), s) == 0  # B = 0: nothing is launched
    torch.cuda.synchronize()
    assert bool((mask == SENTINEL).all()) and bool((one_hot == SENTINEL).all()) and bool((tok == -99).all())
    bad = [(None, p(n), p(i), 3, 2, 4, 6, p(tok), p(mask), p(one_hot)), (p(t), None, p(i), 3, 2, 4, 6, p(tok), p(mask), p(one_hot)),
           (p(t), p(n), None, 3, 2, 4, 6, p(tok), p(mask), p(one_hot)), (p(t), p(n), p(i), 3, 2, 4, 6, p(tok), None, p(one_hot)),
           (p(t), p(n), p(i), 3, 2, 0, 6, p(tok), p(mask), p(one_hot)), (p(t), p(n), p(i), 3, 2, 4, 0, p(tok), p(mask), p(one_hot)),
           (p(t), p(n), p(i), 3, -1, 4, 6, p(tok), p(mask), p(one_hot))]
    for args in bad:
        assert lib.mvk_text_batch(*args, s) == EINVAL, args
    torch.cuda.synchronize()
    assert bool((mask == SENTINEL).all()) and bool((one_hot == SENTINEL).all())


# ---- mvk_u8_image_batch ------------------------------------------------------------------------------------------------------------
def _run_image(store, index, div, phase=0, store_phase=0):
    L_, lib = _lib()
    N, E, B = store.shape[0], store[0].numel(), index.numel()
    raw = torch.zeros(N * E + 8, dtype=torch.uint8, device="cuda")  # the store at any byte phase: 4-byte reads where they fit
    lead = (-raw.data_ptr() % 4 + store_phase) % 4
    s = raw[lead: lead + N * E]
    s.copy_(store.reshape(-1))
    i = index.cuda()
    buf, out = _guarded(B * E, phase)
    rc = lib.mvk_u8_image_batch(L_.ptr(s), L_.ptr(i), N, B, E, div, L_.ptr(out), L_.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and _guards_untouched(buf, out)
    want = store.reshape(N, E).index_select(0, torch.div(index, div, rounding_mode="floor")).float().div(255)
    got = out.cpu().view(B, E)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))  # bitwise
    return got


def _bytes(N, E, seed):
    return torch.randint(0, 256, (N, E), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


@pytest.mark.parametrize("store_phase", [0, 1])
@pytest.mark.parametrize("phase", [0, 1, 2, 3])
def test_image_batch_odd_row(phase, store_phase):
    store = _bytes(4, 75, seed=0).view(4, 3, 5, 5)
    _run_image(store, torch.tensor([31, 0, 9, 10, 25, 39]), 10, phase, store_phase)  # captions of four different pictures


@pytest.mark.parametrize("phase", [0, 3])
def test_image_batch_cub_picture(phase):
    _run_image(_bytes(3, 12288, seed=1).view(3, 3, 64, 64), torch.tensor([2, 0, 2, 1]), 1, phase)


def test_image_batch_other_rows():
    _run_image(_bytes(5, 1, seed=2), torch.tensor([4, 0, 0, 3, 1, 2, 2]), 1, phase=3)  # E = 1
    _run_image(_bytes(2, 1030, seed=3), torch.tensor([1, 0, 1]), 1, phase=1, store_phase=2)  # a body of more than one segment
    _run_image(_bytes(3, 2, seed=4), torch.randint(0, 30, (2500,), generator=torch.Generator().manual_seed(5)), 10)  # strides the grid


@pytest.mark.parametrize("phase", [0, 1])
def test_image_batch_all_bytes_bitwise(phase):
    store = torch.arange(256, dtype=torch.uint8).view(1, 256)
    got = _run_image(torch.cat([store, store.flip(1)]), torch.tensor([0, 1]), 1, phase)
    assert got[0, 0] == 0 and got[0, 255] == 1 and torch.equal(got[0], got[1].flip(0))


def test_image_batch_empty_and_refusals():
    L_, lib = _lib()
    store, i = _bytes(2, 12, seed=6).cuda(), torch.tensor([0, 1]).cuda()
    out = torch.full((2, 12), SENTINEL, device="cuda")
    p, s = L_.ptr, L_.stream_ptr()
    assert lib.mvk_u8_image_batch(p(store), p(i), 2, 0, 12, 1, p(out), s) == 0  # B = 0
    bad = [(None, p(i), 2, 2, 12, 1, p(out)), (p(store), None, 2, 2, 12, 1, p(out)), (p(store), p(i), 2, 2, 12, 1, None),
           (p(store), p(i), 2, 2, 0, 1, p(out)), (p(store), p(i), 2, 2, 12, 0, p(out)), (p(store), p(i), 2, -1, 12, 1, p(out))]
    for args in bad:
        assert lib.mvk_u8_image_batch(*args, s) == EINVAL, args
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ---- the dataset's batcher ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return CF.cub_tree(tmp_path_factory.mktemp("cub_tree"))


def _cub(tree, split, output_type, **kw):
    from multivae_amd.data.datasets import CUB

    return CUB(tree, split, max_words_in_caption=CF.L, im_size=CF.IM_SIZE, output_type=output_type, **kw)


@pytest.mark.parametrize("output_type", ["one_hot", "tokens"])
@pytest.mark.parametrize("split", ["train", "eval", "test"])
def test_device_batcher_equals_the_cpu_batcher(tree, split, output_type):
    ds = _cub(tree, split, output_type)
    gpu, cpu = ds.device_batcher("cuda"), ds.device_batcher("cpu")
    idx = torch.randperm(len(ds), generator=torch.Generator().manual_seed(0))
    a, b = gpu(idx.cuda()), cpu(idx)
    assert a.data["image"].is_cuda and a.data["image"].dtype == torch.float32 and torch.equal(a.data["image"].cpu(), b.data["image"])
    assert set(a.data["text"]) == set(b.data["text"]) == {output_type, "padding_mask"}
    for k, v in b.data["text"].items():
        assert a.data["text"][k].dtype == v.dtype and torch.equal(a.data["text"][k].cpu(), v), k
    assert gpu(idx[:0].cuda()).data["image"].shape == (0, 3, *CF.IM_SIZE)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def _mopoe(V):
    from multivae_amd.models import MoPoE, MoPoEConfig
    from multivae_amd.models.base.base_config import BaseAEConfig
    from multivae_amd.models.nn.cub import CubTextDecoderMLP, CubTextEncoder
    from multivae_amd.models.nn.default_architectures import Decoder_AE_MLP, Encoder_VAE_MLP

    torch.manual_seed(4)
    shape = (3, *CF.IM_SIZE)
    cfg = MoPoEConfig(n_modalities=2, latent_dim=6, input_dims=dict(image=shape, text=(CF.L, V)),
                      decoders_dist=dict(image="normal", text="categorical"))
    enc = CubTextEncoder(6, CF.L, V, embed_size=16, nhead=2, ff_size=32, n_layers=2, dropout=0.0)
    dec = CubTextDecoderMLP(SimpleNamespace(latent_dim=6, input_dim=(CF.L, V)))
    ae = BaseAEConfig(input_dim=shape, latent_dim=6)
    model = MoPoE(cfg, encoders=dict(image=Encoder_VAE_MLP(ae), text=enc), decoders=dict(image=Decoder_AE_MLP(ae), text=dec))
    return model.cuda().train()


def test_mopoe_trains_on_the_tiny_cub_through_the_hook(tmp_path, tree):
    from multivae_amd.trainers import BaseTrainer, BaseTrainerConfig

    hooked, generic = _cub(tree, "train", "tokens"), _cub(tree, "train", "tokens", img_transform=lambda x: x)
    model = _mopoe(hooked.vocab_size)
    cfg = BaseTrainerConfig(output_dir=str(tmp_path), per_device_train_batch_size=18, num_epochs=1, learning_rate=1e-3, steps_saving=None)
    trainer = BaseTrainer(model, train_dataset=hooked, training_config=cfg)
    other = BaseTrainer(model, train_dataset=generic, training_config=cfg)
    assert trainer.train_loader.batcher is not None and other.train_loader.batcher is None and len(trainer.train_loader) == 2
    # the first batch of an epoch on either path: the same seed gives the same order, the inputs are identical, so is the loss
    torch.manual_seed(11)
    a = next(iter(trainer.train_loader))
    torch.manual_seed(11)
    b = next(iter(other.train_loader))
    assert torch.equal(a.data["image"], b.data["image"]) and a.data["text"]["tokens"].dtype == torch.int64
    assert all(torch.equal(a.data["text"][k], b.data["text"][k]) for k in ("tokens", "padding_mask"))
    losses = []
    for batch in (a, b):
        torch.manual_seed(12)
        with torch.no_grad():
            losses.append(float(trainer.model(batch).loss))
    print("first-batch loss on the hook and on the generic path:", losses)
    assert math.isfinite(losses[0]) and losses[0] == losses[1]
    hist = trainer.train()
    assert len(hist) == 1 and math.isfinite(hist[0]["train_epoch_loss"]), hist
