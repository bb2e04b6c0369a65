"""mvk_image_grid (csrc/grid.hip) on the GPU against tests/grid_ref.py: both outputs of the launch, bit for bit -- the float grid is
copies and the bytes are defined operation by operation, so there is no tolerance anywhere.  Then Visualization and
BaseTrainer(steps_predict=1) on the device: their pictures are what grid_ref makes of the tensors the models returned."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import grid_cases as GC
import grid_ref as R

pytestmark = pytest.mark.gpu
D = "cuda"


def _rand(*shape, seed=0):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * 1.5 - 0.25  # values below 0 and above 1 too


def _check(tensors, nrow, padding=2, pad_value=0.0):
    """Both outputs of one launch, and each output alone, against the definition."""
    from multivae_amd import kernels

    want_grid, want_image = R.picture(tensors, nrow, padding, pad_value)
    dev = [t.to(D) for t in tensors]
    grid, image = kernels.image_grid(dev, nrow, padding, pad_value)
    assert grid.is_cuda and image.is_cuda and grid.dtype == torch.float32 and image.dtype == torch.uint8
    assert R.same_bits(grid.cpu(), want_grid) and torch.equal(image.cpu(), want_image)
    only = kernels.image_grid(dev, nrow, padding, pad_value, want=("float",))
    assert only[1] is None and R.same_bits(only[0].cpu(), want_grid)
    only = kernels.image_grid(dev, nrow, padding, pad_value, want=("uint8",))
    assert only[0] is None and torch.equal(only[1].cpu(), want_image)
    return want_grid, want_image


def test_channel_rule():
    """c = 1, 2, 3, 4 in one call, with n = 1, 2, 3, 1."""
    tensors = [_rand(1, 1, 6, 5, seed=1), _rand(2, 2, 6, 5, seed=2), _rand(3, 3, 6, 5, seed=3), _rand(1, 4, 6, 5, seed=4)]
    grid, _ = _check(tensors, 4)
    tile = lambda k: grid[:, 2 + (k // 4) * 8:2 + (k // 4) * 8 + 6, 2 + (k % 4) * 7:2 + (k % 4) * 7 + 5]
    assert torch.equal(tile(0), tensors[0][0].expand(3, 6, 5))
    assert torch.equal(tile(2)[:2], tensors[1][1]) and float(tile(2)[2].abs().sum()) == 0
    assert torch.equal(tile(5), tensors[2][2]) and torch.equal(tile(6), tensors[3][0, :3])


def test_centring_floor_and_ceil():
    """(5,7), (8,4), (1,1) together: odd and even differences in both directions; Wg * 3 = 87 is no multiple of 4 (store tails)."""
    tensors = [_rand(2, 1, 5, 7, seed=1), _rand(2, 3, 8, 4, seed=2), _rand(1, 2, 1, 1, seed=3)]
    grid, image = _check(tensors, 3, pad_value=0.25)
    assert tuple(grid.shape) == (3, 2 * 10 + 2, 3 * 9 + 2) and (grid.shape[2] * 3) % 4 == 3
    assert torch.equal(grid[0, 2 + 1:2 + 6, 2:2 + 7], tensors[0][0, 0]) and float(grid[0, 2, 2:9].abs().sum()) == 0  # floor(3 / 2) above
    assert torch.equal(grid[:, 2:10, 20 + 1:20 + 5], tensors[1][0])  # tile 2: floor(3 / 2) = 1 column in front, 2 behind
    assert torch.equal(grid[:2, 12 + 3, 11 + 3], tensors[2][0, :, 0, 0]) and float(grid[2, 12 + 3, 11 + 3]) == 0  # tile 4: floor(7/2), floor(6/2)
    assert float(grid[0, 12:20, 20:27].min()) == 0.25 == float(grid[0, 0, 0])  # the empty cell and the border are pad_value


GEOMETRY = [
    ("single", [(1, 1, 5, 7)], 8, 2, 0.25),
    ("single-3ch", [(1, 3, 28, 28)], 1, 2, 0.0),
    ("T<nrow", [(3, 3, 4, 4)], 8, 2, 0.0),
    ("T=nrow", [(2, 3, 4, 4), (2, 1, 4, 4)], 4, 2, 0.25),
    ("T=nrow+1", [(5, 3, 4, 5)], 4, 2, 0.25),
    ("nrow=1", [(3, 1, 2, 3)], 1, 2, 0.0),
    ("padding=0", [(5, 3, 3, 3)], 2, 0, 0.25),
    ("padding=1", [(5, 3, 3, 3)], 2, 1, 0.25),
    ("padding=1,pad=0", [(7, 2, 3, 5)], 3, 1, 0.0),
    ("padding=0,pad=0", [(4, 1, 1, 1)], 3, 0, 0.0),
    ("vectors", [(3,), (3, 6), (3, 2, 5)], 3, 2, 0.0),
    ("several-blocks", [(8, 3, 28, 28), (64, 1, 28, 28), (8, 3, 32, 32)], 8, 2, 0.0),  # 95k pixels: 560 workgroups
    ("max-sources", [(1 + i % 3, 1 + i % 4, 1 + i % 7, 1 + i % 5) for i in range(32)], 7, 1, 0.1),
]


@pytest.mark.parametrize("case", GEOMETRY, ids=[c[0] for c in GEOMETRY])
def test_grid_geometry(case):
    from multivae_amd import _lib

    _, spec, nrow, padding, pad_value = case
    assert len(spec) <= _lib.GRID_MAX_SOURCES
    _check([_rand(*s, seed=i) for i, s in enumerate(spec)], nrow, padding, pad_value)


@pytest.mark.parametrize("foff,boff", [(1, 1), (2, 3), (3, 2), (0, 0)])
def test_unaligned_outputs_leave_their_surroundings_alone(foff, boff):
    """The float grid at an odd element offset into a larger buffer (a base pointer that is 4- but not 16-byte aligned), the image
    at an odd byte offset: every element written, nothing around them touched."""
    from multivae_amd import kernels

    tensors = [_rand(2, 1, 5, 7, seed=1), _rand(3, 3, 8, 4, seed=2)]
    want_grid, want_image = R.picture(tensors, 3)
    n = want_grid.numel()
    fbuf = torch.full((n + 16,), -7.0, device=D)
    bbuf = torch.full((n + 16,), 0x5A, dtype=torch.uint8, device=D)
    assert fbuf.data_ptr() % 16 == 0 and bbuf.data_ptr() % 16 == 0
    grid_out, image_out = fbuf[foff:foff + n].view(want_grid.shape), bbuf[boff:boff + n].view(want_image.shape)
    grid, image = kernels.image_grid([t.to(D) for t in tensors], 3, grid_out=grid_out, image_out=image_out)
    assert grid.data_ptr() == fbuf.data_ptr() + 4 * foff and image.data_ptr() == bbuf.data_ptr() + boff
    assert R.same_bits(grid.cpu(), want_grid) and torch.equal(image.cpu(), want_image)
    f, b = fbuf.cpu(), bbuf.cpu()
    assert bool((f[:foff] == -7).all()) and bool((f[foff + n:] == -7).all())
    assert bool((b[:boff] == 0x5A).all()) and bool((b[boff + n:] == 0x5A).all())


def test_quantisation():
    """k / 255 and (k + 0.5) / 255 with its two neighbours for every k, values below 0 and above 1, the infinities, NaN -> 0."""
    k = torch.arange(256, dtype=torch.float32)
    half = (k + 0.5) / 255
    vals = torch.cat([k / 255, half, torch.nextafter(half, torch.zeros(())), torch.nextafter(half, torch.ones(()) * 2),
                      torch.tensor([-0.5, -1e-9, 1.0 + 1e-6, 7.0, float("inf"), float("-inf"), float("nan"), -0.0])])
    _, image = _check([vals.reshape(1, 1, 8, -1)], 8)
    flat = image[:, :, 0].reshape(-1)
    assert torch.equal(flat[:256], torch.arange(256, dtype=torch.uint8)) and flat[-8:].tolist() == [0, 0, 255, 255, 255, 0, 0, 0]
    # the same values as tiles of a padded grid, pad_value a half-way value itself
    _check([vals.reshape(8, 1, 3, 43)], 3, 1, float(half[77]))


def test_refusals():
    from multivae_amd import _lib, kernels

    lib = _lib.load()
    cap = _lib.GRID_MAX_SOURCES
    x = _rand(1, 1, 2, 2).to(D)
    out = torch.full((3 * 4 * 256,), -7.0, device=D)  # room for any grid below

    def descs(entries):
        d = (_lib.GridSrc * len(entries))()
        for e, (ptr, shape) in zip(d, entries):
            e.data, (e.n, e.c, e.h, e.w) = ptr, shape
        return d

    call = lambda d, S, nrow=8: lib.mvk_image_grid(d, S, nrow, 2, 0.0, out.data_ptr(), None, None)
    assert call(descs([(x.data_ptr(), (1, 1, 2, 2))] * (cap + 1)), cap + 1) == -1  # more sources than the launch takes
    assert call(descs([(None, (2, 1, 26754, 26754))]), 1, 2) == -1  # 3 Hg Wg >= 2^31 from the shapes alone, data NULL
    assert call(descs([(None, (2, 1, 2, 2))]), 1) == -1  # a NULL source that has images
    for shape in ((-1, 1, 2, 2), (1, 0, 2, 2), (1, 1, 0, 2), (1, 1, 2, -1)):
        assert call(descs([(x.data_ptr(), shape)]), 1) == -1, shape
    assert call(descs([(x.data_ptr(), (1, 1, 2, 2))]), 1, 0) == -1
    assert lib.mvk_image_grid(descs([(x.data_ptr(), (1, 1, 2, 2))]), 1, 8, -1, 0.0, out.data_ptr(), None, None) == -1
    assert lib.mvk_image_grid(descs([(x.data_ptr(), (1, 1, 2, 2))]), 1, 8, 2, 0.0, out.data_ptr() + 2, None, None) == -1  # not a float address
    # T == 0: a no-op that returns MVK_OK; the wrapper raises
    assert call(None, 0) == 0 and call(descs([(None, (0, 3, 4, 4))]), 1) == 0
    torch.cuda.synchronize()
    assert bool((out == -7).all())  # nothing above launched anything
    with pytest.raises(ValueError, match="no image"):
        kernels.image_grid([torch.zeros(0, 3, 4, 4, device=D)], 4)
    # more tensors than the launch takes, strided and float64 tensors: the plain-torch path, on the device
    many = [_rand(1, 1, 2, 3, seed=i) for i in range(cap + 1)]
    grid, image = kernels.image_grid([t.to(D) for t in many], 6)
    assert grid.is_cuda and R.same_bits(grid.cpu(), R.picture(many, 6)[0]) and torch.equal(image.cpu(), R.picture(many, 6)[1])
    y = _rand(2, 3, 4, 6, seed=9)
    assert torch.equal(kernels.image_grid([y.to(D).transpose(2, 3)], 2)[1].cpu(), R.picture([y.transpose(2, 3)], 2)[1])
    assert torch.equal(kernels.image_grid([y.to(D).double()], 2)[1].cpu(), R.picture([y], 2)[1])
    with pytest.raises(ValueError, match="grid_out"):
        kernels.image_grid([y.to(D).double()], 2, grid_out=torch.empty(3, 6, 14, device=D))


# ---- end to end on the device ------------------------------------------------------------------------------------------------------
DIMS = dict(a=(1, 28, 28), b=(40,))


def _mopoe():
    from multivae_amd.models import MoPoE, MoPoEConfig

    torch.manual_seed(3)
    return MoPoE(MoPoEConfig(n_modalities=2, latent_dim=12, input_dims=dict(DIMS)))


def test_visualization_on_the_device(tmp_path, monkeypatch):
    from multivae_amd.metrics import Visualization, VisualizationConfig

    model, ds = _mopoe(), GC.dataset(12, DIMS)
    seen = GC.Captured(monkeypatch, type(model))
    vis = Visualization(model, ds, str(tmp_path), VisualizationConfig(n_samples=3, n_data_cond=5))
    pic = vis.unconditional_samples()
    dec = seen.decodes[-1]
    assert list(dec) == ["a", "b"] and dec["a"].shape == (3, 1, 28, 28) and dec["b"].shape == (3, 40)
    want = R.picture([dec["a"], dec["b"]], 3)[1]  # tiles of 28 x 40: the vector is a centred row
    assert pic.mode == "RGB" and pic.size == (3 * 42 + 2, 2 * 30 + 2) and torch.equal(torch.from_numpy(np.array(pic)), want)
    assert torch.equal(GC.png_pixels(tmp_path / "unconditional.png"), want)
    pic = vis.conditional_samples_subset(["b"])
    call = seen.predicts[-1]
    want = R.picture([call["data"]["b"], call["out"]["a"], call["out"]["b"]], 5)[1]
    assert call["out"]["a"].shape == (15, 1, 28, 28) and torch.equal(torch.from_numpy(np.array(pic)), want)
    assert torch.equal(GC.png_pixels(tmp_path / "conditional_from_subset_['b'].png"), want)
    assert list(vis.eval().keys()) == ["unconditional_generation"]
    vis.finish()


def _train_and_compare(tmp_path, monkeypatch, model, ds, keys, **kw):
    from multivae_amd.trainers import BaseTrainer, BaseTrainerConfig

    rec = GC.recorder()
    seen = GC.Captured(monkeypatch, type(model))
    cfg = BaseTrainerConfig(output_dir=str(tmp_path), per_device_train_batch_size=32, num_epochs=2, learning_rate=1e-3,
                            steps_predict=1, **kw)
    trainer = BaseTrainer(model, train_dataset=ds, training_config=cfg, callbacks=[rec])
    hist = trainer.train()
    assert len(hist) == 2 and all(np.isfinite(h["train_epoch_loss"]) for h in hist)
    assert [s["global_step"] for s in rec.steps] == [1, 2]
    per_step = len(keys)
    assert len(seen.predicts) == 2 * per_step
    for i, step in enumerate(rec.steps):
        assert list(step["images"]) == keys and set(step["devices"].values()) == {"cuda"}
        want = GC.trainer_pictures(seen.predicts[i * per_step:(i + 1) * per_step])
        for key in keys:
            assert R.same_bits(step["images"][key], R.picture(want[key], 8)[0]), (i, key)
    for key in keys:  # the files are the bytes of the last step's launch
        want = GC.trainer_pictures(seen.predicts[-per_step:])[key]
        assert torch.equal(GC.png_pixels(os.path.join(trainer.training_dir, key + ".png")), R.picture(want, 8)[1]), key
    assert sorted(f for f in os.listdir(trainer.training_dir) if f.endswith(".png")) == sorted(k + ".png" for k in keys)
    return trainer


def test_trainer_predicts_on_the_device(tmp_path, monkeypatch):
    """Two epochs with steps_predict = 1 under hipGraph replay: the prediction runs eagerly on the best model's copy between the
    epochs, and the replayed step trains on."""
    trainer = _train_and_compare(tmp_path, monkeypatch, _mopoe(), GC.dataset(64 + 24, DIMS),
                                 ["recon_from_a", "recon_from_b", "recon_from_all"], use_hip_graph=True)
    assert any(g is not None for g in trainer._graphs.values()) and trainer.model.training


def test_trainer_predicts_a_cvae(tmp_path, monkeypatch):
    from multivae_amd.models import CVAE, CVAEConfig

    dims = dict(x=(2, 5), c1=(6,), c2=(3, 1))
    torch.manual_seed(1)
    model = CVAE(CVAEConfig(conditioning_modalities=["c1", "c2"], main_modality="x", input_dims=dims, latent_dim=5))
    _train_and_compare(tmp_path, monkeypatch, model, GC.dataset(40, dims), ["recon_from_all"])
