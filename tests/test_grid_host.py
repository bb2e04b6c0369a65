"""The image grid without a GPU: adapt_shape against the rules, the plain-torch path of kernels.image_grid against tests/grid_ref.py,
Visualization and BaseTrainer.predict / steps_predict end to end on a plain-PyTorch plugin model, and the C ABI of the new entry
(header, ctypes prototypes, the layout of the descriptor).  Every comparison of pixels is exact: the float grid is copies and the
bytes are defined operation by operation."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import grid_cases as GC
import grid_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rand(*shape, seed=0):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * 1.5 - 0.25  # values below 0 and above 1 too


# ---- adapt_shape -----------------------------------------------------------------------------------------------------------------
def test_adapt_shape_rules():
    from multivae_amd.data.datasets.utils import adapt_shape

    data = dict(v1=_rand(4, seed=1), v2=_rand(4, 6, seed=2), v3=_rand(4, 5, 7, seed=3), c1=_rand(4, 1, 8, 4, seed=4),
                c2=_rand(4, 2, 3, 3, seed=5), c3=_rand(4, 3, 2, 9, seed=6), c4=_rand(4, 4, 1, 1, seed=7))
    want, shape = R.adapt_shape(data)
    got, got_shape = adapt_shape(dict(data))
    assert shape == got_shape == (3, 8, 9) and list(got) == list(data)
    for m in data:
        assert got[m].shape == (4, 3, 8, 9) and R.same_bits(got[m], want[m]), m
    # the rules themselves, by hand
    assert torch.equal(got["v1"][:, :, 3, 4], data["v1"][:, None].expand(4, 3))  # [n] -> one pixel, centred: floor(7 / 2), floor(8 / 2)
    assert torch.equal(got["v2"][:, 0, 3, 1:7], data["v2"]) and float(got["v2"][:, :, :3].abs().sum()) == 0  # [n, a] -> a row
    assert torch.equal(got["v3"][:, 1, 1:6, 1:8], data["v3"])  # [n, a, b] -> one channel, replicated; floor(3 / 2), floor(2 / 2)
    assert torch.equal(got["c1"][:, 2, :, 2:6], data["c1"][:, 0])  # floor(5 / 2) columns in front, ceil behind
    assert torch.equal(got["c2"][:, :2, 2:5, 3:6], data["c2"]) and float(got["c2"][:, 2].abs().sum()) == 0
    assert torch.equal(got["c3"][:, :, 3:5, :], data["c3"])
    assert torch.equal(got["c4"][:, :, 3, 4], data["c4"][:, :3, 0, 0])  # the fourth channel is dropped
    with pytest.raises(AttributeError, match="more than 3 dimensions"):
        adapt_shape(dict(x=torch.zeros(2, 1, 2, 2, 2)))


# ---- the plain-torch path of image_grid ------------------------------------------------------------------------------------------
def _sources(spec, seed=0):
    return [_rand(*s, seed=seed + i) for i, s in enumerate(spec)]


GEOMETRY = [
    ("channels", [(1, 1, 3, 4), (2, 2, 3, 4), (3, 3, 3, 4), (1, 4, 3, 4)], 4, 2, 0.0),
    ("centring", [(2, 1, 5, 7), (2, 3, 8, 4), (1, 2, 1, 1)], 3, 2, 0.0),
    ("single", [(1, 1, 5, 7)], 8, 2, 0.5),
    ("T<nrow", [(3, 3, 4, 4)], 8, 2, 0.25),
    ("T=nrow", [(2, 3, 4, 4), (2, 1, 4, 4)], 4, 1, 0.25),
    ("T=nrow+1", [(5, 3, 4, 5)], 4, 2, 0.25),
    ("nrow=1", [(3, 1, 2, 3)], 1, 1, 0.0),
    ("padding=0", [(5, 3, 3, 3)], 2, 0, 0.25),
    ("vectors", [(3,), (3, 6), (3, 2, 5)], 3, 2, 0.0),
]


@pytest.mark.parametrize("case", GEOMETRY, ids=[c[0] for c in GEOMETRY])
def test_torch_path_matches_the_definition(case):
    from multivae_amd import kernels

    _, spec, nrow, padding, pad_value = case
    tensors = _sources(spec)
    want_grid, want_image = R.picture(tensors, nrow, padding, pad_value)
    grid, image = kernels.image_grid(tensors, nrow, padding, pad_value)
    assert grid.dtype == torch.float32 and image.dtype == torch.uint8 and image.is_contiguous()
    assert R.same_bits(grid, want_grid) and torch.equal(image, want_image)
    assert kernels.image_grid_shape([tuple(R.as_images(t).shape) for t in tensors], nrow, padding)[1:] == tuple(want_grid.shape[1:])
    only = kernels.image_grid(tensors, nrow, padding, pad_value, want=("uint8",))
    assert only[0] is None and torch.equal(only[1], want_image)
    only = kernels.image_grid(tensors, nrow, padding, pad_value, want=("float",))
    assert only[1] is None and R.same_bits(only[0], want_grid)


def test_torch_path_quantisation_and_errors():
    from multivae_amd import kernels

    k = torch.arange(256, dtype=torch.float32)
    half = (k + 0.5) / 255
    vals = torch.cat([k / 255, half, torch.nextafter(half, torch.zeros(())), torch.nextafter(half, torch.ones(()) * 2),
                      torch.tensor([-0.5, -1e-9, 1.0 + 1e-6, 7.0, float("inf"), float("-inf"), float("nan"), -0.0])])
    grid, image = kernels.image_grid([vals.reshape(1, 1, 8, -1)], 8)
    want_grid, want_image = R.picture([vals.reshape(1, 1, 8, -1)], 8)
    assert R.same_bits(grid, want_grid) and torch.equal(image, want_image)
    flat = image[:, :, 0].reshape(-1)
    assert torch.equal(flat[:256], torch.arange(256, dtype=torch.uint8)) and flat[-8:].tolist() == [0, 0, 255, 255, 255, 0, 0, 0]
    # other dtypes are shown in float32; a strided tensor is shown as it reads
    x = _rand(2, 3, 4, 6, seed=9)
    assert torch.equal(kernels.image_grid([x.double()], 2)[1], R.picture([x], 2)[1])
    assert torch.equal(kernels.image_grid([x.transpose(2, 3)], 2)[1], R.picture([x.transpose(2, 3).contiguous()], 2)[1])
    with pytest.raises(ValueError, match="no image"):
        kernels.image_grid([], 4)
    with pytest.raises(ValueError, match="no image"):
        kernels.image_grid([torch.zeros(0, 3, 4, 4)], 4)
    with pytest.raises(ValueError, match="want"):
        kernels.image_grid([x], 4, want=())
    with pytest.raises(ValueError, match="nrow"):
        kernels.image_grid([x], 0)
    with pytest.raises(AttributeError, match="more than 3 dimensions"):
        kernels.image_grid([torch.zeros(2, 1, 2, 2, 2)], 4)


# ---- Visualization ------------------------------------------------------------------------------------------------------------
def test_visualization_end_to_end(tmp_path, monkeypatch):
    from PIL import Image

    import multivae_amd.metrics as M
    from multivae_amd._output import ModelOutput
    from multivae_amd.metrics.visualization import Visualization, VisualizationConfig

    assert M.Visualization is Visualization and M.VisualizationConfig is VisualizationConfig and issubclass(Visualization, M.Evaluator)
    cfg = VisualizationConfig()
    assert (cfg.batch_size, cfg.n_samples, cfg.n_data_cond, cfg.wandb_path) == (20, 5, 5, None)
    model, ds = GC.tiny_model(), GC.dataset()
    seen = GC.Captured(monkeypatch, type(model))
    out = tmp_path / "pictures"
    vis = Visualization(model, ds, str(out), VisualizationConfig(n_samples=3, n_data_cond=4))

    # unconditional: a row of 3 samples per modality; tiles of 8 x 7 (a is 5 x 7, b is 8 x 4)
    pic = vis.unconditional_samples()
    dec = seen.decodes[-1]
    assert list(dec) == ["a", "b"] and dec["a"].shape == (3, 1, 5, 7) and dec["b"].shape == (3, 3, 8, 4)
    assert isinstance(pic, Image.Image) and pic.mode == "RGB" and pic.size == (3 * 9 + 2, 2 * 10 + 2)
    want = R.picture([dec["a"], dec["b"]], 3)[1]
    assert torch.equal(torch.from_numpy(__import__("numpy").array(pic)), want)
    assert torch.equal(GC.png_pixels(out / "unconditional.png"), want)

    # conditional on b: the 4 originals of b, then 3 x 4 generations of a and of b, 4 to a row
    pic = vis.conditional_samples_subset(["b"])
    call = seen.predicts[-1]
    assert call["cond_mod"] == ["b"] and list(call["out"]) == ["a", "b"] and call["out"]["a"].shape == (12, 1, 5, 7)
    want = R.picture([call["data"]["b"], call["out"]["a"], call["out"]["b"]], 4)[1]
    assert pic.size == (4 * 9 + 2, 7 * 10 + 2) and torch.equal(torch.from_numpy(__import__("numpy").array(pic)), want)
    assert torch.equal(GC.png_pixels(out / "conditional_from_subset_['b'].png"), want)

    # conditional on both, generating a only; reconstruction of a
    pic = vis.conditional_samples_subset(["a", "b"], gen_mod="a")
    call = seen.predicts[-1]
    want = R.picture([call["data"]["a"], call["data"]["b"], call["out"]["a"]], 4)[1]
    assert list(call["out"]) == ["a"] and torch.equal(GC.png_pixels(out / "conditional_from_subset_['a', 'b'].png"), want)
    assert torch.equal(torch.from_numpy(__import__("numpy").array(pic)), want)
    pic = vis.reconstruction("a")
    call = seen.predicts[-1]
    assert call["cond_mod"] == ["a"] and list(call["out"]) == ["a"]
    assert torch.equal(GC.png_pixels(out / "conditional_from_subset_['a'].png"), R.picture([call["data"]["a"], call["out"]["a"]], 4)[1])

    res = vis.eval()
    assert isinstance(res, ModelOutput) and list(res.keys()) == ["unconditional_generation"]
    assert isinstance(res.unconditional_generation, Image.Image)
    assert torch.equal(GC.png_pixels(out / "unconditional.png"), R.picture(list(seen.decodes[-1].values()), 3)[1])
    assert sorted(os.listdir(out)) == ["conditional_from_subset_['a', 'b'].png", "conditional_from_subset_['a'].png",
                                       "conditional_from_subset_['b'].png", "metrics.log", "unconditional.png"]
    vis.finish()
    # no output directory: the picture only
    quiet = Visualization(model, ds, None, VisualizationConfig(n_samples=2))
    assert quiet.unconditional_samples().size == (2 * 9 + 2, 2 * 10 + 2)
    quiet.finish()


# ---- BaseTrainer.predict / steps_predict ---------------------------------------------------------------------------------
def _train(tmp_path, monkeypatch, steps_predict, trainer_cls=None, **kw):
    from multivae_amd.trainers import BaseTrainer, BaseTrainerConfig

    monkeypatch.setenv("MVK_TRAINER_ALLOW_CPU", "1")
    model, rec = GC.tiny_model(), GC.recorder()
    seen = GC.Captured(monkeypatch, type(model))
    cfg = BaseTrainerConfig(output_dir=str(tmp_path), num_epochs=2, per_device_train_batch_size=4, learning_rate=1e-2, no_cuda=True,
                            use_fused_adam=False, steps_predict=steps_predict, **kw)
    trainer = (trainer_cls or BaseTrainer)(model, GC.dataset(), training_config=cfg, callbacks=[rec])
    trainer.train()
    return trainer, rec, seen


def test_trainer_writes_the_pictures_it_hands_to_the_callbacks(tmp_path, monkeypatch):
    trainer, rec, seen = _train(tmp_path, monkeypatch, 1)
    keys = ["recon_from_a", "recon_from_b", "recon_from_all"]
    assert [s["global_step"] for s in rec.steps] == [1, 2] and all(list(s["images"]) == keys for s in rec.steps)
    assert len(seen.predicts) == 6 and [c["cond_mod"] for c in seen.predicts] == ["a", "b", "all"] * 2
    # 6 data points, N = 8: a row of 6 originals (two rows for "all"), then 8 rows per generated modality; 8 tiles to a row
    shapes = dict(recon_from_a=(3, 13 * 10 + 2, 8 * 9 + 2), recon_from_b=(3, 13 * 10 + 2, 8 * 9 + 2),
                  recon_from_all=(3, 14 * 10 + 2, 8 * 9 + 2))
    for step, calls in zip(rec.steps, (seen.predicts[:3], seen.predicts[3:])):
        want = GC.trainer_pictures(calls)
        for key in keys:
            grid = step["images"][key]
            assert grid.dtype == torch.float32 and tuple(grid.shape) == shapes[key], key
            assert R.same_bits(grid, R.picture(want[key], 8)[0]), key
    # the files are those of the last prediction step: the bytes of the grids the callbacks saw
    pngs = sorted(f for f in os.listdir(trainer.training_dir) if f.endswith(".png"))
    assert pngs == sorted(k + ".png" for k in keys)
    for key in keys:
        assert torch.equal(GC.png_pixels(os.path.join(trainer.training_dir, key + ".png")), R.quantise(rec.steps[-1]["images"][key])), key
    assert not trainer._best_model.training and "_predict_bytes" not in trainer.__dict__


def test_steps_predict_schedule_and_none(tmp_path, monkeypatch):
    trainer, rec, seen = _train(tmp_path / "none", monkeypatch, None)
    assert rec.steps == [] and seen.predicts == []
    assert [f for f in os.listdir(trainer.training_dir) if f.endswith(".png")] == []
    # steps_predict = 5 over 2 epochs: epoch 1 only (epoch % steps_predict == 0 or epoch == 1)
    trainer, rec, _ = _train(tmp_path / "five", monkeypatch, 5)
    assert [s["global_step"] for s in rec.steps] == [1]
    assert len([f for f in os.listdir(trainer.training_dir) if f.endswith(".png")]) == 3


def test_multistage_trainer_inherits_predict(tmp_path, monkeypatch):
    from multivae_amd.trainers import MultistageTrainer, MultistageTrainerConfig

    monkeypatch.setenv("MVK_TRAINER_ALLOW_CPU", "1")
    model, rec = GC.tiny_model(), GC.recorder()
    cfg = MultistageTrainerConfig(output_dir=str(tmp_path), num_epochs=2, per_device_train_batch_size=4, learning_rate=1e-2,
                                  no_cuda=True, use_fused_adam=False, steps_predict=2)
    trainer = MultistageTrainer(model, GC.dataset(), training_config=cfg, callbacks=[rec])
    trainer.train()
    assert [s["global_step"] for s in rec.steps] == [1, 2]
    assert os.path.exists(os.path.join(trainer.training_dir, "recon_from_all.png"))


def test_an_overridden_predict_is_still_written(tmp_path, monkeypatch):
    """A predict that returns float grids of its own (the reference's contract): the PNG is the quantised grid, as save_image's."""
    from multivae_amd.trainers import BaseTrainer

    picture = _rand(3, 6, 10, seed=4)

    class Own(BaseTrainer):
        def predict(self, model, epoch, n_data=8):
            return {"images": {"mine": picture.clone()}}

    trainer, rec, _ = _train(tmp_path, monkeypatch, 1, trainer_cls=Own)
    assert [list(s["images"]) for s in rec.steps] == [["mine"], ["mine"]]
    assert torch.equal(GC.png_pixels(os.path.join(trainer.training_dir, "mine.png")), R.quantise(picture))


# ---- the C ABI of the new entry ---------------------------------------------------------------------------------------------------
def test_header_prototypes_and_descriptor_layout(tmp_path):
    from multivae_amd import _lib

    header = open(os.path.join(ROOT, "include", "mvk.h")).read()
    assert int(re.search(r"#define MVK_GRID_MAX_SOURCES (\d+)", header).group(1)) == _lib.GRID_MAX_SOURCES >= 16
    assert "NaN gives 0" in re.sub(r"\s+\*?\s*", " ", header)
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("mvk_image_grid", "mvk_image_grid_size"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", code, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.PROTOTYPES[name]), name
        assert hasattr(_lib.load(), name)
    assert _lib.PROTOTYPES["mvk_image_grid"][0]._type_ is _lib.GridSrc
    # the descriptor crosses the ABI as an array: sizeof and every offset as a C compiler lays the header's struct out
    fields = [n for n, _ in _lib.GridSrc._fields_]
    assert fields == ["data", "n", "c", "h", "w"]
    src = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(ROOT, "include", "mvk.h")}"', "int main(void){",
           'printf("%zu\\n", sizeof(mvk_grid_src));']
    src += [f'printf("%zu %zu\\n", offsetof(mvk_grid_src, {f}), sizeof(((mvk_grid_src*)0)->{f}));' for f in fields]
    src.append("return 0;}")
    (tmp_path / "layout.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-std=c11", "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split("\n")
    assert int(out[0]) == C.sizeof(_lib.GridSrc) == 24
    for f, line in zip(fields, out[1:]):
        assert [int(v) for v in line.split()] == [getattr(_lib.GridSrc, f).offset, getattr(_lib.GridSrc, f).size], f


def test_size_query_and_refusals_need_no_gpu():
    """mvk_image_grid_size and every refusal of mvk_image_grid are host code that runs before any launch."""
    from multivae_amd import _lib

    lib = _lib.load()

    def descs(shapes, data=0):
        d = (_lib.GridSrc * max(len(shapes), 1))()
        for e, s in zip(d, shapes):
            e.data, (e.n, e.c, e.h, e.w) = data or None, s
        return d

    def size(shapes, nrow, padding=2):
        T, H, W = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
        rc = lib.mvk_image_grid_size(descs(shapes), len(shapes), nrow, padding, C.byref(T), C.byref(H), C.byref(W))
        return rc, (T.value, H.value, W.value)

    from multivae_amd import kernels

    for shapes, nrow, padding in (([(1, 1, 5, 7)], 8, 2), ([(2, 1, 5, 7), (3, 3, 8, 4), (1, 2, 1, 1)], 4, 2), ([(5, 3, 4, 4)], 4, 0),
                                  ([(3, 1, 2, 2), (0, 3, 50, 50)], 1, 1)):
        assert size(shapes, nrow, padding) == (0, kernels.image_grid_shape(shapes, nrow, padding))
    assert size([], 4) == (0, (0, 0, 0)) and size([(0, 1, 2, 2)], 4) == (0, (0, 0, 0))
    cap = _lib.GRID_MAX_SOURCES
    assert size([(1, 1, 2, 2)] * cap, 8)[0] == 0 and size([(1, 1, 2, 2)] * (cap + 1), 8)[0] == -1
    for bad in ([(-1, 1, 2, 2)], [(1, 0, 2, 2)], [(1, 1, 0, 2)], [(1, 1, 2, -3)]):
        assert size(bad, 4)[0] == -1, bad
    assert size([(2, 1, 2, 2)], 0)[0] == -1 and size([(2, 1, 2, 2)], 4, -1)[0] == -1
    # 3 Hg Wg >= 2^31 from the shapes alone: 2 tiles of 26754 x 26754 side by side give 26758 x 53514 x 3 = 2^31 + 1.2e9;
    # the largest grid below the bound passes
    assert size([(2, 1, 26754, 26754)], 2)[0] == -1
    assert size([(1, 1, 26754, 26754)], 2) == (0, (1, 26754, 26754))  # 3 * 26754^2 = 2147329548 < 2^31
    assert size([(1, 1, 26755, 26755)], 2)[0] == -1  # 3 * 26755^2 = 2147490075 >= 2^31
    assert size([(2 ** 31 - 1, 1, 2 ** 31 - 1, 2 ** 31 - 1)], 2 ** 31 - 1, 2 ** 31 - 1)[0] == -1  # nothing overflows on the way
    # the launch entry: the same refusals with NULL data and NULL outputs, T == 0 a no-op, nothing to write a no-op
    grid = lib.mvk_image_grid
    assert grid(descs([(2, 1, 26754, 26754)]), 1, 2, 2, 0.0, None, None, None) == -1
    assert grid(descs([(1, 1, 2, 2)] * (cap + 1)), cap + 1, 8, 2, 0.0, None, None, None) == -1
    assert grid(descs([(1, 0, 2, 2)]), 1, 8, 2, 0.0, None, None, None) == -1
    assert grid(None, 0, 8, 2, 0.0, None, None, None) == 0 and grid(descs([(0, 1, 2, 2)]), 1, 8, 2, 0.0, None, None, None) == 0
    assert grid(descs([(2, 1, 4, 4)], data=4096), 1, 8, 2, 0.0, None, None, None) == 0  # neither output wanted
