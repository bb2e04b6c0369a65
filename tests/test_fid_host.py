"""CPU tests of the FIDEvaluator's host side: the float64 restatement of tests/fid_ref.py against the values recorded from the
reference (tests/golden/fid_cases.npz), the symmetric-eigh form of the distance against scipy's sqrtm form, what the kernel's shift
buys in fp32 (emulations of csrc/frechet.hip with and without it), and the drop-in surface (config, package names, AdaptShapeFID,
constructor errors)."""
import json

import numpy as np
import pytest
import torch

import fid_ref as F

GOLD = F.load_golden()
NAMES = list(F.GOLDEN_CASES)


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_reference(name):
    g = GOLD[name]
    D, N, seed, offset = F.GOLDEN_CASES[name]
    real, gen = F.make_pair(D, N, seed, offset)
    assert np.array_equal(real, g["real"]) and np.array_equal(gen, g["gen"]), "the fixture's inputs are not make_pair's"
    for acts, mu, sigma in ((real, g["mu0"], g["s0"]), (gen, g["mu1"], g["s1"])):
        m, s = F.stats64(acts)
        assert s.shape == sigma.shape == (() if D == 1 else (D, D))  # np.cov of one column is 0-d
        assert np.max(np.abs(m - mu)) <= 1e-9 * np.max(np.abs(mu)) and np.max(np.abs(s - sigma)) <= 1e-9 * np.max(np.abs(sigma))
    got = F.fd64(g["mu0"], g["s0"], g["mu1"], g["s1"])
    assert abs(got - g["fd"]) <= 1e-9 * abs(g["fd"]), (got, g["fd"])
    if name == "rankdef":
        assert N < D and np.linalg.matrix_rank(g["s0"]) < D


@pytest.mark.parametrize("name", NAMES)
def test_symmetric_eigh_form_agrees_with_sqrtm(name):
    from multivae_amd.metrics.fids import frechet_distance

    g = GOLD[name]
    args = (g["mu0"], g["s0"], g["mu1"], g["s1"])
    sc = F.scale(*args)
    gap = abs(F.fd_eigh64(*args) - g["fd"]) / sc
    print(name, f"eigh form against sqrtm form: {gap:.2e} of scale")
    assert gap <= F.EIGH_BAR
    # the shipped function is that form (torch float64, here on the CPU)
    t = [torch.as_tensor(np.atleast_1d(a)) for a in args]
    got = frechet_distance(*t)
    assert got.dtype == torch.float64 and got.dim() == 0
    assert abs(float(got) - g["fd"]) / sc <= F.EIGH_BAR


@pytest.mark.parametrize("name", NAMES)
def test_shifted_fp32_is_far_inside_the_bar(name):
    g = GOLD[name]
    sc = F.scale(g["mu0"], g["s0"], g["mu1"], g["s1"])
    b = F.GOLDEN_BATCHES[name]
    m0, s0 = F.emulate_shifted_fp32(g["real"], b)
    m1, s1 = F.emulate_shifted_fp32(g["gen"], b)
    gap = abs(F.fd64(m0, s0, m1, s1) - g["fd"]) / sc
    print(name, f"shifted fp32 emulation: {gap:.2e} of scale")
    assert gap <= F.BAR / 10
    for s, ref in ((s0, g["s0"]), (s1, g["s1"])):
        assert np.max(np.abs(np.atleast_2d(s) - np.atleast_2d(ref))) <= F.COV_BAR * np.max(np.abs(ref))
    for m, ref in ((m0, g["mu0"]), (m1, g["mu1"])):
        assert np.max(np.abs(m - ref)) <= F.MEAN_BAR * np.max(np.abs(ref))


def test_unshifted_fp32_misses_the_bar_on_the_offset_case():
    """Why the kernel shifts: raw fp32 second moments of features far from zero lose the covariance to cancellation."""
    g = GOLD[F.OFFSET_CASE]
    assert F.GOLDEN_CASES[F.OFFSET_CASE][3] >= 50.0
    sc = F.scale(g["mu0"], g["s0"], g["mu1"], g["s1"])
    b = F.GOLDEN_BATCHES[F.OFFSET_CASE]
    m0, s0 = F.unshifted_fp32(g["real"], b)
    m1, s1 = F.unshifted_fp32(g["gen"], b)
    gap = abs(F.fd64(m0, s0, m1, s1) - g["fd"]) / sc
    print(f"un-shifted fp32 emulation on the offset case: {gap:.2e} of scale")
    assert gap > 3 * F.BAR


def test_config_round_trip_and_defaults(tmp_path):
    from multivae_amd.metrics import EvaluatorConfig
    from multivae_amd.metrics.fids import FIDEvaluatorConfig

    cfg = FIDEvaluatorConfig()
    assert issubclass(FIDEvaluatorConfig, EvaluatorConfig)
    assert cfg.to_dict() == dict(name="FIDEvaluatorConfig", batch_size=512, wandb_path=None,
                                 inception_weights_path="../fid_model/model.pt", dims_inception=2048)
    other = FIDEvaluatorConfig(batch_size=3, dims_inception=64, inception_weights_path="w.pt")
    other.save_json(str(tmp_path), "fid")
    assert json.load(open(tmp_path / "fid.json"))["dims_inception"] == 64
    back = FIDEvaluatorConfig.from_json_file(str(tmp_path / "fid.json"))
    assert back == other and back.to_dict() == other.to_dict()


def test_package_surface():
    import multivae_amd.metrics as M
    import multivae_amd.metrics.fids as P

    names = ["FIDEvaluator", "FIDEvaluatorConfig", "AdaptShapeFID", "DeviceFrechet", "frechet_distance"]
    assert sorted(P.__all__) == sorted(names)
    for n in names:
        assert getattr(M, n) is getattr(P, n)
    assert issubclass(P.FIDEvaluator, M.Evaluator)
    assert set(M.__all__) == {"Evaluator", "EvaluatorConfig", "LikelihoodsEvaluator", "LikelihoodsEvaluatorConfig", "Reconstruction",
                              "ReconstructionConfig", "CoherenceEvaluator", "CoherenceEvaluatorConfig"}
    for method in ("get_frechet_distance", "calculate_frechet_distance", "unconditional_fids", "eval",
                   "compute_fid_from_conditional_generation", "compute_all_conditional_fids"):
        assert callable(getattr(P.FIDEvaluator, method))


@pytest.mark.parametrize("shape,want", [
    ((4,), (4, 3, 1, 1)), ((4, 6), (4, 3, 1, 6)), ((4, 5, 6), (4, 3, 5, 6)),
    ((4, 1, 5, 6), (4, 3, 5, 6)), ((4, 2, 5, 6), (4, 3, 5, 6)), ((4, 3, 5, 6), (4, 3, 5, 6)), ((4, 5, 5, 6), (4, 3, 5, 6)),
])
def test_adapt_shape(shape, want):
    from multivae_amd.metrics.fids import AdaptShapeFID

    x = torch.rand(*shape, generator=torch.Generator().manual_seed(1))
    y = AdaptShapeFID(resize=False)(x)
    assert tuple(y.shape) == want and y.device == x.device and y.dtype == x.dtype
    x4 = x.reshape(shape[0], *([1] * (4 - len(shape))), *shape[1:]) if len(shape) < 4 else x
    c = x4.shape[1]
    if c == 1:
        assert all(torch.equal(y[:, k], x4[:, 0]) for k in range(3))
    elif c == 2:
        assert torch.equal(y[:, :2], x4) and bool((y[:, 2] == 0).all())
    else:
        assert torch.equal(y, x4[:, :3])
    z = AdaptShapeFID()(x)
    assert tuple(z.shape) == (4, 3, 299, 299) and bool(torch.isfinite(z).all())


def test_adapt_shape_resize_and_five_dimensions():
    from multivae_amd.metrics.fids import AdaptShapeFID

    flat = torch.full((2, 3, 7, 9), 0.25)
    assert torch.allclose(AdaptShapeFID()(flat), torch.full((2, 3, 299, 299), 0.25), atol=1e-6)  # the weights of a resize sum to 1
    with pytest.raises(AttributeError, match="more than 3 dimensions"):
        AdaptShapeFID()(torch.rand(2, 1, 3, 4, 5))


def _tiny():
    from multivae_amd.data.datasets.base import MultimodalBaseDataset
    from multivae_amd.models import MVTCAE, MVTCAEConfig

    torch.manual_seed(1)
    dims = dict(a=(1, 12, 12), b=(3, 11, 13))
    model = MVTCAE(MVTCAEConfig(n_modalities=2, latent_dim=5, input_dims=dims))
    g = torch.Generator().manual_seed(2)
    return model, MultimodalBaseDataset(data={m: torch.rand(7, *dims[m], generator=g) for m in dims})


def test_default_inception_path_is_not_built():
    from multivae_amd.metrics.fids import FIDEvaluator, FIDEvaluatorConfig

    model, ds = _tiny()
    with pytest.raises(NotImplementedError, match="custom_encoders"):
        FIDEvaluator(model, ds, None, FIDEvaluatorConfig(batch_size=3))
    assert "custom_encoders" in FIDEvaluator.__doc__ and "InceptionV3" in FIDEvaluator.__doc__


def test_unfitted_sampler_is_refused_and_host_distance():
    from multivae_amd.metrics.fids import FIDEvaluator, FIDEvaluatorConfig
    from multivae_amd.samplers import GaussianMixtureSampler, GaussianMixtureSamplerConfig

    model, ds = _tiny()
    enc = dict(a=torch.nn.Flatten(), b=torch.nn.Flatten())
    sampler = GaussianMixtureSampler(model, GaussianMixtureSamplerConfig(n_components=2))
    with pytest.raises(AttributeError, match="not fitted"):
        FIDEvaluator(model, ds, None, FIDEvaluatorConfig(batch_size=3), sampler=sampler, custom_encoders=enc)
    ev = FIDEvaluator(model, ds, None, FIDEvaluatorConfig(batch_size=3), custom_encoders=enc)
    assert ev.inception_transform is None and set(ev.model_fds) == {"a", "b"}
    # calculate_frechet_distance: numpy arrays or tensors in, a Python float out; D = 1 comes as 0-d covariances
    for name in NAMES:
        g = GOLD[name]
        sc = F.scale(g["mu0"], g["s0"], g["mu1"], g["s1"])
        got = ev.calculate_frechet_distance(g["mu0"], g["s0"], g["mu1"], g["s1"])
        assert isinstance(got, float) and abs(got - g["fd"]) / sc <= F.EIGH_BAR
        t = [torch.as_tensor(a) for a in (g["mu0"], g["s0"], g["mu1"], g["s1"])]
        assert ev.calculate_frechet_distance(*t, eps=1e-3) == got
    ev.finish()
