"""csrc/frechet.hip through the C ABI against the float64 statistics of tests/fid_ref.py, the device `frechet_distance` against
scipy's sqrtm form, and the FIDEvaluator end to end on a tiny model.

Bars (fid_ref): the distance within BAR = 1e-4 of scale = |mean0 - mean1|^2 + tr cov0 + tr cov1 (the project's parity bar, taken
relative to scale because the distance is a difference of these terms), and for the well-separated cases also within 1e-4 of the
distance itself; covariance entries within 1e-5 of max |cov|; means within 1e-6 of max |mean|.

1. test_kernel_cases: D in {1, 5, T - 1, T, T + 1, 2 T + 3} for the kernel's tile edge T, batch sequences (1,), (3, 3, 1),
   (37, 37, 5) and (chunk + 1, 2) for the kernel's row chunk; streams of different distributions; state and outputs pre-filled with
   NaN; cov exactly symmetric; a second run from a fresh state bit-identical.  One row in all gives the NaN covariance numpy gives.
2. The offset case (features around 500 at unit scale) within the bars.
3. X1 = NULL leaves stream 1 empty and stream 0's statistics bit-identical to the two-stream run.
4. Every MVK_EINVAL branch.
5. frechet_distance on the device against fd64 for every golden case, the rank-deficient one included.
6. FIDEvaluator on a 7-row dataset with input_dims a: (1,12,12), b: (3,11,13) and batch_size 3: every reported distance against
   fd64 of the activations its encoders produced.

Largest distance of the HIP kernel from float64 on an MI355X (test_zz_report prints HIP_MEASURED; first GPU run of the kernel):
    kernel cases, worst over the 18 with more than one row: mean 1.78e-08 of max |mean| (D65-3+3+1; bar 1e-6), cov 3.03e-07 of
        max |cov| (D64-65+2; bar 1e-5), terms 2.08e-08 of scale (D5-65+2), distance 1.08e-07 of scale and 1.16e-07 of itself
        (D131-3+3+1, seven rows for 131 columns; bar 1e-4); the offset case: mean 0, cov 5.80e-08, distance 2.38e-09 of scale
    frechet_distance on the device (float64 eigh) against scipy's sqrtm form: 4.95e-09 of scale (rankdef; bar 1e-6), the other
        cases <= 5e-16; DeviceFrechet on the golden activations: 4.88e-09 of scale (small)
    FIDEvaluator against fd64 of the activations its encoders produced: 1.09e-08 of scale (a to b; bar 1e-4)
"""
import ctypes
import functools
import warnings

import numpy as np
import pytest
import torch

import fid_ref as F

pytestmark = pytest.mark.gpu
D0 = torch.device("cuda:0")
MEASURED = {}
EINVAL = -1


def _mods():
    from multivae_amd import _lib, kernels

    return _lib, kernels


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=D0, dtype=dtype).contiguous()


def nan64(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device=D0)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def note(key, value, name):
    if value > MEASURED.get(key, (-1.0, ""))[0]:
        MEASURED[key] = (value, name)


def run_stream(real, gen, batches):
    """(mean, cov, terms) after the updates of `batches`, from a NaN-filled state and NaN-filled outputs."""
    _, K = _mods()
    D = real.shape[1]
    state = K.fd_new_state(D, D0)
    state.fill_(float("nan"))
    at = 0
    for i, b in enumerate(batches):
        x0, x1 = dev(real[at:at + b]), None if gen is None else dev(gen[at:at + b])
        if i == 0:
            K.fd_begin(state, x0, x1)
        K.fd_update(state, x0, x1)
        at += b
    out = K.fd_finish(state, D, mean=nan64(2, D), cov=nan64(2, D, D), terms=nan64(5))
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def reference(D, batches):
    """Inputs and float64 statistics of a kernel case, computed once."""
    N = sum(batches)
    real, gen = F.make_pair(D, N, 7)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # np.cov of one row divides by zero and says so
        (m0, s0), (m1, s1) = F.stats64(real), F.stats64(gen)
    s0, s1 = np.atleast_2d(s0), np.atleast_2d(s1)
    fd = F.fd64(m0, s0, m1, s1) if N > 1 else float("nan")
    return real, gen, np.stack([m0, m1]), np.stack([s0, s1]), fd, F.scale(m0, s0, m1, s1)


def check_stats(name, mean, cov, terms, m64, s64, fd, scale, n0, n1):
    from multivae_amd.metrics.fids import frechet_distance

    mean_h, cov_h, terms_h = mean.cpu().numpy(), cov.cpu().numpy(), terms.cpu().numpy()
    assert terms_h[3] == n0 and terms_h[4] == n1
    assert np.array_equal(cov_h, cov_h.transpose(0, 2, 1), equal_nan=True), "cov is not exactly symmetric"
    e_mean = float(np.max(np.abs(mean_h - m64)) / np.max(np.abs(m64)))
    e_cov = float(np.max(np.abs(cov_h - s64)) / np.max(np.abs(s64)))
    got = float(frechet_distance(mean[0], cov[0], mean[1], cov[1]))
    e_fd = abs(got - fd) / scale
    d = m64[0] - m64[1]
    want_terms = np.array([d @ d, np.trace(s64[0]), np.trace(s64[1])])
    e_terms = float(np.max(np.abs(terms_h[:3] - want_terms)) / scale)
    print(name, f"mean {e_mean:.2e} cov {e_cov:.2e} terms {e_terms:.2e} distance {e_fd:.2e} of scale, {abs(got - fd) / abs(fd):.2e} of itself")
    note("mean", e_mean, name), note("cov", e_cov, name), note("terms", e_terms, name), note("distance / scale", e_fd, name)
    note("distance / distance", abs(got - fd) / abs(fd), name)
    assert e_mean <= F.MEAN_BAR, f"{name}: mean is {e_mean:.3g} (relative) from float64"
    assert e_cov <= F.COV_BAR, f"{name}: cov is {e_cov:.3g} (of max |cov|) from float64"
    assert e_terms <= F.BAR, f"{name}: terms are {e_terms:.3g} of scale from float64"
    assert e_fd <= F.BAR, f"{name}: the distance is {e_fd:.3g} of scale from float64"
    assert abs(got - fd) <= F.BAR * abs(fd), f"{name}: the distance is {abs(got - fd) / abs(fd):.3g} (relative) from float64"


@pytest.mark.parametrize("batch_index", range(4))
@pytest.mark.parametrize("dim_index", range(6))
def test_kernel_cases(dim_index, batch_index):
    _, K = _mods()
    D = F.kernel_dims(K.fd_tile())[dim_index]
    batches = F.kernel_batches(K.fd_chunk())[batch_index]
    name = f"D{D}-{'+'.join(map(str, batches))}"
    real, gen, m64, s64, fd, scale = reference(D, batches)
    N = sum(batches)
    mean, cov, terms = run_stream(real, gen, batches)
    mean2, cov2, terms2 = run_stream(real, gen, batches)
    assert same_bits(mean, mean2) and same_bits(cov, cov2) and same_bits(terms, terms2), "a second run differs"
    if N == 1:  # np.cov of one row is NaN; the mean is the row itself, exactly
        assert bool(torch.isnan(cov).all()) and np.isnan(s64).all()
        assert np.array_equal(mean.cpu().numpy(), np.stack([real[0], gen[0]]).astype(np.float64))
        assert terms.cpu().numpy()[3:].tolist() == [1.0, 1.0] and bool(torch.isnan(terms[1:3]).all())
        return
    check_stats(name, mean, cov, terms, m64, s64, fd, scale, N, N)


def test_offset_case():
    g = F.load_golden()[F.OFFSET_CASE]
    assert float(np.min(g["real"])) > 50.0
    mean, cov, terms = run_stream(g["real"], g["gen"], F.GOLDEN_BATCHES[F.OFFSET_CASE])
    m64, s64 = np.stack([g["mu0"], g["mu1"]]), np.stack([g["s0"], g["s1"]])
    N = len(g["real"])
    check_stats("offset", mean, cov, terms, m64, s64, g["fd"], F.scale(g["mu0"], g["s0"], g["mu1"], g["s1"]), N, N)


def test_one_stream_alone():
    _, K = _mods()
    T = K.fd_tile()
    batches = (37, 37, 5)
    real, gen, m64, s64, _, _ = reference(T + 1, batches)
    both = run_stream(real, gen, batches)
    alone = run_stream(real, None, batches)
    assert alone[2].cpu().numpy()[3:].tolist() == [float(sum(batches)), 0.0], "stream 1 is not empty"
    assert same_bits(both[0][0], alone[0][0]) and same_bits(both[1][0], alone[1][0]), "stream 0 depends on stream 1"
    assert same_bits(both[2][1:2], alone[2][1:2])  # tr cov0
    assert bool(torch.isnan(alone[0][1]).all()) and bool(torch.isnan(alone[1][1]).all())  # an empty stream: 0 / 0, as np.mean says


def test_invalid_arguments():
    lib_, K = _mods()
    lib, ptr, sp = lib_.load(), lib_.ptr, lib_.stream_ptr
    D, n = 5, 3
    x = torch.rand(n, D, device=D0)
    state = K.fd_new_state(D, D0)
    state.fill_(7.0)
    mean, cov, terms = nan64(2, D), nan64(2, D, D), nan64(5)
    n64 = ctypes.c_int64(-5)
    assert lib.mvk_fd_state_bytes(0, ctypes.byref(n64)) == EINVAL and lib.mvk_fd_state_bytes(-1, ctypes.byref(n64)) == EINVAL
    assert lib.mvk_fd_state_bytes(D, None) == EINVAL and n64.value == -5
    assert lib.mvk_fd_state_bytes(D, ctypes.byref(n64)) == 0 and 0 < n64.value <= state.numel() * 8
    for fn in (lib.mvk_fd_begin, lib.mvk_fd_update):
        def call(x0=x, x1=x, n=n, D=D, st=state):
            return fn(ptr(x0), ptr(x1), n, D, ptr(st), sp())

        assert call(x0=None) == EINVAL and call(st=None) == EINVAL and call(n=0) == EINVAL and call(n=-1) == EINVAL
        assert call(D=0) == EINVAL and call(D=-3) == EINVAL

    def fin(st=state, D=D, mean=mean, cov=cov, terms=terms):
        return lib.mvk_fd_finish(ptr(st), D, ptr(mean), ptr(cov), ptr(terms), sp())

    assert fin(st=None) == EINVAL and fin(D=0) == EINVAL and fin(mean=None) == EINVAL and fin(cov=None) == EINVAL
    assert fin(terms=None) == EINVAL
    torch.cuda.synchronize()
    assert bool((state == 7.0).all()) and bool(torch.isnan(mean).all()) and bool(torch.isnan(cov).all()) and bool(torch.isnan(terms).all())
    # X1 = NULL is no error
    assert lib.mvk_fd_begin(ptr(x), None, n, D, ptr(state), sp()) == 0 and lib.mvk_fd_update(ptr(x), None, n, D, ptr(state), sp()) == 0
    assert fin() == 0
    torch.cuda.synchronize()
    assert terms.cpu().numpy()[3:].tolist() == [3.0, 0.0] and bool(torch.isfinite(mean[0]).all())


@pytest.mark.parametrize("name", list(F.GOLDEN_CASES))
def test_frechet_distance_on_the_device(name):
    from multivae_amd.metrics.fids import frechet_distance

    g = F.load_golden()[name]
    args = (g["mu0"], g["s0"], g["mu1"], g["s1"])
    got = frechet_distance(*[dev(np.atleast_1d(a), torch.float64) for a in args])
    assert got.is_cuda and got.dtype == torch.float64 and got.dim() == 0
    sc = F.scale(*args)
    gap = abs(float(got) - g["fd"]) / sc
    print(name, f"device eigh form against sqrtm form: {gap:.2e} of scale")
    note("frechet_distance / scale", gap, name)
    assert gap <= F.EIGH_BAR
    # and the streaming object on the case's activations
    from multivae_amd.metrics.fids import DeviceFrechet

    stats, at = DeviceFrechet(g["real"].shape[1]), 0
    for b in F.GOLDEN_BATCHES[name]:
        stats.update(dev(g["real"][at:at + b]), dev(g["gen"][at:at + b]))
        at += b
    got = float(stats.compute())
    note("DeviceFrechet / scale", abs(got - g["fd"]) / sc, name)
    assert abs(got - g["fd"]) <= F.BAR * sc
    if name in F.SEPARATED:
        assert abs(got - g["fd"]) <= F.BAR * abs(g["fd"])


# ---- the evaluator -------------------------------------------------------------------------------------------------------------
DIMS = dict(a=(1, 12, 12), b=(3, 11, 13))
N_ROWS, BATCH, WIDTH = 7, 3, 5


def _dataset(n=N_ROWS):
    from multivae_amd.data.datasets.base import MultimodalBaseDataset

    g = torch.Generator().manual_seed(11)
    return MultimodalBaseDataset(data={m: torch.rand(n, *DIMS[m], generator=g) for m in DIMS})


class Embed(torch.nn.Module):
    """Flatten + a fixed Linear to WIDTH features; keeps a host copy of every activation batch it produced."""

    def __init__(self, d, seed, wrap):
        super().__init__()
        lin = torch.nn.Linear(d, WIDTH)
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            lin.weight.copy_(torch.randn(WIDTH, d, generator=g) / d ** 0.5)
            lin.bias.copy_(torch.randn(WIDTH, generator=g))
        self.net = torch.nn.Sequential(torch.nn.Flatten(), lin)
        self.wrap, self.seen = wrap, []

    def forward(self, x):
        from multivae_amd._output import ModelOutput

        out = self.net(x)
        self.seen.append(out.detach().cpu().numpy().copy())
        return ModelOutput(embedding=out) if self.wrap else out


def _fd_of_seen(enc):
    """fd64 and scale of what an encoder recorded since the last call: real and generated batches alternate."""
    real, gen = np.concatenate(enc.seen[0::2]), np.concatenate(enc.seen[1::2])
    enc.seen.clear()
    assert real.shape == gen.shape == (N_ROWS, WIDTH)
    return F.fd_of_acts(real, gen)


def _close(got, enc, name):
    want, sc = _fd_of_seen(enc)
    gap = abs(got - want) / sc
    print(name, f"evaluator distance {got:.6g} against float64 {want:.6g}: {gap:.2e} of scale")
    note("evaluator / scale", gap, name)
    assert isinstance(got, float) and gap <= F.BAR, (name, got, want)


def test_evaluator(tmp_path):
    from multivae_amd._output import ModelOutput
    from multivae_amd.metrics import FIDEvaluator, FIDEvaluatorConfig
    from multivae_amd.models import MVTCAE, MVTCAEConfig
    from multivae_amd.samplers import GaussianMixtureSampler, GaussianMixtureSamplerConfig

    torch.manual_seed(5)
    model = MVTCAE(MVTCAEConfig(n_modalities=2, latent_dim=5, input_dims=dict(DIMS))).to(D0).eval()
    enc = dict(a=Embed(144, 1, wrap=False), b=Embed(429, 2, wrap=True))
    cfg = FIDEvaluatorConfig(batch_size=BATCH)
    ev = FIDEvaluator(model, _dataset(), str(tmp_path), cfg, custom_encoders=enc)
    torch.manual_seed(0)
    out = ev.eval()
    assert isinstance(out, ModelOutput) and list(out.keys()) == ["fd_a_sampler_prior", "fd_b_sampler_prior"]
    for m in DIMS:
        assert len(enc[m].seen) == 6  # three batches, a real and a generated embedding each
        _close(out[f"fd_{m}_sampler_prior"], enc[m], f"prior {m}")
    # conditional generation
    fd = ev.compute_fid_from_conditional_generation(["a"], "b")
    assert ev.metrics["Conditional FD from a to b"] == fd
    _close(fd, enc["b"], "a to b")
    all_b = ev.compute_all_conditional_fids("b")
    _close(all_b["Conditional FD from a to b"], enc["b"], "all: a to b")
    assert all_b["Mean FD from 1 modalities to b"] == np.mean([all_b["Conditional FD from a to b"]])
    all_a = ev.compute_all_conditional_fids("a")
    _close(all_a["Conditional FD from b to a"], enc["a"], "all: b to a")
    assert all_a["Mean FD from 1 modalities to a"] == np.mean([all_a["Conditional FD from b to a"]])
    assert set(all_a.keys()) == {"fd_a_sampler_prior", "fd_b_sampler_prior", "Conditional FD from a to b", "Conditional FD from b to a",
                                 "Mean FD from 1 modalities to b", "Mean FD from 1 modalities to a"}
    ev.finish()
    assert "The FD for modality a with sampler prior" in (tmp_path / "metrics.log").read_text()
    # a fitted sampler
    sampler = GaussianMixtureSampler(model, GaussianMixtureSamplerConfig(n_components=2))
    sampler.fit(_dataset(n=64), generator=torch.Generator(device=D0).manual_seed(3))
    ev2 = FIDEvaluator(model, _dataset(), None, cfg, sampler=sampler, custom_encoders=enc)
    out2 = ev2.unconditional_fids()
    assert list(out2.keys()) == [f"fd_{m}_sampler_{sampler.name}" for m in DIMS] and sampler.name == "GaussianMixtureSampler"
    for m in DIMS:
        _close(out2[f"fd_{m}_sampler_{sampler.name}"], enc[m], f"sampler {m}")
    ev2.finish()


def test_zz_report():
    for k in sorted(MEASURED):
        print("HIP_MEASURED", k, f"{MEASURED[k][0]:.2e}", MEASURED[k][1])
