"""CVAE on the GPU: mvk_cond_latent_fwd / mvk_cond_latent_bwd called directly through the C ABI, entry-wise against float64, and
the public model against the goldens recorded from the reference and the float64 restatement of tests/cvae_ref.py.

Kernel.  Reference, case table (cvae_ref.CASES: L in {5, 64, 130} x B in {1, 3, 5, 260} x K in {1, 4} x conditioning pieces in
{none, (3,), (7,1), (130,), (1024,)} x prior NULL / given, the optional pointers dzc, gkl, kl_rows cycled over it; lv graded over
[-12, 6], plv over [-6, 6]) and error model live in tests/cvae_ref.py.  Per case:
1. every output of the forward and the backward launch, pre-filled with NaN, against the float64 reference:
   |got - ref| <= C_STAGE[stage] * base for EVERY entry; the copied conditioning columns bit for bit; a NaN left anywhere fails.
   The columns L .. L+C of dzc are ALWAYS filled with NaN: none may reach an output;
2. a second launch from the same buffers is bit-identical;
3. without a prior: the NULL form and two arrays of zeros write the same bits (z, kl, dmu, dlv);
4. test_argument_checks: every MVK_EINVAL branch returns without launching, B = 0 is MVK_OK and writes nothing.

Constants (cvae_ref.C_STAGE = 4x the largest |err| / base of the same formulas in plain torch fp32 on the CPU, backward by fp32
autograd, over the case table, rounded up; re-derived by test_cvae_host.py::test_error_constants, never from the HIP kernel):
    stage   torch fp32   C    set by
    z       0.80         4    l130-b260-k4-c1024-prior-null-gkl
    kl      0.44         2    l5-b260-k1-cnone-prior-null-kl_rows
    dmu     0.73         3    l64-b260-k4-cnone-std-null-kl_rows
    dlv     0.96         4    l130-b260-k1-c130-prior
    dpmu    0.55         3    l64-b260-k4-c7x1-prior-null-kl_rows
    dplv    0.93         4    l130-b260-k1-c7x1-prior-null-kl_rows
    cond    exact        -    (bit for bit)

Largest |err| / base of the HIP kernel on an MI355X (test_zz_report prints HIP_MEASURED), first run:
    z 0.80 (l130-b260-k4-c1024-prior-null-gkl), kl 0.37 (l5-b260-k4-c3-prior-null-dzc), dmu 0.73 (l64-b260-k4-cnone-std-null-kl_rows),
    dlv 1.16 (l130-b260-k1-c7x1-prior-null-kl_rows), dpmu 0.55 (l130-b260-k1-c130-prior), dplv 0.95 (same case as dlv); cond exact.
    At most 0.29 of C (dlv).
Factor by which each mutation of the reference exceeded the bound on the kernel's output, weakest named case (HIP_TEETH lines of
test_tolerance_rejects_mutated_reference): no_prior 4.7e5 (kl), sd_no_half 1.1e7 (z) / 2.1e6 (dlv), dpmu_sign 1.9e6 (dpmu),
drop_tail 8.9e5 (dmu) / 1.7e5 (dlv), swap_pieces inf (cond: not bit-equal).  Wall time of the whole file on an MI355X: 5.7 s.

Model.  Every golden case within the 1e-4 relative parity bar (loss, metrics, every gradient against float64 and against the
recorded statistics); encode / decode / predict / generate_from_prior shapes for N in {1, 3} and both flatten values; a custom
BaseConditionalDecoder without forward_concatenated; graph replay against the eager step in the same scope, bit for bit;
BaseTrainer for two epochs and a resume; save + AutoModel.load_from_folder with a pickled prior network, bit for bit.
"""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import cvae_ref as R
import golden_cases as G

pytestmark = pytest.mark.gpu
D = torch.device("cuda:0")
MEASURED = {}
_RUNS = {}


def _lib():
    from multivae_amd import _lib as L

    return L


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=D)


def launch(case, I, zero_prior=False):
    """Forward, then backward, from fresh NaN-filled outputs -> every array written, on the CPU, under the keys of
    cvae_ref.reference (None: not written).  zero_prior: a case without a prior passes two arrays of zeros instead of NULL."""
    Lb = _lib()
    sp = Lb.stream_ptr
    K, B, L = case.K, case.B, case.L
    C = sum(case.pieces)
    dv = lambda t: None if t is None else t.to(D).contiguous()
    mu, lv, eps = dv(I["mu"]), dv(I["lv"]), dv(I["eps"])
    pmu, plv = dv(I["pmu"]), dv(I["plv"])
    if zero_prior:
        pmu, plv = torch.zeros_like(mu), torch.zeros_like(lv)
    pieces = [dv(p) for p in I["pieces"]]
    dims = (ctypes.c_int * max(len(pieces), 1))(*case.pieces)
    zc = nan(K, B, L + C)
    kl = None if "kl_rows" in case.null else nan(B)
    Lb.call("mvk_cond_latent_fwd", Lb.ptr(mu), Lb.ptr(lv), Lb.ptr(pmu), Lb.ptr(plv), Lb.ptr(eps), Lb.ptr_array(pieces), dims,
            len(pieces), K, B, L, Lb.ptr(zc), Lb.ptr(kl), sp())
    dzc = dv(I["dzc"])
    if dzc is not None:
        dzc[..., L:] = float("nan")  # the conditioning columns of the upstream gradient are never read
    gkl = dv(I["gkl"])
    dmu, dlv = nan(B, L), nan(B, L)
    dpmu, dplv = (None, None) if pmu is None else (nan(B, L), nan(B, L))
    Lb.call("mvk_cond_latent_bwd", Lb.ptr(mu), Lb.ptr(lv), Lb.ptr(pmu), Lb.ptr(plv), Lb.ptr(eps), Lb.ptr(dzc), Lb.ptr(gkl), K, B,
            L, C, Lb.ptr(dmu), Lb.ptr(dlv), Lb.ptr(dpmu), Lb.ptr(dplv), sp())
    torch.cuda.synchronize()
    out = dict(z=zc[..., :L], cond=zc[..., L:] if C else None, kl=kl, dmu=dmu, dlv=dlv, dpmu=dpmu, dplv=dplv)
    return {k: (None if v is None else v.cpu().contiguous()) for k, v in out.items()}


def differing(a, b, keys=None):
    """The first array that both hold and that differs in its bits (None: none)."""
    for k in (keys or a):
        if a.get(k) is not None and b.get(k) is not None and not torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)):
            return k
    return None


def run_case(case):
    """(inputs, first launch, second launch, reference, bases) of a case: launched once per session, shared, left unchanged."""
    if case.name not in _RUNS:
        I = R.make_inputs(case)
        ref = R.reference(case, I)
        _RUNS[case.name] = (I, launch(case, I), launch(case, I), ref, R.bases(case, I, ref))
    return _RUNS[case.name]


@pytest.mark.parametrize("L,pieces", R.GROUPS, ids=[f"l{L}-c{'x'.join(map(str, p)) or 'none'}" for L, p in R.GROUPS])
def test_kernel_cases(L, pieces):
    for case in R.group_cases(L, pieces):
        I, got, got2, ref, base = run_case(case)
        assert differing(got, got2) is None, f"{case.name}: a second launch differs"
        for k, t in got.items():
            assert t is None or not bool(torch.isnan(t).any()), f"{case.name}: {k} holds a NaN"
        assert (got["kl"] is None) == ("kl_rows" in case.null) and (got["dpmu"] is None) == (not case.prior)
        ratios = R.ratios(case, I, got, ref=ref, base=base)
        print(case.name, {k: round(v, 3) for k, v in ratios.items()})
        for k, v in ratios.items():
            if v > MEASURED.get(k, (-1.0, ""))[0]:
                MEASURED[k] = (v, case.name)
        for k, v in ratios.items():
            assert v <= R.C_STAGE.get(k, 0.0), f"{case.name}: {k} worst |err| / base = {v:.3g} > C = {R.C_STAGE.get(k, 0.0)}"
        if not case.prior:
            alt = launch(case, I, zero_prior=True)
            k = differing(got, alt, ("z", "cond", "kl", "dmu", "dlv"))
            assert k is None, f"{case.name}: {k} differs between the NULL prior and a prior of zeros"


@pytest.mark.parametrize("mut,stages,names", R.TEETH, ids=[t[0] for t in R.TEETH])
def test_tolerance_rejects_mutated_reference(mut, stages, names):
    """The comparison of test_kernel_cases, with one deliberate mistake in the REFERENCE, must fail on the HIP kernel's output in
    every stage named for it on every case named for it (shown against torch fp32 in test_cvae_host.py)."""
    for name in names:
        case = R.CASE_BY_NAME[name]
        I, got, _, _, base = run_case(case)
        bad = R.ratios(case, I, got, mut=(mut,), base=base)
        for s in stages:
            f = bad[s] / R.C_STAGE.get(s, 1.0)
            print("HIP_TEETH", mut, name, s, f"{f:.3g}")
            assert f > 1.0, f"{mut} passes {s} on {name}: {f:.3g}x the bound"


def test_argument_checks():
    """MVK_EINVAL, without a launch (the sentinel-filled buffers stay as they are), for: NULL mu / lv / eps / zc / dmu / dlv;
    K = 0; L = 0; B < 0; n_cond < 0; n_cond = 9; pieces without cond or cond_dims; a NULL piece; a piece of width 0; pmu without
    plv and the reverse; backward: C < 0, dpmu / dplv without a prior, a prior without dpmu / dplv.  B = 0 is MVK_OK and
    writes nothing."""
    Lb = _lib()
    sp = Lb.stream_ptr
    t = torch.full((4096,), 7.0, device=D)
    p = Lb.ptr(t)

    def fwd(mu=p, lv=p, pmu=None, plv=None, eps=p, n=2, cond=True, dims=(3, 2), hole=None, K=2, B=3, L=5, zc=p, kl=p):
        arr = Lb.ptr_array([t] * max(n, 1))
        if hole is not None:
            arr[hole] = None
        cd = (ctypes.c_int * max(len(dims), 1))(*dims) if dims is not None else None
        Lb.call("mvk_cond_latent_fwd", mu, lv, pmu, plv, eps, arr if cond else None, cd, n, K, B, L, zc, kl, sp())

    def bwd(mu=p, lv=p, pmu=None, plv=None, eps=p, K=2, B=3, L=5, C=5, dmu=p, dlv=p, dpmu=None, dplv=None):
        Lb.call("mvk_cond_latent_bwd", mu, lv, pmu, plv, eps, None, None, K, B, L, C, dmu, dlv, dpmu, dplv, sp())

    bad = [lambda: fwd(mu=None), lambda: fwd(lv=None), lambda: fwd(eps=None), lambda: fwd(zc=None), lambda: fwd(K=0),
           lambda: fwd(L=0), lambda: fwd(B=-1), lambda: fwd(n=-1), lambda: fwd(n=9, dims=(1,) * 9), lambda: fwd(cond=False),
           lambda: fwd(dims=None), lambda: fwd(hole=1), lambda: fwd(dims=(3, 0)), lambda: fwd(pmu=p), lambda: fwd(plv=p),
           lambda: bwd(mu=None), lambda: bwd(lv=None), lambda: bwd(eps=None), lambda: bwd(dmu=None), lambda: bwd(dlv=None),
           lambda: bwd(K=0), lambda: bwd(L=0), lambda: bwd(B=-1), lambda: bwd(C=-1), lambda: bwd(pmu=p), lambda: bwd(plv=p),
           lambda: bwd(dpmu=p, dplv=p), lambda: bwd(pmu=p, plv=p), lambda: bwd(pmu=p, plv=p, dpmu=p),
           lambda: bwd(pmu=p, plv=p, dplv=p)]
    for i, f in enumerate(bad):
        with pytest.raises(Lb.MvkError):
            f()
            pytest.fail(f"bad call {i} was accepted")
    fwd(B=0)
    fwd(B=0, n=0, cond=False, dims=None)
    bwd(B=0)
    bwd(B=0, pmu=p, plv=p, dpmu=p, dplv=p)
    o = torch.zeros(16, device=D)
    fwd(n=8, dims=(1,) * 8, B=1, L=1, K=1, zc=Lb.ptr(o), kl=None)  # n_cond = MVK_MAX_MODALITIES itself is accepted: 9 floats
    torch.cuda.synchronize()
    assert bool((t == 7.0).all()) and bool((o[1:9] == 7.0).all()) and bool((o[9:] == 0.0).all())


def test_autograd_function_matches_the_kernel_reference():
    """kernels.CondLatentFn: pieces of any trailing shape are flattened, no gradient reaches them, want_kl=False gives no KL."""
    from multivae_amd import kernels

    case = R.CASE_BY_NAME["l5-b3-k4-c7x1-prior"]
    I, got, _, _, _ = run_case(case)
    leaves = [I[k].to(D).requires_grad_(True) for k in ("mu", "lv", "pmu", "plv")]
    pieces = [I["pieces"][0].reshape(3, 7, 1).to(D).requires_grad_(True), I["pieces"][1].to(D)]
    zc, kl = kernels.CondLatentFn.apply(I["eps"].to(D), *leaves, True, *pieces)
    (zc * I["dzc"].to(D)).sum().add((kl * I["gkl"].to(D)).sum()).backward()
    assert torch.equal(zc.detach().cpu()[..., :5], got["z"]) and torch.equal(zc.detach().cpu()[..., 5:], got["cond"])
    assert torch.equal(kl.detach().cpu(), got["kl"]) and pieces[0].grad is None
    for t, k in zip(leaves, ("dmu", "dlv", "dpmu", "dplv")):
        assert torch.equal(t.grad.cpu(), got[k]), k
    zc2, none = kernels.CondLatentFn.apply(I["eps"].to(D), leaves[0].detach(), leaves[1].detach(), None, None, False, *pieces)
    assert none is None and torch.equal(zc2.cpu()[..., :5], got["z"])


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def _prior(ccfg):
    from multivae_amd.models.nn.default_architectures import BaseDictEncoders, MultipleHeadJointEncoder

    dims = {m: ccfg.input_dims[m] for m in ccfg.conditioning_modalities}
    return MultipleHeadJointEncoder(BaseDictEncoders(dims, ccfg.latent_dim), args=ccfg)


def _model(cfg, decoder=None):
    from multivae_amd.models import CVAE, CVAEConfig

    params = {"scale": 1.0} if cfg["dist"] in ("normal", "laplace") else {}
    ccfg = CVAEConfig(conditioning_modalities=list(cfg["cond"]), main_modality=cfg["main"], input_dims=dict(R.case_dims(cfg)),
                      latent_dim=cfg["L"], beta=cfg["beta"], decoder_dist=cfg["dist"], decoder_dist_params=params)
    model = CVAE(ccfg, decoder=decoder, prior_network=_prior(ccfg) if cfg["prior"] else None)
    model.load_state_dict({k: G.t(v) for k, v in R.case_state_dict(cfg).items()})
    return model.to(D).train()


def _inputs(cfg):
    from multivae_amd.data.datasets.base import DatasetOutput

    _, data = R.case_inputs(cfg)
    return DatasetOutput(data={m: G.t(v).to(D) for m, v in data.items()})


@pytest.mark.parametrize("case", R.CVAE_CASES)
def test_golden(case):
    cfg, a = G.load_case(case)
    model = _model(cfg)
    model.zero_grad(set_to_none=True)
    out = model(_inputs(cfg), noise=G.t(a["eps"]).to(D), epoch=1, some_unknown_kwarg=3)
    out.loss.backward()
    assert abs(float(out.loss) - float(a["loss"])) <= 1e-4 * abs(float(a["loss"]))
    assert set(out.metrics) == {"kl", "recon_loss"} and set(out.keys()) == {"loss", "metrics"}
    for k in out.metrics:
        ref = float(a["metric/" + k])
        assert abs(float(out.metrics[k]) - ref) <= 1e-4 * max(1.0, abs(ref)), (k, float(out.metrics[k]), ref)
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in model.named_parameters()}
    _, g64 = R.reference_grads(cfg, a)
    for k, g in g64.items():
        err = float((grads[k].double().cpu() - g).abs().max())
        assert err <= 1e-4 * float(g.abs().max()) + 1e-9, (k, err, float(g.abs().max()))
    G.check_grads(a, grads, rtol=1e-4)
    model.eval()
    with torch.no_grad():
        enc = model.encode(_inputs(cfg), return_mean=True)
        assert torch.allclose(enc.z.cpu(), G.t(a["encode/z"]), rtol=1e-4, atol=1e-5)
        assert torch.allclose(model.decode(enc).reconstruction.cpu(), G.t(a["decode/recon"]), rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("case", ["cvae_tiny_stdprior", "cvae_tiny_prior_two_cond"])
def test_inference_shapes(case):
    cfg, a = G.load_case(case)
    model = _model(cfg).eval()
    inputs = _inputs(cfg)
    B, L, dims = cfg["B"], cfg["L"], R.case_dims(cfg)
    main = dims[cfg["main"]]
    cond_data = {m: inputs.data[m] for m in cfg["cond"]}
    for N in (1, 3):
        for flatten in (False, True):
            lead = (B,) if N == 1 else ((N * B,) if flatten else (N, B))
            for emb in (model.encode(inputs, N=N, flatten=flatten), model.generate_from_prior(cond_data, N=N, flatten=flatten)):
                assert tuple(emb.z.shape) == lead + (L,) and list(emb.cond_mod_data) == list(cfg["cond"])
                for m in cfg["cond"]:
                    assert tuple(emb.cond_mod_data[m].shape) == lead + dims[m]
                    assert torch.equal(emb.cond_mod_data[m].reshape(-1, *dims[m])[:B], inputs.data[m])
                C = sum(int(np.prod(dims[m])) for m in cfg["cond"])
                assert tuple(emb.zc.shape) == (N, B, L + C)  # the assembled decoder input the sample came out of
                assert torch.equal(emb.zc[..., :L].reshape(emb.z.shape), emb.z)
                flat = torch.cat([inputs.data[m].reshape(B, -1) for m in cfg["cond"]], 1)
                assert torch.equal(emb.zc[..., L:], flat.unsqueeze(0).expand(N, B, C))
                if flatten or N == 1:
                    assert tuple(model.decode(emb).reconstruction.shape) == lead + main
            if not flatten:  # the reference's decode takes [B, L] or [N, B, L]
                for cm in ("all", [cfg["main"]], list(dims), list(cfg["cond"])):
                    assert tuple(model.predict(inputs, cond_mod=cm, N=N)[cfg["main"]].shape) == lead + main
    mean = model.encode(inputs, N=3, return_mean=True).z
    assert tuple(mean.shape) == (3, B, L) and torch.equal(mean[0], mean[2])
    with pytest.raises(ValueError):
        model.predict(inputs, cond_mod=["nope"])
    if not cfg["prior"]:  # N(0, I) prior: z = 0 + exp(0) eps
        eps = torch.randn(3, B, L, device=D)
        assert torch.equal(model.generate_from_prior(cond_data, N=3, noise=eps).z, eps)


def test_custom_conditional_decoder_gives_the_same_loss():
    """A BaseConditionalDecoder without `forward_concatenated` (the reference contract: z and the conditioning dict) carrying
    the default decoder's weights: same loss, same gradients up to the order of the decoder's first-layer sums."""
    from multivae_amd.models.base.base_utils import ModelOutput
    from multivae_amd.models.nn.base_architectures import BaseConditionalDecoder
    from multivae_amd.models.nn.default_architectures import ConditionalDecoderMLP

    cfg, a = G.load_case("cvae_tiny_prior_two_cond")
    dims = R.case_dims(cfg)

    class Custom(BaseConditionalDecoder):
        def __init__(self):
            BaseConditionalDecoder.__init__(self)
            self.latent_dim = cfg["L"]
            self.network = ConditionalDecoderMLP(cfg["L"], {m: dims[m] for m in cfg["cond"]}, dims[cfg["main"]]).network
            self.calls = []

        def forward(self, z, cond_mods):
            self.calls.append((tuple(z.shape), list(cond_mods)))
            return ModelOutput(reconstruction=self.network(torch.cat([z] + [c.reshape(z.shape[0], -1) for c in cond_mods.values()], 1)).reconstruction)

    noise = G.t(a["eps"]).to(D)
    ref_model, custom = _model(cfg), _model(cfg, decoder=Custom())
    assert custom.model_config.custom_architectures == ["decoder", "prior_network"]
    outs = []
    for m in (ref_model, custom):
        o = m(_inputs(cfg), noise=noise)
        o.loss.backward()
        outs.append(o)
    assert custom.decoder.calls == [((cfg["B"], cfg["L"]), list(cfg["cond"]))]
    assert abs(float(outs[0].loss) - float(outs[1].loss)) <= 1e-6 * abs(float(outs[0].loss))
    g0, g1 = dict(ref_model.named_parameters()), dict(custom.named_parameters())
    for k in g0:
        assert torch.allclose(g0[k].grad, g1[k].grad, rtol=1e-4, atol=1e-6 * float(g0[k].grad.abs().max()) + 1e-12), k


def _synthetic(B=64, prior=True, seed=0):
    from multivae_amd.data.datasets.base import DatasetOutput
    from multivae_amd.models import CVAE, CVAEConfig

    torch.manual_seed(seed)
    dims = dict(x=(2, 5), c1=(6,), c2=(3, 1))
    ccfg = CVAEConfig(conditioning_modalities=["c1", "c2"], main_modality="x", input_dims=dims, latent_dim=5, beta=0.7)
    model = CVAE(ccfg, prior_network=_prior(ccfg) if prior else None).to(D).train()
    inputs = DatasetOutput(data={m: torch.rand(B, *d).to(D) for m, d in dims.items()})
    return model, inputs


@pytest.mark.parametrize("prior", [False, True])
def test_graph_replay_equals_eager(prior):
    from multivae_amd import kernels, schedule
    from multivae_amd.trainers import FlatParams, GraphedStep

    model, inputs = _synthetic(prior=prior)
    noise = torch.randn(64, 5, device=D)
    flat = FlatParams(model)
    res = []
    for _ in range(2):
        flat.zero_grad()
        with schedule.deferred_reductions(flat):  # the eager form of the step the graph captures (GraphedStep._body)
            out = model(inputs, noise=noise)
            out.loss.backward(gradient=kernels.unit_seed(out.loss))
        res.append((out.loss.detach().clone(), out.metrics["kl"].clone(), out.metrics["recon_loss"].clone(), flat.grad.clone()))
    assert all(torch.equal(a, b) for a, b in zip(res[0], res[1]))  # two eager steps: bit-identical
    gs = GraphedStep(model, flat, inputs, noise=noise)
    o = gs(inputs, noise=noise)
    torch.cuda.synchronize()
    assert torch.equal(o.loss.detach(), res[0][0])
    assert torch.equal(o.metrics["kl"], res[0][1]) and torch.equal(o.metrics["recon_loss"], res[0][2])
    diff = (flat.grad - res[0][3]).abs()
    assert torch.equal(flat.grad, res[0][3]), (int((diff > 0).sum()), float(diff.max()), float(res[0][3].abs().max()))


def test_trainer_two_epochs_resume_and_reload(tmp_path):
    from multivae_amd.data.datasets.base import MultimodalBaseDataset
    from multivae_amd.models import CVAE, AutoModel, CVAEConfig
    from multivae_amd.trainers import BaseTrainer, BaseTrainerConfig

    torch.manual_seed(0)
    n = 64
    dims = dict(x=(2, 5), c1=(6,), c2=(3, 1))
    ds = MultimodalBaseDataset(data={m: torch.rand(n, *d) for m, d in dims.items()})

    def make():
        torch.manual_seed(1)
        ccfg = CVAEConfig(conditioning_modalities=["c1", "c2"], main_modality="x", input_dims=dims, latent_dim=5)
        return CVAE(ccfg, prior_network=_prior(ccfg))

    def cfg(out, epochs):
        return BaseTrainerConfig(output_dir=str(out), per_device_train_batch_size=32, num_epochs=epochs, learning_rate=1e-3,
                                 steps_saving=1, use_hip_graph=True)

    t1 = BaseTrainer(make(), train_dataset=ds, training_config=cfg(tmp_path / "a", 2))
    hist = t1.train()
    losses = [h["train_epoch_loss"] for h in hist]
    assert len(losses) == 2 and all(np.isfinite(v) for v in losses) and losses[-1] < losses[0], losses
    ck = os.path.join(t1.training_dir, "checkpoint_epoch_1")
    assert os.path.exists(os.path.join(ck, "prior_network.pkl"))
    t2 = BaseTrainer(make(), train_dataset=ds, training_config=cfg(tmp_path / "b", 2), checkpoint=ck)
    hist2 = t2.train()
    assert len(hist2) == 1 and np.isfinite(hist2[0]["train_epoch_loss"])
    final = AutoModel.load_from_folder(os.path.join(t1.training_dir, "final_model"))
    assert type(final) is CVAE and final.prior_network is not None
    # save, then AutoModel: the trained model's loss bit for bit, the pickled prior network included
    from multivae_amd.data.datasets.base import DatasetOutput

    trained = t1.model.train()
    trained.save(str(tmp_path / "saved"))
    assert os.path.exists(str(tmp_path / "saved" / "prior_network.pkl"))
    back = AutoModel.load_from_folder(str(tmp_path / "saved")).to(D).train()
    assert type(back) is CVAE and back.model_config.custom_architectures == ["prior_network"]
    batch = DatasetOutput(data={m: v[:32].to(D) for m, v in ds.data.items()})
    noise = torch.randn(32, 5, device=D)
    a, b = trained(batch, noise=noise), back(batch, noise=noise)
    assert math.isfinite(float(a.loss)) and torch.equal(a.loss.detach(), b.loss.detach())
    assert torch.equal(a.metrics["kl"], b.metrics["kl"]) and torch.equal(a.metrics["recon_loss"], b.metrics["recon_loss"])


def test_zz_report():
    """Prints the head-room the HIP kernel showed in this session: the largest |err| / base per stage, with the case."""
    print("HIP_MEASURED", {k: (round(v, 2), n) for k, (v, n) in sorted(MEASURED.items())})
