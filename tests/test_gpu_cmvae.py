"""CMVAE on the GPU: mvk_cmvae_latent_fwd / mvk_cmvae_latent_bwd / mvk_cmvae_assign called directly through the C ABI, entry-wise
against the float64 restatement of the reference's literal form, and the public model against the goldens recorded from the
reference.

Kernel.  Reference, case table (cmvae_ref.CASES: 48 cases cycling Ls in {1, 5, 64, 70}, S in {1, 3, 32}, C in {1, 2, 10, 65}, M in
{1, 2, 3}, K in {1, 4}, B in {1, 3, 5, 260}, Normal / Laplace, IWAE / DReG, masks absent / present with row 0 left a single modality,
one logit at -inf, posterior means spread 1 and 6 around the cluster means, cluster stds graded over [0.3, 3]) and error model live
in tests/cmvae_ref.py.  Per case:
1. every output of the three launches, pre-filled with NaN, against float64: |got - ref| <= C_STAGE[stage] * base for EVERY entry
   (for dmeans / dlogits after taking off the literal form's own 1e-20 on underflowed clusters, which is no rounding: cmvae_ref.ratios)
   (z, lpz, lqz, lqw, resp; dmu, dsd, dmeans, dlogits after one mvk_colsum_acc over the partial rows; pc_z, norm_llik), the argmax
   exactly; a NaN left anywhere fails;
2. a second launch from the same buffers is bit-identical;
3. test_argument_checks: every MVK_EINVAL branch returns without launching, B = 0 / R = 0 is MVK_OK and writes nothing;
4. test_tolerance_rejects_mutated_reference: a reference with log pi dropped, with an unweighted mean gradient or with pi omitted
   from dlogits exceeds the bound on the kernel's output.

Constants (cmvae_ref.C_STAGE = 4x the largest |err| / base of the closed form in plain torch fp32 on the CPU, backward by fp32
autograd, over the case table, rounded up; re-derived by test_cmvae_host.py::test_error_constants, never from the HIP kernel):
    stage      torch fp32   C    set by
    z          0.65         3    17-l5-s32-c2-m1-k4-b260-laplace-dreg-sp1
    lpz        0.65         3    19-l70-s3-c65-m2-k1-b260-laplace-iwae-masked-sp1
    lqz        0.49         2    05-l5-s32-c10-m3-k4-b260-laplace-iwae-sp1
    lqw        0.46         2    45-l5-s1-c1-m2-k4-b260-normal-iwae-masked-sp6
    resp       0.90         4    47-l70-s32-c10-m3-k4-b260-normal-dreg-masked-sp1
    dmu        0.74         3    17-l5-s32-c2-m1-k4-b260-laplace-dreg-sp1
    dsd        0.92         4    05-l5-s32-c10-m3-k4-b260-laplace-iwae-sp1
    dmeans     0.45         2    35-l70-s32-c65-m2-k4-b1-laplace-dreg-masked-sp1
    dlogits    5.69         23   31-l70-s3-c10-m3-k1-b5-normal-iwae-pruned-sp1
    pc_z       0.76         4    24-l1-s1-c10-m3-k1-b260-laplace-dreg-pruned-sp1
    norm_llik  1.06         5    05-l5-s32-c10-m3-k4-b260-laplace-iwae-sp1

Largest |err| / base of the HIP kernels on an MI355X (test_zz_report prints HIP_MEASURED):
    z 0.46, lpz 0.57, lqz 0.43, lqw 0.61, resp 0.69, dmu 0.80, dsd 0.94, dmeans 0.39 (28-l1-s3-c65-m2-k4-b1-laplace-dreg-masked-sp1),
    dlogits 0.75, pc_z 1.51 (24-l1-s1-c10-m3-k1-b260-laplace-dreg-pruned-sp1), norm_llik 0.77.  At most 0.38 of C (pc_z).
Factor by which each mutation of the reference exceeded the bound on the kernel's output, weakest named case (HIP_TEETH lines):
no_logpi 5.2e4 (lpz) / 2.8e5 (resp), unweighted_means 3.0e6 (dmeans), no_pi_dlogits 1.0e4 (dlogits).
Wall time of the whole file on an MI355X: 6.4 s (30 items; the slowest, the trainer and the graph replay, 0.8 s each).

Model.  Every golden case within the 1e-4 relative parity bar (loss, lws, us / ws against the reference's float32 run; every
gradient against the reference run again in float64 on the same draws); C = 1 against MMVAEPlus;
encode / decode / predict / generate_from_prior shapes; predict_clusters, prune_clusters and compute_joint_nll against their
goldens; a forward with a pruned cluster; graph replay against the eager step, bit for bit; BaseTrainer for two epochs and a
resume; save + AutoModel.load_from_folder, bit for bit; the reference-written folder through AutoModel.
"""
import math
import os

import numpy as np
import pytest
import torch

import cmvae_ref as R
import golden_cases as G

pytestmark = pytest.mark.gpu
D = torch.device("cuda:0")
FAM = R.FAMILY_CODE
MEASURED = {}
_RUNS = {}


def _lib():
    from multivae_amd import _lib as L

    return L


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=D)


def launch(case, I):
    """The three launches from fresh NaN-filled outputs -> every array written, on the CPU, under the keys of cmvae_ref."""
    Lb = _lib()
    sp, pa = Lb.stream_ptr, Lb.ptr_array
    M, K, B, Ls, C, Dd = case.M, case.K, case.B, case.Ls, case.C, case.D
    fam = FAM[case.family]
    dv = lambda t: t.to(D).contiguous()
    mu, sd, nz = [dv(t) for t in I["mu"]], [dv(t) for t in I["sd"]], [dv(t) for t in I["noise"]]
    masks = None if I["masks"] is None else [dv(m.to(torch.uint8)) for m in I["masks"]]
    marr = pa(masks) if masks is not None else None
    cmean, csd, logits, wsd = dv(I["cmean"]), dv(I["csd"]), dv(I["logits"]), dv(I["wsd"])
    z, lpz, lqz = [nan(K, B, Dd) for _ in range(M)], [nan(K, B) for _ in range(M)], [nan(K, B) for _ in range(M)]
    lq_all, lqw, resp = [nan(M, K, B) for _ in range(M)], [nan(K, B) for _ in range(M)], [nan(K, B, C) for _ in range(M)]
    Lb.call("mvk_cmvae_latent_fwd", pa(mu), pa(sd), pa(nz), marr, Lb.ptr(cmean), Lb.ptr(csd), Lb.ptr(logits), Lb.ptr(wsd), M, K, B,
            Dd, fam, C, pa(z), pa(lpz), pa(lqz), pa(lq_all), Ls, pa(lqw), pa(resp), sp())
    w, dz = [dv(t) for t in I["w"]], [dv(t) for t in I["dz"]]
    gs = torch.tensor([I["gscale"]], dtype=torch.float32, device=D)
    dmu, dsd = [nan(B, Dd) for _ in range(M)], [nan(B, Dd) for _ in range(M)]
    n = C * Ls + C
    rows = nan(B, n)
    Lb.call("mvk_cmvae_latent_bwd", pa(mu), pa(sd), pa(nz), pa(z), marr, Lb.ptr(cmean), Lb.ptr(csd), Lb.ptr(logits), Lb.ptr(wsd),
            pa(w), pa(lq_all), pa(lqz), pa(resp), pa(dz), M, K, B, Dd, fam, case.dreg, C, Lb.ptr(gs), pa(dmu), pa(dsd),
            Lb.ptr(rows), Ls, float(I["beta"]), sp())
    dparams = torch.zeros(n, dtype=torch.float32, device=D)
    ws = torch.empty(max(4 * n * ((B + 63) // 64 + 1), 1024), dtype=torch.float32, device=D)
    Lb.call("mvk_colsum_acc", Lb.ptr(rows), None, 0, Lb.ptr(dparams), B, n, Lb.ptr(ws), ws.numel(), sp())
    R_ = B
    az = dv(I["assign_z"])
    pc, nll = nan(C, R_), nan(R_)
    amax = torch.full((R_,), -7, dtype=torch.int64, device=D)
    Lb.call("mvk_cmvae_assign", Lb.ptr(az), Lb.ptr(cmean), Lb.ptr(csd), Lb.ptr(logits), R_, Ls, fam, C, Lb.ptr(pc), Lb.ptr(amax),
            Lb.ptr(nll), sp())
    torch.cuda.synchronize()
    cpu = lambda t: [x.cpu() for x in t] if isinstance(t, list) else t.cpu()
    return dict(z=cpu(z), lpz=cpu(lpz), lqz=cpu(lqz), lqw=cpu(lqw), resp=cpu(resp), lq_all=cpu(lq_all), dmu=cpu(dmu), dsd=cpu(dsd),
                rows=cpu(rows), dmeans=cpu(dparams[: C * Ls]).view(C, Ls), dlogits=cpu(dparams[C * Ls :]), pc_z=cpu(pc),
                norm_llik=cpu(nll), argmax=cpu(amax))


def differing(a, b):
    """The first array of two launches that differs in its bits (None: none)."""
    for k in a:
        xs, ys = (a[k], b[k]) if isinstance(a[k], list) else ([a[k]], [b[k]])
        for x, y in zip(xs, ys):
            if x.dtype == torch.float32:
                x, y = x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)
            if not torch.equal(x, y):
                return k
    return None


def run_case(case):
    """(inputs, first launch, second launch, references, bases) of a case: launched once per session, shared, left unchanged."""
    if case.name not in _RUNS:
        I = R.make_inputs(case)
        ref = R.reference(case, I)
        aref = R.assign(case, I)
        _RUNS[case.name] = (I, launch(case, I), launch(case, I), ref, R.bases(case, I, ref), aref, R.assign_bases(case, I, aref))
    return _RUNS[case.name]


GROUPS = [R.CASES[i : i + 6] for i in range(0, len(R.CASES), 6)]


@pytest.mark.parametrize("group", GROUPS, ids=[f"cases{g[0].name[:2]}-{g[-1].name[:2]}" for g in GROUPS])
def test_kernel_cases(group):
    for case in group:
        I, got, got2, ref, base, aref, abase = run_case(case)
        assert differing(got, got2) is None, f"{case.name}: a second launch differs in {differing(got, got2)}"
        for k, t in got.items():
            for x in (t if isinstance(t, list) else [t]):
                assert x.dtype != torch.float32 or not bool(torch.isnan(x).any()), f"{case.name}: {k} holds a NaN"
        ratios = R.ratios(got, ref, base, R.FWD_STAGES + R.BWD_STAGES)
        ratios.update(R.ratios(got, aref, abase, R.ASSIGN_STAGES))
        print(case.name, {k: round(v, 3) for k, v in ratios.items()})
        for k, v in ratios.items():
            if v > MEASURED.get(k, (-1.0, ""))[0]:
                MEASURED[k] = (v, case.name)
        for k, v in ratios.items():
            assert v <= R.C_STAGE[k], f"{case.name}: {k} worst |err| / base = {v:.3g} > C = {R.C_STAGE[k]}"
        assert torch.equal(got["argmax"], aref["argmax"]), f"{case.name}: argmax"
        if case.pruned:  # the absent cluster: exactly zero responsibility and gradients
            j = case.seed % case.C
            assert all(bool((r[..., j] == 0).all()) for r in got["resp"])
            assert bool((got["dmeans"][j] == 0).all()) and float(got["dlogits"][j]) == 0.0


@pytest.mark.parametrize("mut,stages,names", R.TEETH, ids=[t[0] for t in R.TEETH])
def test_tolerance_rejects_mutated_reference(mut, stages, names):
    """The comparison of test_kernel_cases, with one deliberate mistake in the REFERENCE, must fail on the HIP kernel's output in
    every stage named for it on every case named for it (shown against torch fp32 in test_cmvae_host.py)."""
    for name in names:
        case = R.CASE_BY_NAME[name]
        I, got, _, _, base, _, _ = run_case(case)
        bad = R.ratios(got, R.reference(case, I, mut=(mut,)), base, stages)
        for s in stages:
            f = bad[s] / R.C_STAGE[s]
            print("HIP_TEETH", mut, name, s, f"{f:.3g}")
            assert f > 1.0, f"{mut} passes {s} on {name}: {f:.3g}x the bound"


def test_argument_checks():
    """MVK_EINVAL, without a launch (the sentinel-filled buffers stay as they are), for: a NULL in every pointer argument and in the
    pointer arrays; M = 0, M = 9; K = 0; D = 1; shared_dims = 0 and = D; family 2; C = 0, C = 129; a cluster table over the LDS
    cap; B < 0; M * K * B >= 2^31; assign: R < 0, Ls = 0.  B = 0 / R = 0 is MVK_OK and writes nothing; C = 128 is accepted."""
    Lb = _lib()
    sp = Lb.stream_ptr
    t = torch.full((1 << 16,), 7.0, device=D)
    p = Lb.ptr(t)

    def arr(M=2, hole=None):
        a = Lb.ptr_array([t] * max(M, 1))
        if hole is not None:
            a[hole] = None
        return a

    def fwd(M=2, K=2, B=3, Dd=5, fam=0, C=3, Ls=3, null=None, hole=None):
        a = {k: arr(M, hole if null == k + "[]" else None) for k in ("mu", "sd", "nz", "z", "lpz", "lqz", "lq_all", "lqw", "resp")}
        q = {k: p for k in ("cmean", "csd", "logits", "wsd")}
        for k in list(a) + list(q):
            if null == k:
                (a if k in a else q)[k] = None
        Lb.call("mvk_cmvae_latent_fwd", a["mu"], a["sd"], a["nz"], None, q["cmean"], q["csd"], q["logits"], q["wsd"], M, K, B, Dd,
                fam, C, a["z"], a["lpz"], a["lqz"], a["lq_all"], Ls, a["lqw"], a["resp"], sp())

    def bwd(M=2, K=2, B=3, Dd=5, fam=0, C=3, Ls=3, null=None, hole=None):
        names = ("mu", "sd", "nz", "z", "w", "lq_all", "lqz", "resp", "dz", "dmu", "dsd")
        a = {k: arr(M, hole if null == k + "[]" else None) for k in names}
        q = {k: p for k in ("cmean", "csd", "logits", "wsd", "dparams")}
        for k in list(a) + list(q):
            if null == k:
                (a if k in a else q)[k] = None
        Lb.call("mvk_cmvae_latent_bwd", a["mu"], a["sd"], a["nz"], a["z"], None, q["cmean"], q["csd"], q["logits"], q["wsd"], a["w"],
                a["lq_all"], a["lqz"], a["resp"], a["dz"], M, K, B, Dd, fam, 0, C, None, a["dmu"], a["dsd"], q["dparams"], Ls, 1.0,
                sp())

    def asg(R_=4, Ls=3, fam=0, C=3, null=None):
        q = {k: (None if null == k else p) for k in ("z", "cmean", "csd", "logits", "pc", "amax")}
        Lb.call("mvk_cmvae_assign", q["z"], q["cmean"], q["csd"], q["logits"], R_, Ls, fam, C, q["pc"], q["amax"], p, sp())

    bad = []
    for f, ptrs, arrs in ((fwd, ("cmean", "csd", "logits", "wsd"), ("mu", "sd", "nz", "z", "lpz", "lqz", "lq_all", "lqw", "resp")),
                          (bwd, ("cmean", "csd", "logits", "wsd", "dparams"),
                           ("mu", "sd", "nz", "z", "w", "lq_all", "lqz", "resp", "dz", "dmu", "dsd"))):
        bad += [lambda f=f, k=k: f(null=k) for k in ptrs + arrs]
        bad += [lambda f=f, k=k: f(null=k + "[]", hole=1) for k in arrs]
        bad += [lambda f=f: f(M=0), lambda f=f: f(M=9), lambda f=f: f(K=0), lambda f=f: f(Dd=1, Ls=1), lambda f=f: f(Ls=0),
                lambda f=f: f(Ls=5), lambda f=f: f(fam=2), lambda f=f: f(fam=-1), lambda f=f: f(C=0), lambda f=f: f(C=129),
                lambda f=f: f(C=128, Ls=64, Dd=65), lambda f=f: f(B=-1), lambda f=f: f(M=8, K=1 << 14, B=1 << 14)]
    bad += [lambda k=k: asg(null=k) for k in ("z", "cmean", "csd", "logits", "pc", "amax")]
    bad += [lambda: asg(R_=-1), lambda: asg(Ls=0), lambda: asg(fam=2), lambda: asg(C=0), lambda: asg(C=129),
            lambda: asg(C=128, Ls=64)]
    for i, f in enumerate(bad):
        with pytest.raises(Lb.MvkError):
            f()
            pytest.fail(f"bad call {i} was accepted")
    fwd(B=0)
    bwd(B=0)
    asg(R_=0)
    torch.cuda.synchronize()
    assert bool((t == 7.0).all())
    # the cap itself is accepted: C = 128 clusters of 3 dims, one row
    zeros, ones, o = torch.zeros(512, device=D), torch.ones(512, device=D), torch.zeros(256, device=D)
    first = torch.full((1,), -7, dtype=torch.int64, device=D)
    Lb.call("mvk_cmvae_assign", Lb.ptr(zeros), Lb.ptr(zeros), Lb.ptr(ones), Lb.ptr(zeros), 1, 3, 0, 128, Lb.ptr(o), Lb.ptr(first), None,
            sp())
    torch.cuda.synchronize()
    assert bool((t == 7.0).all()) and torch.allclose(o[:128].cpu(), torch.full((128,), 1.0 / 128)) and bool((o[128:] == 0).all())
    assert int(first) == 0  # all equal: the first maximum


def test_autograd_function_matches_the_kernel_launches():
    """kernels.CMVAELatentFn + MMVAEState: the same bits as the direct launches, gradients for means / logits / mu / sd, none for the
    stds; kernels.cmvae_assign likewise."""
    from multivae_amd import kernels

    case = R.CASES[1]
    I, got, _, _, _, _, _ = run_case(case)
    M, Ls = case.M, case.Ls
    st = kernels.MMVAEState()
    st.shared_dims, st.beta = Ls, float(I["beta"])
    mus = [t.to(D).requires_grad_(True) for t in I["mu"]]
    sds = [t.to(D).requires_grad_(True) for t in I["sd"]]
    cmean, logits = I["cmean"].to(D).requires_grad_(True), I["logits"].to(D).requires_grad_(True)
    csd, wsd = I["csd"].to(D).requires_grad_(True), I["wsd"].to(D).requires_grad_(True)
    masks = None if I["masks"] is None else [m.to(D) for m in I["masks"]]
    zs = kernels.CMVAELatentFn.apply(st, [t.to(D) for t in I["noise"]], masks, FAM[case.family], case.dreg, wsd, csd, cmean, logits,
                                     *mus, *sds)
    st.w, st.gloss = [t.to(D) for t in I["w"]], torch.tensor([I["gscale"]], device=D)
    sum((z * dz.to(D)).sum() for z, dz in zip(zs, I["dz"])).backward()
    for c in range(M):
        assert torch.equal(zs[c].detach().cpu(), got["z"][c]) and torch.equal(st.lpz[c].cpu(), got["lpz"][c])
        assert torch.equal(st.resp[c].cpu(), got["resp"][c]) and torch.equal(st.lqw[c].cpu(), got["lqw"][c])
        assert torch.equal(mus[c].grad.cpu(), got["dmu"][c]) and torch.equal(sds[c].grad.cpu(), got["dsd"][c])
    assert torch.equal(cmean.grad.cpu(), got["dmeans"]) and torch.equal(logits.grad.cpu(), got["dlogits"])
    assert csd.grad is None and wsd.grad is None
    pc, amax, nll = kernels.cmvae_assign(I["assign_z"].to(D), cmean.detach(), csd.detach(), logits.detach(), FAM[case.family], True)
    assert torch.equal(pc.cpu(), got["pc_z"]) and torch.equal(amax.cpu(), got["argmax"]) and torch.equal(nll.cpu(), got["norm_llik"])


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def _model(cfg, **over):
    from multivae_amd.models import CMVAE, CMVAEConfig

    dims = R.case_dims(cfg)
    kw = dict(n_modalities=len(dims), latent_dim=R.case_latent_dim(cfg), input_dims=dict(dims), K=cfg["K"],
              modalities_specific_dim=cfg["S"], prior_and_posterior_dist=cfg["family"], loss=cfg["loss"], beta=cfg["beta"],
              uses_likelihood_rescaling=cfg["rescaling"], learn_modality_prior=True, number_of_clusters=cfg["C"])
    kw.update(over)
    model = CMVAE(CMVAEConfig(**kw))
    model.load_state_dict({k: G.t(v) for k, v in R.case_state_dict(cfg).items()}, strict=True)
    return model.to(D).train()


def _inputs(cfg, rows=None):
    from multivae_amd.data.datasets.base import DatasetOutput

    _, data, masks = R.case_inputs(cfg)
    sl = slice(None) if rows is None else rows
    kw = dict(data={m: G.t(v)[sl].to(D) for m, v in data.items()})
    if masks is not None:
        kw["masks"] = {m: G.t(v)[sl].to(D) for m, v in masks.items()}
    return DatasetOutput(**kw)


def _noise(a, mods, prefix="noise/"):
    return {c: {k[len(prefix) + len(c) + 1 :]: G.t(v).to(D) for k, v in a.items() if k.startswith(f"{prefix}{c}/")} for c in mods}


@pytest.mark.parametrize("name", R.CMVAE_CASES)
def test_golden(name):
    cfg, a = G.load_case(name)
    model = _model(cfg)
    assert [[k, list(p.shape), bool(p.requires_grad)] for k, p in model.named_parameters()] == cfg["params"]
    inputs = _inputs(cfg)
    mods = [m for m in cfg["names"] if "lws/" + m in a]
    model.zero_grad(set_to_none=True)
    out = model(inputs, noise=_noise(a, mods), detailed_output=True)
    out.loss.backward()
    loss = float(out.loss.detach())
    assert abs(loss - float(a["loss"])) <= 1e-4 * abs(float(a["loss"])), (loss, float(a["loss"]))
    assert abs(loss - float(a["loss64"])) <= 1e-4 * abs(float(a["loss64"])), (loss, float(a["loss64"]))
    L = cfg["L"]
    for m in mods:
        lw, ref = out["lws"][m].cpu(), G.t(a["lws/" + m])
        assert float((lw - ref).abs().max()) <= 1e-4 * float(ref.abs().max()), m
        assert torch.allclose(out["zss"][m][..., :L].cpu(), G.t(a["us/" + m]), rtol=1e-4, atol=1e-5)
        assert torch.allclose(out["zss"][m][..., L:].cpu(), G.t(a["ws/" + m]), rtol=1e-4, atol=1e-5)
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in model.named_parameters()}
    for k in ["_pc_params", "mean_clusters.0", "r_logvars_priors." + mods[-1]]:
        assert "gsum/" + k in a and float(a["gsum/" + k][1]) > 0, k  # the new parameters do receive a gradient in the reference
    # the stored gradient statistics are the reference's run again in float64 on the recorded draws (make_cmvae_golden.py; its
    # own float32 gradients are 3e-6 ... 4e-4 away from those: cfg["ref_fp32_grad_distance"])
    print(name, "worst sampled-entry error:", G.check_grads(a, grads, rtol=1e-4), "reference fp32:", cfg["ref_fp32_grad_distance"])


def test_single_cluster_equals_mmvaeplus():
    """C = 1 with a zero mean and a zero logit is MMVAE+ with a standard shared prior (log-variance 0 in the shared dims, the fixed
    w prior in the private ones): the two latent paths agree on the loss and on the encoder / decoder gradients."""
    from multivae_amd.models import MMVAEPlus, MMVAEPlusConfig

    cfg, a = G.load_case("cmvae_tiny_laplace_dreg")
    cfg = dict(cfg, C=1)
    sd = {k: G.t(v) for k, v in R.case_state_dict(cfg).items()}
    sd["mean_clusters.0"].zero_()
    sd["logvar_clusters.0"].zero_()
    sd["_pc_params"].zero_()
    sd["w_logvar_prior"].zero_()
    cm = _model(cfg)
    cm.load_state_dict(sd, strict=True)
    dims = R.case_dims(cfg)
    mp = MMVAEPlus(MMVAEPlusConfig(n_modalities=len(dims), latent_dim=cfg["L"], input_dims=dict(dims), K=cfg["K"],
                                   modalities_specific_dim=cfg["S"], prior_and_posterior_dist=cfg["family"], loss=cfg["loss"],
                                   beta=cfg["beta"], learn_modality_prior=True))
    shared = {k: v for k, v in sd.items() if k.startswith(("encoders.", "decoders."))}
    missing = mp.load_state_dict(shared, strict=False)
    assert not missing.unexpected_keys
    with torch.no_grad():
        for m in dims:
            mp.logvars_priors[m].copy_(sd["r_logvars_priors." + m])
    mp = mp.to(D).train()
    cm = cm.to(D)
    noise = _noise(a, list(dims))
    oc, om = cm(_inputs(cfg), noise=noise), mp(_inputs(cfg), noise=noise)
    oc.loss.backward()
    om.loss.backward()
    lc, lm = float(oc.loss.detach()), float(om.loss.detach())
    assert abs(lc - lm) <= 1e-4 * abs(lm), (lc, lm)
    gm = dict(mp.named_parameters())
    for k, p in cm.named_parameters():
        if k in shared:
            ref = gm[k].grad
            assert float((p.grad - ref).abs().max()) <= 1e-4 * float(ref.abs().max()) + 1e-9, k


@pytest.mark.parametrize("option", ["joint_prior", "single_prior"])
def test_inference_shapes(option):
    cfg, _ = G.load_case("cmvae_tiny_normal_iwae")
    model = _model(cfg, reconstruction_option=option).eval()
    inputs = _inputs(cfg)
    B, L, S, dims = cfg["B"], cfg["L"], cfg["S"], R.case_dims(cfg)
    for N in (1, 3):
        for flatten in (False, True):
            lead = (B,) if N == 1 else ((N * B,) if flatten else (N, B))
            for cond in ("all", ["mod2"], ["mod1", "mod3"]):
                for mean in (False, True):
                    emb = model.encode(inputs, cond_mod=cond, N=N, flatten=flatten, return_mean=mean)
                    assert tuple(emb.z.shape) == lead + (L,) and emb.one_latent_space is False
                    assert list(emb.modalities_z) == list(dims)
                    assert all(tuple(v.shape) == lead + (S,) for v in emb.modalities_z.values())
                if flatten or N == 1:
                    rec = model.decode(emb)
                    assert all(tuple(rec[m].shape) == lead + dims[m] for m in dims)
            pred = model.predict(inputs, cond_mod="mod1", N=N, flatten=flatten)
            assert all(tuple(pred[m].shape) == lead + dims[m] for m in dims)
    mean = model.encode(inputs, cond_mod=["mod2"], N=3, return_mean=True)
    enc = model.encoders["mod2"](inputs.data["mod2"])
    assert torch.equal(mean.z[0], enc.embedding) and torch.equal(mean.z[2], enc.embedding)  # one modality's mean, not an average
    for n in (1, 3):
        gen = model.generate_from_prior(n)
        assert tuple(gen.z.shape) == (n, L) and gen.one_latent_space is False
        assert all(tuple(gen.modalities_z[m].shape) == (n, S) for m in dims)
        assert all(tuple(v.shape) == (n,) + dims[m] for m, v in model.decode(gen).items())


def test_predict_and_prune_clusters_golden():
    from multivae_amd.data.datasets.base import MultimodalBaseDataset

    cfg, a = G.load_case("cmvae_predict_prune")
    model = _model(cfg).eval()
    mods = cfg["names"]
    pred = model.predict_clusters(_inputs(cfg), compute_lliks=True, noise={m: G.t(a["predict_noise/" + m]).to(D) for m in mods})
    assert set(pred.keys()) == {"clusters", "pc_zs", "norm_lliks"}
    assert torch.equal(pred.clusters.cpu(), G.t(a["clusters"]))
    assert torch.allclose(pred.norm_lliks.cpu(), G.t(a["norm_lliks"]), rtol=1e-4, atol=1e-6)
    for m in mods:
        assert torch.allclose(pred.pc_zs[m].cpu(), G.t(a["pc_zs/" + m]), rtol=1e-4, atol=1e-30), m
    assert set(model.predict_clusters(_inputs(cfg)).keys()) == {"clusters", "pc_zs"}
    _, data, _ = R.case_inputs(cfg)
    ds = MultimodalBaseDataset(data={m: G.t(v) for m, v in data.items()})
    noise = [[{m: G.t(a[f"prune_noise/{p}/{i}/{m}"]).to(D) for m in mods} for i in range(cfg["n_batches"])]
             for p in range(cfg["n_passes"])]
    h = model.prune_clusters(ds, batch_size=cfg["batch_size"], noise=noise)
    ref = a["h_values"]
    print("h_values", [float(x) for x in h], "reference", ref.tolist())
    assert len(h) == len(ref)
    for x, y in zip(h, ref):
        assert (math.isinf(float(x)) and math.isinf(y)) or abs(float(x) - y) <= 1e-4 * abs(y), (float(x), y)
    assert type(model.n_clusters) is int and model.n_clusters == int(a["n_clusters_final"])
    assert torch.equal(model._pc_params.detach().cpu(), G.t(a["pc_params_final"]))
    out = model(_inputs(cfg))  # a forward with pruned clusters (logits of -inf) is finite, and so are its gradients
    out.loss.backward()
    assert math.isfinite(float(out.loss.detach()))
    assert all(bool(torch.isfinite(p.grad).all()) for p in model.parameters() if p.grad is not None)
    dead = torch.isinf(model._pc_params.detach())
    assert bool(dead.any()) and bool((model._pc_params.grad[dead] == 0).all())


def test_vote_ties_on_the_device():
    """The majority vote of predict_clusters is torch.mode on the device: among equally frequent clusters the smallest index, as on
    the host (tests/test_cmvae_host.py) and in the reference."""
    votes = torch.tensor([[3, 1], [1, 3], [2, 2], [4, 0], [5, 5], [0, 7]], device=D)
    assert torch.mode(votes, dim=-1)[0].tolist() == [1, 1, 2, 0, 5, 0]
    three = torch.tensor([[2, 2, 1], [0, 3, 3], [4, 1, 0], [6, 5, 6]], device=D)
    assert torch.mode(three, dim=-1)[0].tolist() == [2, 3, 0, 6]
    # and through the model: two modalities that disagree on every row
    cfg, _ = G.load_case("cmvae_predict_prune")
    model = _model(cfg).eval()
    from multivae_amd import kernels

    real = kernels.cmvae_assign

    def fake(z, *a, **k):
        pc, amax, nll = real(z, *a, **k)
        B = z.shape[0] // 4
        forced = torch.tensor([3, 1, 1, 3], device=D).repeat_interleave(B)  # per modality: 3, 1, 1, 3 -> a 2 : 2 tie
        return pc, forced, nll

    kernels.cmvae_assign = fake
    try:
        assert model.predict_clusters(_inputs(cfg)).clusters.tolist() == [1] * cfg["B"]
    finally:
        kernels.cmvae_assign = real


def test_joint_nll_golden():
    from multivae_amd.data.datasets.base import DatasetOutput

    cfg, a = G.load_case("cmvae_joint_nll")
    model = _model(cfg)
    before = dict(model.rescale_factors)
    assert any(v != 1.0 for v in before.values()) and cfg["beta"] != 1.0  # forcing both to 1 matters in this case
    nll = model.compute_joint_nll(_inputs(cfg), K=cfg["nll_K"], noise=_noise(a, cfg["names"]))
    assert abs(float(nll) - float(a["joint_nll"])) <= 1e-4 * abs(float(a["joint_nll"])), (float(nll), float(a["joint_nll"]))
    assert model.beta == cfg["beta"] and dict(model.rescale_factors) == before  # restored
    inc = _inputs(cfg)
    with pytest.raises(AttributeError):
        model.compute_joint_nll(DatasetOutput(data=inc.data, masks={m: torch.ones(cfg["B"], dtype=torch.bool, device=D) for m in inc.data}))


def _synthetic(B=64, seed=0, **over):
    from multivae_amd.data.datasets.base import DatasetOutput
    from multivae_amd.models import CMVAE, CMVAEConfig

    torch.manual_seed(seed)
    dims = dict(a=(2, 5), b=(6,), c=(3, 1))
    kw = dict(n_modalities=3, latent_dim=5, input_dims=dims, K=3, modalities_specific_dim=3, number_of_clusters=4, beta=0.7)
    kw.update(over)
    model = CMVAE(CMVAEConfig(**kw)).to(D).train()
    inputs = DatasetOutput(data={m: torch.rand(B, *d).to(D) for m, d in dims.items()})
    return model, inputs, dims


@pytest.mark.parametrize("loss", ["dreg_looser", "iwae_looser"])
def test_graph_replay_equals_eager(loss):
    from multivae_amd import kernels, schedule
    from multivae_amd.trainers import FlatParams, GraphedStep

    model, inputs, dims = _synthetic(loss=loss)
    K, B, L, S = 3, 64, 5, 3
    mods = list(dims)
    lo = torch.finfo(torch.float32).eps - 1.0
    u = lambda *s: torch.empty(*s, device=D).uniform_(lo, 1.0)
    noise = {c: dict(u=u(K, B, L), w=u(K, B, S), **{r: u(K, B, S) for r in mods if r != c}) for c in mods}
    flat = FlatParams(model)
    # the graph first, on a model whose parameters have no autograd history yet (as the trainer does): the cluster parameters'
    # gradients arrive through autograd's own accumulation nodes, and such a node kept alive by an earlier eager step stays tied
    # to the stream of that step, which a capture on another stream must not touch
    gs = GraphedStep(model, flat, inputs, noise=noise)
    o = gs(inputs, noise=noise)
    torch.cuda.synchronize()
    graph_loss, graph_grad = o.loss.detach().clone(), flat.grad.clone()
    res = []
    for _ in range(2):
        flat.zero_grad()
        with schedule.deferred_reductions(flat):  # the eager form of the step the graph captures (GraphedStep._body)
            out = model(inputs, noise=noise)
            out.loss.backward(gradient=kernels.unit_seed(out.loss))
        res.append((out.loss.detach().clone(), flat.grad.clone()))
        del out
    assert all(torch.equal(a, b) for a, b in zip(res[0], res[1]))  # two eager steps: bit-identical
    assert float(model._pc_params.grad.abs().sum()) > 0 and float(model.mean_clusters[0].grad.abs().sum()) > 0
    assert torch.equal(graph_loss, res[0][0])
    diff = (graph_grad - res[0][1]).abs()
    assert torch.equal(graph_grad, res[0][1]), (int((diff > 0).sum()), float(diff.max()), float(res[0][1].abs().max()))


def test_trainer_two_epochs_resume_and_reload(tmp_path):
    from multivae_amd.data.datasets.base import DatasetOutput, MultimodalBaseDataset
    from multivae_amd.models import CMVAE, AutoModel, CMVAEConfig
    from multivae_amd.trainers import BaseTrainer, BaseTrainerConfig

    torch.manual_seed(0)
    n = 64
    dims = dict(a=(2, 5), b=(6,), c=(3, 1))
    ds = MultimodalBaseDataset(data={m: torch.rand(n, *d) for m, d in dims.items()})

    def make():
        torch.manual_seed(1)
        return CMVAE(CMVAEConfig(n_modalities=3, latent_dim=5, input_dims=dims, K=2, modalities_specific_dim=3, number_of_clusters=4))

    def cfg(out, epochs):
        return BaseTrainerConfig(output_dir=str(out), per_device_train_batch_size=32, num_epochs=epochs, learning_rate=1e-3,
                                 steps_saving=1, use_hip_graph=True)

    t1 = BaseTrainer(make(), train_dataset=ds, training_config=cfg(tmp_path / "a", 2))
    start = {k: v.detach().clone() for k, v in t1.model.state_dict().items()}
    hist = t1.train()
    losses = [h["train_epoch_loss"] for h in hist]
    assert len(losses) == 2 and all(np.isfinite(v) for v in losses) and losses[-1] < losses[0], losses
    end = t1.model.state_dict()
    for k in ("_pc_params", "mean_clusters.0", "r_logvars_priors.a"):  # the new parameters train
        assert not torch.equal(end[k].cpu(), start[k].cpu()), k
    for k in ("logvar_clusters.0", "w_logvar_prior", "w_mean_prior", "r_mean_priors.a"):  # the fixed ones do not
        assert torch.equal(end[k].cpu(), start[k].cpu()), k
    ck = os.path.join(t1.training_dir, "checkpoint_epoch_1")
    t2 = BaseTrainer(make(), train_dataset=ds, training_config=cfg(tmp_path / "b", 2), checkpoint=ck)
    hist2 = t2.train()
    assert len(hist2) == 1 and np.isfinite(hist2[0]["train_epoch_loss"])
    assert type(AutoModel.load_from_folder(os.path.join(t1.training_dir, "final_model"))) is CMVAE
    trained = t1.model.train()
    trained.save(str(tmp_path / "saved"))
    assert sorted(os.listdir(str(tmp_path / "saved"))) == ["environment.json", "model.pt", "model_config.json"]
    back = AutoModel.load_from_folder(str(tmp_path / "saved")).to(D).train()
    assert type(back) is CMVAE and back.n_clusters == 4
    batch = DatasetOutput(data={m: v[:32].to(D) for m, v in ds.data.items()})
    K, B = 2, 32
    noise = {c: dict(u=torch.rand(K, B, 5, device=D) - 0.5, w=torch.rand(K, B, 3, device=D) - 0.5,
                     **{r: torch.rand(K, B, 3, device=D) - 0.5 for r in dims if r != c}) for c in dims}
    x, y = trained(batch, noise=noise), back(batch, noise=noise)
    assert math.isfinite(float(x.loss.detach())) and torch.equal(x.loss.detach(), y.loss.detach())


def test_reference_written_folder_loads():
    """A folder written by the reference's `model.save` (model.pt and model_config.json) loads through AutoModel with
    strict=True: names, shapes and values."""
    from multivae_amd.data.datasets.base import DatasetOutput
    from multivae_amd.models import CMVAE, AutoModel

    folder = os.path.join(R.GOLDEN, "cmvae_reference_folder")
    assert sorted(os.listdir(folder)) == ["model.pt", "model_config.json"]
    model = AutoModel.load_from_folder(folder)
    assert type(model) is CMVAE and model.n_clusters == 4 and model.reconstruction_option == "single_prior"
    assert model.model_config.beta == 2.5 and model.objective == "iwae_looser"
    for i, p in enumerate(model.parameters()):
        n = p.numel()
        v = ((torch.arange(n, dtype=torch.float64) + 13 * i) % 127) / 32 - 2 + i / 4096
        assert torch.equal(p.detach().cpu(), v.reshape(p.shape).to(p.dtype)), i
    flags = {k: p.requires_grad for k, p in model.named_parameters()}
    assert flags["_pc_params"] and flags["mean_clusters.3"] and flags["r_logvars_priors.mod2"]
    assert not (flags["logvar_clusters.0"] or flags["w_logvar_prior"] or flags["w_mean_prior"] or flags["r_mean_priors.mod1"])
    pred = model.to(D).eval().predict_clusters(DatasetOutput(data=dict(mod1=torch.zeros(4, 2, device=D), mod2=torch.zeros(4, 3, device=D))))
    assert tuple(pred.clusters.shape) == (4,) and tuple(pred.pc_zs["mod1"].shape) == (4, 4)


def test_zz_report():
    """Prints the head-room the HIP kernel showed in this session: the largest |err| / base per stage, with the case."""
    print("HIP_MEASURED", {k: (round(v, 2), n) for k, (v, n) in sorted(MEASURED.items())})
