"""The seven MMVAE / MMVAE+ entry points of csrc/mmvae.hip (mvk_mmvae_std_fwd/bwd, mvk_mmvae_latent_fwd/bwd,
mvk_mmvae_objective_fwd, mvk_mmvaeplus_cross_latent_fwd/bwd) called directly, stage by stage, against float64.

Reference, case table (mmvae_ref.CASES: every case says which edge it is there for) and error model live in tests/mmvae_ref.py;
tests/test_mmvae_ref_host.py pins that reference to oracle.elbo on the CPU.  Per case:

1. every output array of latent_fwd, objective_fwd, latent_bwd and the mvk_colsum_acc finish of the prior gradient against the
   float64 reference of that stage evaluated on the fp32 arrays the kernel consumed (its own z, lpz, lqz, lqw, w, read back),
   |got - ref| <= C_STAGE[stage] * base for EVERY entry (no entry is excluded: the Laplace sign(z - mu) is decided on the
   same fp32 z on both sides);
2. exact properties: rows whose conditioning modality is absent have lw == 0, w == 1/K, rowcoef == 0 and add exactly nothing
   to dmu / dsd; sum_k w within K * 2^-23 of 1 (every w is one expf over a sum of K terms: relative error of the sum
   <= (K - 1) 2^-24, of a quotient 2^-24);
3. a second launch from the same buffers is bit-identical;
4. the loss equals -sum (lse_k lw - log K) / n_avail (IWAE) or -sum (w lw) / n_avail (DReG) of the kernel's OWN lw in float64
   within C_STAGE["loss"] * u * (2 S + (K + 2) M B), S = sum |obj_b| / n_avail (the accumulation alone, suspect 2).

Constants (mmvae_ref.C_STAGE = 4x the largest |err| / base of the same stage in plain torch fp32 on the CPU over the case table,
rounded up; re-derived by test_mmvae_ref_host.py::test_error_constants):
    stage    torch fp32   C     set by
    z        1.29         6     big-m2-k10-b64-l20-laplace-dreg
    lpz      3.43         14    p-m2-k10-b512-l130-ls64-normal-dreg-b0.5
    lq_all   5.73         23    big-m8-k2-b512-l5-normal-iwae
    lqz      1.43         6     m2-k1-b512-l5-normal-iwae-mixed
    lqw      1.63         7     p-m3-k2-b64-l100-ls70-laplace-iwae-random-b2.5-g1B
    lw       3.19         13    big-m8-k2-b512-l5-normal-dreg-random
    w        0.99         4     big-m8-k2-b512-l5-normal-iwae
    rowcoef  0.99         4     big-m8-k2-b512-l5-normal-iwae
    loss     0.34         2     big-p-m2-k10-b5-l70-ls64-laplace-iwae-b2.5
    dmu      1.85         8     p-m2-k10-b512-l130-ls64-normal-dreg-b0.5
    dsd      1.94         8     p-m2-k10-b512-l130-ls64-normal-dreg-b0.5
    dprior   2.20         9     big-m8-k2-b512-l5-normal-dreg-random
    std      1.43         6     laplace_with_softmax 9x20
    std_bwd  1.49         6     normal_with_softplus 33x130
    cross    0.91         4     laplace
    cross_bwd 0.13        1     laplace, 640 rows

Largest |err| / base the HIP kernels showed on an MI355X (test_zz_report prints it; compare with C above):
    z 0.99, lpz 2.72, lq_all 5.06, lqz 1.12, lqw 1.50, lw 3.19, w 0.89, rowcoef 0.89, loss 0.29, dmu 1.84, dsd 2.09, dprior 2.11,
    std 1.42, std_bwd 1.23, cross 0.92, cross_bwd 0.64; the loss accumulation alone (check 4) 0.94 of u (2 S + (K + 2) M B).
Factor by which each mutation of the reference exceeded the bound on its weakest named case (HIP output): logM 1.9e4 (lqz),
beta_lpx 3.6e5 (lw), no_hook 1.0e4 (dmu), iwae_detached_q 4.7e3 (dsd), private_mixture 3.1e5 (lq_all), prior_shift 6.3e4 (lpz),
resp_shift 2.4e4 (dmu), two_piece 3.7 (lw, big-m8-k2-b512-l5-normal-iwae).  Wall time of this file on the GPU: 6 s (77 tests).

Suspects (each decided by a test here):
 1. std_bwd, softmax family, recovering p from the stored sd: real.  Emulated in torch fp32 the recovered-p formula reaches 29x
    the per-entry base at L = 64, logits +-12, against C = 6 (test_mmvae_ref_host.py; more at +-20); the kernel now recomputes the softmax
    from lv and shows 1.23 (test_std, test_std_softmax_backward_small_probabilities).
 2. objective_kernel's loss accumulation over M * B / 1024 trips: cleared, 0.94 of the bound's unit at M * B = 4096, rows ~ 3e3.
    The sum_k w property of check 2 did fail by design of w = expf(lw - lse) (rounding lse at |lw| ~ 3e3 scales a whole column
    by up to 1.2e-4); the kernel now writes expf(lw - max) / sum.
 3. int casts in latent_fwd: include/mvk.h states M * K * B < 2^31; test_argument_checks covers the rejection.
 4. a row without any modality: NaN as in the oracle; include/mvk.h says masks must leave one; not in the case table.
"""
import pytest
import torch

import mmvae_ref as R
from oracle import elbo

pytestmark = pytest.mark.gpu

U = R.U
FAM = {"normal": 0, "laplace_with_softmax": 1, "normal_with_softplus": 2}


def dev():
    return torch.device("cuda:0")


def _lib():
    from multivae_amd import _lib as L

    return L


def to_dev(ts):
    return [t.to(dev()).contiguous() for t in ts]


class Hip:
    """Device buffers of one case and the three launches, callable twice from the same inputs."""

    def __init__(self, case, inp):
        d = dev()
        self.case, self.inp = case, inp
        M, K, B, L = case.M, case.K, case.B, case.L
        self.mus, self.sds, self.noises = to_dev(inp["mus"]), to_dev(inp["sds"]), to_dev(inp["noises"])
        self.pm, self.ps = inp["pm"].to(d), inp["ps"].to(d)
        self.masks = None if inp["masks"] is None else [m.to(torch.uint8).to(d).contiguous() for m in inp["masks"]]
        self.rows = [to_dev(rr) for rr in inp["rows"]]
        self.gloss = torch.tensor([inp["gloss"]], dtype=torch.float32, device=d)

    def new(self, *shape):
        return torch.full(shape, float("nan"), dtype=torch.float32, device=dev())

    def forward(self):
        Lb = _lib()
        c = self.case
        M, K, B, L, Ls = c.M, c.K, c.B, c.L, c.shared
        o = dict(z=[self.new(K, B, L) for _ in range(M)], lpz=[self.new(K, B) for _ in range(M)],
                 lqz=[self.new(K, B) for _ in range(M)], lq_all=[self.new(M, K, B) for _ in range(M)],
                 lqw=[self.new(K, B) for _ in range(M)] if Ls < L else None)
        marr = Lb.ptr_array(self.masks) if self.masks is not None else None
        Lb.call("mvk_mmvae_latent_fwd", Lb.ptr_array(self.mus), Lb.ptr_array(self.sds), Lb.ptr_array(self.noises), marr,
                Lb.ptr(self.pm), Lb.ptr(self.ps), M, K, B, L, FAM[c.family], Lb.ptr_array(o["z"]), Lb.ptr_array(o["lpz"]),
                Lb.ptr_array(o["lqz"]), Lb.ptr_array(o["lq_all"]), Ls,
                Lb.ptr_array(o["lqw"]) if o["lqw"] is not None else None, Lb.stream_ptr())
        o.update(lw=[self.new(K, B) for _ in range(M)], w=[self.new(K, B) for _ in range(M)],
                 rowcoef=[self.new(K, B) for _ in range(M)], loss=self.new(1))
        flat_rows = [self.rows[a][b] for a in range(M) for b in range(M)]
        Lb.call("mvk_mmvae_objective_fwd", Lb.ptr_array(flat_rows), Lb.ptr_array(o["lpz"]), Lb.ptr_array(o["lqz"]), marr, M,
                K, B, int(c.dreg), Lb.ptr_array(o["lw"]), Lb.ptr_array(o["w"]), Lb.ptr_array(o["rowcoef"]), Lb.ptr(o["loss"]),
                Lb.ptr_array(o["lqw"]) if o["lqw"] is not None else None, float(c.beta), Lb.stream_ptr())
        return o

    def backward(self, o, dz_dec):
        Lb = _lib()
        from multivae_amd import kernels as Kn

        c = self.case
        M, K, B, L, Ls = c.M, c.K, c.B, c.L, c.shared
        marr = Lb.ptr_array(self.masks) if self.masks is not None else None
        g = dict(dmu=[self.new(B, L) for _ in range(M)], dsd=[self.new(B, L) for _ in range(M)], dprior_rows=self.new(B, L))
        Lb.call("mvk_mmvae_latent_bwd", Lb.ptr_array(self.mus), Lb.ptr_array(self.sds), Lb.ptr_array(self.noises),
                Lb.ptr_array(o["z"]), marr, Lb.ptr(self.pm), Lb.ptr(self.ps), Lb.ptr_array(o["w"]), Lb.ptr_array(o["lq_all"]),
                Lb.ptr_array(o["lqz"]), Lb.ptr_array(dz_dec), M, K, B, L, FAM[c.family], int(c.dreg), Lb.ptr(self.gloss),
                Lb.ptr_array(g["dmu"]), Lb.ptr_array(g["dsd"]), Lb.ptr(g["dprior_rows"]), Ls, float(c.beta), Lb.stream_ptr())
        g["dprior"] = torch.zeros(L, dtype=torch.float32, device=dev())
        ws = Kn._ws(g["dprior_rows"])
        Lb.call("mvk_colsum_acc", Lb.ptr(g["dprior_rows"]), None, Kn.NONE, Lb.ptr(g["dprior"]), B, L, Lb.ptr(ws), ws.numel(),
                Lb.stream_ptr())
        return g


def cpu(o):
    out = {}
    for k, v in o.items():
        if v is None:
            out[k] = None
        elif isinstance(v, list):
            out[k] = [t.detach().cpu() for t in v]
        else:
            out[k] = v.detach().cpu()
    return out


def same_bits(a, b):
    for k in a:
        xs = a[k] if isinstance(a[k], list) else [a[k]]
        ys = b[k] if isinstance(b[k], list) else [b[k]]
        if a[k] is None:
            continue
        for x, y in zip(xs, ys):
            if not torch.equal(x.view(torch.int32), y.view(torch.int32)):
                return k
    return None


MEASURED = {}


def run_case(case):
    inp = R.make_inputs(case)
    h = Hip(case, inp)
    o = h.forward()
    dz_dev = to_dev(R.dz_dec_from(inp, [t.cpu() for t in o["rowcoef"]]))
    g = h.backward(o, dz_dev)
    o2 = h.forward()
    g2 = h.backward(o2, dz_dev)
    torch.cuda.synchronize()
    got, got2 = cpu({**o, **g}), cpu({**o2, **g2})
    got["loss"], got2["loss"] = got["loss"].reshape(()), got2["loss"].reshape(())
    got["dz_dec"] = [t.cpu() for t in dz_dev]
    return inp, got, got2


@pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
def test_case(case):
    inp, got, got2 = run_case(case)
    M, K, B, L, Ls = case.M, case.K, case.B, case.L, case.shared
    # 3. determinism
    assert same_bits({k: v for k, v in got.items() if k != "dz_dec"}, got2) is None
    # 1. every output of every stage
    ratios = R.staged_ratios(case, inp, got)
    print(case.name, {k: round(v, 3) for k, v in ratios.items()})
    for k, v in ratios.items():
        MEASURED[k] = max(MEASURED.get(k, 0.0), v)
        assert v <= R.C_STAGE[k], f"{case.name}: {k} worst |err| / base = {v:.3g} > C = {R.C_STAGE[k]}"
    pr64 = got["dprior_rows"].double()
    r = R.worst_ratio(got["dprior"], pr64.sum(0), U * 2 * pr64.abs().sum(0) + R.TINY)
    assert r <= R.C_STAGE["dprior"], f"colsum finish of dprior: {r:.3g}"
    # 2. exact properties
    av, _ = R.avail_of(inp["masks"], M, B)
    for c in range(M):
        gone = ~av[c]
        assert bool((got["lw"][c][:, gone] == 0).all()) and bool((got["rowcoef"][c][:, gone] == 0).all())
        assert bool((got["w"][c][:, gone] == float(torch.tensor(1.0 / K, dtype=torch.float32))).all())
        assert float((got["w"][c].double().sum(0) - 1).abs().max()) <= K * 2.0 ** -23, "sum_k w"
    if inp["masks"] is not None:
        for c in range(M):
            if bool((~av[c]).any()) and bool(av[c].any()):
                # rows where c is absent add exactly nothing: poison everything the kernel could read for (c, those rows)
                h = Hip(case, inp)
                o = h.forward()
                dz = to_dev(got["dz_dec"])
                gone = (~av[c]).to(dev())
                for t in (dz[c], o["z"][c]):
                    t[:, gone, :] = 1e30
                for t in (o["w"][c], o["lqz"][c]):
                    t[:, gone] = 1e30
                o["lq_all"][c][:, :, gone] = 1e30
                gp = cpu(h.backward(o, dz))
                assert same_bits({k: got[k] for k in ("dmu", "dsd", "dprior_rows")}, gp) is None, \
                    f"rows with modality {c} absent contribute to the gradients"
                break
    # 4. the loss from the kernel's own lw
    ref, S = R.loss_from_lw(got["lw"], inp["masks"], case.dreg, w=got["w"] if case.dreg else None)
    bound = R.C_STAGE["loss"] * U * (2 * float(S) + (K + 2) * M * B)
    err = abs(float(got["loss"].double()) - float(ref))
    MEASURED["loss_accumulation"] = max(MEASURED.get("loss_accumulation", 0.0), err / (bound / R.C_STAGE["loss"]))
    assert err <= bound, f"loss accumulation: |err| = {err:.3g} > {bound:.3g} (S = {float(S):.3g})"


@pytest.mark.parametrize("mut,stages,names", R.TEETH, ids=[t[0] for t in R.TEETH])
def test_tolerance_rejects_mutated_reference(mut, stages, names):
    """The comparison of test_case, with one deliberate mistake in the REFERENCE, must fail on the HIP kernels' output in
    every stage named for it (the same is shown against torch fp32 on the CPU in test_mmvae_ref_host.py)."""
    for name in names:
        case = R.CASE_BY_NAME[name]
        inp, got, _ = run_case(case)
        if mut == "two_piece":
            ratios = R.staged_ratios(case, inp, got, two_piece_rows=True)
        else:
            ratios = R.staged_ratios(case, inp, got, mut=(mut,))
        for s in stages:
            print(mut, name, s, round(ratios[s] / R.C_STAGE[s], 2))
            assert ratios[s] > R.C_STAGE[s], f"{mut} passes {s} on {name}: {ratios[s]:.3g} <= C = {R.C_STAGE[s]}"


# ---- std ---------------------------------------------------------------------------------------------------------------------
def std_inputs(family, rows, L, spread, seed):
    gen = torch.Generator().manual_seed(seed)
    lv = ((torch.rand(rows, L, generator=gen) * 2 - 1) * spread).float()
    if family == "normal_with_softplus" and lv.numel() >= 3:  # the threshold of F.softplus, just above it, and deep in the tail
        lv.view(-1)[:3] = torch.tensor([20.0, float(torch.nextafter(torch.tensor(20.0), torch.tensor(30.0))), -100.0])
    dsd = (torch.randn(rows, L, generator=gen) * (0.5 + torch.rand(rows, 1, generator=gen))).float()
    return lv, dsd


STD_SHAPES = [(1, 1, 2.0), (9, 20, 2.0), (33, 64, 12.0), (33, 130, 12.0), (33, 64, 20.0), (5, 65, 4.0), (3, 70, 6.0)]


def hip_std(lv, dsd, family):
    Lb = _lib()
    d = dev()
    lvd, dsdd = lv.to(d), dsd.to(d)
    sd, dlv = torch.empty_like(lvd), torch.empty_like(lvd)
    Lb.call("mvk_mmvae_std_fwd", Lb.ptr(lvd), lv.shape[0], lv.shape[1], FAM[family], Lb.ptr(sd), Lb.stream_ptr())
    Lb.call("mvk_mmvae_std_bwd", Lb.ptr(lvd), Lb.ptr(sd), Lb.ptr(dsdd), lv.shape[0], lv.shape[1], FAM[family], Lb.ptr(dlv),
            Lb.stream_ptr())
    torch.cuda.synchronize()
    return sd.cpu(), dlv.cpu()


@pytest.mark.parametrize("family", list(FAM))
@pytest.mark.parametrize("rows,L,spread", STD_SHAPES, ids=[f"r{r}-l{l}-s{int(s)}" for r, l, s in STD_SHAPES])
def test_std(family, rows, L, spread):
    """std and its backward, every entry: |err| <= C * u * (sd | S_i) * (2 + |lv - max|) with, for the softmax backward,
    S_i = L p_i (|dsd_i| + sum_j |dsd_j| p_j): where dsd_i - sum_j dsd_j p_j cancels, S_i carries the scale."""
    lv, dsd = std_inputs(family, rows, L, spread, 11 + rows + L)
    sd, dlv = hip_std(lv, dsd, family)
    sd2, dlv2 = hip_std(lv, dsd, family)
    assert torch.equal(sd, sd2) and torch.equal(dlv, dlv2)
    r = R.worst_ratio(sd, R.std(lv, family), R.std_base(lv, family))
    MEASURED["std"] = max(MEASURED.get("std", 0.0), r)
    assert r <= R.C_STAGE["std"], f"std: {r:.3g}"
    # the backward's reference consumes the fp32 sd the kernel stored only through lv: the function is sd(lv)
    rb = R.worst_ratio(dlv, R.std_vjp(lv, dsd, family), R.std_vjp_base(lv, dsd, family))
    print(family, rows, L, spread, "std", round(r, 3), "std_bwd", round(rb, 3))
    MEASURED["std_bwd"] = max(MEASURED.get("std_bwd", 0.0), rb)
    assert rb <= R.C_STAGE["std_bwd"], f"std_bwd: {rb:.3g}"


@pytest.mark.parametrize("L,spread", [(64, 12.0), (130, 12.0), (64, 20.0)])
def test_std_softmax_backward_small_probabilities(L, spread):
    """Suspect 1: on entries with p L < 1e-7 the gradient L p_i (dsd_i - dot) keeps its RELATIVE accuracy (the error model of
    test_std, which scales with p_i) — a p recovered as (sd - 1e-6) / L cancels there and does not."""
    lv, dsd = std_inputs("laplace_with_softmax", 33, L, spread, 5)
    _, dlv = hip_std(lv, dsd, "laplace_with_softmax")
    p = torch.softmax(lv.double(), -1)
    small = p * L < 1e-7
    assert bool(small.any())
    ref, base = R.std_vjp(lv, dsd, "laplace_with_softmax"), R.std_vjp_base(lv, dsd, "laplace_with_softmax")
    r = R.worst_ratio(dlv[small], ref[small], base[small])
    rel = float(((dlv.double() - ref).abs() / ref.abs().clamp_min(1e-300))[small].max())
    print(f"L={L} spread={spread}: {int(small.sum())} small entries, worst |err|/base {r:.3g}, worst relative {rel:.3g}")
    assert r <= R.C_STAGE["std_bwd"], f"worst |err| / base on p L < 1e-7: {r:.3g} (relative {rel:.3g})"


# ---- cross latent ------------------------------------------------------------------------------------------------------------------
CROSS = [(1, 1, 2, 1, "normal"), (2, 3, 20, 12, "laplace_with_softmax"), (33, 64, 70, 64, "normal"),
         (10, 64, 100, 70, "laplace_with_softmax"), (5, 37, 130, 64, "normal"), (2, 512, 65, 64, "laplace_with_softmax")]


@pytest.mark.parametrize("K,B,D,Ls,family", CROSS, ids=[f"k{k}-b{b}-d{d}-ls{ls}-{f[:3]}" for k, b, d, ls, f in CROSS])
def test_cross_latent(K, B, D, Ls, family):
    """mvk_mmvaeplus_cross_latent_fwd / bwd: shared dims copied bit for bit, private dims = prior_sd t(noise); backward:
    dz[..., :Ls] bit-equal to dzc, dz[..., Ls:] == 0 exactly, dprior_sd over up to 2112 rows per column (4-wave finish)."""
    Lb = _lib()
    gen = torch.Generator().manual_seed(K * 1000 + B + D)
    S = D - Ls
    z = torch.randn(K, B, D, generator=gen).float()
    ps = (0.5 + 1.5 * torch.rand(S, generator=gen)).float()
    if family == "normal":
        noise = torch.randn(K, B, S, generator=gen).float()
    else:
        noise = (torch.rand(K, B, S, generator=gen) * 2 - 1).float().clamp(-R.ONE_MINUS, R.ONE_MINUS)
        noise.view(-1)[0] = 0.0
    dzc = torch.randn(K, B, D, generator=gen).float()
    d = dev()
    zd, psd, nd, dzcd = z.to(d), ps.to(d), noise.to(d), dzc.to(d)
    outs = []
    for _ in range(2):
        zc, dz, dps = (torch.full_like(zd, float("nan")), torch.full_like(zd, float("nan")),
                       torch.full((S,), float("nan"), device=d))
        Lb.call("mvk_mmvaeplus_cross_latent_fwd", Lb.ptr(zd), Lb.ptr(psd), Lb.ptr(nd), K * B, D, Ls, FAM[family], Lb.ptr(zc),
                Lb.stream_ptr())
        Lb.call("mvk_mmvaeplus_cross_latent_bwd", Lb.ptr(dzcd), Lb.ptr(nd), K * B, D, Ls, FAM[family], Lb.ptr(dz), Lb.ptr(dps),
                Lb.stream_ptr())
        torch.cuda.synchronize()
        outs.append((zc.cpu(), dz.cpu(), dps.cpu()))
    (zc, dz, dps), second = outs
    assert all(torch.equal(a, b) for a, b in zip(outs[0], second))
    assert torch.equal(zc[..., :Ls], z[..., :Ls]) and torch.equal(dz[..., :Ls], dzc[..., :Ls])
    assert bool((dz[..., Ls:] == 0).all())
    ref = R.cross_latent(z, ps, noise, Ls, family)
    r = R.worst_ratio(zc[..., Ls:], ref[..., Ls:], U * 2 * ref[..., Ls:].abs() + R.TINY)
    dz_ref, dps_ref, b_dps = R.cross_latent_vjp(dzc, z, ps, noise, Ls, family)
    assert torch.equal(dz.double(), dz_ref)
    rb = R.worst_ratio(dps, dps_ref, b_dps)
    print("cross", K, B, D, Ls, family, round(r, 3), round(rb, 3))
    MEASURED["cross"] = max(MEASURED.get("cross", 0.0), r)
    MEASURED["cross_bwd"] = max(MEASURED.get("cross_bwd", 0.0), rb)
    assert r <= R.C_STAGE["cross"] and rb <= R.C_STAGE["cross_bwd"], (r, rb)


# ---- argument checks -----------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    """MVK_EINVAL for: M = 9; Ls = 0; Ls > L; Ls < L without lqw; family 2 on the latent kernels; D = Ls in the cross-latent
    kernels; M * K * B >= 2^31.  B = 0 (rows = 0) is a no-op returning MVK_OK in all seven entry points (include/mvk.h): nothing
    is launched and no output is written, the loss scalar included."""
    Lb = _lib()
    d = dev()
    sp = Lb.stream_ptr
    t = torch.full((4096,), 7.0, device=d)
    p = Lb.ptr(t)

    def arr(n):
        return Lb.ptr_array([t] * n)

    def fwd(M=2, K=2, B=3, L=5, fam=0, Ls=5, lqw=True):
        n = max(M, 1)
        Lb.call("mvk_mmvae_latent_fwd", arr(n), arr(n), arr(n), None, p, p, M, K, B, L, fam, arr(n), arr(n), arr(n), arr(n), Ls,
                arr(n) if lqw else None, sp())

    def bwd(M=2, K=2, B=3, L=5, fam=0, Ls=5):
        n = max(M, 1)
        Lb.call("mvk_mmvae_latent_bwd", arr(n), arr(n), arr(n), arr(n), None, p, p, arr(n), arr(n), arr(n), arr(n), M, K, B, L,
                fam, 0, None, arr(n), arr(n), p, Ls, 1.0, sp())

    def obj(M=2, K=2, B=3):
        n = max(M, 1)
        Lb.call("mvk_mmvae_objective_fwd", arr(n * n), arr(n), arr(n), None, M, K, B, 0, arr(n), arr(n), arr(n), p, None, 1.0,
                sp())

    bad = [lambda: fwd(M=9), lambda: bwd(M=9), lambda: obj(M=9), lambda: fwd(M=0), lambda: fwd(Ls=0), lambda: bwd(Ls=0),
           lambda: fwd(Ls=6), lambda: bwd(Ls=6), lambda: fwd(Ls=3, lqw=False), lambda: fwd(fam=2), lambda: bwd(fam=2),
           lambda: fwd(B=-1), lambda: bwd(B=-1), lambda: obj(B=-1), lambda: fwd(K=0), lambda: obj(K=0),
           lambda: fwd(M=8, K=1 << 14, B=1 << 14), lambda: bwd(M=8, K=1 << 14, B=1 << 14),
           lambda: obj(M=8, K=1 << 14, B=1 << 14),
           lambda: Lb.call("mvk_mmvaeplus_cross_latent_fwd", p, p, p, 4, 5, 5, 0, p, sp()),
           lambda: Lb.call("mvk_mmvaeplus_cross_latent_bwd", p, p, 4, 5, 5, 0, p, p, sp()),
           lambda: Lb.call("mvk_mmvaeplus_cross_latent_fwd", p, p, p, 4, 5, 0, 0, p, sp()),
           lambda: Lb.call("mvk_mmvaeplus_cross_latent_fwd", p, p, p, 4, 5, 2, 2, p, sp()),
           lambda: Lb.call("mvk_mmvae_std_fwd", p, 3, 5, 3, p, sp()),
           lambda: Lb.call("mvk_mmvae_std_bwd", p, p, p, 3, 0, 0, p, sp())]
    for i, f in enumerate(bad):
        with pytest.raises(Lb.MvkError):
            f()
            pytest.fail(f"bad call {i} was accepted")
    # zero rows: OK, nothing written
    fwd(B=0)
    bwd(B=0)
    obj(B=0)
    Lb.call("mvk_mmvae_std_fwd", p, 0, 5, 1, p, sp())
    Lb.call("mvk_mmvae_std_bwd", p, p, p, 0, 5, 1, p, sp())
    Lb.call("mvk_mmvaeplus_cross_latent_fwd", p, p, p, 0, 5, 2, 0, p, sp())
    Lb.call("mvk_mmvaeplus_cross_latent_bwd", p, p, 0, 5, 2, 0, p, p, sp())
    torch.cuda.synchronize()
    assert bool((t == 7.0).all())


# ---- the four autograd Functions, end to end -------------------------------------------------------------------------------------
def e2e_inputs(plus):
    gen = torch.Generator().manual_seed(77 + plus)
    M, B, K, L = 3, 37, 5, 70
    Ls = 50 if plus else L
    names = ["a", "b", "c"]
    mu = {m: torch.randn(B, L, generator=gen).float() for m in names}
    lv = {m: (torch.randn(B, L, generator=gen) * 0.7).float() for m in names}
    x = {m: torch.randn(B, L, generator=gen).float() for m in names}
    a = {m: (0.5 + torch.rand(L, generator=gen)).float() for m in names}
    b = {m: (0.3 * torch.randn(L, generator=gen)).float() for m in names}
    masks = {m: torch.rand(B, generator=gen) > 0.35 for m in names}
    masks["a"][:] = True
    masks["c"][0] = False
    pl = (0.3 * torch.randn(1, L, generator=gen)).float()
    pls = {m: (0.3 * torch.randn(1, L - Ls, generator=gen)).float() for m in names} if plus else None
    return dict(M=M, B=B, K=K, L=L, Ls=Ls, names=names, mu=mu, lv=lv, x=x, a=a, b=b, masks=masks, pl=pl, pls=pls, gen=gen)


def e2e_oracle(I, plus, family, loss, dtype, noise):
    names, Ls = I["names"], I["Ls"]
    leaves = {}

    def leaf(k, t):
        leaves[k] = t.to(dtype).clone().requires_grad_()
        return leaves[k]

    mu = {m: leaf("mu_" + m, I["mu"][m]) for m in names}
    lv = {m: leaf("lv_" + m, I["lv"][m]) for m in names}
    a = {m: leaf("a_" + m, I["a"][m]) for m in names}
    b = {m: leaf("b_" + m, I["b"][m]) for m in names}
    pl = leaf("prior_lv", I["pl"])
    data = {m: I["x"][m].to(dtype) for m in names}
    dec = {m: (lambda z, m=m: a[m] * z + b[m]) for m in names}
    mk = {m: I["masks"][m] for m in names}
    if not plus:
        enc = {m: (mu[m], lv[m]) for m in names}
        out = elbo.mmvae_forward(enc, data, dec, {m: noise[m].to(dtype) for m in names}, names=names, K=I["K"], family=family,
                                 loss=loss, prior_log_var=pl, masks=mk)
    else:
        pls = {m: leaf("prior_lv_" + m, I["pls"][m]) for m in names}
        enc = {m: (mu[m][:, :Ls], lv[m][:, :Ls], mu[m][:, Ls:], lv[m][:, Ls:]) for m in names}
        nz = {c: dict({"u": noise[c][..., :Ls].to(dtype), "w": noise[c][..., Ls:].to(dtype)},
                      **{r: noise[(c, r)].to(dtype) for r in names if r != c}) for c in names}
        out = elbo.mmvaeplus_forward(enc, data, dec, nz, names=names, K=I["K"], family=family, loss=loss, beta=2.5,
                                     prior_logvars=dict({"shared": pl}, **pls), masks=mk)
    out["loss"].backward()
    return out["loss"].detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}


@pytest.mark.parametrize("loss", ["iwae_looser", "dreg_looser"])
@pytest.mark.parametrize("plus", [0, 1], ids=["mmvae", "mmvaeplus"])
def test_functions_end_to_end(plus, loss):
    """MMVAEStdFn -> MMVAELatentFn -> (MMVAEPlusCrossLatentFn ->) elementwise decoder a_r z + b_r on the GPU ->
    MMVAEObjectiveFn -> backward, against oracle.elbo in float64; L = 70, M = 3, B = 37, K = 5, masked.  Tolerance per
    tensor, relative to the tensor's maximum: 4x the distance of the fp32 oracle from its own float64 evaluation on these
    inputs, measured on the CPU right here (never on the HIP result); the softmax scale family needs whole-latent softmax in
    MMVAE+, so MMVAE+ runs the normal family and MMVAE the Laplace one.  One modality's z is left unused by the loss in a
    third pass to exercise the zeros substitution for a missing dz_dec."""
    from multivae_amd import kernels as Kn

    I = e2e_inputs(plus)
    family = "normal" if plus else "laplace_with_softmax"
    names, M, B, K, L, Ls = I["names"], I["M"], I["B"], I["K"], I["L"], I["Ls"]
    gen = I["gen"]

    def draw(shape):
        if family == "normal":
            return torch.randn(*shape, generator=gen).float()
        return (torch.rand(*shape, generator=gen) * 2 - 1).float().clamp(-R.ONE_MINUS, R.ONE_MINUS)

    noise = {m: draw((K, B, L)) for m in names}
    if plus:
        noise.update({(c, r): draw((K, B, L - Ls)) for c in names for r in names if r != c})
    l64, g64 = e2e_oracle(I, plus, family, loss, torch.float64, noise)
    l32, g32 = e2e_oracle(I, plus, family, loss, torch.float32, noise)

    def rel(x, ref):
        return float((x.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))

    d = dev()
    leaves = {}

    def leaf(k, t):
        leaves[k] = t.to(d).clone().requires_grad_()
        return leaves[k]

    mu = [leaf("mu_" + m, I["mu"][m]) for m in names]
    lv = [leaf("lv_" + m, I["lv"][m]) for m in names]
    a = [leaf("a_" + m, I["a"][m]) for m in names]
    b = [leaf("b_" + m, I["b"][m]) for m in names]
    pl = leaf("prior_lv", I["pl"])
    fam_std, fam = FAM[family], FAM[family]
    sds = [Kn.MMVAEStdFn.apply(t, fam_std) for t in lv]
    prior_std = Kn.MMVAEStdFn.apply(pl, fam_std)
    state = Kn.MMVAEState()
    if plus:
        state.shared_dims, state.beta = Ls, 2.5
        pls = [leaf("prior_lv_" + m, I["pls"][m]) for m in names]
    masks = [I["masks"][m].to(d).contiguous() for m in names]
    noises = [noise[m].to(d) for m in names]
    dreg = loss == "dreg_looser"
    zs = Kn.MMVAELatentFn.apply(state, noises, masks, torch.zeros(1, L, device=d), fam, int(dreg), prior_std, *mu, *sds)
    recons = []
    for ci, c in enumerate(names):
        for ri, r in enumerate(names):
            zin = zs[ci]
            if plus and r != c:
                zin = Kn.MMVAEPlusCrossLatentFn.apply(zs[ci], Kn.MMVAEStdFn.apply(pls[ri], fam_std), noise[(c, r)].to(d), Ls, fam)
            recons.append(a[ri] * zin + b[ri])
    spec = dict(K=K, B=B, x=[I["x"][m].to(d).contiguous() for m in names], dist=[_lib().DIST["normal"]] * M, scale=[1.0] * M,
                rescale=[1.0] * M, masks=masks)
    out = Kn.MMVAEObjectiveFn.apply(state, spec, M, dreg, *recons)
    out.backward()
    torch.cuda.synchronize()
    assert abs(float(out) - float(l64)) <= 4 * max(abs(float(l32) - float(l64)), 2.0 ** -23 * abs(float(l64))), \
        (float(out), float(l64), float(l32))
    for k, ref in g64.items():
        tol = 4 * max(rel(g32[k], ref), 2.0 ** -23)
        got = rel(leaves[k].grad.cpu(), ref)
        print(f"e2e plus={plus} {loss} {k}: HIP {got:.3g}, fp32 oracle {tol / 4:.3g}")
        assert got <= tol, f"{k}: {got:.3g} > 4 x {tol / 4:.3g}"


def test_latent_fn_missing_dz():
    """MMVAELatentFn.backward substitutes zeros for a modality whose z received no gradient."""
    from multivae_amd import kernels as Kn

    case = R.CASE_BY_NAME["m3-k10-b5-l20-normal-dreg-random-g1B"]
    inp = R.make_inputs(case)
    d = dev()
    M, K, B, L = case.M, case.K, case.B, case.L
    mu = [t.to(d).requires_grad_() for t in inp["mus"]]
    sd = [t.to(d).requires_grad_() for t in inp["sds"]]
    ps = inp["ps"].to(d).reshape(1, L).requires_grad_()
    masks = [m.to(d).contiguous() for m in inp["masks"]]
    state = Kn.MMVAEState()
    zs = Kn.MMVAELatentFn.apply(state, to_dev(inp["noises"]), masks, inp["pm"].to(d).reshape(1, L), 0, 1, ps, *mu, *sd)
    o = R.objective(inp["rows"], [t.cpu() for t in state.lpz], [t.cpu() for t in state.lqz], None, inp["masks"], 1.0, True)
    state.w = to_dev([t.float() for t in o["w"]])
    state.gloss = torch.tensor([inp["gloss"]], device=d)
    dz = R.dz_dec_from(inp, o["rowcoef"])
    (zs[0] * dz[0].to(d)).sum().add((zs[2] * dz[2].to(d)).sum()).backward()  # zs[1] gets no gradient
    torch.cuda.synchronize()
    dz[1] = torch.zeros_like(dz[1])
    args = (inp["mus"], inp["sds"], inp["noises"], inp["masks"], inp["pm"], inp["ps"], "normal", L, 1.0, True, dz, inp["gloss"])
    zk = [t.detach().cpu() for t in zs]
    dmu, dsd, dpr = R.latent_bwd(*args, w=[t.cpu() for t in state.w], zs=zk)
    fw = R.latent_fwd(inp["mus"], inp["sds"], inp["noises"], inp["masks"], inp["pm"], inp["ps"], "normal", L, zs=zk,
                      want_base=True)
    b_mu, b_sd, b_pr = R.latent_bwd_base(*args, [t.cpu() for t in state.w], zk, fw["b_lq_all"], [t.cpu() for t in state.lqz])
    for m in range(M):
        assert R.worst_ratio(mu[m].grad.cpu(), dmu[m], b_mu[m]) <= R.C_STAGE["dmu"]
        assert R.worst_ratio(sd[m].grad.cpu(), dsd[m], b_sd[m]) <= R.C_STAGE["dsd"]
    assert R.worst_ratio(ps.grad.cpu().reshape(-1), dpr.sum(0), b_pr.sum(0) + U * 2 * dpr.abs().sum(0)) <= R.C_STAGE["dprior"]


def test_zz_report():
    """Prints the head-room the HIP kernels showed in this session (largest |err| / base per stage)."""
    print("HIP_MEASURED", {k: round(v, 3) for k, v in sorted(MEASURED.items())})
