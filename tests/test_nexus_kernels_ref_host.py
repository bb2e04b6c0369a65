"""CPU checks of tests/nexus_kernels_ref.py, the references behind tests/test_gpu_nexus_kernels.py:

- the references are pinned to independent definitions: the top-level likelihood to torch.distributions.Normal with the adapted
  scale attached and float64 autograd for dr (the path through s2 included), the aggregation gradient to float64 autograd of the
  masked mean;
- the float32 FPD model agrees with the float64 evaluation of the same formula on every row of the random and of the crafted
  tables (no row needs the float32 model as the authority, and why), draws every subset size and every modality, and keeps
  exactly `size` modalities;
- the constants of the measured stages are 4x what the plain fp32 evaluation shows, rounded up; the derived ones hold;
- every `check_*` routine of the GPU file passes on every case with a stand-in backend (the same formulas in plain torch fp32);
- every wrong variant of nexus_kernels_ref.TEETH leaves the bound (FPD: changes bits) on each of its named cases.
"""
import numpy as np
import pytest
import torch

import nexus_kernels_ref as R
import test_gpu_nexus_kernels as G

F64 = torch.float64
NAN = float("nan")


# ---- the stand-in backend: the formulas in plain torch fp32 ---------------------------------------------------------------------------------
class Standin:
    def agg_fwd(self, msgs, masks, keep_in, u, p):
        M, (B, D) = len(msgs), msgs[0].shape
        keep = R.keep_set(M, B, keep_in, masks, u, p)
        s = torch.zeros(B, D)
        for m in range(M):
            s = s + torch.where(keep[:, m:m + 1] != 0, msgs[m], torch.zeros(()))
        cnt = keep.sum(1, keepdim=True)
        return dict(agg=s * torch.where(cnt > 0, 1.0 / cnt, torch.zeros(())), keep=keep, guards=True)

    def agg_bwd(self, keep, g):
        cnt = keep.sum(1, keepdim=True)
        gi = torch.where(cnt > 0, g / cnt, torch.zeros(()))
        return dict(dmsgs=torch.stack([torch.where(keep[:, m:m + 1] != 0, gi, torch.zeros(())) for m in range(keep.shape[1])]), guards=True)

    def top_fwd(self, inp, dims, adapt):
        B = inp["z"][0].shape[0]
        res = [R.top_fp32(inp["z"][m], inp["r"][m], D, inp["gamma"][m], adapt[m], None if inp["masks"] is None else inp["masks"][m], inp["g"][m])
               for m, D in enumerate(dims)]
        work = torch.stack([torch.cat([r["q"], torch.zeros(-B % 4)]).reshape(-1, 4).sum(1) for r in res]).reshape(-1)
        return dict(rows=torch.stack([r["rows"] for r in res]), q=torch.stack([r["q"] for r in res]), s2=torch.stack([r["s2"] for r in res]),
                    work=work, guards=True)

    def top_bwd(self, inp, dims, adapt, q, s2):
        B, M = inp["z"][0].shape[0], len(dims)
        res = [R.top_fp32(inp["z"][m], inp["r"][m], D, inp["gamma"][m], adapt[m], None if inp["masks"] is None else inp["masks"][m], inp["g"][m],
                          q=q[m], s2=s2[m]) for m, D in enumerate(dims)]
        work = torch.full((M * ((B + 3) // 4),), NAN)
        if any(adapt):
            part = torch.stack([r["cpart"] for r in res]).reshape(-1)
            work[:part.numel()] = part
        return dict(dr=[r["dr"] for r in res], work=work, guards=True)


BE = Standin()


# ---- independent definitions ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["top-ones-b300", "top-sign-b300", "top-maskmost-b300", "top-mixed-null", "top-b3", "top-b5-m8"])
def test_top_reference_is_normal_log_prob_and_autograd(name):
    case = R.TOP_BY_NAME[name]
    inp = R.top_inputs(case)
    for m, D in enumerate(case.dims):
        z, gamma = inp["z"][m].double(), inp["gamma"][m]
        r = inp["r"][m].double().requires_grad_(True)
        mask = None if inp["masks"] is None or inp["masks"][m] is None else inp["masks"][m]
        g = torch.zeros(case.B, dtype=F64) if inp["g"][m] is None else inp["g"][m].double()
        var = ((z - r) ** 2).mean() if case.adapt[m] else torch.ones((), dtype=F64)
        nll = -torch.distributions.Normal(r, var.sqrt()).log_prob(z).sum(1)
        rows = gamma * (nll if mask is None else nll * mask.double())
        (rows * g).sum().backward()
        q, _ = R.q_rows(inp["z"][m], inp["r"][m])
        s2 = R.s2_of(q, D, case.adapt[m], mask)
        ref_rows, _ = R.rows_of(q, s2, D, gamma, mask)
        ref_dr, base = R.dr_of(inp["z"][m], inp["r"][m], q, s2, gamma, case.adapt[m], inp["g"][m], mask)
        assert abs(float(s2) - float(var.detach())) <= 1e-14 * float(var.detach())
        assert float((ref_rows - rows.detach()).abs().max()) <= 1e-12 * float(rows.detach().abs().max() + 1)
        assert bool(((ref_dr - r.grad).abs() <= 1e-11 * base + 1e-300).all()), (name, m)


@pytest.mark.parametrize("name", ["agg-keepin-m3-b37-d70", "agg-masks-m4-b5-d64", "agg-u-m8-b37-d5"])
def test_agg_reference_is_the_masked_mean_and_autograd(name):
    case = R.AGG_BY_NAME[name]
    inp = R.agg_inputs(case)
    keep = R.keep_set(case.M, case.B, inp["keep_in"], inp["masks"], inp["u"], case.p)
    msgs = [t.double().requires_grad_(True) for t in inp["msgs"]]
    rows = []
    for b in range(case.B):  # the definition, row by row: the mean of the kept messages, 0 when there is none
        kept = [msgs[m][b] for m in range(case.M) if keep[b, m] != 0]
        rows.append(torch.stack(kept).mean(0) if kept else torch.zeros(case.D, dtype=F64))
    want = torch.stack(rows)
    ref, _ = R.agg(inp["msgs"], keep)
    assert float((ref - want.detach()).abs().max()) <= 1e-15 * float(want.detach().abs().max() + 1)
    grads = torch.autograd.grad(want, msgs, inp["gout"].double(), allow_unused=True)
    dref, _ = R.dmsgs(keep, inp["gout"])
    for m in range(case.M):
        got = torch.zeros(case.B, case.D, dtype=F64) if grads[m] is None else grads[m]
        assert float((dref[m] - got).abs().max()) <= 1e-15 * float(got.abs().max() + 1)


# ---- the FPD model ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", R.FPD_M)
def test_fpd_model_float32_against_float64_and_its_statistics(M):
    u = R.fpd_random(M)
    k32, k64 = R.fpd_keep(u, 1.0, M), R.fpd_keep64(u, 1.0, M)
    assert np.array_equal(k32, k64), "a random row sits on an integer boundary of a float32 product: move it to the crafted table"
    sizes = k32.sum(1)
    assert sizes.min() >= 1 and sizes.max() <= max(M - 1, 1)
    want_size = np.clip(1 + np.floor(u[:, 1].astype(np.float64) * (M - 1)), 1, M - 1)
    assert np.array_equal(sizes, want_size)  # the shuffle keeps exactly `size` distinct modalities
    assert set(sizes.tolist()) == set(range(1, M))
    share = k32.mean(0)
    assert share.max() - share.min() <= 0.06, share  # every modality is kept equally often (3000 rows: 3 sigma is about 0.03)
    assert np.array_equal(R.fpd_keep(u, 0.0, M), np.ones_like(k32))
    part = R.fpd_keep(u, 0.3, M)
    dropped = u[:, 0] < np.float32(0.3)
    assert np.array_equal(part[dropped], k32[dropped]) and bool((part[~dropped] == 1).all())


def test_fpd_crafted_rows_where_float32_decides():
    """On the crafted tables the float32 model is the authority.  The float64 evaluation of the same formula agrees on every row
    of them too: (1 - 2^-24) n for n <= 7 lies n units of 2^-24 below the integer n, more than half a float32 spacing there (2 or 4
    units), so the float32 product never rounds up to the integer, and the products with 0 and 1.0 are exact.  The clamps are
    therefore reached by u = 1.0 alone, which mvk_device_rng never draws."""
    for M in R.FPD_M:
        u = R.fpd_crafted(M, 1.0)
        assert np.array_equal(R.fpd_keep(u, 1.0, M), R.fpd_keep64(u, 1.0, M))
        for n in range(1, M):
            assert np.float32(R.ONE_M) * np.float32(n) < np.float32(n)
        size_clamped = u[:, 1] == 1.0
        assert size_clamped.any() and bool((R.fpd_keep(u, 1.0, M)[size_clamped].sum(1) == max(M - 1, 1)).all())


# ---- the constants ------------------------------------------------------------------------------------------------------------------------------
def measure():
    worst = {}
    for case in R.AGG_CASES:
        inp, f, _, b, _ = G.run_agg(case, BE)
        for k, v in G.agg_ratios(case, inp, f, b).items():
            G.note(worst, k, v, case.name)
    for case in R.TOP_CASES:
        inp, f, _, b, _ = G.run_top(case, BE)
        for k, v in G.top_ratios(case, inp, f, b).items():
            G.note(worst, k, v, case.name)
    return worst


def test_error_constants():
    """Measured stages: C = 4x the largest |err| / (U base) of the stand-in against the float64 reference over the case tables,
    rounded up: never below 4x the measured value, never above 8x (or 1).  Derived stages: the stand-in stays inside.  The figures
    and the cases that set them are in the docstring of tests/test_gpu_nexus_kernels.py."""
    worst = measure()
    print({k: (round(v, 3), n) for k, (v, n) in sorted(worst.items())})
    assert set(worst) == set(R.C_STAGE)
    for k in R.MEASURED_STAGES:
        v, name = worst[k]
        assert 4 * v <= R.C_STAGE[k], f"{k}: fp32 on the CPU shows {v:.3g} on {name}; C = {R.C_STAGE[k]} is less than 4x that"
        assert R.C_STAGE[k] <= max(8 * v, 1), f"{k}: C = {R.C_STAGE[k]} is more than 8x the measured {v:.3g}"
    for k in R.DERIVED:
        assert worst[k][0] <= R.C_STAGE[k], (k, worst[k])


# ---- the GPU file's comparison routines on the stand-in ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.AGG_CASES, ids=[c.name for c in R.AGG_CASES])
def test_check_agg(case):
    G.check_agg(case, BE)


@pytest.mark.parametrize("name", G.FPD_TABLES)
def test_check_fpd(name):
    G.check_fpd(name, BE)


@pytest.mark.parametrize("case", R.TOP_CASES, ids=[c.name for c in R.TOP_CASES])
def test_check_top(case):
    G.check_top(case, BE)


# ---- teeth ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mut,family,stages,name", G.TEETH_IDS, ids=[f"{t[0]}-{t[3]}" for t in G.TEETH_IDS])
def test_tolerance_rejects_mutated_reference(mut, family, stages, name):
    f = G.teeth_factor(mut, family, stages, name, BE)
    print(mut, name, f"{f:.3g}x the bound" if family != "fpd" else f"{f:.0f} rows differ")
    assert f > 1.0 if family != "fpd" else f >= 1.0, f"{mut} passes on {name}"


def test_case_tables_hold_the_edges():
    """The shapes of the issue, read off the launch code of nexus.hip."""
    ac, tc = R.AGG_CASES, R.TOP_CASES
    assert all(c.why for c in ac + tc)
    assert {c.B for c in ac} >= {1, 3, 4, 5} and {c.D for c in ac} >= {1, 63, 64, 65, 130} and {c.M for c in ac} >= {1, 8}
    assert {c.src for c in ac} >= {(), ("keep_in",), ("masks",), ("u",), ("masks", "u"), ("keep_in", "masks", "u")} and any(c.odd for c in ac)
    assert {c.B for c in tc} >= {1, 3, 4, 5, 1025, 2049, 65537} and (1025 + 3) // 4 > 256 and (2049 + 3) // 4 > 512 and (65537 + 255) // 256 > 256
    for B in (1, 3, 4, 5):
        assert {d for c in tc if c.B == B for d in c.dims} >= {1, 63, 64, 65, 130}
    assert any(len(c.dims) == 8 for c in tc) and any(not any(c.adapt) for c in tc) and {c.g for c in tc} == {"ones", "sign", "randn"}
    narrow = R.TOP_BY_NAME["top-narrow-adapted"]
    assert narrow.dims[narrow.adapt.index(1)] == min(narrow.dims) and sum(narrow.adapt) == 1
    wide = R.TOP_BY_NAME["top-wide-adapted"]
    assert wide.dims[wide.adapt.index(1)] == max(wide.dims) and sum(wide.adapt) == 1
    assert any(None in c.masks and any(f is not None for f in c.masks) for c in tc) and any(c.gnull for c in tc)
    assert 65537 * 2 * 4 < 2 ** 20  # the largest allocation stays under a megabyte
    for M in R.FPD_M:
        u = R.fpd_crafted(M, 0.3)
        assert {float(v) for v in u[:, 1]} >= {0.0, R.ONE_M, 1.0} and {float(v) for v in u[:, 2:].reshape(-1)} >= {0.0, R.ONE_M, 1.0}
        assert np.float32(0.3) in u[:, 0] and np.nextafter(np.float32(0.3), np.float32(1)) in u[:, 0] and np.nextafter(np.float32(0.3), np.float32(0)) in u[:, 0]
