"""CPU checks of tests/misc_ref.py, the references behind tests/test_gpu_misc.py:

- the references are pinned to independent definitions: the pack layouts to F.conv2d / F.conv_transpose2d and their autograd on
  one small layer (and to plain loops over the index definitions on every case), Adam to torch.optim.Adam in float64, pooling and
  upsampling to F.avg_pool2d / F.interpolate and their autograd, Philox4x32-10 to three published known answers, the bf16 cast to
  a round-to-nearest-even on the bit pattern;
- a + (b + c) of the three host pieces returns the input bit for bit on 2^20 random normal values on scales 2^-90 .. 2^90
  (|x| >= 2^-100) and on hand-picked patterns: the condition of the GPU round-trip test;
- the constants of the measured stages are 4x what the plain fp32 CPU evaluation shows, rounded up;
- every `check_*` routine of the GPU file passes on every case with a stand-in backend (the fp32 CPU evaluation);
- every wrong variant of misc_ref.TEETH leaves the bound (or, for a bit-exact model, changes bits) on its named case.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import misc_ref as R
import test_gpu_misc as G

F64 = torch.float64


# ---- independent definitions ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctr,key,want", R.PHILOX_KAT)
def test_philox_known_answers(ctr, key, want):
    assert [int(v) for v in R.philox(ctr, key)[:, 0]] == list(want)


def test_rng_words_follow_the_counter_layout():
    """Thread t of a launch at `offset` runs counter (offset + t) split into two words, the upper two words 0, key = seed."""
    seed, off = R.SEED_HI, 2 ** 32 - 3
    w = R.rng_words(seed, off, 24)
    for t in range(6):
        c = off + t
        assert [int(v) for v in w[t]] == [int(v) for v in R.philox((c & 0xFFFFFFFF, c >> 32, 0, 0), (seed & 0xFFFFFFFF, seed >> 32))[:, 0]]
    assert [int(v) for v in R.rng_words(0, 0, 4)[0]] == list(R.PHILOX_KAT[0][2])


def _im2col(x, k, stride, pad):
    """x [n][C][H][W] -> patches [n][L][tap][C] (F.unfold orders rows as c * k * k + tap)."""
    n, C = x.shape[:2]
    cols = F.unfold(x, k, padding=pad, stride=stride)  # [n][C * k * k][L]
    return cols.reshape(n, C, k * k, -1).permute(0, 3, 2, 1)


def test_pack_layouts_through_convolutions():
    g = R.gen(3)
    Cv, Cu, n, h, w = 5, 3, 2, 3, 4
    # kind 0: Wref[cv][cu][4][4] is the weight of conv2d(U -> V, 4, stride 2, pad 1) and of conv_transpose2d(V -> U)
    W = torch.randn(Cv, Cu, 16, generator=g, dtype=F64)
    down, up = R.pack_ref(0, W)
    Uimg = torch.randn(n, Cu, 2 * h, 2 * w, generator=g, dtype=F64)
    want = F.conv2d(Uimg, W.reshape(Cv, Cu, 4, 4), stride=2, padding=1)
    got = (_im2col(Uimg, 4, 2, 1).reshape(n, h * w, 16 * Cu) @ down).permute(0, 2, 1).reshape(n, Cv, h, w)
    assert torch.allclose(got, want, rtol=0, atol=1e-12)
    V = torch.randn(n, Cv, h, w, generator=g, dtype=F64)
    want = F.conv_transpose2d(V, W.reshape(Cv, Cu, 4, 4), stride=2, padding=1)
    Vp = F.pad(V, (1, 1, 1, 1))
    got = torch.zeros_like(want)
    for ph in range(2):
        for pw in range(2):
            for a in range(2):
                for b in range(2):  # out[2 i + ph][2 j + pw] += V[i + ph - a][j + pw - b] . Wup[ph * 2 + pw][(a * 2 + b) * Cv + cv][cu]
                    src = Vp[:, :, 1 + ph - a:1 + ph - a + h, 1 + pw - b:1 + pw - b + w]
                    blk = up[ph * 2 + pw, (a * 2 + b) * Cv:(a * 2 + b + 1) * Cv]  # [cv][cu]
                    got[:, :, ph::2, pw::2] += torch.einsum("nvij,vu->nuij", src, blk)
    assert torch.allclose(got, want, rtol=0, atol=1e-12)
    # kind 1: conv_transpose2d of a 1x1 map with a 4x4 kernel: out[co][tap] = sum_ci x[ci] Wref[ci][co][tap]
    Cin, Cout = 5, 7
    W1 = torch.randn(Cin, Cout, 16, generator=g, dtype=F64)
    x = torch.randn(n, Cin, generator=g, dtype=F64)
    want = F.conv_transpose2d(x.reshape(n, Cin, 1, 1), W1.reshape(Cin, Cout, 4, 4))  # [n][co][4][4]
    got = (x @ R.pack_ref(1, W1)[1]).reshape(n, 16, Cout).permute(0, 2, 1).reshape(n, Cout, 4, 4)
    assert torch.allclose(got, want, rtol=0, atol=1e-12)
    # kind 2: conv2d(3, pad 1) forward through Wdown, its data gradient through Wup (the mirrored taps)
    W2 = torch.randn(Cv, Cu, 9, generator=g, dtype=F64)
    down, up = R.pack_ref(2, W2)
    X = torch.randn(n, Cu, h, w, generator=g, dtype=F64, requires_grad=True)
    Y = F.conv2d(X, W2.reshape(Cv, Cu, 3, 3), padding=1)
    got = (_im2col(X.detach(), 3, 1, 1).reshape(n, h * w, 9 * Cu) @ down).permute(0, 2, 1).reshape(n, Cv, h, w)
    assert torch.allclose(got, Y.detach(), rtol=0, atol=1e-12)
    dY = torch.randn(n, Cv, h, w, generator=g, dtype=F64)
    dX, = torch.autograd.grad(Y, X, dY)
    got = (_im2col(dY, 3, 1, 1).reshape(n, h * w, 9 * Cv) @ up).permute(0, 2, 1).reshape(n, Cu, h, w)
    assert torch.allclose(got, dX, rtol=0, atol=1e-12)
    for mut, kind, Wk in (("khkw_swapped", 0, W), ("parity_flipped", 0, W), ("k2_not_mirrored", 2, W2)):
        bad, good = R.pack_ref(kind, Wk, mut=(mut,)), R.pack_ref(kind, Wk)
        assert not (torch.equal(bad[0], good[0]) and torch.equal(bad[1], good[1])), mut


@pytest.mark.parametrize("case", R.PACK_CASES, ids=[c.name for c in R.PACK_CASES])
def test_pack_reference_is_the_index_definition(case):
    W = R.pack_weight(case)
    a, b = R.pack_ref(case.kind, W), R.pack_ref_loops(case.kind, W)
    assert (a[0] is None) == (b[0] is None) == (case.kind == 1)
    assert (a[0] is None or R.same_bits(a[0], b[0])) and R.same_bits(a[1], b[1])
    assert case.why and float(W.abs().max()) > 0


@pytest.mark.parametrize("case", R.ADAM_CASES, ids=[c.name for c in R.ADAM_CASES])
def test_adam_reference_is_torch_in_float64(case):
    """Two float64 evaluations of one rule: they differ by float64 rounding of the operands (base / U), a factor 1e-12 is ample."""
    inp = R.adam_inputs(case)
    ref, base = R.adam_ref(case, inp)
    t64 = R.adam_torch(case, inp, F64)
    for k in ("p", "m", "v", "vmax"):
        assert (k in ref) == (k in t64) == (k != "vmax" or case.ams)
        if k in ref:
            assert R.worst_ratio(t64[k], ref[k], 1e-12 * base[k] / R.U) <= 1.0, (case.name, k)


@pytest.mark.parametrize("shape", R.POOL_SHAPES, ids=[R.pool_name(s) for s in R.POOL_SHAPES])
def test_pool_references_are_torch_in_float64(shape):
    n, H, W, C = shape
    x = R.pool_inputs(shape, "pool.fwd").double().requires_grad_(True)
    y = F.avg_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1, count_include_pad=True).permute(0, 2, 3, 1)
    ref, mag = R.pool_fwd_ref(x.detach())
    assert ref.shape == y.shape and torch.allclose(ref, y.detach(), rtol=0, atol=1e-14) and bool((mag >= ref.abs() * 9 - 1e-12).all())
    dy = R.pool_inputs(shape, "pool.bwd")
    dx, = torch.autograd.grad(y, x, dy.double())
    assert torch.allclose(R.pool_bwd_ref(dy, H, W)[0], dx, rtol=0, atol=1e-14)
    x = R.pool_inputs(shape, "up.fwd").double().requires_grad_(True)
    y = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="nearest").permute(0, 2, 3, 1)
    assert torch.equal(R.up_fwd_ref(x.detach()), y.detach())
    dy = R.pool_inputs(shape, "up.bwd")
    dx, = torch.autograd.grad(y, x, dy.double())
    assert torch.allclose(R.up_bwd_ref(dy)[0], dx, rtol=0, atol=1e-14)


def _bf16_rne_bits(x):
    """Round-to-nearest-even to bfloat16 on the bit pattern (finite inputs): the upper 16 bits as int16."""
    u = x.numpy().view(np.uint32).astype(np.uint64)
    r = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)
    return torch.from_numpy((r & np.uint64(0xFFFF)).astype(np.uint16).view(np.int16).copy())


def _split_by_bits(x):
    x = x.reshape(-1).float()
    out, r = [], x
    for _ in range(3):
        p = _bf16_rne_bits(r)
        out.append(p)
        r = r - (p.to(torch.int32) << 16).view(torch.float32)
    return torch.stack(out)


def test_bf3_roundtrip_condition():
    """a + (b + c) == x bit for bit, and the split is three RNE casts of exact residues, over 2^20 normal values on scales
    2^-90 .. 2^90 with |x| >= 2^-100 plus the patterns (all-ones mantissa, powers of two, ties of the first and second cast)."""
    x = torch.cat([R.bf3_input(1 << 20, seed=s) for s in (0, 1)] + [R.BF3_PATTERNS, -R.BF3_PATTERNS])
    assert float(x.abs().min()) >= 2.0 ** -100 and bool(torch.isfinite(x).all())
    planes = R.bf3_split(x)
    assert torch.equal(planes, _split_by_bits(x)), "torch's bfloat16 cast is not the round-to-nearest-even of the bit pattern"
    assert R.same_bits(R.bf3_join(planes), x), "a + (b + c) does not return the input"
    assert bool(torch.isfinite(planes.view(torch.bfloat16).float()).all())
    for n in (1, 2, 3, 511, 512, 513):
        xi = R.bf3_input(n)
        assert float(xi.abs().min()) >= 2.0 ** -100 and R.same_bits(R.bf3_join(R.bf3_split(xi)), xi)


# ---- the stand-in backend: the plain fp32 CPU evaluation of every entry -------------------------------------------------------------------
class Standin:
    rc = 0

    def pack(self, descs, via="multi", n_arg=None, may_fail=False):
        outs = []
        for d in descs:
            W, want = d["W"], d["want"]
            Cv, Cu, _ = W.shape
            down, up = R.pack_ref_loops(d["kind"], W)
            o = dict(guards=True, untouched=False, Wdown=None, Wup=None, Fdown=None, Fup=None, amax=None)
            if "Wdown" in want:
                o["Wdown"] = R.place_down(down, d.get("ld") or Cv, d.get("col_off", 0))
            if "Wup" in want:
                o["Wup"] = up
            for k in ("Fdown", "Fup"):  # the host pieces in element order: a permutation of what the kernel lays out by role and lane
                if k in want:
                    o[k] = _split_by_bits(W).reshape(3, -1, 512).permute(1, 0, 2).reshape(-1).contiguous()
            if "amax" in want and via == "multi":
                o["amax"] = torch.tensor([max(float(W.abs().max()), d.get("preset", 0.0))])
            outs.append(o)
        return outs

    def adam(self, case, inp, names=None):
        out = R.adam_torch(case, inp)
        pub = torch.tensor(R.adam_scalars(case.lr, case.step, case.wd, case.gscale), dtype=torch.float32)
        out.update(guards=True, kernels=None, pub=pub if case.entry in ("pub", "dev") else None)
        return out

    def act_bwd(self, dY, Y, act, off=None, names=None):
        return dict(out=dY * R.act_grad32(Y, act), guards=True, kernels=None, Y_kept=True)

    def act_bwd_scaled(self, g, a, Y, act, off=None, names=None):
        return dict(out=(torch.tensor(a) * g) * R.act_grad32(Y, act), guards=True, kernels=None)

    def axpby(self, x, a, y, b, act, n, off=None, names=None):
        v = (a * x if x is not None else torch.zeros(n)) + (b * y if y is not None else torch.zeros(n))
        v = {R.NONE: v, R.RELU: torch.where(v > 0, v, torch.zeros_like(v)), R.LEAKY: torch.where(v > 0, v, R.F02 * v),
             R.SIGMOID: torch.sigmoid(v)}[act]
        return dict(out=v, guards=True, kernels=None)

    def f32_to_bf3(self, x, off=False):
        return dict(out=_split_by_bits(x), guards=True)

    def bf3_to_f32(self, planes, off=False):
        return dict(out=R.bf3_join(planes), guards=True)

    def layout(self, x, to_nhwc):
        return dict(out=(x.permute(0, 2, 3, 1) if to_nhwc else x.permute(0, 3, 1, 2)).contiguous(), guards=True)

    def pool(self, op, x, shape, off=False, names=None):
        n, H, W, C = shape
        nchw = lambda t: t.permute(0, 3, 1, 2)  # noqa: E731
        if op in ("pool.fwd", "up.fwd"):
            y = F.avg_pool2d(nchw(x), 3, 2, 1) if op == "pool.fwd" else F.interpolate(nchw(x), scale_factor=2, mode="nearest")
        else:
            src = torch.zeros(n, C, H, W, requires_grad=True)
            fwd = F.avg_pool2d(src, 3, 2, 1) if op == "pool.bwd" else F.interpolate(src, scale_factor=2, mode="nearest")
            y, = torch.autograd.grad(fwd, src, nchw(x).contiguous())
        return dict(out=y.permute(0, 2, 3, 1).contiguous(), guards=True, kernels=None)

    def rng(self, state, n, uniform, lo=0.0, hi=1.0, off=False):
        seed, offset, _ = state
        words = R.rng_words(seed, offset, n)
        if uniform:
            u = (words >> np.uint64(8)).astype(np.float32).reshape(-1)[:n] * np.float32(2.0 ** -24)
            out = torch.from_numpy((np.float32(lo) + u * (np.float32(hi) - np.float32(lo))).astype(np.float32))
        else:
            out = R.rng_normal_ref(words, n, dtype=np.float32)[0]
        grid = ((n + 3) // 4 + 255) // 256
        return dict(out=out, guards=True, state=[seed, (offset + grid * 256) % 2 ** 64, 0])


BE = Standin()


def measure():
    worst = {}
    for case in R.ADAM_CASES:
        inp = R.adam_inputs(case)
        ref, base = R.adam_ref(case, inp)
        for k, v in R.adam_ratios(case, R.adam_torch(case, inp), ref, base).items():
            G.note(worst, k, v, case.name)
    for case in R.RNG_CASES:
        words = R.rng_words(case.seed, case.offset, case.n)
        ref, base = R.rng_normal_ref(words, case.n)
        G.note(worst, "rng.normal", R.worst_ratio(R.rng_normal_ref(words, case.n, dtype=np.float32)[0], ref, R.U * base), case.name)
    return worst


def test_error_constants():
    """The measured constants: C = 4x the largest |err| / base of the plain fp32 CPU evaluation (torch.optim.Adam(foreach=False);
    numpy float32 Box-Muller) against the float64 reference over the case table, rounded up: never below 4x the measured value,
    never more than 8x above it.  The measured values and the cases that set them are in the docstring of tests/test_gpu_misc.py."""
    worst = measure()
    print({k: (round(v, 3), n) for k, (v, n) in sorted(worst.items())})
    assert set(worst) == set(R.MEASURED_STAGES)
    for k, (v, name) in worst.items():
        assert 4 * v <= R.C_STAGE[k], f"{k}: fp32 on the CPU shows {v:.3g} on {name}; C = {R.C_STAGE[k]} is less than 4x that"
        assert R.C_STAGE[k] <= 8 * v, f"{k}: C = {R.C_STAGE[k]} is more than 8x the measured {v:.3g}"


# ---- the GPU file's comparison routines on the stand-in -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.PACK_CASES, ids=[c.name for c in R.PACK_CASES])
def test_check_pack(case):
    G.check_pack(case, BE)


@pytest.mark.parametrize("case", R.ADAM_CASES, ids=[c.name for c in R.ADAM_CASES])
def test_check_adam(case):
    G.check_adam(case, BE)


@pytest.mark.parametrize("act", R.ACTS)
def test_check_activations(act):
    for n in R.ACT_BWD_N + [R.BIG + 3]:
        G.check_act_bwd(n, act, None, BE)
    for n in R.ACT_SCALED_N:
        G.check_act_bwd_scaled(n, act, "g", BE)


@pytest.mark.parametrize("mode", ["xy", "x", "y"])
def test_check_axpby(mode):
    for n in (1, 4, 5, 1023, 1028):
        G.check_axpby(n, mode, None, BE)


def test_check_bf3_and_layout():
    for n in (1, 2, 3, 511, 512, 513):
        G.check_bf3(n, BE)
    for shape in R.LAYOUT_SHAPES:
        G.check_layout(shape, BE)


@pytest.mark.parametrize("op", ["pool.fwd", "pool.bwd", "up.fwd", "up.bwd"])
def test_check_pool(op):
    for shape in R.POOL_SHAPES:
        G.check_pool(op, shape, BE)


@pytest.mark.parametrize("case", R.RNG_CASES, ids=[c.name for c in R.RNG_CASES])
def test_check_rng(case):
    G.check_rng(case, BE)


# ---- teeth ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mut,family,name", R.TEETH, ids=[t[0] for t in R.TEETH])
def test_tolerance_rejects_mutated_reference(mut, family, name):
    """The clean fp32 evaluation against the WRONG reference leaves the bound (bit-exact models: differs in bits) on the named case,
    while it stays inside against the right one."""
    m = (mut,)
    if family == "pack":
        case = R.PACK_BY_NAME[name]
        W = R.pack_weight(case)
        got, bad = R.pack_ref_loops(case.kind, W), R.pack_ref(case.kind, W, mut=m)
        assert not (R.same_bits(got[0], bad[0]) and R.same_bits(got[1], bad[1]))
        return
    if family == "adam":
        case = R.ADAM_BY_NAME[name]
        inp = R.adam_inputs(case)
        got = R.adam_torch(case, inp)
        clean = R.adam_ratios(case, got, *R.adam_ref(case, inp))
        bad = R.adam_ratios(case, got, *R.adam_ref(case, inp, mut=m))
    elif family in ("pool.fwd", "pool.bwd", "up.bwd"):
        shape = tuple(int(v) for v in name.split("x"))
        x = R.pool_inputs(shape, family)
        got = BE.pool(family, x, shape)["out"]
        fn = {"pool.fwd": lambda mu: R.pool_fwd_ref(x, mu), "pool.bwd": lambda mu: R.pool_bwd_ref(x, shape[1], shape[2], mu),
              "up.bwd": lambda mu: R.up_bwd_ref(x, mu)}[family]
        scale = 1.0 if family == "up.bwd" else 1.0 / 9
        (ref, mag), (wrong, _) = fn(()), fn(m)
        clean = {family: R.worst_ratio(got, ref, R.U * mag * scale + R.SUB)}
        bad = {family: R.worst_ratio(got, wrong, R.U * mag * scale + R.SUB)}
    elif family == "act":
        n = int(name[1:])
        act = R.LEAKY if mut == "leaky_001" else R.SIGMOID
        dY, Y = R.act_inputs(n, act)
        got = BE.act_bwd(dY, Y, act)["out"]
        ref, wrong = dY.double() * R.act_grad64(Y, act), dY.double() * R.act_grad64(Y, act, m)
        clean = {"act_bwd.sigmoid": R.worst_ratio(got, ref, R.U * ref.abs() + R.SUB)}
        bad = {"act_bwd.sigmoid": R.worst_ratio(got, wrong, R.U * wrong.abs() + R.SUB)}  # (bit-exact forms: far outside one rounding too)
    else:
        case = R.RNG_BY_NAME[name]
        w, wm = R.rng_words(case.seed, case.offset, case.n), R.rng_words(case.seed, case.offset, case.n, m)
        if family == "rng.uniform":
            got = BE.rng((case.seed, case.offset, 0), case.n, True)["out"]
            assert R.same_bits(got, R.rng_uniform_ref(w, case.n)[0].float()) and not R.same_bits(got, R.rng_uniform_ref(wm, case.n)[0].float())
            return
        got = BE.rng((case.seed, case.offset, 0), case.n, False)["out"]
        (ref, base), (wrong, _) = R.rng_normal_ref(w, case.n), R.rng_normal_ref(wm, case.n, m)
        clean = {family: R.worst_ratio(got, ref, R.U * base)}
        bad = {family: R.worst_ratio(got, wrong, R.U * base)}
    assert all(v <= R.C_STAGE[k] for k, v in clean.items()), clean
    f = max(v / R.C_STAGE[k] for k, v in bad.items())
    print(mut, name, f"{f:.3g}x the bound")
    assert f > 1.0, f"{mut} passes on {name}: {f:.3g}x the bound"


def test_case_tables_hold_the_edges():
    """The shapes of the issue, read off the launch code of misc.hip."""
    pc = R.PACK_CASES
    assert len(pc) == 16 and all(c.why for c in pc)  # MVK_PACK_MAX: test_pack_one_launch_of_sixteen launches the whole table at once
    assert {(c.Cv, c.Cu) for c in pc if c.kind == 0 and not c.off and c.Cv % 8 == 0 and c.Cu % 8 == 0} >= {(8, 8), (16, 24), (64, 32), (128, 64), (256, 128)}
    assert {(c.Cv, c.Cu) for c in pc if c.kind == 0 and (c.Cv % 8 or c.Cu % 8)} == {(32, 3), (3, 32), (1, 1)}
    assert {(c.Cv, c.Cu) for c in pc if c.frags and c.off} == {(64, 32), (128, 64)} == {(c.Cv, c.Cu) for c in pc if c.frags and not c.off}
    assert {c.col_off for c in pc if c.ld_mul == 2} == {8, 2}
    assert {(c.Cv, c.Cu) for c in pc if c.kind == 1} == {(5, 7), (20, 128)} and {(c.Cv, c.Cu) for c in pc if c.kind == 2} == {(20, 20), (128, 128)}
    assert 9 * 128 * 128 > 65536 and 256 * 128 // 64 > 256
    ac = R.ADAM_CASES
    assert {c.n for c in ac} >= {1, 3, 4, 1028, 4 * 256 + 4, R.BIG + 5} and {c.step for c in ac} == {1, 2, 1000}
    assert {c.off for c in ac} == {None, "p", "g", "m", "v", "vmax"} and {c.entry for c in ac} == {"step", "amsgrad", "fused", "pub", "dev"}
    assert {c.wd for c in ac} == {0.0, 0.01} and {c.gscale for c in ac} == {1.0, 0.5} and {c.zero for c in ac} == {True, False}
    for c in ac:
        assert c.why and (c.entry != "dev" or (c.n % 4 == 0 and not c.off))
        if c.ams:
            inp = R.adam_inputs(c)
            v1 = R.adam_ref(c, inp)[0]["v"]
            assert c.n < 2 or (bool((inp["vmax"].double() > v1).any()) and bool((inp["vmax"].double() < v1).any())), c.name
    assert {c.n for c in R.RNG_CASES} >= {1, 4, 5, 1024, 4 * 256 + 1} and any(c.off for c in R.RNG_CASES)
    carry = R.RNG_BY_NAME["hi-carry-n1024"]
    t = np.arange(256, dtype=np.uint64) + np.uint64(carry.offset)
    assert len(set((t >> np.uint64(32)).tolist())) == 2
    assert set(R.ACT_SPECIAL) >= {0.0, 1.0, -1.5, 1e-40} and math.copysign(1, R.ACT_SPECIAL[1]) == -1
    assert {s[1] for s in R.POOL_SHAPES} >= {1, 2} and {s[2] for s in R.POOL_SHAPES} >= {1, 2} and (2, 7, 7, 20) in R.POOL_SHAPES
