"""The 3x3 / stride-2 kernels of csrc/polyconv.hip, entry by entry against float64 (tests/convmmnist_ref.py), the fused trunks, the
autograd nodes and the four PolyMNIST convolutional modules against the fixtures of tests/golden/make_convmmnist_golden.py.

Layer entries: every entry of every output, |got - ref| <= C_ENTRY * bound (bound = op(|a|, |b|) + |bias| (+ |initial content|), times
the mask), on the three architecture layers in both directions and one non-square odd / even map, n in {1, 5, 17}, NCHW flag on and
off, ReLU / none, with and without mask, weight gradient with and without either bias gradient, overwriting and accumulating onto a
non-zero target.  The operands and float64 references are computed once per shape at n = 17; n = 1 and n = 5 use their first
images (every image is on its own).  tests/test_convmmnist_host.py shows that the same check rejects 16-bit operands.

Properties: a second run gives the same bits; image i at n = 17 has the bits of the same image at n = 1; shapes mvk_conv3s2_ok
refuses raise MvkError.

Fused trunks: against the float64 chain within the propagated tolerance of convmmnist_ref.trunk_down_chain / trunk_up_chain, and
against the three layer launches BIT FOR BIT (they run the same device routine on the same operands in the same order).

Nodes and modules: outputs, dz and every parameter gradient within 1e-4 of the tensor's largest magnitude, against the fixture (all
outputs, dz, the sampled gradient entries and sums) and against the float64 networks entry by entry (which
tests/test_convmmnist_host.py ties to the fixture); the measured ratios are printed.  The no-grad forward (fused trunk) against the
grad-mode forward (layer launches): the trunk bit for bit, the module outputs within twice the propagated bound.
"""
import functools
import types

import numpy as np
import pytest
import torch

import convmmnist_ref as CR
from golden_cases import P, load_case, t

pytestmark = pytest.mark.gpu

NONE, RELU, C_ENTRY = CR.NONE, CR.RELU, CR.C_ENTRY
NMAX = 17


def dev(x):
    return None if x is None else x.float().contiguous().cuda()


def K():
    from multivae_amd import kernels

    return kernels


def held(name, got, ref, what=""):
    """got: float tensor on the CPU laid out like ref.ref.  -> worst |got - ref| / (C_ENTRY bound)."""
    tol = C_ENTRY * ref.bound + 1e-30
    ratio = float(((got.double() - ref.ref).abs() / tol).max())
    print(f"{name}{what}: worst |got - ref| / tolerance = {ratio:.3f}")
    assert ratio <= 1.0, (name, what, ratio)
    return ratio


@functools.lru_cache(maxsize=None)
def down_data(H, W, Cu, Cv):
    return CR.down_operands(1000 + H * 7 + Cu, NMAX, H, W, Cu, Cv)


@functools.lru_cache(maxsize=None)
def up_data(H, W, Cu, Cv):
    return CR.up_operands(2000 + H * 7 + Cu, NMAX, H, W, Cu, Cv)


def run_down(U, Wt, b, act=NONE, nchw_in=False, src=None, mact=NONE):
    n, Cu, H, W = U.shape
    V = K().conv3s2_down(dev(U) if nchw_in else dev(CR.nhwc(U)), dev(Wt), dev(b), n, H, W, Cu, Wt.shape[0], act, u_nchw=nchw_in,
                         v_act_src=None if src is None else dev(CR.nhwc(src)), v_act=mact)
    return V


def run_up(V, Wt, b, H, W, act=NONE, nchw_out=False, src=None, mact=NONE):
    n, Cu = V.shape[0], Wt.shape[1]
    s = None if src is None else (dev(src) if nchw_out else dev(CR.nhwc(src)))
    U = K().conv3s2_up(dev(CR.nhwc(V)), dev(Wt), dev(b), n, H, W, Cu, Wt.shape[0], act, u_nchw=nchw_out, u_act_src=s, u_act=mact)
    return U


def variants(Cu):
    """(act, mask, nchw flag)"""
    v = [(NONE, False, False), (RELU, False, False), (NONE, True, False), (RELU, True, False)]
    if Cu == 3:
        v += [(NONE, False, True), (RELU, True, True)]
    return v


@pytest.mark.parametrize("n", [1, 5, NMAX])
@pytest.mark.parametrize("H,W,Cu,Cv", CR.LAYER_SHAPES)
def test_down_against_float64(H, W, Cu, Cv, n):
    assert K().conv3s2_ok(H, W, Cu, Cv)
    U, Wt, b, src = (x[:n] if i in (0, 3) else x for i, x in enumerate(down_data(H, W, Cu, Cv)))
    for act, mask, flag in variants(Cu):
        ref = CR.down(U, Wt, b, act, src if mask else None, RELU)
        got = run_down(U, Wt, b, act, flag, src if mask else None, RELU)
        again = run_down(U, Wt, b, act, flag, src if mask else None, RELU)
        assert torch.equal(got, again)
        held(f"down {H}x{W} {Cu}->{Cv} n={n}", CR.nchw(got.cpu()), ref, f" act={act} mask={mask} nchw={flag}")
    ref = CR.down(U, Wt, None)
    held(f"down {H}x{W} {Cu}->{Cv} n={n}", CR.nchw(run_down(U, Wt, None).cpu()), ref, " no bias")


@pytest.mark.parametrize("n", [1, 5, NMAX])
@pytest.mark.parametrize("H,W,Cu,Cv", CR.LAYER_SHAPES)
def test_up_against_float64(H, W, Cu, Cv, n):
    V, Wt, b, src = (x[:n] if i in (0, 3) else x for i, x in enumerate(up_data(H, W, Cu, Cv)))
    for act, mask, flag in variants(Cu):
        ref = CR.up(V, Wt, H, W, b, act, src if mask else None, RELU)
        got = run_up(V, Wt, b, H, W, act, flag, src if mask else None, RELU)
        again = run_up(V, Wt, b, H, W, act, flag, src if mask else None, RELU)
        assert torch.equal(got, again)
        assert tuple(got.shape) == ((n, Cu, H, W) if flag else (n, H, W, Cu))
        held(f"up {H}x{W} {Cv}->{Cu} n={n}", got.cpu() if flag else CR.nchw(got.cpu()), ref, f" act={act} mask={mask} nchw={flag}")
    held(f"up {H}x{W} {Cv}->{Cu} n={n}", CR.nchw(run_up(V, Wt, None, H, W).cpu()), CR.up(V, Wt, H, W, None), " no bias")


@pytest.mark.parametrize("H,W,Cu,Cv", CR.LAYER_SHAPES)
def test_image_bits_do_not_depend_on_n(H, W, Cu, Cv):
    U, Wt, b, _ = down_data(H, W, Cu, Cv)
    full = run_down(U, Wt, b, RELU, Cu == 3)
    V, Wu, bu, _ = up_data(H, W, Cu, Cv)
    fullu = run_up(V, Wu, bu, H, W, RELU, Cu == 3)
    for i in (0, 3, NMAX - 1):
        assert torch.equal(run_down(U[i:i + 1], Wt, b, RELU, Cu == 3)[0], full[i]), ("down", i)
        assert torch.equal(run_up(V[i:i + 1], Wu, bu, H, W, RELU, Cu == 3)[0], fullu[i]), ("up", i)


@pytest.mark.parametrize("n", [1, 5, NMAX])
@pytest.mark.parametrize("H,W,Cu,Cv", CR.LAYER_SHAPES)
def test_wgrad_against_float64(H, W, Cu, Cv, n):
    from multivae_amd import _lib
    from multivae_amd.schedule import _ws

    U, dV, init, binit_v, binit_u = CR.wgrad_operands(3000 + H * 7 + Cu + n, n, H, W, Cu, Cv)
    dVd = dev(CR.nhwc(dV))
    ws = _ws(dVd)
    # (bias gradient side, accumulate onto the non-zero target, U is the NCHW image)
    cases = [(0, False, False), (1, True, False), (2, True, False), (1, False, False), (0, True, False)]
    if Cu == 3:
        cases += [(1, True, True), (2, False, True)]
    for side, acc, flag in cases:
        Ud = dev(U) if flag else dev(CR.nhwc(U))
        binit = (None, binit_v, binit_u)[side]
        ref = CR.wgrad(U, dV, init if acc else None, side, binit if acc else None)

        def launch():
            dw, db = dev(init).clone(), (dev(binit).clone() if side else None)
            _lib.call("mvk_conv3s2_wgrad", _lib.ptr(Ud), _lib.ptr(dVd), _lib.ptr(dw), _lib.ptr(db), side, n, H, W, Cu, Cv, int(flag),
                      int(acc), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
            return dw, db

        dw, db = launch()
        dw2, db2 = launch()
        assert torch.equal(dw, dw2) and (db is None or torch.equal(db, db2))
        what = f" db_side={side} accumulate={acc} nchw={flag}"
        held(f"wgrad {H}x{W} {Cu}->{Cv} n={n}", dw.cpu(), ref["dw"], what)
        if side:
            held(f"wgrad db {H}x{W} {Cu}->{Cv} n={n}", db.cpu(), ref["db"], what)


def test_wgrad_node_helper_accumulates_into_grad():
    """kernels.conv3s2_wgrad writes straight into an existing .grad (the flat-gradient-buffer view of the trainer)."""
    H, W, Cu, Cv, n = 7, 7, 64, 128, 5
    U, dV, init, binit_v, _ = CR.wgrad_operands(77, n, H, W, Cu, Cv)
    w = torch.nn.Parameter(torch.zeros(Cv, Cu, 3, 3, device="cuda"))
    b = torch.nn.Parameter(torch.zeros(Cv, device="cuda"))
    w.grad, b.grad = dev(init).clone(), dev(binit_v).clone()
    rw, rb = K().conv3s2_wgrad(dev(CR.nhwc(U)), dev(CR.nhwc(dV)), w, b, n, H, W, Cu, Cv)
    assert rw is None and rb is None
    ref = CR.wgrad(U, dV, init, 1, binit_v)
    held("wgrad into .grad", w.grad.cpu(), ref["dw"])
    held("wgrad db into .grad", b.grad.cpu(), ref["db"])


def test_refused_shapes_raise():
    from multivae_amd import _lib

    Kn = K()
    x = torch.zeros(1, 8, 8, 16, device="cuda")
    w = torch.zeros(32, 16, 3, 3, device="cuda")
    for Cu, Cv in ((16, 32), (3, 64), (32, 32), (128, 64)):
        assert not Kn.conv3s2_ok(8, 8, Cu, Cv)
    assert not Kn.conv3s2_ok(0, 8, 3, 32)
    with pytest.raises(_lib.MvkError):
        Kn.conv3s2_down(x, w, None, 1, 8, 8, 16, 32)
    with pytest.raises(_lib.MvkError):
        Kn.conv3s2_up(x, w, None, 1, 8, 8, 16, 32)
    with pytest.raises(_lib.MvkError):
        _lib.call("mvk_conv3s2_down", _lib.ptr(x), _lib.ptr(w), None, _lib.ptr(x), 1, 8, 8, 16, 32, 0, 0, None, 0, _lib.stream_ptr())
    with pytest.raises(_lib.MvkError):
        _lib.call("mvk_conv3s2_up", _lib.ptr(x), _lib.ptr(w), None, _lib.ptr(x), 1, 8, 8, 16, 32, 0, 0, None, 0, _lib.stream_ptr())
    ws = torch.zeros(1 << 16, device="cuda")
    with pytest.raises(_lib.MvkError):
        _lib.call("mvk_conv3s2_wgrad", _lib.ptr(x), _lib.ptr(x), _lib.ptr(w), None, 0, 1, 8, 8, 16, 32, 0, 0, _lib.ptr(ws), ws.numel(),
                  _lib.stream_ptr())
    with pytest.raises(_lib.MvkError):  # the NCHW flag is the 3-channel image's
        Kn.conv3s2_down(torch.zeros(1, 14, 14, 32, device="cuda"), torch.zeros(64, 32, 3, 3, device="cuda"), None, 1, 14, 14, 32, 64,
                        u_nchw=True)
    with pytest.raises(_lib.MvkError):
        Kn.polyenc_forward(torch.zeros(2, 3, 32, 32, device="cuda"), *[torch.zeros(s, device="cuda") for s in
                                                                      ((32, 3, 3, 3), (32,), (64, 32, 3, 3), (64,), (128, 64, 3, 3), (128,))])


# ---- fused trunks ------------------------------------------------------------------------------------------------------------------------
def _trunk_params():
    sds = CR.golden_state_dicts(4100, 5, 3)
    enc = [t(sds["adapted"][f"shared_encoder.{i}.{w}"]) for i in (0, 2, 4) for w in ("weight", "bias")]
    dec = [t(sds["dec"][f"decoder.{i}.{w}"]) for i in (3, 5, 7) for w in ("weight", "bias")]
    return enc, dec


@functools.lru_cache(maxsize=None)
def _trunk_refs():
    enc, dec = _trunk_params()
    x = t(P.uniform((NMAX, 3, 28, 28), 91))
    h0 = t(P.uniform((NMAX, 128, 4, 4), 92, -1.0, 1.0)).clamp_min(0)
    return x, CR.trunk_down_chain(x, enc), h0, CR.trunk_up_chain(h0, dec)


@pytest.mark.parametrize("n", [1, 5, NMAX])
def test_fused_encoder_trunk(n):
    """Against the float64 chain within its propagated tolerance; against the three layer launches bit for bit."""
    enc, _ = _trunk_params()
    x, (h3, e3), _, _ = _trunk_refs()
    ep = [dev(p) for p in enc]
    xd = dev(x[:n])
    got = K().polyenc_forward(xd, *ep)
    assert tuple(got.shape) == (n, 4, 4, 128) and torch.equal(got, K().polyenc_forward(xd, *ep))
    ratio = float(((CR.nchw(got.cpu()).double() - h3[:n]).abs() / e3[:n]).max())
    print(f"polyenc n={n}: worst |got - chain| / propagated tolerance = {ratio:.3f}")
    assert ratio <= 1.0
    h1 = K().conv3s2_down(xd, ep[0], ep[1], n, 28, 28, 3, 32, RELU, u_nchw=True)
    h2 = K().conv3s2_down(h1, ep[2], ep[3], n, 14, 14, 32, 64, RELU)
    assert torch.equal(got, K().conv3s2_down(h2, ep[4], ep[5], n, 7, 7, 64, 128, RELU))
    if n == NMAX:  # an image's bits do not depend on n or on its place in a tile
        for i in (0, 5, NMAX - 1):
            assert torch.equal(K().polyenc_forward(xd[i:i + 1], *ep)[0], got[i])


@pytest.mark.parametrize("n", [1, 5, NMAX])
def test_fused_decoder_trunk(n):
    _, dec = _trunk_params()
    _, _, h0, (img, e3) = _trunk_refs()
    dp = [dev(p) for p in dec]
    hd = dev(CR.nhwc(h0[:n]))
    got = K().polydec_forward(hd, *dp)
    assert tuple(got.shape) == (n, 3, 28, 28) and torch.equal(got, K().polydec_forward(hd, *dp))
    ratio = float(((got.cpu().double() - img[:n]).abs() / e3[:n]).max())
    print(f"polydec n={n}: worst |got - chain| / propagated tolerance = {ratio:.3f}")
    assert ratio <= 1.0
    d1 = K().conv3s2_up(hd, dp[0], dp[1], n, 7, 7, 64, 128, RELU)
    d2 = K().conv3s2_up(d1, dp[2], dp[3], n, 14, 14, 32, 64, RELU)
    assert torch.equal(got, K().conv3s2_up(d2, dp[4], dp[5], n, 28, 28, 3, 32, NONE, u_nchw=True))
    if n == NMAX:
        for i in (0, 5, NMAX - 1):
            assert torch.equal(K().polydec_forward(hd[i:i + 1], *dp)[0], got[i])


# ---- autograd nodes and modules against the fixtures ----------------------------------------------------------------------------------------
def _classes():
    from multivae_amd.models.nn import mmnist as M

    return dict(conv=M.EncoderConvMMNIST, adapted=M.EncoderConvMMNIST_adapted, multi=M.EncoderConvMMNIST_multilatents, dec=M.DecoderConvMMNIST)


def _build(kind, cfg, sd_np):
    m = _classes()[kind](types.SimpleNamespace(latent_dim=cfg["L"], style_dim=cfg["S"]))
    m.load_state_dict({k: t(v) for k, v in sd_np.items()})  # the reference's keys and shapes, strict
    return m.cuda()


def _parity(name, got, ref, scale=None):
    ref = torch.as_tensor(ref).double()
    scale = float(ref.abs().max()) if scale is None else scale
    r = float((got.detach().cpu().double() - ref).abs().max()) / scale
    print(f"{name}: |got - ref| / max |ref| = {r:.2e}")
    assert r <= CR.PARITY, (name, r)


def _sd64(sd_np):
    return {k: t(v).double().requires_grad_(True) for k, v in sd_np.items()}


def _outs(o):
    return [o[k] for k in ("embedding", "log_covariance", "style_embedding", "style_log_covariance") if k in o]


@pytest.fixture(scope="module", params=CR.GOLDEN_CASES)
def case(request):
    cfg, arrays = load_case(request.param)
    return cfg, arrays, CR.golden_inputs(cfg["seed"], cfg["B"], cfg["K"], cfg["L"], cfg["S"]), CR.golden_state_dicts(cfg["seed"], cfg["L"], cfg["S"])


@pytest.mark.parametrize("kind", CR.KINDS)
def test_encoders_against_fixture(case, kind):
    cfg, arrays, (x, _z2, _z3, pe, _pd2, _pd3), sds = case
    m = _build(kind, cfg, sds[kind])
    xd = dev(t(x))
    outs = _outs(m(xd))
    assert len(outs) == (4 if (kind == "multi" and cfg["S"] > 0) else 2)
    sum((a * dev(t(p))).sum() for a, p in zip(outs, pe)).backward()
    s64 = _sd64(sds[kind])
    o64 = CR.encoder64(kind, s64, t(x).double())
    sum((a * t(p).double()).sum() for a, p in zip(o64, pe)).backward()
    for a, a64, nme in zip(outs, o64, CR.OUT_NAMES):
        assert tuple(a.shape) == tuple(arrays[f"{kind}.{nme}"].shape)
        _parity(f"{kind}.{nme} vs fixture", a, arrays[f"{kind}.{nme}"])
        _parity(f"{kind}.{nme} vs float64", a, a64.detach())
    grads = {f"{kind}.{n_}": p.grad for n_, p in m.named_parameters()}
    assert all(g is not None for g in grads.values())
    print(f"{kind}: sampled gradient entries, worst / max = {CR.check_grad_stats(arrays, grads):.2e}")
    for n_, p in m.named_parameters():
        _parity(f"{kind}.{n_} grad vs float64", p.grad, s64[n_].grad)
    # the reference's squeezes at n = 1, and the no-grad forward (fused trunk) against the grad-mode one
    with torch.no_grad():
        o1 = m(xd[:1])
        assert [list(v.shape) for v in o1.values()] == cfg["shapes_n1"][kind]
        ng = _outs(m(xd))
    K_ = K()
    seq = m.shared_encoder if kind != "multi" else m.encoder_class
    params = [q for i in (0, 2, 4) for q in (seq[i].weight, seq[i].bias)]
    h3_grad = K_.PolyConvEncoderFn.apply(xd, *params)
    with torch.no_grad():
        h3_ng = K_.PolyConvEncoderFn.run(xd, *params)
    assert h3_grad.requires_grad and not h3_ng.requires_grad and torch.equal(h3_grad, h3_ng)
    # module outputs: twice the bound propagated through the trunk and the layers behind it
    h3c, e3 = CR.trunk_down_chain(t(x), [t(sds[kind][f"{'shared_encoder' if kind != 'multi' else 'encoder_class'}.{i}.{w}"])
                                         for i in (0, 2, 4) for w in ("weight", "bias")])
    for a, b_, nme in zip(outs, ng, CR.OUT_NAMES[:2]):
        tol = CR.heads_tol(kind, sds[kind], nme, h3c, e3).reshape(a.shape)
        assert bool(((a.detach() - b_).abs().cpu().double() <= 2 * tol).all()), (kind, nme)


@pytest.mark.parametrize("tag", ["dec2", "dec3"])
def test_decoder_against_fixture(case, tag):
    cfg, arrays, (_x, z2, z3, _pe, pd2, pd3), sds = case
    z_np, pd = (z2, pd2) if tag == "dec2" else (z3, pd3)
    m = _build("dec", cfg, sds["dec"])
    assert m.rows_independent and [tuple(p.shape) for p in m.late_leaf_params()] == [(128, 64, 3, 3), (64, 32, 3, 3), (32, 3, 3, 3)]
    z = dev(t(z_np)).requires_grad_(True)
    rec = m(z).reconstruction
    assert tuple(rec.shape) == tuple(z_np.shape[:-1]) + (3, 28, 28)
    (rec * dev(t(pd))).sum().backward()
    s64 = _sd64(sds["dec"])
    z64 = t(z_np).double().requires_grad_(True)
    r64 = CR.decoder64(s64, z64)
    (r64 * t(pd).double()).sum().backward()
    idx = P.hash_indices(rec.numel(), 512, 77)
    _parity(f"{tag}.recon samples vs fixture", rec.reshape(-1)[torch.as_tensor(idx, device="cuda")], arrays[tag + ".recon_sample"],
            scale=float(arrays[tag + ".recon_sum"][2]))
    _parity(f"{tag}.recon vs float64", rec, r64.detach())
    _parity(f"{tag}.dz vs fixture", z.grad, arrays[tag + ".dz"])
    _parity(f"{tag}.dz vs float64", z.grad, z64.grad)
    grads = {f"{tag}.{n_}": p.grad for n_, p in m.named_parameters()}
    print(f"{tag}: sampled gradient entries, worst / max = {CR.check_grad_stats(arrays, grads):.2e}")
    for n_, p in m.named_parameters():
        _parity(f"{tag}.{n_} grad vs float64", p.grad, s64[n_].grad)
    with torch.no_grad():
        ng = m(z.detach()).reconstruction
    assert not ng.requires_grad and tuple(ng.shape) == tuple(rec.shape)
    # the trunk is the same device routine either way; the linear layer in front of it is the same launch
    assert torch.equal(ng, rec.detach())


def test_nodes_take_the_fused_trunks_when_nothing_is_kept(monkeypatch):
    """Under torch.no_grad(), or with no input that requires a gradient, a node is ONE trunk launch; in grad mode it is the layers."""
    Kn = K()
    calls = []
    for name in ("polyenc_forward", "polydec_forward"):
        orig = getattr(Kn, name)
        monkeypatch.setattr(Kn, name, lambda *a, _o=orig, _n=name: (calls.append(_n), _o(*a))[1])
    enc, dec = _trunk_params()
    x, h0 = dev(t(P.uniform((3, 3, 28, 28), 5))), dev(t(P.uniform((3, 4, 4, 128), 6)))
    for node, inp, params, name in ((Kn.PolyConvEncoderFn, x, enc, "polyenc_forward"), (Kn.PolyConvDecoderFn, h0, dec, "polydec_forward")):
        frozen = [dev(p) for p in params]
        live = [dev(p).requires_grad_(True) for p in params]
        del calls[:]
        a = node.apply(inp, *frozen)
        with torch.no_grad():
            b = node.run(inp, *live)
        assert calls == [name, name]
        c = node.run(inp, *live)
        assert calls == [name, name] and c.requires_grad and not a.requires_grad and not b.requires_grad
        assert torch.equal(a, b) and torch.equal(a, c.detach())


def test_encoder_node_refuses_image_gradient():
    from multivae_amd import _lib

    enc, _ = _trunk_params()
    ep = [dev(p).requires_grad_(True) for p in enc]
    x = dev(t(P.uniform((2, 3, 28, 28), 5))).requires_grad_(True)
    h3 = K().PolyConvEncoderFn.apply(x, *ep)
    with pytest.raises(_lib.MvkError):
        h3.sum().backward()
