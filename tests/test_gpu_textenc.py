"""GPU tests of the CUB text networks: every stage of csrc/textenc.hip (mvk_txt_*) entry by entry against the float64 reference
tests/textenc_ref.py over its case table, the whole kernels.TextEncoderFn forward and every gradient, the CubTextEncoder module
(fused path against its own torch path, padded rows, seeded noise) and MoPoE with an image and a caption modality.

Bounds: |got - ref| <= C_STAGE * base per entry for the stages and C_WHOLE * whole_base for the whole encoder (textenc_ref's module
docstring; the constants come from plain torch fp32 on the CPU, the whole encoder's base from the tiled engine's pinned entrywise
bound).  Two fp32 evaluations that are each held to a bound against float64 are held to twice that bound against one another."""
import copy
import math
from types import SimpleNamespace

import pytest
import torch

import elbo_ref
import textenc_ref as R

pytestmark = pytest.mark.gpu


def _check(got, ref, base, consts, what):
    fails, report = [], []
    for k, g in got.items():
        r = R.worst_ratio(g.detach().cpu().reshape(ref[k].shape), ref[k], base[k])
        report.append(f"{k} {r:.3g}/{consts[k]:g}")
        if not r <= consts[k]:
            fails.append(f"{k}: {r:.3g}x base, allowed {consts[k]:g}")
    print(what, "; ".join(report))
    assert not fails, (what, fails)


@pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
def test_stages(case):
    from multivae_amd import kernels as K

    I = R.make_inputs(case)
    ref, base = R.stage_outputs(case, I), R.stage_bases(case, I)
    E, nh, S, B, F, V, p, null = case.E, case.nh, case.S, case.B, case.F, case.V, case.p, case.null
    _, pos_off, offs = I["layout"]
    d = lambda k: I[k].cuda()
    u = d("noise")
    site = lambda off, n: None if p == 0 else u[off:off + n]
    keep, affine, sums = "keep" not in null, "affine" not in null, "sums" not in null
    mask = None if "mask" in null else d("mask")
    second = "dy2" not in null
    got = {}

    tok = d("tok")
    got["embed"] = K.txt_embed_fwd(tok, d("emb"), d("pe"), site(pos_off, B * S * E), p)
    dE = K.txt_embed_bwd(tok, d("g"), V, d("g2") if second else None, site(pos_off, B * S * E), p)
    got["dE"] = dE
    unused = torch.ones(V, dtype=torch.bool)
    unused[I["tok"].reshape(-1)] = False
    assert bool(unused.any()) and bool((dE.cpu()[unused] == 0).all())  # a row that no token names is written, as zeros
    acc = torch.zeros_like(dE)
    K.txt_embed_bwd(tok, d("g"), V, d("g2") if second else None, site(pos_off, B * S * E), p, out=acc)
    assert torch.equal(acc, dE)  # the accumulating form onto zeros, and a second run: the same bits

    qkv = d("qkv")
    asite = site(offs[0][0], B * nh * S * S)
    ctx, P = K.txt_attn_fwd(qkv, nh, mask, asite, p, keep=keep)
    got["ctx"] = ctx
    if keep:
        got["P"] = P
    else:
        assert P is None
        P = ref["P"].float().cuda()
    got["dqkv"] = K.txt_attn_bwd(qkv, P, d("dctx"), nh, asite, p)
    assert torch.equal(got["dqkv"], K.txt_attn_bwd(qkv, P, d("dctx"), nh, asite, p))
    assert torch.equal(ctx, K.txt_attn_fwd(qkv, nh, mask, asite, p, keep=False)[0])

    gamma, beta = (d("gamma"), d("beta")) if affine else (None, None)
    rsite = site(offs[0][1], B * S * E)
    x, t = d("x"), d("t")
    y, z, mean, rstd = K.txt_add_ln_fwd(x, t.clone(), gamma, beta, R.EPS, rsite, p, z_in_t=True)
    got["y"], got["mean"], got["rstd"] = y, mean, rstd
    if not keep:  # nothing kept for a backward: the same y
        y2, z2, m2, r2 = K.txt_add_ln_fwd(x, t, gamma, beta, R.EPS, rsite, p, keep=False)
        assert z2 is None and m2 is None and r2 is None and torch.equal(y2, y)
    got["y_zero"] = K.txt_add_ln_fwd(x, t, gamma, beta, R.EPS, rsite, p, rowmask=d("mask"), zero_pads=True, keep=False)[0]
    pad = I["mask"] == 0
    assert bool((got["y_zero"].cpu()[pad] == 0).all())
    dg, db = (torch.zeros(E, device="cuda"), torch.zeros(E, device="cuda")) if sums else (None, None)
    dy2 = d("dy2") if second else None
    dx, dt = K.txt_add_ln_bwd(d("dy"), z, mean, rstd, gamma, dy2, rsite, p, dgamma=dg, dbeta=db)
    got["dx"], got["dt"] = dx, dt
    if sums:
        got["dgamma"], got["dbeta"] = dg, db
        dg2, db2 = torch.zeros_like(dg), torch.zeros_like(db)
        dx2, _ = K.txt_add_ln_bwd(d("dy"), z, mean, rstd, gamma, dy2, rsite, p, dgamma=dg2, dbeta=db2)
        assert torch.equal(dg2, dg) and torch.equal(db2, db) and torch.equal(dx2, dx)

    got["drop"] = K.txt_drop(d("ff").clone(), site(offs[0][2], B * S * F), p)
    _check(got, ref, base, R.C_STAGE, case.name)


def test_bad_arguments_are_refused():
    from multivae_amd import _lib
    from multivae_amd import kernels as K

    qkv = torch.zeros(1, 65, 24, device="cuda")
    with pytest.raises(_lib.MvkError):
        K.txt_attn_fwd(qkv, 2)  # S > 64
    with pytest.raises(_lib.MvkError):
        K.txt_attn_fwd(torch.zeros(1, 4, 3 * 129, device="cuda"), 1)  # head_dim > 128
    with pytest.raises(_lib.MvkError):
        K.txt_attn_fwd(torch.zeros(1, 4, 24, device="cuda"), 3)  # E % nhead
    x = torch.zeros(2, 3, 8, device="cuda")
    with pytest.raises(_lib.MvkError):
        K.txt_drop(x, torch.zeros(48, device="cuda"), 1.0)  # p = 1
    with pytest.raises(_lib.MvkError):
        K.txt_add_ln_fwd(x, x.clone(), None, None, -1.0)  # eps < 0
    assert not K.text_encoder_ok(1, 65, 8, 2, 16) and not K.text_encoder_ok(1, 4, 129, 1, 16) and K.text_encoder_ok(128, 32, 512, 4, 1024)


WHOLE = R.whole_cases()


@pytest.mark.parametrize("case,nl", WHOLE, ids=[f"{c.name}-l{nl}" for c, nl in WHOLE])
def test_text_encoder_fn(case, nl):
    """Forward and every gradient of the one-node encoder; with dropout the noise is the reference's."""
    from multivae_amd import kernels as K

    I = R.make_inputs(case, nl)
    ro, rg = R.whole_reference(case, nl)
    emb = I["emb"].cuda().requires_grad_(True)
    params = [t.cuda().requires_grad_(True) for t in I["params"]]
    noise = I["noise"].cuda() if case.p else None
    out = K.TextEncoderFn.apply(I["tok"].cuda(), I["mask"].cuda(), case.p, noise, False, case.nh, R.EPS, emb, I["pe"].cuda(), *params)
    gr = torch.autograd.grad(out, [emb] + params, I["dout"].cuda())
    names = list(rg)
    got = dict(zip(names, gr))
    got["out"] = out
    ref = dict(rg, out=ro)
    base = {k: R.whole_base(v, nl, k != "out") for k, v in ref.items()}
    consts = {k: R.C_WHOLE["out" if k == "out" else "grad"] for k in ref}
    _check(got, ref, base, consts, f"{case.name}-l{nl}")
    # evaluation without autograd: padded rows are exactly 0 and the real ones the same bound
    with torch.no_grad():
        ev = K.TextEncoderFn.apply(I["tok"].cuda(), I["mask"].cuda(), 0.0, None, True, case.nh, R.EPS, emb, I["pe"].cuda(), *params)
    if case.p == 0:
        rz, _ = R.whole_reference(case, nl, zero_pads=True, grad=False)
        assert bool((ev.cpu()[I["mask"] == 0] == 0).all())
        _check(dict(out=ev), dict(out=rz), dict(out=R.whole_base(ro, nl, False)), dict(out=R.C_WHOLE["out"]), "zero pads")


def _module(S=32, V=50, E=64, nh=4, F=128, nl=2, p=0.0, L=6, B=5, seed=0):
    from multivae_amd.models.nn.cub import CubTextEncoder

    torch.manual_seed(seed)
    enc = CubTextEncoder(L, S, V, embed_size=E, nhead=nh, ff_size=F, n_layers=nl, dropout=p).cuda()
    g = torch.Generator().manual_seed(seed + 1)
    tok = torch.randint(0, V, (B, S), generator=g)
    pm = torch.ones(B, S)
    for b in range(1, B):
        pm[b, max(1, S - 3 * b):] = 0
    return enc, dict(tokens=tok.cuda(), padding_mask=pm.cuda())


def _f64_module_out(enc, x, zero_pads):
    ref = copy.deepcopy(enc).double().cpu()
    ref.train(not zero_pads)
    xin = dict(tokens=x["tokens"].cpu(), padding_mask=x["padding_mask"].cpu())
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if zero_pads:
            with torch.no_grad():
                return ref(xin)
        return ref(xin)


def _head_tol(enc, h64, base_h):
    """Entrywise bound of a head over the flattened sequence: the engine's own C_ENTRY sum|a b| plus what the input's bound becomes."""
    w = enc.mu.weight.detach().double().cpu().abs()
    flat, eb = h64.reshape(h64.shape[0], -1).abs(), (R.C_WHOLE["out"] * base_h).reshape(h64.shape[0], -1)
    return R.C_ENTRY * (flat @ w.t() + enc.mu.bias.detach().double().cpu().abs()) + eb @ w.t()


def test_module_fused_path_is_its_torch_path_in_train_mode():
    enc, x = _module()
    enc.train()
    assert enc._fused_plan(x["tokens"]) is not None
    a = enc(x)
    enc.use_fused = False
    b = enc(x)
    ref = _f64_module_out(enc, x, False)
    h64 = ref.transformer_output.detach()
    base = R.whole_base(h64, 2, False)
    ra = R.worst_ratio(a.transformer_output.detach().cpu(), h64, base)
    rb = R.worst_ratio(b.transformer_output.detach().cpu(), a.transformer_output.detach().cpu().double(), base)
    print("fused vs float64", ra, "fused vs torch path", rb)
    assert ra <= R.C_WHOLE["out"] and rb <= 2 * R.C_WHOLE["out"]
    tol = _head_tol(enc, h64, base)
    assert bool(((a.embedding.detach().cpu().double() - ref.embedding.detach()).abs() <= tol).all())
    assert bool(((a.embedding - b.embedding).detach().cpu().double().abs() <= 2 * tol).all())


def test_module_eval_without_grad_zeroes_padded_rows():
    enc, x = _module(p=0.5)
    enc.eval()
    with torch.no_grad():
        a = enc(x)
        enc.use_fused = False
        b = enc(x)
    pad = (x["padding_mask"] == 0).cpu()
    assert bool(pad.any()) and bool((a.transformer_output.cpu()[pad] == 0).all())
    assert bool((b.transformer_output.cpu()[pad] == 0).all())  # torch's fast path on this build: the same convention
    ref = _f64_module_out(enc, x, True)
    base = R.whole_base(ref.transformer_output, 2, False)
    assert R.worst_ratio(a.transformer_output.cpu(), ref.transformer_output, base) <= R.C_WHOLE["out"]
    assert R.worst_ratio(b.transformer_output.cpu(), a.transformer_output.cpu().double(), base) <= 2 * R.C_WHOLE["out"]
    tol = _head_tol(enc, ref.transformer_output, base)
    assert bool(((a.embedding.cpu().double() - ref.embedding).abs() <= tol).all())  # the heads read the zeros


def test_module_eval_ignores_p_and_grad_mode_keeps_padded_rows():
    enc, x = _module(p=0.5)
    enc0, _ = _module(p=0.0)
    enc0.load_state_dict(enc.state_dict())
    enc.eval(), enc0.eval()
    a, b = enc(x), enc0(x)  # autograd on: the ordinary path, padded rows computed
    assert torch.equal(a.transformer_output, b.transformer_output) and torch.equal(a.embedding, b.embedding)
    pad = x["padding_mask"] == 0
    assert bool((a.transformer_output[pad] != 0).any())


def test_module_seeded_noise():
    enc, x = _module(p=0.5)
    enc.train()
    drawn = []
    draw = enc._draw_noise
    enc._draw_noise = lambda n, dev: drawn.append(draw(n, dev)) or drawn[-1]
    torch.manual_seed(11)
    a = enc(x).transformer_output
    torch.manual_seed(11)
    b = enc(x).transformer_output
    torch.manual_seed(12)
    c = enc(x).transformer_output
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert torch.equal(drawn[0], drawn[1]) and len(drawn) == 3
    B, S = x["tokens"].shape
    n = B * S * 64  # the positional site
    total, _, _ = R.noise_layout(B, S, 64, 4, 128, 2)
    assert drawn[0].numel() == total and float(drawn[0].min()) >= 0.0 and float(drawn[0].max()) < 1.0
    share = float((drawn[0][:n] >= 0.5).float().mean())
    assert abs(share - 0.5) <= 5 * math.sqrt(0.25 / n), share
    from multivae_amd import kernels as K

    kept = K.txt_drop(torch.ones(n, device="cuda"), drawn[0][:n], 0.5)
    assert abs(float((kept != 0).float().mean()) - 0.5) <= 5 * math.sqrt(0.25 / n) and float(kept.max()) == 2.0


def test_long_sentences_take_the_torch_path():
    enc, x = _module(S=70, nl=1, B=2)
    enc.eval()
    assert enc._fused_plan(x["tokens"]) is None
    a = enc(x)
    enc.use_fused = False
    b = enc(x)
    assert torch.equal(a.transformer_output, b.transformer_output) and torch.equal(a.embedding, b.embedding)
    assert a.transformer_output.shape == (2, 70, 64)


def test_large_training_batches_take_the_torch_path_unless_forced(monkeypatch):
    """Measured slower there (FUSED_TRAIN_MAX_ROWS): opt-in with use_fused = "always"; evaluation without autograd stays fused."""
    from multivae_amd.models.nn.cub import CubTextEncoder

    enc, x = _module(p=0.0)
    assert enc._fused_plan(x["tokens"]) is not None
    monkeypatch.setattr(CubTextEncoder, "FUSED_TRAIN_MAX_ROWS", 5 * 32 - 1)
    assert enc._fused_plan(x["tokens"]) is None
    with torch.no_grad():
        assert enc._fused_plan(x["tokens"]) is not None
    a = enc(x)
    enc.use_fused = "always"
    assert enc._fused_plan(x["tokens"]) is not None
    b = enc(x)
    base = R.whole_base(a.transformer_output.detach().cpu(), 2, False)
    assert R.worst_ratio(b.transformer_output.detach().cpu(), a.transformer_output.detach().cpu().double(), base) <= 2 * R.C_WHOLE["out"]
    assert not torch.equal(a.transformer_output, b.transformer_output)  # two different paths ran


# ---- MoPoE with the default image networks and the text networks ------------------------------------------------------------------
S_, V_, B_ = 8, 12, 16


def _mopoe(p=0.0):
    from multivae_amd.models import MoPoE, MoPoEConfig
    from multivae_amd.models.base.base_config import BaseAEConfig
    from multivae_amd.models.nn.cub import CubTextDecoderMLP, CubTextEncoder
    from multivae_amd.models.nn.default_architectures import Decoder_AE_MLP, Encoder_VAE_MLP

    torch.manual_seed(4)
    cfg = MoPoEConfig(n_modalities=2, latent_dim=6, input_dims=dict(img=(1, 5, 5), text=(S_, V_)),
                      decoders_dist=dict(img="normal", text="categorical"))
    enc = CubTextEncoder(6, S_, V_, embed_size=16, nhead=2, ff_size=32, n_layers=2, dropout=p)
    dec = CubTextDecoderMLP(SimpleNamespace(latent_dim=6, input_dim=(S_, V_)))
    ae = BaseAEConfig(input_dim=(1, 5, 5), latent_dim=6)  # the default (MLP) image networks
    model = MoPoE(cfg, encoders=dict(img=Encoder_VAE_MLP(ae), text=enc), decoders=dict(img=Decoder_AE_MLP(ae), text=dec))
    return model.cuda().train()


def _batch(n=B_, seed=0):
    g = torch.Generator().manual_seed(seed)
    tok = torch.randint(0, V_, (n, S_), generator=g)
    pm = torch.ones(n, S_)
    for b in range(n):
        pm[b, 2 + b % (S_ - 1):] = 0
    return torch.rand(n, 1, 5, 5, generator=g), tok, pm


def _mlp64(seqs, x):
    for seq in seqs:
        x = seq(x)
    return x


def test_mopoe_step_against_float64():
    """One training step (text dropout 0): loss and a sample of gradients against the same step in float64 on the CPU, with the same
    latent noise.  The float64 step: the torch submodules of the networks, tests/elbo_ref.py's MoPoE posterior, Normal(1) and
    categorical log-likelihoods, loss = (sum_m NLL_m + beta sum_b KL_b) / B."""
    from multivae_amd.data.datasets.base import DatasetOutput

    model = _mopoe()
    img, tok, pm = _batch()
    eps = torch.randn(1, B_, 6, generator=torch.Generator().manual_seed(9))
    inputs = DatasetOutput(data=dict(img=img.cuda(), text=dict(tokens=tok.cuda(), padding_mask=pm.cuda())))
    out = model(inputs, noise=eps.cuda())
    out.loss.backward()

    ref = copy.deepcopy(model).double().cpu()
    for q in ref.parameters():
        q.grad = None
    ei, di = ref.encoders["img"], ref.decoders["img"]
    h = _mlp64(ei.layers, img.double().reshape(B_, -1))
    t = ref.encoders["text"](dict(tokens=tok, padding_mask=pm))
    enc = dict(img=(ei.embedding(h), ei.log_var(h)), text=(t.embedding, t.log_covariance))
    order = model._poe_order
    post = elbo_ref.mopoe_fwd(dict(mus=[enc[m][0] for m in order], lvs=[enc[m][1] for m in order]),
                              dict(bits=model._subset_bits, weights=None, sel=model._row_range_selection(B_, torch.device("cpu")),
                                   eps=eps[0].double()))
    z = post["z"]
    rec_img = _mlp64(di.layers, z).reshape(B_, 1, 5, 5)
    nll_img = (0.5 * (img.double() - rec_img) ** 2 + 0.5 * math.log(2 * math.pi)).sum()
    logits = _mlp64(ref.decoders["text"].layers, z).reshape(B_, S_, V_)
    nll_txt = -(torch.nn.functional.one_hot(tok, V_).double() * torch.log_softmax(logits, -1)).sum()
    loss = (nll_img + nll_txt + float(model.model_config.beta) * post["kld"].sum()) / B_
    loss.backward()

    sites = 1 + 8 * 2 + 6
    err = abs(float(out.loss.detach()) - float(loss.detach()))
    print("loss", float(out.loss.detach()), float(loss.detach()), err / abs(float(loss.detach())))
    assert err <= R.C_WHOLE["out"] * R.C_ENTRY * sites * abs(float(loss.detach()))
    got, want = dict(model.named_parameters()), dict(ref.named_parameters())
    sample = ["encoders.text.token_embedding.weight", "encoders.text.transformer_encoder.layers.0.self_attn.in_proj_weight",
              "encoders.text.transformer_encoder.layers.1.norm2.weight", "encoders.text.transformer_encoder.layers.1.linear1.bias",
              "encoders.text.mu.weight", "decoders.text.layers.1.0.weight", "encoders.img.layers.0.0.weight"]
    for k in sample:
        r = R.worst_ratio(got[k].grad.cpu(), want[k].grad, R.whole_base(want[k].grad, 3, True))
        print(k, r)
        assert r <= R.C_WHOLE["grad"], (k, r)


def test_mopoe_encode_and_predict_take_the_text_dict():
    from multivae_amd.data.datasets.base import DatasetOutput

    model = _mopoe(p=0.5)
    img, tok, pm = _batch()
    inputs = DatasetOutput(data=dict(img=img.cuda(), text=dict(tokens=tok.cuda(), padding_mask=pm.cuda())))
    z = model.encode(inputs, cond_mod="text").z
    assert z.shape == (B_, 6) and bool(torch.isfinite(z).all())
    rec = model.predict(inputs, cond_mod="text", gen_mod="all")
    assert rec["img"].shape == (B_, 1, 5, 5) and rec["text"].shape == (B_, S_, V_) and bool(torch.isfinite(rec["text"]).all())


def test_trainer_runs_three_epochs(tmp_path):
    from multivae_amd.data.datasets.base import DatasetOutput
    from multivae_amd.trainers import BaseTrainer, BaseTrainerConfig

    img, tok, pm = _batch(16, seed=2)

    class Captions(torch.utils.data.Dataset):
        def __len__(self):
            return 16

        def __getitem__(self, i):
            return DatasetOutput(data=dict(img=img[i], text=dict(tokens=tok[i], padding_mask=pm[i])))

    model = _mopoe(p=0.5)
    cfg = BaseTrainerConfig(output_dir=str(tmp_path), per_device_train_batch_size=8, num_epochs=3, learning_rate=1e-3, steps_saving=None,
                            use_hip_graph=True)  # a batch with a text dict is not captured: it runs eagerly
    trainer = BaseTrainer(model, train_dataset=Captions(), training_config=cfg)
    hist = trainer.train()
    with torch.no_grad():
        model.eval()
        out = model(DatasetOutput(data=dict(img=img.cuda(), text=dict(tokens=tok.cuda(), padding_mask=pm.cuda()))))
    assert math.isfinite(float(out.loss))
    assert len(hist) == 3 and all(math.isfinite(h["train_epoch_loss"]) for h in hist), hist
