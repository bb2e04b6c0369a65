"""Host tests of the CUB text networks (models/nn/cub.py CubTextEncoder, CubTextDecoderMLP): the float64 reference
tests/textenc_ref.py against torch's own nn.TransformerEncoder, its error constants and teeth, and the modules' CPU surface (state
dict, save / reload, shapes, the text dict through the base model's helpers).  No GPU.

MoPoE itself has no CPU compute path (tests/test_host_logic.py::test_no_cpu_compute_path): what runs on the CPU of a two-modality
batch with a text dict is every step before the first kernel — branch order, both encoders forward and backward, the reconstruction
target — and the model's forward then refuses the CPU exactly as it does for tensor batches."""
import math
import warnings
from types import SimpleNamespace

import pytest
import torch
from torch import nn

import textenc_ref as R

F64 = torch.float64


def test_text_networks_are_importable():
    from multivae_amd.models.nn.cub import CubTextDecoderMLP, CubTextEncoder, PositionalEncoding

    assert issubclass(CubTextEncoder, nn.Module) and issubclass(CubTextDecoderMLP, nn.Module) and PositionalEncoding


def _torch_encoder(case, I, n_layers, p=0.0):
    """float64 nn.TransformerEncoder (+ embedding) holding the case's parameters."""
    layer = nn.TransformerEncoderLayer(case.E, case.nh, case.F, p, batch_first=True, layer_norm_eps=R.EPS)
    enc = nn.TransformerEncoder(layer, n_layers).double()
    ps = []
    for l in enc.layers:
        ps += [l.self_attn.in_proj_weight, l.self_attn.in_proj_bias, l.self_attn.out_proj.weight, l.self_attn.out_proj.bias,
               l.linear1.weight, l.linear1.bias, l.linear2.weight, l.linear2.bias, l.norm1.weight, l.norm1.bias, l.norm2.weight,
               l.norm2.bias]
    with torch.no_grad():
        for dst, src in zip(ps, I["params"]):
            dst.copy_(src.double())
    emb = I["emb"].double().requires_grad_(True)
    return enc, ps, emb


def _torch_forward(enc, emb, case, I):
    src = emb[I["tok"]] * math.sqrt(case.E) + I["pe"].double()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return enc(src, src_key_padding_mask=I["mask"] == 0)


WHOLE_P0 = [(c, nl) for c, nl in R.whole_cases() if c.p == 0]


@pytest.mark.parametrize("case,nl", WHOLE_P0, ids=[f"{c.name}-l{nl}" for c, nl in WHOLE_P0])
def test_reference_is_torchs_encoder_in_train_mode(case, nl):
    """p = 0, train mode: forward and every gradient of textenc_ref against float64 autograd through torch's modules."""
    I = R.make_inputs(case, nl)
    enc, ps, emb = _torch_encoder(case, I, nl)
    enc.train()
    out = _torch_forward(enc, emb, case, I)
    gr = torch.autograd.grad(out, [emb] + ps, I["dout"].double())
    ro, rg = R.whole_reference(case, nl)
    assert (out.detach() - ro).abs().max() <= 1e-12
    for g, (name, r) in zip(gr, rg.items()):
        assert (g - r).abs().max() <= 1e-11 * (1 + r.abs().max()), name


@pytest.mark.parametrize("case,nl", WHOLE_P0, ids=[f"{c.name}-l{nl}" for c, nl in WHOLE_P0])
def test_reference_is_torchs_encoder_in_eval_without_grad(case, nl):
    """eval + no_grad (torch's nested-tensor fast path where it applies): equal at real positions, exactly 0 at padded ones."""
    I = R.make_inputs(case, nl)
    enc, ps, emb = _torch_encoder(case, I, nl, p=0.5)  # eval ignores p
    enc.eval()
    with torch.no_grad():
        out = _torch_forward(enc, emb, case, I)
    ro, _ = R.whole_reference(case, nl, zero_pads=True, grad=False)
    pad = I["mask"] == 0
    if bool(pad.any()) and bool((out[pad] == 0).all()):  # the fast path ran
        assert (ro[pad] == 0).all()
        assert (out - ro).abs().max() <= 1e-12
    else:  # torch took the ordinary path (it decides by shape and build): the real positions still agree
        assert (out[~pad] - ro[~pad]).abs().max() <= 1e-12


def test_zeroed_padded_rows_are_what_torch_gives():
    """At least one case of the table exercises torch's fast path, so the zero_pads semantics are pinned by torch itself."""
    hit = 0
    for case, nl in WHOLE_P0:
        I = R.make_inputs(case, nl)
        pad = I["mask"] == 0
        if not bool(pad.any()):
            continue
        enc, ps, emb = _torch_encoder(case, I, nl)
        enc.eval()
        with torch.no_grad():
            out = _torch_forward(enc, emb, case, I)
        hit += bool((out[pad] == 0).all())
    assert hit >= 1


def _worst(fn):
    worst = {}
    for c in R.CASES:
        I = R.make_inputs(c)
        base = R.stage_bases(c, I)
        ref, got = R.stage_outputs(c, I, F64), fn(c, I)
        for k in ref:
            r = R.worst_ratio(got[k], ref[k], base[k])
            if r >= worst.get(k, (-1.0, ""))[0]:
                worst[k] = (r, c.name)
    return worst


def test_error_constants():
    """C_STAGE / C_WHOLE = 4x the largest |err| / base of the same formulas in plain torch fp32 (gradients: fp32 autograd), rounded up."""
    worst = _worst(lambda c, I: R.stage_outputs(c, I, torch.float32))
    assert set(worst) == set(R.C_STAGE)
    for k, (v, name) in worst.items():
        assert 4 * v <= R.C_STAGE[k], f"{k}: torch fp32 shows {v:.3g} on {name}; C = {R.C_STAGE[k]} is less than 4x that"
        assert R.C_STAGE[k] <= 4 * v * 1.25 + 1, f"{k}: C = {R.C_STAGE[k]} is looser than 4 x {v:.3g} rounded up"
    ww = {"out": 0.0, "grad": 0.0}
    for c, nl in R.whole_cases():
        ro, rg = R.whole_reference(c, nl)
        go, gg = R.whole_reference(c, nl, torch.float32)
        ww["out"] = max(ww["out"], R.worst_ratio(go, ro, R.whole_base(ro, nl, False)))
        for k in rg:
            ww["grad"] = max(ww["grad"], R.worst_ratio(gg[k], rg[k], R.whole_base(rg[k], nl, True)))
    for k, v in ww.items():
        assert 4 * v <= R.C_WHOLE[k] <= 4 * v * 1.25 + 1, (k, v, R.C_WHOLE[k])


# the stage and the case at which each deliberate mistake of the reference matters
TEETH = {
    "no_qscale": ("dqkv", "P", "ctx"),
    "no_keymask": ("P", "ctx", "dqkv"),
    "no_dropscale": ("drop", "embed", "ctx", "y", "dt"),
    "no_sqrtE": ("embed", "dE"),
    "no_pos": ("embed",),
    "no_eps": ("rstd",),
    "no_zero_pads": ("y_zero",),
}


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_the_bounds_reject_each_mistake(mut):
    hit = {}
    for c in R.CASES:
        I = R.make_inputs(c)
        base = R.stage_bases(c, I)
        ref, bad = R.stage_outputs(c, I), R.stage_outputs(c, I, mut=(mut,))
        for s in TEETH[mut]:
            f = R.worst_ratio(bad[s], ref[s], base[s]) / R.C_STAGE[s]
            hit[s] = max(hit.get(s, 0.0), f)
    for s in TEETH[mut]:
        assert hit[s] > 2, f"{mut} passes the bound of {s} everywhere (worst {hit[s]:.3g}x)"


def test_whole_bounds_reject_each_mistake():
    """... of the whole encoder's forward.  (The LayerNorm epsilon is the stage test's: behind GEMMs a row's variance is some 1e5
    times 1e-5, and leaving it out moves the output by less than the GEMMs may.)"""
    for mut in R.MUTATIONS:
        if mut == "no_eps":
            continue
        worst = 0.0
        for c, nl in R.whole_cases():
            zp = mut == "no_zero_pads"
            ro, _ = R.whole_reference(c, nl, zero_pads=zp, grad=False)
            bo, _ = R.whole_reference(c, nl, zero_pads=zp, grad=False, mut=(mut,))
            worst = max(worst, R.worst_ratio(bo, ro, R.whole_base(ro, nl, False)) / R.C_WHOLE["out"])
        assert worst > 2, (mut, worst)


ENC_KEYS = [("token_embedding.weight", (11, 8)), ("pos_encoder.pe", (1, 5000, 8))]
for _l in range(2):
    _p = f"transformer_encoder.layers.{_l}."
    ENC_KEYS += [(_p + "self_attn.in_proj_weight", (24, 8)), (_p + "self_attn.in_proj_bias", (24,)),
                 (_p + "self_attn.out_proj.weight", (8, 8)), (_p + "self_attn.out_proj.bias", (8,)),
                 (_p + "linear1.weight", (16, 8)), (_p + "linear1.bias", (16,)), (_p + "linear2.weight", (8, 16)),
                 (_p + "linear2.bias", (8,)), (_p + "norm1.weight", (8,)), (_p + "norm1.bias", (8,)), (_p + "norm2.weight", (8,)),
                 (_p + "norm2.bias", (8,))]
ENC_KEYS += [("mu.weight", (5, 48)), ("mu.bias", (5,)), ("log_covariance.weight", (5, 48)), ("log_covariance.bias", (5,))]
DEC_KEYS = [("layers.0.0.weight", (512, 5)), ("layers.0.0.bias", (512,)), ("layers.1.0.weight", (66, 512)), ("layers.1.0.bias", (66,))]


def _small():
    from multivae_amd.models.nn.cub import CubTextDecoderMLP, CubTextEncoder

    torch.manual_seed(3)
    enc = CubTextEncoder(5, 6, 11, embed_size=8, nhead=2, ff_size=16, n_layers=2, dropout=0.5)
    dec = CubTextDecoderMLP(SimpleNamespace(latent_dim=5, input_dim=(6, 11)))
    tok = torch.randint(0, 11, (3, 6))
    pm = torch.ones(3, 6)
    pm[1, 4:] = 0
    pm[2, 1:] = 0
    return enc, dec, dict(tokens=tok, padding_mask=pm)


def test_state_dict_keys_and_shapes():
    enc, dec, _ = _small()
    assert [(k, tuple(v.shape)) for k, v in enc.state_dict().items()] == ENC_KEYS
    assert [(k, tuple(v.shape)) for k, v in dec.state_dict().items()] == DEC_KEYS
    w = enc.token_embedding.weight
    w = w.detach()
    assert float(w.min()) >= -0.1 and float(w.max()) <= 0.1 and float(w.abs().max()) > 0.05
    assert torch.equal(enc.pos_encoder.pe[0, :6], R.positions(6, 8))
    from inspect import signature

    from multivae_amd.models.nn.cub import CubTextEncoder

    d = {k: v.default for k, v in signature(CubTextEncoder.__init__).parameters.items()}
    assert (d["embed_size"], d["nhead"], d["ff_size"], d["n_layers"], d["dropout"]) == (512, 4, 1024, 4, 0.5)
    assert dec.rows_independent is True and dec.depth == 2


def test_save_and_reload(tmp_path):
    enc, dec, x = _small()
    torch.save(dict(e=enc.state_dict(), d=dec.state_dict()), tmp_path / "m.pt")
    enc2, dec2, _ = _small()
    with torch.no_grad():
        for q in list(enc2.parameters()) + list(dec2.parameters()):
            q.add_(1.0)
    sd = torch.load(tmp_path / "m.pt", weights_only=True)
    enc2.load_state_dict(sd["e"])
    dec2.load_state_dict(sd["d"])
    enc.eval(), enc2.eval()
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a, b = enc(x), enc2(x)
        assert torch.equal(a.embedding, b.embedding) and torch.equal(a.transformer_output, b.transformer_output)
        z = torch.randn(4, 5)
        assert torch.equal(dec(z).reconstruction, dec2(z).reconstruction)


def test_cpu_forward_shapes_and_padded_rows():
    enc, dec, x = _small()
    out = enc(x)  # train mode: the ordinary path
    assert set(out.keys()) == {"embedding", "log_covariance", "transformer_output"}
    assert out.embedding.shape == (3, 5) and out.log_covariance.shape == (3, 5) and out.transformer_output.shape == (3, 6, 8)
    (out.embedding.sum() + out.log_covariance.sum()).backward()
    assert enc.token_embedding.weight.grad is not None and enc.mu.weight.grad is not None
    enc.eval()
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ev = enc(x)
    pad = x["padding_mask"] == 0
    assert (ev.transformer_output[pad] == 0).all() and (ev.transformer_output[~pad] != 0).any()
    flat = ev.transformer_output.reshape(3, -1)
    assert torch.allclose(ev.embedding, flat @ enc.mu.weight.t() + enc.mu.bias, atol=1e-6)  # the heads read the zeros


def test_cpu_module_is_the_reference_in_float64():
    """The CPU path (the torch submodules) at p = 0 against textenc_ref with the module's own parameters."""
    from multivae_amd.models.nn.cub import CubTextEncoder

    torch.manual_seed(5)
    enc = CubTextEncoder(4, 5, 7, embed_size=8, nhead=2, ff_size=16, n_layers=2, dropout=0.0).double()
    tok = torch.randint(0, 7, (3, 5))
    pm = torch.ones(3, 5, dtype=torch.int32)
    pm[0, 2:] = 0
    out = enc(dict(tokens=tok, padding_mask=pm)).transformer_output
    ps = []
    for l in enc.transformer_encoder.layers:
        ps += [l.self_attn.in_proj_weight, l.self_attn.in_proj_bias, l.self_attn.out_proj.weight, l.self_attn.out_proj.bias,
               l.linear1.weight, l.linear1.bias, l.linear2.weight, l.linear2.bias, l.norm1.weight, l.norm1.bias, l.norm2.weight,
               l.norm2.bias]
    ref = R.encoder(tok, pm, enc.token_embedding.weight, enc.pos_encoder.pe[0], ps, None, 0.0, 2, 1e-5,
                    R.noise_layout(3, 5, 8, 2, 16, 2))
    assert (out - ref).abs().max() <= 1e-12


def test_decoder_on_stacked_latents():
    _, dec, _ = _small()
    z = torch.randn(2, 3, 5)
    rec = dec(z).reconstruction
    assert rec.shape == (2, 3, 6, 11)
    assert torch.allclose(rec[1], dec(z[1]).reconstruction, atol=1e-6)


def _mopoe():
    from multivae_amd.models import MoPoE, MoPoEConfig
    from multivae_amd.models.nn.default_architectures import Decoder_AE_MLP, Encoder_VAE_MLP
    from multivae_amd.models.base.base_config import BaseAEConfig

    enc, dec, x = _small()
    cfg = MoPoEConfig(n_modalities=2, latent_dim=5, input_dims=dict(img=(1, 4, 4), text=(6, 11)),
                      decoders_dist=dict(img="normal", text="categorical"))
    ae = BaseAEConfig(input_dim=(1, 4, 4), latent_dim=5)
    model = MoPoE(cfg, encoders=dict(img=Encoder_VAE_MLP(ae), text=enc), decoders=dict(img=Decoder_AE_MLP(ae), text=dec))
    return model, x


def test_recon_spec_builds_the_categorical_target():
    model, x = _mopoe()
    img = torch.rand(3, 1, 4, 4)
    logits = torch.zeros(3, 6, 11)
    spec = model._recon_spec(["img", "text"], dict(img=img, text=x), None, 1, 3, [img, logits])
    want = torch.nn.functional.one_hot(x["tokens"], 11).float()
    assert spec["x"][0] is img and torch.equal(spec["x"][1], want) and spec["x"][1].dtype == torch.float32
    assert torch.equal(model._recon_spec(["text"], dict(text=x), None, 1, 3)["x"][0], want)  # class count from input_dims
    soft = torch.rand(3, 6, 11)
    spec = model._recon_spec(["text"], dict(text=dict(x, one_hot=soft)), None, 1, 3, [logits])
    assert spec["x"][0] is soft


def test_mopoe_takes_a_text_dict_up_to_the_first_kernel():
    from multivae_amd import _lib
    from multivae_amd.data.datasets.base import DatasetOutput
    from multivae_amd.models.base.base_ae_model import first_tensor

    model, x = _mopoe()
    inputs = DatasetOutput(data=dict(img=torch.rand(3, 1, 4, 4), text=x))
    assert first_tensor(x) is x["tokens"] and first_tensor(inputs.data["img"]) is inputs.data["img"]
    assert model._branch_order(inputs) == ["text", "img"]  # 66 > 16 entries
    out = model.encoders["text"](x)
    (out.embedding.sum() + out.log_covariance.sum()).backward()
    assert model.encoders["text"].token_embedding.weight.grad.abs().sum() > 0
    rec = model.decoders["text"](torch.randn(3, 5)).reconstruction
    assert rec.shape == (3, 6, 11)
    with pytest.raises(_lib.MvkError):  # the posterior kernel: no CPU compute path, as for tensor batches
        model(inputs)


def test_trainer_loader_collates_text_dicts():
    from multivae_amd.data.datasets.base import DatasetOutput
    from multivae_amd.trainers.base.base_trainer import _BatchIterator

    class Captions(torch.utils.data.Dataset):
        def __len__(self):
            return 5

        def __getitem__(self, i):
            return DatasetOutput(data=dict(img=torch.full((2,), float(i)),
                                           text=dict(tokens=torch.full((4,), i), padding_mask=torch.ones(4))))

    batches = list(_BatchIterator(Captions(), 2, False, torch.device("cpu")))
    assert len(batches) == 3
    b = batches[1]
    assert b.data["img"].shape == (2, 2) and b.data["text"]["tokens"].shape == (2, 4)
    assert b.data["text"]["tokens"][:, 0].tolist() == [2, 3] and b.data["text"]["padding_mask"].shape == (2, 4)
