"""CUB / 64x64-image ResNet encoder and decoder (`multivae/models/nn/cub.py:144-293`, adapted there from
github.com/epalu/mmvaeplus) on the HIP kernels.  Same building blocks as models/nn/mmnist.py; the ResnetBlock here
is the pre-activation variant  x_s + 0.1 * conv_1(lrelu(conv_0(lrelu(x))))  (`cub.py:274-280`).  Module structure and
parameter names follow the reference.

The text networks (`cub.py:16-137`): CubTextEncoder, a token embedding with sinusoidal positions, post-norm transformer encoder
layers under a key padding mask and two linear heads over the flattened sequence; CubTextDecoderMLP, latent -> 512 -> logits.  Both
hold plain torch submodules (the state dict is the reference's by construction) and are written from the architecture's definition
and torch's documented formulas.  On the GPU in fp32, for sentences of at most 64 tokens, the encoder is one autograd node on
csrc/textenc.hip and the tiled GEMM engine (kernels.TextEncoderFn); everything else runs the torch submodules."""
import math

import numpy as np
import torch
from torch import nn

from ... import kernels
from ..base.base_utils import ModelOutput
from .base_architectures import BaseDecoder, BaseEncoder
from .mmnist import _add_block, _add_conv, _add_sequential


class ResnetBlock(nn.Module):
    order = "pre"

    def __init__(self, fin, fout, fhidden=None, is_bias=True):
        super().__init__()
        self.is_bias = is_bias
        self.learned_shortcut = fin != fout
        self.fin, self.fout = fin, fout
        self.fhidden = min(fin, fout) if fhidden is None else fhidden
        self.conv_0 = nn.Conv2d(self.fin, self.fhidden, 3, stride=1, padding=1)
        self.conv_1 = nn.Conv2d(self.fhidden, self.fout, 3, stride=1, padding=1, bias=is_bias)
        if self.learned_shortcut:
            self.conv_s = nn.Conv2d(self.fin, self.fout, 1, stride=1, padding=0, bias=False)

    def forward(self, x):  # NCHW in / out
        prog, params = [], []
        _add_block(prog, params, self)
        return kernels.ResnetStackFn.apply(x.permute(0, 2, 3, 1), prog, *params).permute(0, 3, 1, 2)


class CUB_Resnet_Encoder(BaseEncoder):
    """`cub.py:144-196`: conv_img -> ResnetBlock -> [AvgPool, ResnetBlock] x log2(64/s0) -> flatten -> fc(lrelu(.))."""

    def __init__(self, latent_dim, s0=16, nfilter=64, nfilter_max=1024):
        super().__init__()
        self.latent_dim = latent_dim
        size = 64
        self.s0 = s0
        nf = self.nf = nfilter
        nf_max = self.nf_max = nfilter_max
        nlayers = int(np.log2(size / s0))
        self.nf0 = min(nf_max, nf * 2 ** nlayers)
        blocks = [ResnetBlock(nf, nf)]
        for i in range(nlayers):
            nf0 = min(nf * 2 ** i, nf_max)
            nf1 = min(nf * 2 ** (i + 1), nf_max)
            blocks += [nn.AvgPool2d(3, stride=2, padding=1), ResnetBlock(nf0, nf1)]
        self.conv_img = nn.Conv2d(3, 1 * nf, 3, padding=1)
        self.resnet = nn.Sequential(*blocks)
        self.fc_mu = nn.Linear(self.nf0 * s0 * s0, self.latent_dim)
        self.fc_logvar = nn.Linear(self.nf0 * s0 * s0, self.latent_dim)

    def forward(self, x):
        prog, params = [], []
        _add_conv(prog, params, self.conv_img, kernels.NONE)
        _add_sequential(prog, params, self.resnet)
        h = kernels.ResnetStackFn.apply(x.permute(0, 2, 3, 1).contiguous(), prog, *params)
        # fc_mu(actvn(out)), fc_logvar(actvn(out)): the activation and the NCHW flatten in one pass
        flat = kernels.nhwc_to_flat_nchw(h, kernels.LEAKY)
        mu, lv = kernels.MLPHeadsFn.apply(flat, 2, self.fc_mu.weight, self.fc_mu.bias, self.fc_logvar.weight,
                                          self.fc_logvar.bias)
        return ModelOutput(embedding=mu, log_covariance=lv)


class CUB_Resnet_Decoder(BaseDecoder):
    """`cub.py:199-247`: fc -> [ResnetBlock, Upsample] x log2(64/s0) -> ResnetBlock -> conv_img(lrelu(.)) (logits)."""
    rows_independent = True


    def __init__(self, latent_dim, s0=16, nfilter=64, nfilter_max=512, **kwargs):
        super().__init__()
        size = 64
        self.latent_dim = latent_dim
        self.s0 = s0
        nf = self.nf = nfilter
        nf_max = self.nf_max = nfilter_max
        nlayers = int(np.log2(size / s0))
        self.nf0 = min(nf_max, nf * 2 ** nlayers)
        self.fc = nn.Linear(self.latent_dim, self.nf0 * s0 * s0)
        blocks = []
        for i in range(nlayers):
            nf0 = min(nf * 2 ** (nlayers - i), nf_max)
            nf1 = min(nf * 2 ** (nlayers - i - 1), nf_max)
            blocks += [ResnetBlock(nf0, nf1), nn.Upsample(scale_factor=2)]
        blocks += [ResnetBlock(nf, nf)]
        self.resnet = nn.Sequential(*blocks)
        self.conv_img = nn.Conv2d(nf, 3, 3, padding=1)
        self.sigmoid = nn.Sigmoid()

    def forward(self, z):
        # the reference's `view(z.size(0), ...)` only supports 2-D latents; leading dims are flattened here so that the
        # K-sample models can decode [K, B, L] as with every other in-package decoder
        z2 = z.reshape(-1, z.shape[-1])
        (h,) = kernels.MLPHeadsFn.apply(z2, 1, self.fc.weight, self.fc.bias)
        h = kernels.flat_nchw_to_nhwc(h, self.nf0, self.s0, self.s0)
        prog, params = [], []
        _add_sequential(prog, params, self.resnet)
        prog.append(("act", kernels.LEAKY))
        _add_conv(prog, params, self.conv_img, kernels.NONE)
        out = kernels.ResnetStackFn.apply(h, prog, *params).permute(0, 3, 1, 2)
        return ModelOutput(reconstruction=out.reshape(*z.shape[:-1], *out.shape[1:]))


class PositionalEncoding(nn.Module):
    """x + pe[:, :S] and dropout; pe[0, t, 2i] = sin(t w_i), pe[0, t, 2i + 1] = cos(t w_i), w_i = 10000^(-2i / d_model)."""

    def __init__(self, d_model: int, dropout: float = 0.1, max_len: int = 5000):
        super().__init__()
        self.dropout = nn.Dropout(p=dropout)
        position = torch.arange(max_len, dtype=torch.float32).unsqueeze(1)
        rate = torch.exp(torch.arange(0, d_model, 2, dtype=torch.float32) * (-math.log(10000.0) / d_model))
        pe = torch.zeros(1, max_len, d_model)
        pe[0, :, 0::2] = torch.sin(position * rate)
        pe[0, :, 1::2] = torch.cos(position * rate)[:, : d_model // 2]
        self.register_buffer("pe", pe)

    def forward(self, x):
        return self.dropout(x + self.pe[:, : x.size(1)])


class CubTextEncoder(BaseEncoder):
    """inputs = {"tokens": int64 [B,S], "padding_mask": [B,S] (1 = real token)} -> embedding, log_covariance [B,latent_dim] and
    transformer_output [B,S,E].  In eval mode without autograd transformer_output is zero at padded positions (what torch's
    nested-tensor fast path gives; the heads read those zeros); otherwise padded rows are computed like any other."""

    def __init__(self, latent_dim, max_sentence_length: int, ntokens: int, embed_size: int = 512, nhead: int = 4,
                 ff_size: int = 1024, n_layers: int = 4, dropout: float = 0.5):
        super().__init__()
        self.latent_dim = latent_dim
        self.embed_size = embed_size
        self.token_embedding = nn.Embedding(ntokens, embed_size)
        self.pos_encoder = PositionalEncoding(embed_size, dropout)
        encoder_layer = nn.TransformerEncoderLayer(embed_size, nhead, ff_size, dropout, batch_first=True)
        self.transformer_encoder = nn.TransformerEncoder(encoder_layer, n_layers)
        self.mu = nn.Linear(embed_size * max_sentence_length, self.latent_dim)
        self.log_covariance = nn.Linear(embed_size * max_sentence_length, self.latent_dim)
        self.init_weights()
        # True: the fused path where it is the faster one; "always": wherever it covers the call (opt-in); False: never (A/B)
        self.use_fused = True

    # MEASURED (profiles/NOTES_textenc.md; S = 32, E = 512, 4 heads, F = 1024, 4 layers, p = 0.5, forward + backward): the fused path
    # against the torch path 2.73 / 3.41 ms at 1024 rows (B S) and 3.28 / 4.34 ms at 2048, but 4.29 / 3.78 ms at 3072, 4.59 / 4.18 at
    # 3584 and 4.54 / 4.15 at 4096: its sixty GEMMs are the split-bf16 tiled engine's.  The evaluation forward is ahead at every size
    # (0.67 / 1.62 ms at 2048 rows, 0.86 / 1.58 at 4096).  So with autograd on, larger batches take the torch path unless use_fused
    # is "always".
    FUSED_TRAIN_MAX_ROWS = 2048

    def init_weights(self):
        nn.init.uniform_(self.token_embedding.weight, -0.1, 0.1)

    def _fused_plan(self, tokens):
        """(nhead, eps, p, flat layer parameters) when the fused path covers this call, else None."""
        w = self.token_embedding.weight
        if not (self.use_fused and tokens.is_cuda and w.is_cuda and w.dtype == torch.float32 and tokens.dim() == 2):
            return None
        if self.token_embedding.padding_idx is not None or self.token_embedding.max_norm is not None:
            return None
        layers = self.transformer_encoder.layers
        if len(layers) == 0 or self.transformer_encoder.norm is not None:
            return None
        first = layers[0]
        nhead, eps, p = first.self_attn.num_heads, first.norm1.eps, float(self.pos_encoder.dropout.p)
        params = []
        for l in layers:
            at = l.self_attn
            act = getattr(l, "activation", None)
            relu = act is torch.nn.functional.relu or isinstance(act, nn.ReLU)
            if not (type(l) is nn.TransformerEncoderLayer and relu and not l.norm_first and at._qkv_same_embed_dim
                    and at.batch_first and at.num_heads == nhead and at.in_proj_bias is not None and at.bias_k is None
                    and not at.add_zero_attn and at.out_proj.bias is not None and l.linear1.bias is not None
                    and l.linear2.bias is not None and l.norm1.elementwise_affine and l.norm1.bias is not None
                    and l.norm2.elementwise_affine and l.norm2.bias is not None and l.norm1.eps == eps and l.norm2.eps == eps
                    and float(at.dropout) == p and l.dropout.p == p and l.dropout1.p == p and l.dropout2.p == p):
                return None
            params += [at.in_proj_weight, at.in_proj_bias, at.out_proj.weight, at.out_proj.bias, l.linear1.weight, l.linear1.bias,
                       l.linear2.weight, l.linear2.bias, l.norm1.weight, l.norm1.bias, l.norm2.weight, l.norm2.bias]
        B, S = tokens.shape
        if torch.is_grad_enabled() and B * S > self.FUSED_TRAIN_MAX_ROWS and self.use_fused != "always":
            return None
        E, F = self.embed_size, layers[0].linear1.out_features
        if not (0.0 <= p < 1.0 and kernels.text_encoder_ok(B, S, E, nhead, F) and all(q.dtype == torch.float32 for q in params)):
            return None
        return nhead, eps, p, params

    def _draw_noise(self, n, device):
        """All of one forward's dropout noise, U[0, 1), in one launch."""
        return kernels.device_randn((n,), device, uniform=True)

    def forward(self, inputs):
        tokens, padding_mask = inputs["tokens"], inputs["padding_mask"]
        plan = self._fused_plan(tokens)
        if plan is not None:
            nhead, eps, p, params = plan
            B, S = tokens.shape
            noise = None
            if self.training and p > 0:
                n, _, _ = kernels.text_noise_layout(B, S, self.embed_size, nhead, params[4].shape[0], len(params) // 12)
                noise = self._draw_noise(n, tokens.device)
            zero_pads = not self.training and not torch.is_grad_enabled()
            out = kernels.TextEncoderFn.apply(tokens, padding_mask, p if noise is not None else 0.0, noise, zero_pads, nhead, eps,
                                              self.token_embedding.weight, self.pos_encoder.pe[0], *params)
            mu, lv = kernels.MLPHeadsFn.apply(out.reshape(B, -1), 2, self.mu.weight, self.mu.bias, self.log_covariance.weight,
                                              self.log_covariance.bias)
        else:
            src = self.pos_encoder(self.token_embedding(tokens) * math.sqrt(self.embed_size))
            out = self.transformer_encoder(src, src_key_padding_mask=~padding_mask.bool())
            flat = out.reshape(src.shape[0], -1)
            mu, lv = self.mu(flat), self.log_covariance(flat)
        return ModelOutput(embedding=mu, log_covariance=lv, transformer_output=out)


class CubTextDecoderMLP(BaseDecoder):
    """latent -> 512 (ReLU) -> prod(input_dim) logits, reshaped to [..., *input_dim].  args: anything with `latent_dim` and
    `input_dim` (attributes)."""
    rows_independent = True

    def __init__(self, args):
        super().__init__()
        self.input_dim = tuple(args.input_dim)
        self.layers = nn.ModuleList([nn.Sequential(nn.Linear(args.latent_dim, 512), nn.ReLU()),
                                     nn.Sequential(nn.Linear(512, int(np.prod(args.input_dim))))])
        self.depth = len(self.layers)

    def forward(self, z):
        l0, l1 = self.layers[0][0], self.layers[1][0]
        if z.is_cuda and z.dtype == torch.float32 and l0.weight.dtype == torch.float32:
            # leading latent dimensions are flattened, as in every other in-package decoder
            (out,) = kernels.MLPHeadsFn.apply(z.reshape(-1, z.shape[-1]), 1, l0.weight, l0.bias, l1.weight, l1.bias)
        else:
            out = z
            for layer in self.layers:
                out = layer(out)
        return ModelOutput(reconstruction=out.reshape(*z.shape[:-1], *self.input_dim))
