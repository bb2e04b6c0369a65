"""PolyMNIST architectures (`multivae/models/nn/mmnist.py`) on the HIP kernels.

The convolutional networks (`:36-206`): three 3x3 / stride-2 layers on 28 -> 14 -> 7 -> 4 and their transposes, one autograd
node per trunk (kernels.PolyConvEncoderFn / PolyConvDecoderFn on csrc/polyconv.hip; without a gradient the trunk is one
launch), the linear layers and heads on kernels.MLPHeadsFn.

The ResNet architectures of MMVAE+ (`:214-366`, adapted there from github.com/epalu/mmvaeplus): 3x3 convolutions on the
implicit-GEMM engine, AvgPool / Upsample / residual kernels, the whole convolutional stack of a network as ONE autograd node
(kernels.ResnetStackFn).

Module structure and parameter names follow the reference, so its state_dicts load unchanged."""
import numpy as np
import torch
from torch import nn

from ... import kernels
from ..base.base_utils import ModelOutput
from .base_architectures import BaseDecoder, BaseEncoder


class Flatten(torch.nn.Module):
    """`mmnist.py:13-17`."""

    def forward(self, x):
        return x.view(x.size(0), -1)


class Unflatten(torch.nn.Module):
    """`mmnist.py:20-28`."""

    def __init__(self, ndims):
        super(Unflatten, self).__init__()
        self.ndims = ndims

    def forward(self, x):
        return x.view(x.size(0), *self.ndims)


def _conv_trunk():
    """The three Conv2d(3, 2, 1) + ReLU layers every convolutional encoder starts with (parameter containers)."""
    return [nn.Conv2d(3, 32, kernel_size=3, stride=2, padding=1, bias=True), nn.ReLU(),
            nn.Conv2d(32, 64, kernel_size=3, stride=2, padding=1, bias=True), nn.ReLU(),
            nn.Conv2d(64, 128, kernel_size=3, stride=2, padding=1, bias=True), nn.ReLU()]


def _trunk_flat(x, seq):
    """x [n, 3, 28, 28] -> the trunk's output flattened in the reference's NCHW order [n, 2048]."""
    h3 = kernels.PolyConvEncoderFn.run(x, seq[0].weight, seq[0].bias, seq[2].weight, seq[2].bias, seq[4].weight, seq[4].bias)
    return kernels.nhwc_to_flat_nchw(h3)


def _conv_heads(flat, c_mu, c_lv):
    """The two Conv2d(128, L, 4, 2, 0) heads on the 4x4 map: one linear layer each over the flattened map -> [n, L, 1, 1]."""
    L = c_mu.weight.shape[0]
    mu, lv = kernels.PolyConvHeadsFn.apply(flat, c_mu.weight, c_mu.bias, c_lv.weight, c_lv.bias)
    return mu.reshape(-1, L, 1, 1), lv.reshape(-1, L, 1, 1)


class EncoderConvMMNIST(BaseEncoder):
    """`mmnist.py:36-75`: trunk -> nn.Flatten -> Linear(2048, L) + ReLU -> bias-free class_mu / class_logvar."""

    def __init__(self, model_config, bias=False):
        super(EncoderConvMMNIST, self).__init__()
        self.latent_dim = model_config.latent_dim
        self.shared_encoder = nn.Sequential(*_conv_trunk(), nn.Flatten(), nn.Linear(2048, self.latent_dim), nn.ReLU())
        self.class_mu = nn.Linear(self.latent_dim, self.latent_dim, bias=bias)
        self.class_logvar = nn.Linear(self.latent_dim, self.latent_dim, bias=bias)

    def forward(self, x):
        e = self.shared_encoder
        mu, lv = kernels.MLPHeadsFn.apply(_trunk_flat(x, e), 2, e[7].weight, e[7].bias, self.class_mu.weight, self.class_mu.bias,
                                          self.class_logvar.weight, self.class_logvar.bias)
        return ModelOutput(embedding=mu, log_covariance=lv)


class EncoderConvMMNIST_adapted(BaseEncoder):
    """`mmnist.py:78-109`: trunk -> two Conv2d(128, L, 4, 2, 0) heads; the reference squeezes ALL unit dims of [n, L, 1, 1]."""

    def __init__(self, model_config):
        super(EncoderConvMMNIST_adapted, self).__init__()
        self.latent_dim = model_config.latent_dim
        self.style_dim = 0
        self.shared_encoder = nn.Sequential(*_conv_trunk())
        self.class_mu = nn.Conv2d(128, self.latent_dim, 4, 2, 0)
        self.class_logvar = nn.Conv2d(128, self.latent_dim, 4, 2, 0)

    def forward(self, x):
        mu, lv = _conv_heads(_trunk_flat(x, self.shared_encoder), self.class_mu, self.class_logvar)
        return ModelOutput(embedding=mu.squeeze(), log_covariance=lv.squeeze())


class EncoderConvMMNIST_multilatents(BaseEncoder):
    """`mmnist.py:112-170`: a content trunk with heads and, with style_dim > 0, a style trunk with heads."""

    def __init__(self, model_config):
        super(EncoderConvMMNIST_multilatents, self).__init__()
        self.latent_dim = model_config.latent_dim
        self.style_dim = model_config.style_dim
        self.encoder_class = nn.Sequential(*_conv_trunk())
        self.class_mu = nn.Conv2d(128, self.latent_dim, 4, 2, 0)
        self.class_logvar = nn.Conv2d(128, self.latent_dim, 4, 2, 0)
        if self.style_dim > 0:
            self.encoder_style = nn.Sequential(*_conv_trunk())
            self.style_mu = nn.Conv2d(128, self.style_dim, 4, 2, 0)
            self.style_logvar = nn.Conv2d(128, self.style_dim, 4, 2, 0)

    def forward(self, x):
        output = ModelOutput()
        mu, lv = _conv_heads(_trunk_flat(x, self.encoder_class), self.class_mu, self.class_logvar)
        output["embedding"] = mu.squeeze(-1, -2)
        output["log_covariance"] = lv.squeeze(-1, -2)
        if self.style_dim > 0:
            smu, slv = _conv_heads(_trunk_flat(x, self.encoder_style), self.style_mu, self.style_logvar)
            output["style_embedding"] = smu.squeeze(-1, -2)
            output["style_log_covariance"] = slv.squeeze(-1, -2)
        return output


class DecoderConvMMNIST(BaseDecoder):
    """`mmnist.py:173-206`: Linear(L, 2048) + ReLU -> Unflatten (128, 4, 4) -> ConvT(128, 64) + ReLU -> ConvT(64, 32, op 1) + ReLU ->
    ConvT(32, 3, op 1), no output activation."""
    rows_independent = True

    def __init__(self, model_config):
        super(DecoderConvMMNIST, self).__init__()
        self.latent_dim = model_config.latent_dim
        self.decoder = nn.Sequential(
            nn.Linear(self.latent_dim, 2048), nn.ReLU(), Unflatten((128, 4, 4)),
            nn.ConvTranspose2d(128, 64, kernel_size=3, stride=2, padding=1), nn.ReLU(),
            nn.ConvTranspose2d(64, 32, kernel_size=3, stride=2, padding=1, output_padding=1), nn.ReLU(),
            nn.ConvTranspose2d(32, 3, kernel_size=3, stride=2, padding=1, output_padding=1),
        )

    def late_leaf_params(self):
        """The transposed convolutions' weights: their gradients are leaves of the backward pass (trainers.FlatParams keeps them
        together at the end of its buffers, as for Decoder_VAE_SVHN)."""
        d = self.decoder
        return [d[3].weight, d[5].weight, d[7].weight]

    def forward(self, z):
        d = self.decoder
        z2 = z.reshape(-1, z.shape[-1])
        (pre,) = kernels.MLPHeadsFn.apply(z2, 1, d[0].weight, d[0].bias)  # [N, 2048] in (c, h, w) order, before the ReLU
        h0 = kernels.TransposeActFn.apply(pre.reshape(-1, 128, 16), kernels.RELU).reshape(-1, 4, 4, 128)  # ReLU on the way to NHWC
        out = kernels.PolyConvDecoderFn.run(h0, d[3].weight, d[3].bias, d[5].weight, d[5].bias, d[7].weight, d[7].bias)
        return ModelOutput(reconstruction=out.reshape(*z.shape[:-1], *out.shape[1:]))


###############################################################################
### ResNet architectures
###############################################################################


class ResnetBlock(nn.Module):
    """x_s + 0.1 * lrelu(conv2(lrelu(conv1(x))))  (`mmnist.py:214-252`).  Parameter container: the arithmetic runs
    inside kernels.ResnetStackFn."""

    order = "post"

    def __init__(self, nb_channels_in, nb_channels_out, nb_channels_hidden=None, bias=True):
        super().__init__()
        self.learn_shortcut = nb_channels_in != nb_channels_out
        if nb_channels_hidden is None:
            nb_channels_hidden = min(nb_channels_in, nb_channels_out)
        self.conv_layers = nn.Sequential(
            nn.Conv2d(nb_channels_in, nb_channels_hidden, 3, stride=1, padding=1),
            nn.LeakyReLU(2e-1),
            nn.Conv2d(nb_channels_hidden, nb_channels_out, 3, stride=1, padding=1, bias=bias),
            nn.LeakyReLU(2e-1),
        )
        if self.learn_shortcut:
            self.shortcut_layer = nn.Conv2d(nb_channels_in, nb_channels_out, 1, stride=1, padding=0, bias=False)

    def forward(self, x):  # NCHW in / out, like the reference module
        prog, params = [], []
        _add_block(prog, params, self)
        y = kernels.ResnetStackFn.apply(x.permute(0, 2, 3, 1), prog, *params)
        return y.permute(0, 3, 1, 2)


def _add_conv(prog, params, conv, act):
    params.append(conv.weight)
    iw = len(params) - 1
    ib = None
    if conv.bias is not None:
        params.append(conv.bias)
        ib = len(params) - 1
    prog.append(("conv", iw, ib, act))


def _add_block(prog, params, blk):
    if hasattr(blk, "conv_layers"):  # mmnist.py naming
        c1, c2, sc = blk.conv_layers[0], blk.conv_layers[2], getattr(blk, "shortcut_layer", None)
    else:  # cub.py naming
        c1, c2, sc = blk.conv_0, blk.conv_1, getattr(blk, "conv_s", None)
    idx = []
    for t in (c1.weight, c1.bias, c2.weight, c2.bias):
        if t is None:
            idx.append(None)
        else:
            params.append(t)
            idx.append(len(params) - 1)
    isc = None
    if sc is not None:
        params.append(sc.weight)
        isc = len(params) - 1
    prog.append(("block", blk.order, idx[0], idx[1], idx[2], idx[3], isc))


def _add_sequential(prog, params, seq):
    for m in seq:
        if hasattr(m, "order") and (hasattr(m, "conv_layers") or hasattr(m, "conv_0")):
            _add_block(prog, params, m)
        elif isinstance(m, nn.AvgPool2d):
            prog.append(("pool",))
        elif isinstance(m, nn.Upsample):
            prog.append(("up",))
        else:
            raise TypeError(f"unsupported layer in a ResNet stack: {type(m).__name__}")


class EncoderResnetMMNIST(BaseEncoder):
    """`mmnist.py:255-321`: conv_img -> ResnetBlock(64,64) -> [AvgPool, ResnetBlock] x 2 -> flatten (NCHW order) ->
    fc_mu / fc_lv, once for the shared latent (u) and once for the private latent (w, if private_latent_dim > 0)."""

    def __init__(self, private_latent_dim, shared_latent_dim):
        super().__init__()
        self.latent_dim = shared_latent_dim
        self.style_dim = private_latent_dim
        s0 = self.s0 = 7
        nf = self.nf = 64
        nf_max = self.nf_max = 1024
        size = 28
        self.multiple_latent = private_latent_dim > 0
        nlayers = int(np.log2(size / s0))
        self.nf0 = min(nf_max, nf * 2 ** nlayers)
        blocks_w = [ResnetBlock(nf, nf)]
        blocks_u = [ResnetBlock(nf, nf)]
        for i in range(nlayers):
            nf0 = min(nf * 2 ** i, nf_max)
            nf1 = min(nf * 2 ** (i + 1), nf_max)
            blocks_w += [nn.AvgPool2d(3, stride=2, padding=1), ResnetBlock(nf0, nf1)]
            blocks_u += [nn.AvgPool2d(3, stride=2, padding=1), ResnetBlock(nf0, nf1)]
        if self.multiple_latent:
            self.conv_img_w = nn.Conv2d(3, 1 * nf, 3, padding=1)
            self.resnet_w = nn.Sequential(*blocks_w)
            self.fc_mu_w = nn.Linear(self.nf0 * s0 * s0, private_latent_dim)
            self.fc_lv_w = nn.Linear(self.nf0 * s0 * s0, private_latent_dim)
        self.conv_img_u = nn.Conv2d(3, 1 * nf, 3, padding=1)
        self.resnet_u = nn.Sequential(*blocks_u)
        self.fc_mu_u = nn.Linear(self.nf0 * s0 * s0, shared_latent_dim)
        self.fc_lv_u = nn.Linear(self.nf0 * s0 * s0, shared_latent_dim)

    def _branch(self, x_nhwc, conv_img, resnet, fc_mu, fc_lv):
        prog, params = [], []
        _add_conv(prog, params, conv_img, kernels.NONE)
        _add_sequential(prog, params, resnet)
        h = kernels.ResnetStackFn.apply(x_nhwc, prog, *params)  # [B, 7, 7, nf0]
        flat = kernels.nhwc_to_flat_nchw(h)  # the reference flattens NCHW
        return kernels.MLPHeadsFn.apply(flat, 2, fc_mu.weight, fc_mu.bias, fc_lv.weight, fc_lv.bias)

    def forward(self, x):
        x_nhwc = x.permute(0, 2, 3, 1).contiguous()
        mu, lv = self._branch(x_nhwc, self.conv_img_u, self.resnet_u, self.fc_mu_u, self.fc_lv_u)
        output = ModelOutput(embedding=mu, log_covariance=lv)
        if self.multiple_latent:
            smu, slv = self._branch(x_nhwc, self.conv_img_w, self.resnet_w, self.fc_mu_w, self.fc_lv_w)
            output["style_embedding"] = smu
            output["style_log_covariance"] = slv
        return output


class DecoderResnetMMNIST(BaseDecoder):
    """`mmnist.py:324-366`: fc -> [ResnetBlock, Upsample] x 2 -> ResnetBlock(64,64) -> Conv(64,3,3) + LeakyReLU(0.2).
    latent_dim is the total (shared + private) latent dimension."""
    rows_independent = True


    def __init__(self, latent_dim):
        super().__init__()
        s0 = self.s0 = 7
        nf = self.nf = 64
        nf_max = self.nf_max = 512
        size = 28
        nlayers = int(np.log2(size / s0))
        self.nf0 = min(nf_max, nf * 2 ** nlayers)
        self.fc = nn.Linear(latent_dim, self.nf0 * s0 * s0)
        blocks = []
        for i in range(nlayers):
            nf0 = min(nf * 2 ** (nlayers - i), nf_max)
            nf1 = min(nf * 2 ** (nlayers - i - 1), nf_max)
            blocks += [ResnetBlock(nf0, nf1), nn.Upsample(scale_factor=2)]
        blocks += [ResnetBlock(nf, nf)]
        self.resnet = nn.Sequential(*blocks)
        self.conv_img = nn.Sequential(nn.Conv2d(nf, 3, 3, padding=1), nn.LeakyReLU(2e-1))

    def forward(self, z):
        z2 = z.reshape(-1, z.shape[-1])
        (h,) = kernels.MLPHeadsFn.apply(z2, 1, self.fc.weight, self.fc.bias)  # [N, nf0*7*7] in NCHW order
        h = kernels.flat_nchw_to_nhwc(h, self.nf0, self.s0, self.s0)
        prog, params = [], []
        _add_sequential(prog, params, self.resnet)
        _add_conv(prog, params, self.conv_img[0], kernels.LEAKY)
        out = kernels.ResnetStackFn.apply(h, prog, *params).permute(0, 3, 1, 2)  # NCHW [N, 3, 28, 28]
        lead = z.shape[:1] if z.dim() == 2 else z.shape[:2]
        return ModelOutput(reconstruction=out.reshape(*lead, *out.shape[1:]))
