"""Normalizing flows: the masked autoregressive flow (MAF, Papamakarios et al. 2017) and the inverse autoregressive flow (IAF, Kingma
et al. 2016) over MADE blocks (Germain et al. 2015), written from the published definitions with the module layout and state-dict
keys of `pythae.models.normalizing_flows` (`BaseNF`, `MADE`, `MAF`, `IAF`), which the reference's JNF and flow samplers take their
flows from.

These modules are plain torch: they run on the CPU, and on the GPU they are the path for everything the fused kernels decline
(`kernels.maf_fused_ok`, custom `BaseNF` flows).  JNF binds fusable `MAF`s to `mvk_maf_fwd/bwd/inverse` (csrc/maf.hip), which
compute the masks from the degree formulas below instead of reading the `mask` buffers; the flow samplers bind a fusable `IAF` to
`mvk_iaf_fwd/bwd/inverse` in the same way.

Degrees ("sequential" ordering), D = prod(input_dim): the inputs have m[-1] = arange(D), hidden layer i has m[i][k] = k % (D - 1).
Hidden masks: mask_i[o, k] = m[i][o] >= m[i-1][k]; output mask [D, H]: mask[d, k] = m[last][k] < d, stacked twice ([2D, H]: the rows
of mu, then those of the log-scale, which pythae calls `log_var`)."""
from dataclasses import field
from typing import List, Tuple, Union

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from pydantic.dataclasses import dataclass

from ..base.base_config import BaseConfig
from ..base.base_utils import ModelOutput


class BaseNF(nn.Module):
    """Base class of the flows: subclass it for a custom flow.  `input_dim` is a tuple; `forward(x)` and `inverse(y)` return
    ModelOutput(out, log_abs_det_jac)."""

    def __init__(self):
        nn.Module.__init__(self)
        self.input_dim = None

    def forward(self, x: torch.Tensor, **kwargs) -> ModelOutput:
        raise NotImplementedError()

    def inverse(self, y: torch.Tensor, **kwargs) -> ModelOutput:
        raise NotImplementedError()


class MaskedLinear(nn.Linear):
    """A linear layer whose weight is multiplied by the fixed 0/1 buffer `mask` ([out, in])."""

    def __init__(self, in_features, out_features, mask):
        nn.Linear.__init__(self, in_features=in_features, out_features=out_features)
        self.register_buffer("mask", mask)

    def forward(self, x):
        return F.linear(x, self.mask * self.weight, self.bias)


@dataclass
class MADEConfig(BaseConfig):
    input_dim: Union[Tuple[int, ...], None] = None
    output_dim: Union[Tuple[int, ...], None] = None
    hidden_sizes: List[int] = field(default_factory=lambda: [128, 128, 128])
    degrees_ordering: str = "sequential"


@dataclass
class MAFConfig(BaseConfig):
    input_dim: Union[Tuple[int, ...], None] = None
    n_made_blocks: int = 2
    n_hidden_in_made: int = 3
    hidden_size: int = 128
    include_batch_norm: bool = False


@dataclass
class IAFConfig(BaseConfig):
    input_dim: Union[Tuple[int, ...], None] = None
    n_made_blocks: int = 2
    n_hidden_in_made: int = 3
    hidden_size: int = 128
    include_batch_norm: bool = False


def sequential_degrees(D, hidden_sizes):
    """[m[-1], m[0], ..., m[last]] as int64 tensors."""
    return [torch.arange(D)] + [torch.arange(h) % (D - 1) for h in hidden_sizes]


def sequential_masks(D, hidden_sizes):
    """The masks of the len(hidden_sizes) + 1 layers of a MADE with D inputs, as float tensors [out, in]."""
    deg = sequential_degrees(D, hidden_sizes)
    masks = [(d1.unsqueeze(-1) >= d0.unsqueeze(0)).float() for d0, d1 in zip(deg[:-1], deg[1:])]
    masks.append((deg[-1].unsqueeze(0) < deg[0].unsqueeze(-1)).float().repeat(2, 1))
    return masks


class MADE(BaseNF):
    """Masked autoencoder for distribution estimation: `forward(x) -> ModelOutput(mu, log_var)`, output d of either depending on
    x[:, :d] only."""

    def __init__(self, model_config: MADEConfig):
        BaseNF.__init__(self)
        if model_config.input_dim is None or model_config.output_dim is None:
            raise AttributeError("MADEConfig needs input_dim and output_dim (tuples): the network is built from them")
        if model_config.degrees_ordering == "random":
            raise NotImplementedError("MADE: degrees_ordering='random' is not built here; use 'sequential'")
        if model_config.degrees_ordering != "sequential":
            raise AttributeError(f"MADE: unknown degrees_ordering '{model_config.degrees_ordering}' (supported: 'sequential')")
        self.model_config = model_config
        self.input_dim = int(np.prod(model_config.input_dim))
        self.output_dim = int(np.prod(model_config.output_dim))
        self.hidden_sizes = list(model_config.hidden_sizes)
        if self.input_dim < 2:
            raise ValueError(f"MADE needs an input dimension of at least 2, got {self.input_dim}: the hidden degrees are "
                             "k % (D - 1), and with one coordinate there is nothing to condition on")
        if self.output_dim != self.input_dim:
            raise ValueError(f"MADE: output_dim {self.output_dim} must equal input_dim {self.input_dim} (the net emits a mean and "
                             "a log-scale per coordinate)")
        if not self.hidden_sizes:
            raise ValueError("MADE needs at least one hidden layer")
        masks = sequential_masks(self.input_dim, self.hidden_sizes)
        sizes = [self.input_dim] + self.hidden_sizes
        layers = []
        for i, (inp, out) in enumerate(zip(sizes[:-1], sizes[1:])):
            layers.extend([MaskedLinear(inp, out, masks[i]), nn.ReLU()])
        layers.append(MaskedLinear(sizes[-1], 2 * self.output_dim, masks[-1]))
        self.net = nn.Sequential(*layers)

    def forward(self, x: torch.Tensor, **kwargs) -> ModelOutput:
        net_output = self.net(x.reshape(x.shape[0], -1))
        return ModelOutput(mu=net_output[:, : self.input_dim], log_var=net_output[:, self.input_dim :])


class MAF(BaseNF):
    """Masked autoregressive flow.  Forward, per block in order: x = (x - mu(x)) exp(-log_var(x)); ladj -= log_var.sum(-1);
    x = x.flip(1).  Inverse, per block in reverse: y = y.flip(1), then coordinate by coordinate from x = 0:
    x[:, i] = y[:, i] exp(log_var(x)[:, i]) + mu(x)[:, i], ladj += log_var[:, i]."""

    def __init__(self, model_config: MAFConfig):
        BaseNF.__init__(self)
        if model_config.input_dim is None:
            raise AttributeError("MAFConfig needs input_dim (a tuple): the network is built from it")
        if model_config.include_batch_norm:
            raise NotImplementedError("MAF: include_batch_norm=True is not built here (JNF's default flows do not use it)")
        self.model_config = model_config
        self.model_name = "MAF"
        self.input_dim = tuple(model_config.input_dim)
        self.hidden_size = model_config.hidden_size
        self.net = nn.ModuleList()
        made_config = MADEConfig(input_dim=self.input_dim, output_dim=self.input_dim,
                                 hidden_sizes=[self.hidden_size] * model_config.n_hidden_in_made,
                                 degrees_ordering="sequential")
        for _ in range(model_config.n_made_blocks):
            self.net.append(MADE(made_config))

    def forward(self, x: torch.Tensor, **kwargs) -> ModelOutput:
        x = x.reshape(x.shape[0], -1)
        sum_log_abs_det_jac = torch.zeros(x.shape[0], dtype=x.dtype, device=x.device)
        for layer in self.net:
            layer_out = layer(x)
            x = (x - layer_out.mu) * (-layer_out.log_var).exp()
            sum_log_abs_det_jac = sum_log_abs_det_jac - layer_out.log_var.sum(dim=-1)
            x = x.flip(dims=(1,))
        return ModelOutput(out=x, log_abs_det_jac=sum_log_abs_det_jac)

    def inverse(self, y: torch.Tensor, **kwargs) -> ModelOutput:
        y = y.reshape(y.shape[0], -1)
        D = y.shape[1]
        sum_log_abs_det_jac = torch.zeros(y.shape[0], dtype=y.dtype, device=y.device)
        for layer in self.net[::-1]:
            y = y.flip(dims=(1,))
            x = torch.zeros_like(y)
            for i in range(D):
                layer_out = layer(x.clone())
                mu, log_var = layer_out.mu, layer_out.log_var
                x[:, i] = y[:, i] * log_var[:, i].exp() + mu[:, i]
                sum_log_abs_det_jac = sum_log_abs_det_jac + log_var[:, i]
            y = x
        return ModelOutput(out=y, log_abs_det_jac=sum_log_abs_det_jac)


class IAF(BaseNF):
    """Inverse autoregressive flow: the MADEs of a MAF run the other way round, so that `inverse` (sampling) is one MADE pass per
    block and `forward` (the density) is the coordinate-by-coordinate sweep.  With (m, s) = MADE(.) (pythae: `mu`, `log_var`):
    forward, per block in order, from y = 0: y[:, i] = (x[:, i] - m(y)[:, i]) exp(-s(y)[:, i]), ladj -= s(y)[:, i] for i = 0..D-1,
    then x = y.flip(1).  Inverse, per block in reverse: y = y.flip(1); y = y exp(s(y)) + m(y); ladj += s.sum(-1)."""

    def __init__(self, model_config: IAFConfig):
        BaseNF.__init__(self)
        if model_config.input_dim is None:
            raise AttributeError("IAFConfig needs input_dim (a tuple): the network is built from it")
        if model_config.include_batch_norm:
            raise NotImplementedError("IAF: include_batch_norm=True is not built here")
        self.model_config = model_config
        self.model_name = "IAF"
        self.input_dim = tuple(model_config.input_dim)
        self.hidden_size = model_config.hidden_size
        self.net = nn.ModuleList()
        made_config = MADEConfig(input_dim=self.input_dim, output_dim=self.input_dim,
                                 hidden_sizes=[self.hidden_size] * model_config.n_hidden_in_made,
                                 degrees_ordering="sequential")
        for _ in range(model_config.n_made_blocks):
            self.net.append(MADE(made_config))

    def forward(self, x: torch.Tensor, **kwargs) -> ModelOutput:
        x = x.reshape(x.shape[0], -1)
        D = x.shape[1]
        sum_log_abs_det_jac = torch.zeros(x.shape[0], dtype=x.dtype, device=x.device)
        for layer in self.net:
            cols = []  # y_0 .. y_{i-1}; the MADE's outputs at i do not see the zeros behind them
            for i in range(D):
                y = torch.cat(cols + [x.new_zeros(x.shape[0], D - i)], dim=1) if cols else torch.zeros_like(x)
                layer_out = layer(y)
                mu, log_var = layer_out.mu, layer_out.log_var
                cols.append(((x[:, i] - mu[:, i]) * (-log_var[:, i]).exp()).unsqueeze(1))
                sum_log_abs_det_jac = sum_log_abs_det_jac - log_var[:, i]
            x = torch.cat(cols, dim=1).flip(dims=(1,))
        return ModelOutput(out=x, log_abs_det_jac=sum_log_abs_det_jac)

    def inverse(self, y: torch.Tensor, **kwargs) -> ModelOutput:
        y = y.reshape(y.shape[0], -1)
        sum_log_abs_det_jac = torch.zeros(y.shape[0], dtype=y.dtype, device=y.device)
        for layer in self.net[::-1]:
            y = y.flip(dims=(1,))
            layer_out = layer(y)
            y = y * layer_out.log_var.exp() + layer_out.mu
            sum_log_abs_det_jac = sum_log_abs_det_jac + layer_out.log_var.sum(dim=-1)
        return ModelOutput(out=y, log_abs_det_jac=sum_log_abs_det_jac)


def fused_layout(flow, kind=MAF):
    """(D, H, n_hidden, n_blocks, [MaskedLinear of every block in order]) when `flow` is a flow of class `kind` (MAF or IAF) that the
    fused kernels can stand in for — the layer shapes they assume and `mask` buffers equal to the sequential masks they compute from
    indices — else None."""
    if kind not in (MAF, IAF) or type(flow) is not kind or len(flow.net) < 1:
        return None
    D = int(np.prod(flow.input_dim))
    layers = []
    n_hidden = H = None
    for made in flow.net:
        if type(made) is not MADE:
            return None
        lin = [mod for mod in made.net if isinstance(mod, MaskedLinear)]
        if len(lin) != (len(made.net) + 1) // 2 or len(lin) < 2 or any(type(mod) is not MaskedLinear for mod in lin):
            return None
        if any(not isinstance(mod, nn.ReLU) for mod in list(made.net)[1::2]):
            return None
        if n_hidden is None:
            n_hidden, H = len(lin) - 1, lin[0].out_features
        sizes = [D] + [H] * n_hidden
        if len(lin) != n_hidden + 1:
            return None
        masks = sequential_masks(D, sizes[1:])
        for i, mod in enumerate(lin):
            shape = (sizes[i + 1], sizes[i]) if i < n_hidden else (2 * D, H)
            if tuple(mod.weight.shape) != shape or mod.bias is None or tuple(mod.mask.shape) != shape:
                return None
            if not torch.equal(mod.mask.detach().cpu().float(), masks[i]):
                return None
        layers.extend(lin)
    return D, H, n_hidden, len(flow.net), layers
