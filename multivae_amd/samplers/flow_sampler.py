"""What MAFSampler and IAFSampler share (`multivae/samplers/maf_sampler/maf_sampler.py`, `iaf_sampler/iaf_sampler.py`): one
normalizing flow per latent space, fitted on the training embeddings by maximum likelihood under N(0, I); a sample is
z = flow.inverse(u), u ~ N(0, I).  The reference wraps each flow in pythae's `NFModel`, trains it with pythae's `BaseTrainer` on a
host dataset and reloads the best checkpoint from disk; here the embeddings stay on the device and `flow_fit.fit_flow` fits the flow
in place (fused kernels where they apply), and `sample` inverts with `mvk_maf_inverse` / `mvk_iaf_inverse`."""
import logging
import os

import torch
from torch.utils.data import DataLoader

from .. import kernels as K
from .._output import ModelOutput
from ..data.utils import set_inputs_to_device
from ..models.nn.flows import MAF
from .base import BaseSampler
from .flow_fit import fit_flow, flow_dims, load_flow, save_flow

logger = logging.getLogger(__name__)


class FlowSampler(BaseSampler):
    """flow_cls / flow_config_cls / name are set by the subclass.  `flows_dims`: {"shared": latent_dim} plus the model's
    `style_dims` when it has private latent spaces; `flows_models[key]`: the flow of that space.  `fit` must be called (or
    `load_flows_from_folder`) before `sample`."""

    flow_cls = flow_config_cls = config_cls = None
    sampler_name = None

    def __init__(self, model, sampler_config=None):
        if sampler_config is None:
            sampler_config = self.config_cls()
        BaseSampler.__init__(self, model=model, sampler_config=sampler_config)
        if sampler_config.include_batch_norm:
            raise NotImplementedError(f"{type(self).__name__}: include_batch_norm=True is not built here")
        self.flows_dims = dict(shared=model.model_config.latent_dim)
        if self.model.multiple_latent_spaces:
            self.flows_dims.update(self.model.style_dims)
        self.flows_models = {}
        for key, dim in self.flows_dims.items():
            config = self.flow_config_cls(input_dim=(int(dim),), n_made_blocks=sampler_config.n_made_blocks,
                                          n_hidden_in_made=sampler_config.n_hidden_in_made,
                                          hidden_size=sampler_config.hidden_size,
                                          include_batch_norm=sampler_config.include_batch_norm)
            self.flows_models[key] = self.flow_cls(config).to(self.device)
        self.fit_history = {}
        self.name = self.sampler_name

    def _codes(self, data):
        loader = DataLoader(dataset=data, batch_size=100, shuffle=False)  # the fit draws its own seeded batch order
        zs = {key: [] for key in self.flows_models}
        with torch.no_grad():
            for inputs in loader:
                out = self.model.encode(set_inputs_to_device(inputs, self.device))
                zs["shared"].append(out.z.detach())
                if self.model.multiple_latent_spaces:
                    for m in out.modalities_z:
                        zs[m].append(out.modalities_z[m].detach())
        return {key: torch.cat(v).float() for key, v in zs.items()}

    def fit(self, train_data, eval_data=None, training_config=None, **kwargs):
        """Encode train_data (and eval_data) in batches of 100, keep the codes on the device and fit one flow per latent space
        (flow_fit.fit_flow: which fields of `training_config`, a BaseTrainerConfig, are honoured).  kwargs: fused (None, True,
        False: flow_fit.fit_flow)."""
        train = self._codes(train_data)
        evals = None if eval_data is None else self._codes(eval_data)
        for key, flow in self.flows_models.items():
            self.fit_history[key] = fit_flow(flow, train[key], None if evals is None else evals[key], training_config,
                                             fused=kwargs.get("fused"))
        self.is_fitted = True

    def _inverse(self, flow, u):
        lay = flow_dims(flow) if u.is_cuda else None
        if lay is None:
            with torch.no_grad():
                return flow.inverse(u).out
        dims, Ws, bs = lay
        Ws, bs = [w.detach() for w in Ws], [b.detach() for b in bs]
        return (K.maf_inverse if type(flow) is MAF else K.iaf_inverse)(u, dims, Ws, bs)[0]

    def sample(self, n_samples: int = 1, batch_size: int = 500, **kwargs):
        """A ModelOutput like `encode` returns: z [n_samples, latent_dim], one_latent_space, and modalities_z for a model with
        private latent spaces.  kwargs (for tests): generator (a torch.Generator on the sampler's device)."""
        if not self.is_fitted:
            raise ArithmeticError("The sampler needs to be fitted by calling sampler.fit() method before sampling.")
        generator = kwargs.get("generator")
        sizes = [batch_size] * int(n_samples / batch_size)
        if n_samples % batch_size != 0:
            sizes.append(n_samples % batch_size)
        z_gen = {key: [] for key in self.flows_models}
        for b in sizes:
            for key, flow in self.flows_models.items():
                u = torch.randn(b, int(self.flows_dims[key]), generator=generator, device=self.device, dtype=torch.float32)
                z_gen[key].append(self._inverse(flow, u))
        output = ModelOutput(z=torch.cat(z_gen.pop("shared")), one_latent_space=not self.model.multiple_latent_spaces)
        if self.model.multiple_latent_spaces:
            output["modalities_z"] = {m: torch.cat(z_gen[m]) for m in z_gen}
        return output

    def save(self, dir_path):
        """`sampler_config.json` and one folder per latent space with `model_config.json` and `model.pt`."""
        super().save(dir_path=dir_path)
        if not self.is_fitted:
            raise ArithmeticError("The sampler needs to be fitted by calling sampler.fit() method before sampling.")
        for key, flow in self.flows_models.items():
            save_flow(flow, os.path.join(dir_path, key))

    def load_flows_from_folder(self, dir_path):
        """Instead of `fit`: reload the flows a sampler of the same model and config saved to dir_path."""
        for key in self.flows_models:
            try:
                self.flows_models[key] = load_flow(self.flow_cls, self.flow_config_cls, os.path.join(dir_path, key)).to(self.device)
            except Exception as exc:
                raise AttributeError("Error when trying to load the flows from the folder.",
                                     f"Check that you provided the right path. Exception raised: {exc}")
        self.is_fitted = True
