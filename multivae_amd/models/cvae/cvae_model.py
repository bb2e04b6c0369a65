"""CVAE (Sohn et al. 2015), the conditional VAE, on the HIP kernels.  Mirrors `multivae/models/cvae/cvae_model.py`:
constructor and its checks :34-134, forward :136-180, encode :182-229, decode :231-262, generate_from_prior :264-312,
predict :314-362.

One joint encoder over all modalities gives q(z | x, c); an optional prior network over the conditioning modalities gives
p(z | c) (N(0, I) without one); one conditional decoder reconstructs the main modality from [z, c].  The sample, the KL to the
prior and the decoder's input [z, c] come out of ONE launch (`mvk_cond_latent_fwd/bwd`, kernels.CondLatentFn) in place of rsample + kl_divergence + stack + reshape +
cat; the loss and both metrics come out of the assembly launch of ReconLossFn."""
from copy import deepcopy
from typing import Dict, Union

import torch

from ... import kernels
from ..base import BaseModel, BaseMultiVAE
from ..base.base_utils import ModelOutput, decoder_dist_code, set_decoder_dist
from ..nn.base_architectures import BaseConditionalDecoder, BaseJointEncoder
from ..nn.default_architectures import BaseDictEncoders, ConditionalDecoderMLP, MultipleHeadJointEncoder
from .cvae_config import CVAEConfig


class CVAE(BaseModel):
    def __init__(self, model_config: CVAEConfig, encoder: Union[BaseJointEncoder, None] = None,
                 decoder: Union[BaseConditionalDecoder, None] = None, prior_network: Union[BaseJointEncoder, None] = None):
        super().__init__(model_config)
        self.latent_dim = model_config.latent_dim
        self.model_name = "CVAE"
        if model_config.decoder_dist_params is None:
            model_config.decoder_dist_params = {}
        self._set_decoder_dist(model_config.decoder_dist, model_config.decoder_dist_params)
        self.main_modality = model_config.main_modality
        self.conditioning_modalities = model_config.conditioning_modalities
        self.device = None
        # parameter order of the reference: encoder, decoder, prior_network
        self._set_encoder(encoder, model_config)
        self._set_decoder(decoder, model_config)
        self._set_prior_network(prior_network)

    # -- configuration (the reference's checks and defaults) ------------------------------------------------------------------
    def _set_encoder(self, encoder, model_config):
        if encoder is None:
            encoder = self._default_encoder(model_config)
        else:
            self.model_config.custom_architectures.append("encoder")
        if not isinstance(encoder, BaseJointEncoder):
            raise ValueError("The encoder must be an instance of BaseJointEncoder")
        self.encoder = encoder

    def _set_decoder(self, decoder, model_config):
        if decoder is None:
            decoder = self._default_decoder(model_config)
        else:
            self.model_config.custom_architectures.append("decoder")
        if not isinstance(decoder, BaseConditionalDecoder):
            raise ValueError("The decoder must be an instance of BaseConditionalDecoder")
        self.decoder = decoder

    def _set_prior_network(self, prior_network):
        if prior_network is None:
            self.prior_network = None  # the prior is the standard normal distribution
        elif not isinstance(prior_network, BaseJointEncoder):
            raise ValueError("The prior network must be an instance of BaseJointEncoder")
        else:
            self.prior_network = prior_network
            self.model_config.custom_architectures.append("prior_network")

    def _set_decoder_dist(self, dist_name, dist_params):
        """(distribution code, scale) for mvk_recon_nll_*, and the reference's element-wise `recon_log_prob` for user code."""
        code = decoder_dist_code(dist_name)
        scale = float(dist_params.get("scale", 1.0)) if dist_name in ("normal", "laplace") else 1.0
        self.recon_dist = (code, scale)
        self.recon_log_prob = set_decoder_dist(dist_name, deepcopy(dist_params))

    def _default_encoder(self, model_config):
        if model_config.input_dims is None:
            raise AttributeError("No encoder was provided but model_config.input_dims is None",
                                 "Please provide the input_dims of the model or an encoder architecture")
        return MultipleHeadJointEncoder(dict_encoders=BaseDictEncoders(model_config.input_dims, model_config.latent_dim),
                                        args=model_config, hidden_dim=512, n_hidden_layers=2)

    def _default_decoder(self, model_config):
        if model_config.input_dims is None:
            raise AttributeError("No decoder was provided but model_config.input_dims is None",
                                 "Please provide the input_dims of the model or a decoder architecture")
        return ConditionalDecoderMLP(latent_dim=model_config.latent_dim,
                                     data_dim=model_config.input_dims[model_config.main_modality],
                                     cond_data_dims={m: model_config.input_dims[m] for m in model_config.conditioning_modalities})

    def _cond(self, data):
        return {m: data[m] for m in self.conditioning_modalities}

    @staticmethod
    def _pieces(cond_mod_data):
        return [v if v.dtype == torch.float32 else v.float() for v in cond_mod_data.values()]

    def _sample(self, mu, lv, cond_mod_data, N, noise=None):
        """-> zc [N, B, L + C] without autograd: the samples of N(mu, exp(lv)) beside the conditioning data (one launch)."""
        B, L = mu.shape
        if noise is not None and noise.dim() == 2:
            noise = noise.unsqueeze(0)
        eps = BaseMultiVAE._noise((N, B, L), mu.device, noise)
        with torch.no_grad():
            return kernels.CondLatentFn.apply(eps, mu, lv, None, None, False, *self._pieces(cond_mod_data))[0]

    def _shape_outputs(self, z, cond_mod_data, N, flatten):
        """The reference's shapes: N == 1: z [B, L]; N > 1: z [N, B, L] with stacked conditioning data, or flattened [N B, ...]."""
        if N > 1 and not flatten:
            cond_mod_data = {m: torch.stack([v] * N) for m, v in cond_mod_data.items()}
        elif N > 1 and flatten:
            cond_mod_data = {m: torch.cat([v] * N) for m, v in cond_mod_data.items()}
            z = z.reshape(N * z.shape[1], z.shape[2])
        else:
            z = z[0] if z.dim() == 3 else z
        return ModelOutput(z=z, cond_mod_data=cond_mod_data)

    # -- training -------------------------------------------------------------------------------------------------------------
    def forward(self, inputs, **kwargs) -> ModelOutput:
        """kwargs: noise [B, L] (the reparameterisation eps; drawn on the device without it).  Other kwargs are ignored."""
        noise = kwargs.pop("noise", None)
        data = inputs.data
        cond_mod_data = self._cond(data)
        x = data[self.main_modality]
        B, device = x.shape[0], x.device
        # The encoder and the prior network are independent, but each is a joint encoder that forks its own per-modality branches
        # (schedule.run_branches); an outer fork around the two nests those forks, and a hipGraph capture of the nested form
        # crashed at capture end on the MI355X.  They run one after the other on the caller's stream, each with its own branches.
        out = self.encoder(data)
        pmu = plv = None
        if self.prior_network is not None:
            pout = self.prior_network(cond_mod_data)
            pmu, plv = pout.embedding, pout.log_covariance
        mu, lv = out.embedding, out.log_covariance
        L = mu.shape[-1]
        eps = BaseMultiVAE._noise((1, B, L), device, None if noise is None else noise.reshape(1, B, L))
        zc, kl_rows = kernels.CondLatentFn.apply(eps, mu, lv, pmu, plv, True, *self._pieces(cond_mod_data))
        if hasattr(self.decoder, "forward_concatenated"):
            recon = self.decoder.forward_concatenated(zc).reconstruction  # [1, B, *dims]: no slice node in the graph
        else:  # a user's conditional decoder: the reference contract
            recon = self.decoder(zc[0, :, :L], cond_mod_data).reconstruction
        code, scale = self.recon_dist
        xf = (x if x.dtype == torch.float32 else x.float()).contiguous()
        # terms [recon (sum over the elements, mean over the batch) | KL (mean over the batch)], loss = recon + beta KL
        spec = dict(K=1, B=B, x=[xf], masks=[None], dist=[code], scale=[scale], rescale=[1.0], coef=[1.0 / B], lossw=[1.0],
                    extra_coef=[1.0 / B], extra_lossw=[float(self.model_config.beta)], extra_split=[1], loss_sum_scale=float(B))
        loss, terms = kernels.ReconLossFn.apply(spec, 1, recon, kl_rows)
        return ModelOutput(loss=loss, metrics={"kl": terms[1], "recon_loss": terms[0]})

    # -- inference helpers ----------------------------------------------------------------------------------------------------
    def encode(self, inputs, N: int = 1, **kwargs) -> ModelOutput:
        """z ~ q(z | x, c): [B, L] for N == 1, [N, B, L] for N > 1 ([N B, L] with flatten=True), with the conditioning data shaped
        alike.  kwargs: return_mean, flatten, noise [N, B, L].  A sampled output also carries `zc`, the assembled decoder input
        [N, B, L + C] the sample was written into."""
        return_mean = kwargs.pop("return_mean", False)
        flatten = kwargs.pop("flatten", False)
        out = self.encoder(inputs.data)
        mu, lv = out.embedding, out.log_covariance
        cond_mod_data = self._cond(inputs.data)
        if return_mean:
            return self._shape_outputs(torch.stack([mu] * N) if N > 1 else mu, cond_mod_data, N, flatten)
        zc = self._sample(mu, lv, cond_mod_data, N, kwargs.pop("noise", None))
        res = self._shape_outputs(zc[..., :mu.shape[-1]], cond_mod_data, N, flatten)
        res.zc = zc
        return res

    def decode(self, embedding: ModelOutput, **kwargs) -> ModelOutput:
        with torch.no_grad():
            z, cond_mod_data = embedding.z, embedding.cond_mod_data
            if z.dim() == 3:
                N, n, d = z.shape
                cond_mod_data = {m: v.reshape(N * n, *v.shape[2:]) for m, v in cond_mod_data.items()}
                output = self.decoder(z.reshape(N * n, d), cond_mod_data)
                output.reconstruction = output.reconstruction.reshape(N, n, *output.reconstruction.shape[1:])
                return output
            return self.decoder(z, cond_mod_data)

    def generate_from_prior(self, cond_mod_data: Dict[str, torch.Tensor], N: int = 1, **kwargs) -> ModelOutput:
        """z ~ p(z | c) with the shapes of `encode`.  kwargs: flatten, noise [N, B, L]."""
        flatten = kwargs.pop("flatten", False)
        first = list(cond_mod_data.values())[0]
        B, device = first.shape[0], first.device
        cond_mod_data = {m: cond_mod_data[m] for m in self.conditioning_modalities}
        if self.prior_network is None:
            pmu = torch.zeros((B, self.latent_dim), dtype=torch.float32, device=device)
            plv = torch.zeros_like(pmu)
        else:
            out = self.prior_network(cond_mod_data)
            pmu, plv = out.embedding, out.log_covariance
        zc = self._sample(pmu, plv, cond_mod_data, N, kwargs.pop("noise", None))
        res = self._shape_outputs(zc[..., :pmu.shape[-1]], cond_mod_data, N, flatten)
        res.zc = zc
        return res

    def predict(self, inputs, cond_mod: Union[str, list] = "all", N=1, **kwargs) -> ModelOutput:
        """Reconstruction (cond_mod = "all", the main modality, or every modality) or generation from the prior (cond_mod = the
        conditioning modalities) of the main modality."""
        if (cond_mod == "all" or set(cond_mod) == {self.main_modality}
                or set(cond_mod) == set([self.main_modality] + list(self.conditioning_modalities))):
            embeddings = self.encode(inputs, N, **kwargs)
        elif set(cond_mod) == set(self.conditioning_modalities):
            embeddings = self.generate_from_prior(self._cond(inputs.data), N, **kwargs)
        else:
            raise ValueError("The conditioning modalities must be either 'all' or the list of conditioning modalities")
        output = ModelOutput()
        output[self.main_modality] = self.decode(embeddings).reconstruction
        return output
