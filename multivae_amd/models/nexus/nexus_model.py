"""Nexus (Vasco et al. 2022), the two-level multimodal VAE, on the HIP kernels.  Mirrors `multivae/models/nexus/nexus_model.py`:
_compute_bottom_elbos :80-137, forward :139-207, _aggregate_during_training :209-254, encode :256-316, decode :318-360.

First level: every modality has its own VAE (encoder -> z_m -> decoder, `mvk_gauss_sample_kl_fwd/bwd` for the sample and its
KL).  Second level: the DETACHED z_m go through the top encoders to messages, the messages are averaged over the kept
modalities (`mvk_nexus_aggregate_fwd/bwd`: dataset masks, an explicit keep matrix or forced perceptual dropout drawn on the
device), the joint encoder gives z_sigma, and the top decoders score z_m under N(r_m, s_m) (`mvk_nexus_top_nll_fwd/bwd`, s_m
optionally adapted to the batch).  Every term of the loss and every metric comes out of ONE assembly launch (ReconLossFn)."""
from typing import Union

import torch
from torch import nn

from ... import kernels, schedule
from ..base import BaseMultiVAE
from ..base.base_config import BaseAEConfig
from ..base.base_utils import ModelOutput, rsample_from_gaussian
from ..nn.base_architectures import BaseDecoder, BaseEncoder
from ..nn.default_architectures import Decoder_AE_MLP, Encoder_VAE_MLP
from .nexus_config import NexusConfig


class Nexus(BaseMultiVAE):
    def __init__(self, model_config: NexusConfig, encoders: dict = None, decoders: dict = None, top_encoders: dict = None,
                 joint_encoder: Union[BaseEncoder, None] = None, top_decoders: dict = None, **kwargs):
        super().__init__(model_config, encoders, decoders)
        self.model_name = "NEXUS"
        # parameter order of the reference: decoders, encoders, top_decoders, top_encoders, joint_encoder
        self._set_top_decoders(top_decoders, model_config)
        self._set_top_encoders(top_encoders, model_config)
        self._set_joint_encoder(joint_encoder, model_config)
        self._set_bottom_betas(model_config.bottom_betas)
        self._set_gammas(model_config.gammas)
        self.warmup = model_config.warmup
        self.start_keep_best_epoch = model_config.warmup + 1
        self.adapt_top_decoder_variance = self._set_top_decoder_variance(model_config)
        self.check_aggregator(model_config)

    # -- configuration (the reference's checks and defaults) ------------------------------------------------------------------
    def _set_top_decoder_variance(self, config):
        if config.adapt_top_decoder_variance is None:
            return []
        for m in config.adapt_top_decoder_variance:
            if m not in self.modalities_name:
                raise AttributeError("A string provided in *adapt_top_decoder_variance* field doesn't match any of the "
                                     f"modalities name : {m} is not in {self.modalities_name}")
        return config.adapt_top_decoder_variance

    def _set_bottom_betas(self, bottom_betas):
        if bottom_betas is None:
            bottom_betas = {m: 1.0 for m in self.encoders}
        if bottom_betas.keys() != self.encoders.keys():
            raise AttributeError("The bottom_betas keys do not match the modalitiesnames in encoders.")
        self.bottom_betas = bottom_betas

    def _set_gammas(self, gammas):
        if gammas is None:
            self.gammas = {m: 1.0 for m in self.encoders}
        elif gammas.keys() != self.encoders.keys():
            raise AttributeError("The gammas keys do not match the modalitiesnames in encoders.")
        else:
            self.gammas = gammas

    def _check_dims(self, model_config, what, need_inputs=True):
        if (need_inputs and model_config.input_dims is None) or model_config.modalities_specific_dim is None:
            raise AttributeError(f"Please provide {what} architectures or valid input_dims and modalities_specific_dim in "
                                 "the model configuration")

    def default_encoders(self, model_config: NexusConfig):
        self._check_dims(model_config, "encoders")
        return nn.ModuleDict({m: Encoder_VAE_MLP(BaseAEConfig(input_dim=model_config.input_dims[m],
                                                              latent_dim=model_config.modalities_specific_dim[m]))
                              for m in model_config.input_dims})

    def default_decoders(self, model_config: NexusConfig):
        self._check_dims(model_config, "decoders")
        return nn.ModuleDict({m: Decoder_AE_MLP(BaseAEConfig(input_dim=model_config.input_dims[m],
                                                             latent_dim=model_config.modalities_specific_dim[m]))
                              for m in model_config.input_dims})

    def _default_top_encoders(self, model_config: NexusConfig):
        self._check_dims(model_config, "top_encoders", need_inputs=False)
        return nn.ModuleDict({m: Encoder_VAE_MLP(BaseAEConfig(input_dim=(model_config.modalities_specific_dim[m],),
                                                              latent_dim=model_config.msg_dim))
                              for m in model_config.input_dims})

    def _default_top_decoders(self, model_config: NexusConfig):
        self._check_dims(model_config, "top_decoders", need_inputs=False)
        return nn.ModuleDict({m: Decoder_AE_MLP(BaseAEConfig(input_dim=(model_config.modalities_specific_dim[m],),
                                                             latent_dim=model_config.latent_dim))
                              for m in model_config.input_dims})

    def _set_top_encoders(self, top_encoders, model_config):
        if top_encoders is None:
            top_encoders = self._default_top_encoders(model_config)
        else:
            self.model_config.custom_architectures.append("top_encoders")
        self.top_encoders = nn.ModuleDict()
        for k in top_encoders:
            if not isinstance(top_encoders[k], BaseEncoder):
                raise AttributeError("Top Encoders must be instances of multivae.models.base.BaseEncoder")
            self.top_encoders[k] = top_encoders[k]

    def _set_top_decoders(self, top_decoders, model_config):
        if top_decoders is None:
            top_decoders = self._default_top_decoders(model_config)
        else:
            self.model_config.custom_architectures.append("top_decoders")
        self.top_decoders = nn.ModuleDict()
        for k in top_decoders:
            if not isinstance(top_decoders[k], BaseDecoder):
                raise AttributeError("Top Decoders must be instances of multivae.models.base.BaseDecoder")
            self.top_decoders[k] = top_decoders[k]

    def _set_joint_encoder(self, joint_encoder, model_config):
        if joint_encoder is None:
            joint_encoder = Encoder_VAE_MLP(BaseAEConfig(input_dim=(model_config.msg_dim,), latent_dim=model_config.latent_dim))
        else:
            self.model_config.custom_architectures.append("joint_encoder")
        if not isinstance(joint_encoder, BaseEncoder):
            raise AttributeError("Joint encoder must be an instance of multivae.models.base.BaseEncoder")
        self.joint_encoder = joint_encoder

    def check_aggregator(self, model_config):
        if model_config.aggregator not in ["mean"]:
            raise AttributeError(f"This aggregator {model_config.aggregator} is not supported at the moment")

    def graph_key(self, epoch=1, **kwargs):
        """What a captured training graph depends on besides the batch shape: the annealing factor."""
        return min(int(epoch), int(self.warmup))

    # -- training -------------------------------------------------------------------------------------------------------------
    def forward(self, inputs, **kwargs) -> ModelOutput:
        """kwargs: epoch (annealing = min(epoch / warmup, 1)); noise = {"bottom": {m: [B, S_m]}, "joint": [B, L]} (the
        reparameterisation eps of the two levels); keep [B, M] (1 = the message of modality m enters row b's mean, modalities
        in `inputs.data` order) replaces the forced-perceptual-dropout draw.  Without them every draw comes from the device
        generator.  As in the reference, dropout applies whatever `self.training` is, and never to a dataset with masks."""
        epoch = kwargs.pop("epoch", 1)
        noise = kwargs.pop("noise", None) or {}
        keep = kwargs.pop("keep", None)
        a = min(epoch / self.model_config.warmup, 1.0)
        names = list(inputs.data.keys())
        M = len(names)
        x0 = inputs.data[names[0]]
        B, device = x0.shape[0], x0.device
        masks = inputs.masks if hasattr(inputs, "masks") else None
        spec = self._recon_spec(names, inputs.data, masks, 1, B)
        bmasks = spec["masks"] if masks is not None else None

        # first level: z_m ~ q(z_m | x_m), KL(q || N(0, I)) rows, reconstruction
        order = self._branch_order(inputs, names)
        enc = schedule.run_branches(order, lambda m: self.encoders[m](inputs.data[m]), device)
        z, kl = {}, {}
        bottom_noise = noise.get("bottom") or {}
        for m in names:
            mu, lv = enc[m].embedding, enc[m].log_covariance
            S = mu.shape[-1]
            eps = bottom_noise.get(m)
            z[m], kl[m] = kernels.GaussSampleKLFn.apply(self._noise((1, B, S), device, None if eps is None else eps.reshape(1, B, S)),
                                                        mu, lv)
        rec = schedule.run_branches(order, lambda m: self.decoders[m](z[m][0]).reconstruction, device)
        # second level: messages of the detached z_m, their mean over the kept modalities, z_sigma
        zd = {m: z[m][0].detach() for m in names}
        msg = schedule.run_branches(order, lambda m: self.top_encoders[m](zd[m]).embedding, device)
        msgs = [msg[m] for m in names]
        if bmasks is not None:
            agg, keep_used = kernels.NexusAggregateFn.apply(bmasks, None, None, 0.0, *msgs)
        elif keep is not None:
            keep = keep.to(device=device, dtype=torch.float32).contiguous()
            if tuple(keep.shape) != (B, M):
                raise ValueError(f"keep has shape {tuple(keep.shape)}, expected {(B, M)}")
            agg, keep_used = kernels.NexusAggregateFn.apply(None, keep, None, 0.0, *msgs)
        else:
            p = float(self.model_config.dropout_rate)
            u = self._uniforms((B, M + 1), device) if p > 0 else None
            agg, keep_used = kernels.NexusAggregateFn.apply(None, None, u, p, *msgs)
        jout = self.joint_encoder(agg)
        L = jout.embedding.shape[-1]
        jeps = noise.get("joint")
        zj, jkl = kernels.GaussSampleKLFn.apply(self._noise((1, B, L), device, None if jeps is None else jeps.reshape(1, B, L)),
                                                jout.embedding, jout.log_covariance)
        tnames = list(self.top_decoders.keys())
        top = schedule.run_branches(order, lambda m: self.top_decoders[m](zj[0]).reconstruction, device)
        rs = [top[m].reshape(B, -1) for m in tnames]
        tmasks = None if bmasks is None else [bmasks[names.index(m)] for m in tnames]
        top_rows, _ = kernels.NexusTopNLLFn.apply(tmasks, [float(self.gammas[m]) for m in tnames],
                                                  [m in self.adapt_top_decoder_variance for m in tnames],
                                                  *[zd[m] for m in tnames], *rs)
        # assembly: terms [recon_m (masked means) | KL_m (masked means) | top rows_m (mean) | joint KL (mean)], loss = sum of
        # the weighted terms = the batch mean of the per-row loss, loss_sum = B loss
        kl_loss = [kl[m] if masks is None else kl[m] * bmasks[i].to(kl[m].dtype) for i, m in enumerate(names)]
        rows_out = []
        spec.update(coef=[1.0 / B] * M, lossw=[1.0] * M, extra_coef=[1.0 / B] * (M + 2),
                    extra_lossw=[float(self.bottom_betas[m]) * a for m in names] + [1.0, float(self.model_config.top_beta) * a],
                    extra_split=[1] * M + [len(tnames), 1], loss_sum_scale=float(B), rows_out=rows_out)
        loss, terms = kernels.ReconLossFn.apply(spec, M, *[rec[m] for m in names], *kl_loss, top_rows, jkl)
        T = len(tnames)
        with torch.no_grad():
            metrics = {}
            for i, m in enumerate(names):
                metrics["recon_loss_" + m] = terms[i] if masks is None else rows_out[i].mean()
                metrics["kl_" + m] = kl[m].mean()
            for j, m in enumerate(tnames):
                metrics["recon_z_" + m] = terms[2 * M + j]
            bottom = terms[0]
            for i, m in enumerate(names):
                bottom = (bottom if i == 0 else bottom + terms[i]) + float(self.bottom_betas[m]) * a * terms[M + i]
            joint_kld = terms[2 * M + T]
            metrics.update(annealing=a, bottom_loss=bottom,
                           top_loss=terms[2 * M:2 * M + T].sum() + float(self.model_config.top_beta) * a * joint_kld,
                           joint_KLD=joint_kld)
        return ModelOutput(loss=loss, loss_sum=terms[2 * M + T + 2], metrics=metrics, keep=keep_used)

    @staticmethod
    def _uniforms(shape, device):
        """U[0, 1) for the dropout decisions: the device generator (a replayed graph draws fresh subsets) on a CUDA device."""
        if torch.device(device).type == "cuda":
            return kernels.device_randn(tuple(shape), device, uniform=True, lo=0.0, hi=1.0)
        return torch.rand(shape, device=device, dtype=torch.float32)

    # -- inference helpers ----------------------------------------------------------------------------------------------------
    def encode(self, inputs, cond_mod: Union[list, str] = "all", N: int = 1, return_mean=False, **kwargs):
        cond_mod = super().encode(inputs, cond_mod, N, **kwargs).cond_mod
        flatten = kwargs.pop("flatten", False)
        modalities_z, msgs = {}, []
        for m in cond_mod:
            out = self.encoders[m](inputs.data[m])
            modalities_z[m] = rsample_from_gaussian(out.embedding, out.log_covariance, N, return_mean, flatten=True)
            msgs.append(self.top_encoders[m](modalities_z[m]).embedding)
        agg = kernels.NexusAggregateFn.apply(None, None, None, 0.0, *msgs)[0]  # the plain mean over cond_mod
        jout = self.joint_encoder(agg)
        z = rsample_from_gaussian(jout.embedding, jout.log_covariance, N=1, return_mean=return_mean)
        if N > 1 and not flatten:
            z = z.reshape(N, -1, *z.shape[1:])
            modalities_z = {m: v.reshape(N, -1, *v.shape[1:]) for m, v in modalities_z.items()}
        return ModelOutput(z=z, one_latent_space=True, modalities_z=modalities_z)

    def decode(self, embedding: ModelOutput, modalities: Union[list, str] = "all", **kwargs):
        self.eval()
        with torch.no_grad():
            if modalities == "all":
                modalities = list(self.encoders.keys())
            elif isinstance(modalities, str):
                modalities = [modalities]
            use_bottom = kwargs.pop("use_bottom_z_for_recon", True)
            if not hasattr(embedding, "modalities_z"):
                use_bottom = False
            outputs = ModelOutput()
            reshape = len(embedding.z.shape) == 3
            if reshape:
                N, bs, _ = embedding.z.shape
            for m in modalities:
                if use_bottom and m in embedding.modalities_z.keys():
                    z_m = embedding.modalities_z[m]
                    if reshape:
                        z_m = z_m.reshape(N * bs, -1)
                else:
                    z = embedding.z.reshape(N * bs, -1) if reshape else embedding.z
                    z_m = self.top_decoders[m](z).reconstruction
                recon = self.decoders[m](z_m).reconstruction
                if reshape:
                    recon = recon.reshape(N, bs, *recon.shape[1:])
                outputs[m] = recon
            return outputs

    def compute_joint_nll(self, inputs, K: int = 1000, batch_size_K: int = 100, **kwargs):
        raise NotImplementedError("The joint likelihood of Nexus is not implemented (as in the reference).")
