"""TELBO (Vedantam et al. 2018, the "triple ELBO") on the fused HIP path.  Mirrors `multivae/models/telbo/telbo_model.py`:
constructor :35-56, the freeze :58-63, forward :65-124, encode :126-174.

Two stages.  Up to `warmup` epochs the joint encoder and the decoders train on the joint ELBO (the unimodal encoders do not run);
afterwards they are frozen and every unimodal encoder trains on its own ELBO against the frozen decoder — with the reference's
row "KL", which takes the JOINT encoder's log-variance in the place of the modality's own (:118-120).  Stage two's M samples and M
row sums come out of ONE launch (`mvk_telbo_latent_fwd/bwd`, kernels.TELBOLatentFn); the joint encoder runs without autograd for
its log-variance only (the reference also samples and decodes the joint posterior there and discards the result).  Both stages
assemble the loss and the metrics in ReconLossFn.  `MultistageTrainer` drives the stage change (`reset_optimizer_epochs`,
`stage_parameters`)."""
from typing import Union

import torch

from ... import kernels, schedule
from ..base.base_utils import ModelOutput
from ..joint_models import BaseJointModel
from ..nn.base_architectures import BaseJointEncoder
from .telbo_config import TELBOConfig


class TELBO(BaseJointModel):
    def __init__(self, model_config: TELBOConfig, encoders: dict = None, decoders: dict = None,
                 joint_encoder: Union[BaseJointEncoder, None] = None, **kwargs):
        super().__init__(model_config, encoders, decoders, joint_encoder, **kwargs)
        self.model_name = "TELBO"
        self.warmup = model_config.warmup
        self.reset_optimizer_epochs = [self.warmup]  # the reference resets one epoch BEFORE the stage change (:47)
        self.lambda_factors = self.rescale_factors if model_config.lambda_factors is None else model_config.lambda_factors
        self.gamma_factors = self.rescale_factors if model_config.gamma_factors is None else model_config.gamma_factors

    def _set_torch_no_grad_on_joint_vae(self):
        """Freeze the joint encoder and the decoders (:58-63).  Their gradients are dropped as well: left in place they stay views
        of the trainer's flat gradient buffer, and the kernels would go on accumulating into it (kernels._grad_target)."""
        for module in (self.joint_encoder, self.decoders):
            for p in module.parameters():
                p.requires_grad_(False)
                p.grad = None

    def stage_parameters(self, epoch):
        """The parameters that receive gradients in `epoch`, in `parameters()` order: what a trainer builds its optimizer state
        over.  A stage-two epoch freezes the rest here, before the first forward pass of that stage does."""
        if epoch <= self.warmup:
            skip = {id(p) for p in self.encoders.parameters()}
        else:
            self._set_torch_no_grad_on_joint_vae()
            skip = set()
        return [p for p in self.parameters() if p.requires_grad and id(p) not in skip]

    def graph_key(self, epoch=1, **kwargs):
        """What a captured training graph of this model depends on besides the batch shape: the stage."""
        return 1 if int(epoch) <= int(self.warmup) else 2

    def forward(self, inputs, **kwargs) -> ModelOutput:
        """kwargs: epoch (<= warmup: stage one), noise (explicit eps: [B,L] in stage one, [M,B,L] in `encoders` order in stage two)."""
        super().forward(inputs)
        epoch = kwargs.pop("epoch", 1)
        noise = kwargs.pop("noise", None)
        if epoch <= self.warmup:
            return self._joint_elbo(inputs, noise)
        return self._unimodal_elbos(inputs, noise)

    def _joint_elbo(self, inputs, noise):
        joint = self.joint_encoder(inputs.data)
        mu, lv = joint.embedding, joint.log_covariance
        B, L = mu.shape
        device = mu.device
        eps = self._noise((1, B, L), device, None if noise is None else noise.reshape(1, B, L))
        z, kld_rows = kernels.GaussSampleKLFn.apply(eps, mu, lv)
        names = list(self.decoders.keys())
        rec = schedule.run_branches(self._branch_order(inputs, names), lambda m: self.decoders[m](z[0]).reconstruction, device)
        M = len(names)
        spec = self._recon_spec(names, inputs.data, None, 1, B)
        spec.update(rescale=[float(self.lambda_factors[m]) for m in names], coef=[1.0 / B] * M, lossw=[1.0] * M,
                    extra_coef=[1.0 / B], extra_lossw=[1.0], loss_sum_scale=float(B))
        loss, terms = kernels.ReconLossFn.apply(spec, M, *[rec[m] for m in names], kld_rows)
        recon = terms[:M].sum()  # terms[i] = term_i / B
        return ModelOutput(recon_loss=recon, KLD=terms[M], loss=loss, metrics=dict(kld_joint=terms[M] * float(B), recon_joint=recon))

    def _unimodal_elbos(self, inputs, noise):
        self._set_torch_no_grad_on_joint_vae()
        with torch.no_grad():
            jlv = self.joint_encoder(inputs.data).log_covariance
        B, L = jlv.shape
        device = jlv.device
        names = list(self.encoders.keys())
        M = len(names)
        enc = schedule.run_branches(self._branch_order(inputs, names), lambda m: self.encoders[m](inputs.data[m]), device)
        eps = self._noise((M, B, L), device, noise)
        out = kernels.TELBOLatentFn.apply(eps, jlv, *[enc[m].embedding for m in names], *[enc[m].log_covariance for m in names])
        kld_rows, z = out[0], dict(zip(names, out[1:]))
        rec = schedule.run_branches(self._branch_order(inputs, names), lambda m: self.decoders[m](z[m]).reconstruction, device)
        spec = self._recon_spec(names, inputs.data, None, 1, B)
        # terms [rec_m (sums over the batch) | kld_m]; loss = sum of all / B, loss_sum = loss * B
        spec.update(rescale=[float(self.gamma_factors[m]) for m in names], coef=[1.0] * M, lossw=[1.0 / B] * M,
                    extra_coef=[1.0], extra_lossw=[1.0 / B], extra_split=[M], loss_sum_scale=float(B))
        loss, terms = kernels.ReconLossFn.apply(spec, M, *[rec[m] for m in names], kld_rows)
        elbos = terms[:M] + terms[M:2 * M]
        return ModelOutput(loss=loss, loss_sum=terms[2 * M + 1], metrics={m: elbos[i] for i, m in enumerate(names)})

    def encode(self, inputs, cond_mod: Union[list, str] = "all", N: int = 1, return_mean=False, **kwargs):
        self.eval()
        cond_mod = super().encode(inputs, cond_mod, N, **kwargs).cond_mod
        flatten = kwargs.pop("flatten", False)
        with torch.no_grad():
            if len(cond_mod) == 1:
                out = self.encoders[cond_mod[0]](inputs.data[cond_mod[0]])
            elif len(cond_mod) == self.n_modalities:
                out = self.joint_encoder(inputs.data)
            else:
                raise ValueError(f" Conditioning on subset {cond_mod} is not handled. "
                                 f" Possible subsets are  {list(self.encoders.keys())} and 'all'. ")
            z = self._gaussian_encoding(out.embedding, out.log_covariance, N, return_mean, flatten, kwargs.get("noise"))
        return ModelOutput(z=z, one_latent_space=True)
