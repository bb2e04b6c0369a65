"""`multivae/samplers/maf_sampler/maf_sampler.py`: a masked autoregressive flow per latent space."""
from ...models.nn.flows import MAF, MAFConfig
from ..flow_sampler import FlowSampler
from .maf_sampler_config import MAFSamplerConfig


class MAFSampler(FlowSampler):
    """Fits a masked autoregressive flow in the latent space of a trained model (one more per private latent space).  The fit is
    one fused pass per step (mvk_maf_fwd / mvk_maf_bwd); a sample costs the flow's sequential inverse (mvk_maf_inverse)."""

    flow_cls, flow_config_cls, config_cls = MAF, MAFConfig, MAFSamplerConfig
    sampler_name = "MAFsampler"
