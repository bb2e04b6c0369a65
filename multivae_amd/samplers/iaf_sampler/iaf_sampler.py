"""`multivae/samplers/iaf_sampler/iaf_sampler.py`: an inverse autoregressive flow per latent space."""
from ...models.nn.flows import IAF, IAFConfig
from ..flow_sampler import FlowSampler
from .iaf_sampler_config import IAFSamplerConfig


class IAFSampler(FlowSampler):
    """Fits an inverse autoregressive flow in the latent space of a trained model (one more per private latent space).  A sample
    is one MADE pass per block (mvk_iaf_inverse); the fit runs the flow's sequential direction (mvk_iaf_fwd / mvk_iaf_bwd)."""

    flow_cls, flow_config_cls, config_cls = IAF, IAFConfig, IAFSamplerConfig
    sampler_name = "IAFsampler"
