"""MAFSampler, IAFSampler and samplers/flow_fit.py on the host (the torch-module path): configs, refusals, the unfitted sampler,
shapes and keys of `sample`, its batching, save -> load_flows_from_folder, a bad folder, an evaluator that takes the fitted
sampler, which fields of the trainer config the fit honours or refuses, the best-epoch rule, and the learning condition.

The learning condition is stated in tests/flow_samplers_ref.py; tests/test_gpu_flow_samplers.py repeats it on the fused path with
the same data, seed and configuration."""
import json
import os

import pytest
import torch

from flow_samplers_ref import DIMS, KINDS, check_learning, classes, eval_nll, fit_config, learning_setup, two_modalities


class TinyModel(torch.nn.Module):
    """What the samplers touch of a model, in plain torch (the package's models encode on the GPU only: tests/test_gpu_flow_samplers.py
    runs MVAE and DMVAE through both paths): `model_config.latent_dim`, `multiple_latent_spaces`, `style_dims`, `encoders`,
    `encode` and `decode`.  Two modalities, a shared space of 4 and, with `private`, style spaces of 2 and 3 dimensions."""

    def __init__(self, private, seed=0):
        from multivae_amd.models import MVAEConfig

        super().__init__()
        torch.manual_seed(seed)
        self.model_config = MVAEConfig(n_modalities=2, latent_dim=4, input_dims=DIMS)
        self.multiple_latent_spaces = private
        self.style_dims = dict(a=2, b=3) if private else None
        self.n_modalities = 2
        self.encoders = torch.nn.ModuleDict(dict(a=torch.nn.Linear(12, 4 + 2), b=torch.nn.Linear(10, 4 + 3)))
        self.decoders = torch.nn.ModuleDict(dict(a=torch.nn.Linear(4 + 2, 12), b=torch.nn.Linear(4 + 3, 10)))

    def encode(self, inputs, **kwargs):
        from multivae_amd._output import ModelOutput

        h = {m: self.encoders[m](inputs.data[m].flatten(1)) for m in self.encoders}
        out = ModelOutput(z=h["a"][:, :4] + h["b"][:, :4], one_latent_space=not self.multiple_latent_spaces)
        if self.multiple_latent_spaces:
            out["modalities_z"] = {m: h[m][:, 4:] for m in h}
        return out

    def decode(self, embedding, modalities="all", **kwargs):
        rec = {}
        for m, shape in DIMS.items():
            style = embedding.modalities_z[m] if self.multiple_latent_spaces else embedding.z.new_zeros(len(embedding.z), self.decoders[m].in_features - 4)
            rec[m] = self.decoders[m](torch.cat([embedding.z, style], 1)).reshape(-1, *shape)
        return rec


def tiny_model(private, seed=0):
    return TinyModel(private, seed)


# ---- configs and construction ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_config_and_unfitted_sampler(kind, tmp_path):
    Sampler, Config, Flow, _ = classes(kind)
    cfg = Config()
    assert (cfg.n_made_blocks, cfg.n_hidden_in_made, cfg.hidden_size, cfg.include_batch_norm) == (2, 3, 128, False)
    assert cfg.name == Config.__name__
    model = tiny_model(private=True)
    sampler = Sampler(model, Config(n_made_blocks=1, n_hidden_in_made=2, hidden_size=8))
    assert sampler.name == dict(maf="MAFsampler", iaf="IAFsampler")[kind] and sampler.is_fitted is False and not model.training
    assert sampler.flows_dims == dict(shared=4, a=2, b=3) and set(sampler.flows_models) == {"shared", "a", "b"}
    for key, flow in sampler.flows_models.items():
        assert type(flow) is Flow and flow.input_dim == (sampler.flows_dims[key],) and len(flow.net) == 1
    assert set(Sampler(tiny_model(private=False)).flows_models) == {"shared"}
    with pytest.raises(ArithmeticError, match="needs to be fitted"):
        sampler.sample(3)
    with pytest.raises(ArithmeticError, match="needs to be fitted"):
        sampler.save(str(tmp_path / "s"))
    with pytest.raises(NotImplementedError, match="include_batch_norm"):
        Sampler(model, Config(include_batch_norm=True))
    path = os.path.join(str(tmp_path / "s"), "sampler_config.json")  # written before the refusal, as in the reference
    assert json.load(open(path)) == {"name": Config.__name__, "n_made_blocks": 1, "n_hidden_in_made": 2, "hidden_size": 8,
                                     "include_batch_norm": False}


# ---- fit, sample, save, load ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("private", [False, True], ids=["shared", "private"])
@pytest.mark.parametrize("kind", KINDS)
def test_fit_sample_save_load(kind, private, tmp_path):
    from multivae_amd.metrics.base import Evaluator, EvaluatorConfig

    Sampler, Config, _, _ = classes(kind)
    model = tiny_model(private)
    config = Config(n_made_blocks=2, n_hidden_in_made=1, hidden_size=8)
    sampler = Sampler(model, config)
    before = {k: [p.detach().clone() for p in f.parameters()] for k, f in sampler.flows_models.items()}
    sampler.fit(two_modalities(70), eval_data=two_modalities(30, seed=1), training_config=fit_config())
    assert sampler.is_fitted
    for key, flow in sampler.flows_models.items():
        assert any(not torch.equal(p, q) for p, q in zip(flow.parameters(), before[key])), key
        h = sampler.fit_history[key]
        assert len(h["train_loss"]) == len(h["eval_loss"]) == 2 and h["fused"] is False
        assert h["best_epoch"] == min(range(2), key=lambda e: h["eval_loss"][e])
    dev = torch.device(sampler.device)
    out = sampler.sample(7, batch_size=3, generator=torch.Generator(device=dev).manual_seed(3))  # 3 + 3 + 1 rows
    assert out.z.shape == (7, 4) and out.one_latent_space == (not private) and bool(torch.isfinite(out.z).all())
    if private:
        assert set(out.keys()) == {"z", "one_latent_space", "modalities_z"}
        assert out.modalities_z["a"].shape == (7, 2) and out.modalities_z["b"].shape == (7, 3)
    else:
        assert set(out.keys()) == {"z", "one_latent_space"}
    rec = model.decode(out)
    assert rec["a"].shape == (7, 12) and rec["b"].shape == (7, 2, 5)
    # the batches draw from the generator in order: space by space within a batch
    g = torch.Generator(device=dev).manual_seed(3)
    first = {k: torch.randn(3, d, generator=g, device=dev) for k, d in sampler.flows_dims.items()}
    with torch.no_grad():
        assert torch.equal(out.z[:3], sampler.flows_models["shared"].inverse(first["shared"]).out)
    # save -> a new sampler -> load: identical samples under the same generator
    folder = str(tmp_path / "saved")
    sampler.save(folder)
    for key in sampler.flows_models:
        assert sorted(os.listdir(os.path.join(folder, key))) == ["model.pt", "model_config.json"]
        state = torch.load(os.path.join(folder, key, "model.pt"), weights_only=True)
        assert set(state) == {"model_state_dict"} and set(state["model_state_dict"]) == set(sampler.flows_models[key].state_dict())
    again = Sampler(model, config)
    again.load_flows_from_folder(folder)
    assert again.is_fitted
    out2 = again.sample(7, batch_size=3, generator=torch.Generator(device=dev).manual_seed(3))
    assert torch.equal(out2.z, out.z)
    if private:
        assert all(torch.equal(out2.modalities_z[m], out.modalities_z[m]) for m in ("a", "b"))
    with pytest.raises(AttributeError, match="Error when trying to load the flows from the folder."):
        Sampler(model, config).load_flows_from_folder(str(tmp_path / "nothing-here"))
    # an evaluator takes the fitted sampler and refuses an unfitted one
    ev = Evaluator(model, two_modalities(6), None, EvaluatorConfig(), sampler=sampler)
    assert ev.sampler is sampler
    ev.finish()
    with pytest.raises(AttributeError, match="not fitted"):
        Evaluator(model, two_modalities(6), None, EvaluatorConfig(), sampler=Sampler(model, config))


# ---- the fit ----------------------------------------------------------------------------------------------------------------------------
def test_fit_config_refusals_and_rules(tmp_path):
    from multivae_amd.models.nn.flows import MAF, MAFConfig
    from multivae_amd.samplers.flow_fit import batch_order, fit_flow, load_flow

    def flow():
        torch.manual_seed(3)
        return MAF(MAFConfig(input_dim=(3,), n_made_blocks=1, n_hidden_in_made=1, hidden_size=5))

    x = torch.randn(50, 3, generator=torch.Generator().manual_seed(0)) * 2 + 1
    for kw, name in [(dict(optimizer_cls="SGD"), "optimizer_cls"), (dict(optimizer_params=dict(amsgrad=True)), "amsgrad"),
                     (dict(scheduler_cls="StepLR", scheduler_params=dict(step_size=1)), "scheduler_cls"),
                     (dict(gradient_clipping_max_norm=1.0), "gradient_clipping_max_norm"), (dict(steps_saving=1), "steps_saving"),
                     (dict(steps_predict=1), "steps_predict"), (dict(use_hip_graph=True), "use_hip_graph"),
                     (dict(world_size=2), "world_size")]:
        with pytest.raises(NotImplementedError, match=name):
            fit_flow(flow(), x, training_config=fit_config(**kw))
    with pytest.raises(ValueError, match=r"\[N, D\]"):
        fit_flow(flow(), x[0], training_config=fit_config())
    with pytest.raises(ValueError, match="fused=True"):
        fit_flow(flow(), x, training_config=fit_config(), fused=True)  # the codes are on the CPU
    # the batches: a seeded permutation, the last one short (or dropped)
    g = torch.Generator().manual_seed(5)
    order = batch_order(50, 32, g)
    assert [b.numel() for b in order] == [32, 18] and sorted(torch.cat(order).tolist()) == list(range(50))
    assert [b.numel() for b in batch_order(50, 32, g, drop_last=True)] == [32]
    assert torch.equal(torch.cat(batch_order(50, 32, torch.Generator().manual_seed(5))), torch.cat(order))
    # the loss: the batch's summed rows, the epoch's mean over batches; one step by hand under torch.optim.Adam
    from multivae_amd.samplers.flow_fit import nll_rows

    f1, f2 = flow(), flow()
    h = fit_flow(f1, x, training_config=fit_config(num_epochs=1, optimizer_params=dict(betas=(0.8, 0.9), eps=1e-6)), max_steps=2)
    opt = torch.optim.Adam(f2.parameters(), lr=1e-3, betas=(0.8, 0.9), eps=1e-6)
    shuffled = x[torch.cat(order)]
    sums = []
    for xb in (shuffled[:32], shuffled[32:]):
        opt.zero_grad()
        loss = nll_rows(f2, xb).sum()
        loss.backward()
        opt.step()
        sums.append(float(loss.detach()))
    assert [float(v) for v in h["step_loss"]] == pytest.approx(sums, rel=1e-6)
    assert h["train_loss"] == pytest.approx([sum(sums) / 2], rel=1e-6)
    assert all(torch.allclose(p, q, rtol=0, atol=1e-7) for p, q in zip(f1.parameters(), f2.parameters()))
    # best epoch: without eval codes the lowest train loss; the flow is left with that epoch's parameters; same seed, same fit
    f3, f4 = flow(), flow()
    cfg = fit_config(num_epochs=6, learning_rate=0.3, output_dir=str(tmp_path / "out"))  # a rate that overshoots: not monotone
    h3 = fit_flow(f3, x, training_config=cfg)
    assert h3["eval_loss"] is None and h3["best_epoch"] == min(range(6), key=lambda e: h3["train_loss"][e])
    h4 = fit_flow(f4, x, training_config=fit_config(num_epochs=h3["best_epoch"] + 1, learning_rate=0.3))
    assert h4["train_loss"] == h3["train_loss"][: h3["best_epoch"] + 1]
    assert h4["best_epoch"] == h3["best_epoch"] and all(torch.equal(p, q) for p, q in zip(f3.parameters(), f4.parameters()))
    saved = load_flow(MAF, MAFConfig, str(tmp_path / "out"))  # output_dir set: the fitted flow is written there
    assert all(torch.equal(p, q) for p, q in zip(saved.parameters(), f3.parameters()))
    # with eval codes the eval loss decides, unless keep_best_on_train
    h5 = fit_flow(flow(), x, x[:20] * 3, training_config=fit_config(num_epochs=4, learning_rate=0.3))
    assert h5["best_epoch"] == min(range(4), key=lambda e: h5["eval_loss"][e])
    h6 = fit_flow(flow(), x, x[:20] * 3, training_config=fit_config(num_epochs=4, learning_rate=0.3, keep_best_on_train=True))
    assert h6["best_epoch"] == min(range(4), key=lambda e: h6["train_loss"][e]) and h6["train_loss"] == h5["train_loss"]


@pytest.mark.parametrize("kind", KINDS)
def test_learning_condition(kind):
    from multivae_amd.samplers.flow_fit import fit_flow

    flow, train, evals, cfg = learning_setup(kind)
    before = eval_nll(flow, evals)
    hist = fit_flow(flow, train, evals, training_config=cfg)
    assert hist["fused"] is False
    check_learning(flow, evals, before, hist)
