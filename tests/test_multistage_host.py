"""MultistageTrainer's host logic on the CPU with a small plain-PyTorch plugin model (MVK_TRAINER_ALLOW_CPU=1, torch.optim.Adam
over the flat buffers): the order of the hooks, the reset at an epoch of `reset_optimizer_epochs`, the rebuild of the flat buffers
when the trainable set changes, and BaseTrainer's refusal of a multistage model.  Weight decay is on throughout: a parameter
that is not trained in a stage must not move by a bit, which only holds when it is outside the buffers (no gradient at all, not a
gradient of zeros)."""
import os

import pytest
import torch


def _model(seed=3, reset=(2,), freeze_at=3):
    from multivae_amd._output import ModelOutput
    from multivae_amd.models.base.base_config import BaseMultiVAEConfig
    from multivae_amd.models.base.base_model import BaseModel

    class TwoStage(BaseModel):
        """first: trained up to `freeze_at - 1`, frozen from `freeze_at` on (in forward, as TELBO does, and in the stage hook);
        second: trained from `freeze_at` on, unused before (it requires a gradient all along, like TELBO's unimodal encoders)."""

        def __init__(self):
            super().__init__(BaseMultiVAEConfig(n_modalities=2))
            self.model_name = "TwoStage"
            g = torch.Generator().manual_seed(seed)
            self.first = torch.nn.Linear(4, 3)
            self.second = torch.nn.Linear(3, 3)
            for p in self.parameters():
                p.data.copy_(torch.randn(p.shape, generator=g))
            self.reset_optimizer_epochs = list(reset)
            self.freeze_at = freeze_at

        def stage_parameters(self, epoch):
            if epoch < self.freeze_at:
                return list(self.first.parameters())
            self.first.requires_grad_(False)
            return list(self.second.parameters())

        def forward(self, inputs, **kwargs):
            x, y = inputs.data["a"], inputs.data["b"]
            h = self.first(x)
            if kwargs.get("epoch", 1) >= self.freeze_at:
                self.first.requires_grad_(False)
                h = self.second(h.detach())
            s = ((h - y) ** 2).sum()
            return ModelOutput(loss=s / x.shape[0], loss_sum=s, metrics=dict(rows=torch.tensor(float(x.shape[0]))))

    return TwoStage()


def _dataset(n=12):
    from multivae_amd.data.datasets.base import MultimodalBaseDataset

    g = torch.Generator().manual_seed(77)
    return MultimodalBaseDataset(dict(a=torch.randn(n, 4, generator=g), b=torch.randn(n, 3, generator=g)))


def _config(tmp_path, **kw):
    from multivae_amd.trainers import MultistageTrainerConfig

    base = dict(output_dir=str(tmp_path), num_epochs=4, per_device_train_batch_size=4, learning_rate=1e-2, no_cuda=True,
                use_fused_adam=False, optimizer_params=dict(weight_decay=0.1), scheduler_cls="StepLR",
                scheduler_params=dict(step_size=1, gamma=0.5))
    base.update(kw)
    return MultistageTrainerConfig(**base)


def _bits(module):
    return {k: v.detach().clone() for k, v in module.state_dict().items()}


def _same(a, b):
    return list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_config_is_the_reference_s():
    from multivae_amd.trainers import BaseTrainerConfig, MultistageTrainerConfig

    cfg = MultistageTrainerConfig(num_epochs=3)
    assert isinstance(cfg, BaseTrainerConfig) and cfg.name_trainer == "TwoStepsTrainerConfig" and cfg.num_epochs == 3
    assert cfg.name == "MultistageTrainerConfig"


def test_base_trainer_refuses_a_multistage_model(tmp_path, monkeypatch):
    from multivae_amd.trainers import BaseTrainer, BaseTrainerConfig, MultistageTrainer

    monkeypatch.setenv("MVK_TRAINER_ALLOW_CPU", "1")
    with pytest.raises(AttributeError, match="MultistageTrainer"):
        BaseTrainer(_model(), _dataset(), training_config=BaseTrainerConfig(output_dir=str(tmp_path), no_cuda=True))
    BaseTrainer(_model(reset=()), _dataset(), training_config=BaseTrainerConfig(output_dir=str(tmp_path), no_cuda=True))
    assert BaseTrainer.prepare_train_step(None, 3, 0.5, 0.25) == (0.5, 0.25)
    MultistageTrainer(_model(), _dataset(), training_config=_config(tmp_path))


def test_hooks_reset_and_rebuild(tmp_path, monkeypatch):
    from multivae_amd.trainers import MultistageTrainer, TrainingCallback

    monkeypatch.setenv("MVK_TRAINER_ALLOW_CPU", "1")
    log, seen = [], {}

    class Order(TrainingCallback):
        def on_epoch_begin(self, training_config, **kwargs):
            log.append(("epoch_begin", kwargs["epoch"]))

    class Traced(MultistageTrainer):
        def prepare_train_step(self, epoch, best_train_loss, best_eval_loss):
            log.append(("prepare", epoch))
            before = dict(model=self.model, optimizer=self.optimizer, scheduler=self.scheduler, flat=self.flat,
                          best=_bits(self._best_model), first=_bits(self.model.first), second=_bits(self.model.second))
            out = super().prepare_train_step(epoch, best_train_loss, best_eval_loss)
            seen[epoch] = dict(before=before, out=out, given=(best_train_loss, best_eval_loss), model=self.model, bits=_bits(self.model),
                               optimizer=self.optimizer, scheduler=self.scheduler, flat=self.flat, lr=self.optimizer.param_groups[0]["lr"],
                               state=len(self.optimizer.state), trainable=[id(p) for p in self.flat.params])
            return out

        def train_step(self, epoch):
            log.append(("train_step", epoch))
            out = super().train_step(epoch)
            seen[epoch]["after"] = dict(first=_bits(self.model.first), second=_bits(self.model.second))
            return out

    model = _model()
    trainer = Traced(model, _dataset(), training_config=_config(tmp_path), callbacks=[Order()])
    trainer.train()
    assert log == [(what, e) for e in (1, 2, 3, 4) for what in ("epoch_begin", "prepare", "train_step")]

    # epoch 1: nothing changes; the buffers hold the first stage's parameters only
    e1 = seen[1]
    assert e1["out"] == e1["given"] and e1["model"] is model and e1["flat"] is e1["before"]["flat"]
    assert e1["trainable"] == [id(p) for p in model.first.parameters()]
    assert all(p.grad is None for p in model.second.parameters())
    assert not _same(e1["after"]["first"], e1["before"]["first"])
    assert _same(e1["after"]["second"], e1["before"]["second"])  # weight decay 0.1 would have moved a gradient of zeros

    # epoch 2, in reset_optimizer_epochs: checkpoint of the best model, the model is a copy of it, fresh optimizer and scheduler
    e2 = seen[2]
    ckpt = os.path.join(trainer.training_dir, "checkpoint_epoch_1")
    assert sorted(os.listdir(ckpt)) == ["environment.json", "info_checkpoint.json", "metrics_best_model.json", "model.pt",
                                        "model_config.json", "optimizer.pt", "scheduler.pt", "training_config.json",
                                        "training_config_mvk.json"]
    assert e2["out"] == (1e12, 1e12)
    assert e2["model"] is not e2["before"]["model"] and e2["model"].training
    assert _same(e2["bits"], e2["before"]["best"])
    saved = torch.load(os.path.join(ckpt, "model.pt"), map_location="cpu")["model_state_dict"]
    assert _same({k: v for k, v in saved.items()}, e2["before"]["best"])
    assert e2["optimizer"] is not e2["before"]["optimizer"] and e2["scheduler"] is not e2["before"]["scheduler"]
    assert e2["flat"] is not e2["before"]["flat"] and e2["state"] == 0
    assert e2["lr"] == 1e-2 and seen[1]["lr"] == 1e-2  # epoch 1 ended at 5e-3: the scheduler was made anew
    assert e2["trainable"] == [id(p) for p in e2["model"].first.parameters()]
    assert trainer.callback_handler.model is trainer.model

    # epoch 3: the trainable set changes -> new buffers over `second`, the optimizer and the scheduler carry on
    e3 = seen[3]
    assert e3["out"] == e3["given"] and e3["model"] is e2["model"]
    assert e3["flat"] is not e2["flat"] and e3["optimizer"] is e2["optimizer"] and e3["scheduler"] is e2["scheduler"]
    assert e3["lr"] == 5e-3 and seen[4]["lr"] == 2.5e-3 and seen[4]["flat"] is e3["flat"]
    m = e3["model"]
    assert e3["trainable"] == [id(p) for p in m.second.parameters()]
    assert all((not p.requires_grad) and p.grad is None for p in m.first.parameters())
    for e in (3, 4):  # frozen: not a bit moves (Adam momentum of epoch 2, weight decay); the second stage trains
        assert _same(seen[e]["after"]["first"], seen[2]["after"]["first"]), e
        assert not _same(seen[e]["after"]["second"], seen[e]["before"]["second"]), e
    assert _same(seen[2]["after"]["second"], seen[2]["before"]["second"])
    # torch.optim.Adam began the second stage's state with its first gradient: 3 steps per epoch, two epochs
    steps = {k: int(trainer.optimizer.state[p]["step"]) for k, p in m.named_parameters() if p in trainer.optimizer.state}
    assert steps == {"first.weight": 3, "first.bias": 3, "second.weight": 6, "second.bias": 6}
    assert os.path.isdir(os.path.join(trainer.training_dir, "final_model"))


def test_flat_params_over_a_subset():
    from multivae_amd.trainers import FlatParams

    model = _model()
    every = FlatParams(model)
    assert [id(p) for p in every.params] == [id(p) for p in model.parameters()] and all(p.grad is not None for p in model.parameters())
    before = _bits(model)
    sub = FlatParams(model, params=list(model.second.parameters()))
    assert [id(p) for p in sub.params] == [id(p) for p in model.second.parameters()]
    assert [id(p) for p in sub.all_params] == [id(p) for p in model.parameters()]
    assert all(p.grad is None for p in model.first.parameters())
    lo, hi = sub.grad.data_ptr(), sub.grad.data_ptr() + 4 * sub.numel
    assert all(lo <= p.grad.data_ptr() < hi for p in model.second.parameters())
    assert _same(_bits(model), before)
    model.first.requires_grad_(False)
    with pytest.raises(ValueError):
        FlatParams(model, params=list(model.parameters()))  # a frozen parameter cannot be trained
    with pytest.raises(ValueError):
        FlatParams(model, params=[torch.nn.Parameter(torch.zeros(2))])
