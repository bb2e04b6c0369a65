"""Fit one normalizing flow (models/nn/flows.py: MAF or IAF) to latent codes that already sit on the device, by maximum likelihood
under N(0, I).  The reference hands the codes to pythae's `BaseTrainer` around an `NFModel`; here there is no data loader and no
output directory (unless `output_dir` is set), and the codes never leave the device.

Fused path (codes on the GPU, `kernels.maf_fused_ok` / `iaf_fused_ok`): one step is four launches — the flow's forward with the NLL
rows, the data backward, the weight sums, and one fused Adam launch over a flat buffer that the flow's parameters are views of.  No
host synchronisation inside an epoch: the epoch's loss is reduced once, at its end.  Otherwise the flow runs as a torch module
under `torch.optim.Adam`, with the same batches.

Loss: the SUM over the batch of the NLL rows -(log N(flow(x); 0, I) + log|det J|), as pythae's `NFModel` returns it; the epoch's
loss is the mean over its batches.  As pythae's trainer does, the parameters of the best epoch are what the fit leaves in the flow:
best = lowest eval epoch loss, or lowest train epoch loss without eval codes (or with `keep_best_on_train`)."""
import logging
import os

import torch

from .. import kernels as K
from ..models.nn.flows import IAF, MAF, fused_layout
from ..trainers.base.base_trainer_config import BaseTrainerConfig

logger = logging.getLogger(__name__)

LOG_2PI = 1.8378770664093453
_ADAM_PARAMS = ("betas", "eps", "weight_decay")


def nll_rows(flow, x):
    """The rows of the loss through the torch module: -(log N(flow(x); 0, I) + log|det J|), [B]."""
    out = flow(x)
    return 0.5 * (out.out ** 2 + LOG_2PI).sum(-1) - out.log_abs_det_jac


def _check_config(cfg, device):
    """Refuse by name what this fit cannot honour."""
    if cfg.optimizer_cls != "Adam":
        raise NotImplementedError(f"flow fit: optimizer_cls='{cfg.optimizer_cls}' is not built here (supported: 'Adam')")
    for k in (cfg.optimizer_params or {}):
        if k not in _ADAM_PARAMS:
            raise NotImplementedError(f"flow fit: optimizer_params['{k}'] is not built here (supported: {', '.join(_ADAM_PARAMS)})")
    for name, off in (("scheduler_cls", None), ("gradient_clipping_max_norm", None), ("steps_saving", None), ("steps_predict", None),
                      ("use_hip_graph", False)):
        if getattr(cfg, name) != off:
            raise NotImplementedError(f"flow fit: {name}={getattr(cfg, name)!r} is not built here")
    if cfg.world_size > 1:
        raise NotImplementedError(f"flow fit: world_size={cfg.world_size} is not built here (the fit runs on one device)")
    if cfg.no_cuda and device.type == "cuda":
        raise NotImplementedError("flow fit: no_cuda=True with codes on the GPU: the fit runs where the codes are")


def flow_dims(flow):
    """(dims, Ws, bs) of the fused kernels for a MAF / IAF they can stand in for, else None."""
    lay = fused_layout(flow, type(flow)) if type(flow) in (MAF, IAF) else None
    if lay is None:
        return None
    D, H, n_hidden, n_blocks, layers = lay
    ok = K.maf_fused_ok(D, H, n_hidden, n_blocks) if type(flow) is MAF else K.iaf_fused_ok(D, H, n_hidden, n_blocks)
    if not ok:
        return None
    return (n_blocks, n_hidden, D, H), [m.weight for m in layers], [m.bias for m in layers]


class _Fused:
    """The flow's parameters as views of one flat buffer, with flat gradient and Adam moments beside it."""

    def __init__(self, flow, dims, Ws, bs, cfg):
        self.flow, self.dims, self.kind = flow, dims, type(flow)
        params = [p for pair in zip(Ws, bs) for p in pair]
        n = sum(p.numel() for p in params)
        dev = params[0].device
        self.p = torch.empty(n, dtype=torch.float32, device=dev)
        self.g, self.m, self.v = torch.zeros_like(self.p), torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.gW, self.gb, at = [], [], 0
        for i, q in enumerate(params):
            view = self.p[at:at + q.numel()].view(q.shape)
            view.copy_(q.detach())
            q.data = view
            (self.gW if i % 2 == 0 else self.gb).append(self.g[at:at + q.numel()].view(q.shape))
            at += q.numel()
        self.Ws, self.bs = [w.detach() for w in Ws], [b.detach() for b in bs]
        opt = dict(cfg.optimizer_params or {})
        self.lr, self.betas = float(cfg.learning_rate), tuple(opt.get("betas", (0.9, 0.999)))
        self.eps, self.wd = float(opt.get("eps", 1e-8)), float(opt.get("weight_decay", 0.0))
        self.steps = 0
        self.ones = self.zeros = self.deltas = None

    def _consts(self, x):
        B, D = x.shape
        if self.ones is None or self.ones.shape[-1] < B:
            self.ones = torch.ones(1, B, dtype=torch.float32, device=x.device)
            self.zeros = torch.zeros(B, D, dtype=torch.float32, device=x.device)
        return self.ones[:, :B], self.zeros[:B]

    def rows(self, x, keep=False):
        """-> rows [B] (and what the backward needs)."""
        ones, zeros = self._consts(x)
        if self.kind is MAF:
            z0, _, rows, ws = K.maf_forward(x, self.dims, self.Ws, self.bs, [zeros], [zeros], keep=keep)
            return rows[0], (z0, ws, zeros, ones)
        z0, _, rows, ws = K.iaf_forward(x, self.dims, self.Ws, self.bs, want_rows=True, keep=keep)
        return rows, (z0, ws, zeros, ones)

    def step(self, x):
        """Forward, data backward, weight sums, Adam: four launches.  -> the NLL rows of the batch (before the update)."""
        rows, (z0, ws, zeros, ones) = self.rows(x, keep=True)
        if self.kind is MAF:
            K.maf_backward(self.dims, self.Ws, z0, ws, [zeros], [zeros], grows=ones.contiguous(), dWs=self.gW, dbs=self.gb)
        else:
            if self.deltas is None or self.deltas.numel() != ws.numel():
                self.deltas = torch.empty_like(ws)
            K.iaf_backward(self.dims, self.Ws, z0, ws, grows=ones[0].contiguous(), dWs=self.gW, dbs=self.gb, deltas=self.deltas)
        self.steps += 1
        K.adam_step(self.p, self.g, self.m, self.v, self.steps, self.lr, self.betas[0], self.betas[1], self.eps, self.wd,
                    zero_grad=True)
        return rows


class _Module:
    """The torch path: the flow as a module under torch.optim.Adam."""

    def __init__(self, flow, cfg):
        self.flow = flow
        self.params = [p for p in flow.parameters() if p.requires_grad]
        self.opt = torch.optim.Adam(self.params, lr=cfg.learning_rate, **dict(cfg.optimizer_params or {}))

    def rows(self, x, keep=False):
        with torch.set_grad_enabled(keep):
            return nll_rows(self.flow, x), None

    def step(self, x):
        self.opt.zero_grad()
        rows, _ = self.rows(x, keep=True)
        rows.sum().backward()
        self.opt.step()
        return rows.detach()


def batch_order(N, batch_size, generator, drop_last=False):
    """One epoch's batches as index tensors: a seeded permutation cut into batches (the order of a shuffling data loader)."""
    perm = torch.randperm(N, generator=generator)
    stop = N - N % batch_size if drop_last and N >= batch_size else N
    return [perm[i:i + batch_size] for i in range(0, stop, batch_size)]


def _epoch_loss(rows):
    """The mean over the batches of the batch's summed rows (one reduction, on the device)."""
    return torch.cat(rows).sum() / len(rows)


def fit_flow(flow, train_codes, eval_codes=None, training_config=None, fused=None, max_steps=None):
    """Fit `flow` (moved to the codes' device) to train_codes [N,D] in place and leave the best epoch's parameters in it.
    fused: None = the fused kernels where they apply, False = the torch module, True = the fused kernels or an error.
    max_steps (for tests): stop after that many optimizer steps.
    -> dict(train_loss=[per epoch], eval_loss=[per epoch] or None, best_epoch, step_loss=[the summed rows of every step, device
    tensors; recorded with max_steps only], fused)."""
    cfg = BaseTrainerConfig() if training_config is None else training_config
    x = train_codes.detach().float().contiguous()
    if x.dim() != 2:
        raise ValueError(f"flow fit: the codes must be [N, D], got {tuple(x.shape)}")
    dev = x.device
    _check_config(cfg, dev)
    xe = None if eval_codes is None else eval_codes.detach().float().contiguous().to(dev)
    flow.to(dev)
    flow.train()
    lay = flow_dims(flow) if dev.type == "cuda" else None
    if fused is True and lay is None:
        raise ValueError("flow fit: fused=True, but the fused kernels do not take this flow on this device")
    use_fused = lay is not None and fused is not False
    run = _Fused(flow, *lay, cfg) if use_fused else _Module(flow, cfg)
    params = [p for p in flow.parameters()]
    gen = torch.Generator().manual_seed(int(cfg.seed))
    N, bs, ebs = x.shape[0], int(cfg.per_device_train_batch_size), int(cfg.per_device_eval_batch_size)
    best, best_loss, best_epoch = None, None, -1
    hist = dict(train_loss=[], eval_loss=None if xe is None else [], best_epoch=-1, step_loss=[], fused=use_fused)
    on_train = xe is None or cfg.keep_best_on_train
    steps = 0
    for epoch in range(int(cfg.num_epochs)):
        order = batch_order(N, bs, gen, cfg.drop_last)
        shuffled = x[torch.cat(order).to(dev)]  # one gather per epoch: the batches are contiguous slices
        rows, at = [], 0
        for idx in order:
            if max_steps is not None and steps >= max_steps:
                break
            rows.append(run.step(shuffled[at:at + idx.numel()]))
            at += idx.numel()
            steps += 1
        if not rows:
            break
        if max_steps is not None:
            hist["step_loss"].extend(r.sum() for r in rows)
        train_loss = _epoch_loss(rows)
        eval_loss = None
        if xe is not None:
            with torch.no_grad():
                eval_loss = _epoch_loss([run.rows(xe[i:i + ebs])[0] for i in range(0, xe.shape[0], ebs)])
        # the one host read of the epoch: the best-epoch decision
        losses = torch.stack([train_loss] if eval_loss is None else [train_loss, eval_loss]).tolist()
        score = losses[0] if on_train else losses[1]
        hist["train_loss"].append(losses[0])
        if eval_loss is not None:
            hist["eval_loss"].append(losses[1])
        if best_loss is None or score < best_loss:
            best_loss, best_epoch = score, epoch
            if use_fused:
                best = run.p.clone() if best is None else best.copy_(run.p)
            else:
                best = [p.detach().clone() for p in params]
        if max_steps is not None and steps >= max_steps:
            break
    if best is not None:
        with torch.no_grad():
            if use_fused:
                run.p.copy_(best)
            else:
                for p, q in zip(params, best):
                    p.copy_(q)
    hist["best_epoch"] = best_epoch
    flow.eval()
    if cfg.output_dir is not None:
        save_flow(flow, cfg.output_dir)
    return hist


def save_flow(flow, dir_path):
    """`model_config.json` and `model.pt` ({"model_state_dict": ...}): the files pythae's flows save."""
    os.makedirs(dir_path, exist_ok=True)
    flow.model_config.save_json(dir_path, "model_config")
    torch.save({"model_state_dict": {k: v.detach().cpu() for k, v in flow.state_dict().items()}}, os.path.join(dir_path, "model.pt"))


def load_flow(cls, config_cls, dir_path):
    """The flow that `save_flow` wrote to dir_path."""
    config = config_cls.from_json_file(os.path.join(dir_path, "model_config.json"))
    flow = cls(config)
    state = torch.load(os.path.join(dir_path, "model.pt"), map_location="cpu", weights_only=True)
    flow.load_state_dict(state["model_state_dict"])
    return flow
