"""MultistageTrainer (`multivae/trainers/multistage/multistage_trainer.py`): BaseTrainer for the models that train in stages.

Two things happen between epochs (`prepare_train_step`):

* at an epoch of `model.reset_optimizer_epochs` the reference's reset (:53-71): the best model so far is checkpointed and becomes
  the model, the optimizer and the scheduler are made anew, both best losses become 1e12;
* when the set of parameters that receive gradients changes (TELBO freezes its joint encoder and decoders behind the warm-up) the
  flat buffers and the fused Adam follow it.  The reference's `torch.optim.Adam` gets there by itself — it skips a parameter
  without a gradient and starts a parameter's state at its first one; here the frozen parameters leave the buffers (no residual
  momentum and no weight decay can move them), the newly trained ones start from step 0 and zero moments, and the learning rate
  and the scheduler carry on.  A model says which parameters an epoch trains through `stage_parameters(epoch)`; without that
  hook it is the parameters that require a gradient when the epoch begins.

Either way every captured graph is dropped: it replays the old model object on the old buffers."""
import json
import logging
import os
from copy import deepcopy
from typing import List, Optional

from ..base import BaseTrainer, TrainingCallback
from ..flat import FlatParams, FusedAdam
from .multistage_trainer_config import MultistageTrainerConfig

logger = logging.getLogger(__name__)


class MultistageTrainer(BaseTrainer):
    def __init__(self, model, train_dataset, eval_dataset=None, training_config: Optional[MultistageTrainerConfig] = None,
                 callbacks: List[TrainingCallback] = None, checkpoint: str = None):
        if training_config is None and checkpoint is not None:  # resuming: the configuration saved with the checkpoint
            cfg_file = os.path.join(checkpoint, "training_config.json")
            if os.path.exists(cfg_file):
                training_config = MultistageTrainerConfig.from_json_file(cfg_file)
        if training_config is None:
            training_config = MultistageTrainerConfig()
        self._stage_epoch = 1
        super().__init__(model, train_dataset, eval_dataset, training_config, callbacks, checkpoint)

    def checktrainer(self, model):
        return

    def _trainable_params(self):
        hook = getattr(self.model, "stage_parameters", None)
        return hook(self._stage_epoch) if hook is not None else None

    def resume_training(self, checkpoint):
        """The buffers are built over the trainable set of the epoch the run continues with, BEFORE `optimizer.pt` is read."""
        with open(os.path.join(checkpoint, "info_checkpoint.json"), "r") as fp:
            self._stage_epoch = json.load(fp)["trained_epochs"] + 1
        super().resume_training(checkpoint)

    def _drop_captured(self):
        self._drain_rotation()
        self.__dict__.pop("_graphs", None)
        self.__dict__.pop("_graph_tail", None)

    def prepare_train_step(self, epoch, best_train_loss, best_eval_loss):
        self._stage_epoch = epoch
        if epoch in getattr(self.model, "reset_optimizer_epochs", ()):
            logger.info(f"Epoch {epoch} : reset the optimizer and losses.")
            logger.info("Keeping the best model obtained until here for the rest of training.")
            self._drop_captured()
            if self.is_main_process:
                self.save_checkpoint(self._best_model, self.training_dir, epoch - 1)
            if self.distributed and self.flat is not None:
                self.flat.close()  # every rank resets at the same epoch: the next collective makes the communicator anew
            self.model = deepcopy(self._best_model).train()
            self.callback_handler.model = self.model
            self.set_optimizer()
            self.set_scheduler()
            return 1e12, 1e12
        self._follow_trainable_set()
        return best_train_loss, best_eval_loss

    def _follow_trainable_set(self):
        want = self._trainable_params()
        if want is None:
            want = [p for p in self.model.parameters() if p.requires_grad]
        if [id(p) for p in want] == [id(p) for p in self.flat.params]:
            return
        logger.info(f"Epoch {self._stage_epoch} : {len(want)} of {len(self.flat.all_params)} parameters train from here on.")
        self._drop_captured()
        if self.distributed:
            self.flat.close()
        self.flat = FlatParams(self.model, params=want)
        if isinstance(self.optimizer, FusedAdam):
            self.optimizer.rebind(self.flat)
