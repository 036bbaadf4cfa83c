"""What BCVAETrainer and UNetTrainer share: the optimizer's settings and its per-step scalars, the access to the copies of the trainable
tensors, and the checks on an epoch's accumulated losses.  Both contexts run the same update (said_amd/csrc/train_opt.hip)."""
from __future__ import annotations

from collections import OrderedDict
from typing import List, Optional, Tuple

import numpy as np
import torch

from .. import _engine
from ..util.scheduler import constant_with_warmup_lambda, ema_decay

# the optimizer's slots of the step record are the same in both contexts (SAID_TRAIN_S_* and SAID_UT_S_*)
assert all(getattr(_engine, "TRAIN_S_" + n) == getattr(_engine, "UT_S_" + n)
           for n in ("LR", "WD_FACTOR", "STEP_SIZE", "BC2_SQRT", "EMA_OMD", "OMB1", "B2", "OMB2", "EPS", "USE_EMA"))


def parse_std(std) -> Optional[np.ndarray]:
    """The coefficient std (32,) that reweights the losses, or None."""
    if std is None:
        return None
    s = np.asarray(torch.as_tensor(std, dtype=torch.float32).reshape(-1), dtype=np.float32)
    if s.size != 32:
        raise ValueError(f"the coefficient std must have 32 values (one per blendshape), got {s.size}")
    return s


class TrainerBase:
    """A trainer over one engine context `self.eng` (a said_amd._engine._TrainContext).  The subclass sets `eng` and `_shapes` (name -> shape of
    every tensor of the context) and, where not every tensor is trainable, `param_names`."""

    def _set_optimizer(self, learning_rate: float, num_warmup_steps: float, weight_decay: float, betas: Tuple[float, float], eps: float, ema: bool,
                       decay: float) -> None:
        self.base_lr, self.weight_decay, self.betas, self.adam_eps = float(learning_rate), float(weight_decay), tuple(betas), float(eps)
        self.ema, self.ema_decay = bool(ema), float(decay)
        self.lr_lambda = constant_with_warmup_lambda(num_warmup_steps)

    @property
    def names(self) -> List[str]:
        return [t[0] for t in self.eng.tensors]

    @property
    def param_names(self) -> List[str]:
        return self.names

    def _get(self, which: int, name: str) -> torch.Tensor:
        shape = self._shapes[name]
        return torch.from_numpy(self.eng.get_tensor(which, name, int(np.prod(shape)))).reshape(shape)

    def parameters_of(self, which: int) -> "OrderedDict[str, torch.Tensor]":
        """One copy of every trainable tensor: the context's STATE, EMA, GRAD, EXP_AVG or EXP_AVG_SQ (_engine.TRAIN_* / UT_*)."""
        return OrderedDict((n, self._get(which, n)) for n in self.param_names)

    def lr_at(self, k: int) -> float:
        return self.base_lr * self.lr_lambda(k)

    def _optimizer_scalars(self, k: int) -> np.ndarray:
        """The step record of optimizer step k (0-based) with the optimizer's slots filled, in double as torch / diffusers compute them; the
        caller adds its own slots and casts to float32."""
        b1, b2 = self.betas
        lr = self.lr_at(k)
        n = k + 1
        s = np.zeros(_engine.TRAIN_NSCAL, dtype=np.float64)
        s[_engine.TRAIN_S_LR] = lr
        s[_engine.TRAIN_S_WD_FACTOR] = 1 - lr * self.weight_decay
        s[_engine.TRAIN_S_STEP_SIZE] = lr / (1 - b1 ** n)
        s[_engine.TRAIN_S_BC2_SQRT] = (1 - b2 ** n) ** 0.5
        s[_engine.TRAIN_S_EMA_OMD] = 1 - ema_decay(n, self.ema_decay)
        s[_engine.TRAIN_S_OMB1] = 1 - b1
        s[_engine.TRAIN_S_B2] = b2
        s[_engine.TRAIN_S_OMB2] = 1 - b2
        s[_engine.TRAIN_S_EPS] = self.adam_eps
        s[_engine.TRAIN_S_USE_EMA] = 1.0 if self.ema else 0.0
        return s

    def _epoch_sums(self, val: bool) -> np.ndarray:
        """The accumulated losses since the last call (times the batch size; [4]: the samples), zeroed afterwards."""
        acc, status = self.eng.read_losses(val, reset=True)
        if status != _engine.TRAIN_OK:
            raise FloatingPointError(f"{int(acc[5])} {'validation' if val else 'training'} step(s) had a non-finite loss")
        if acc[4] <= 0:
            raise ValueError("no samples in the epoch")
        return acc

    def close(self) -> None:
        self.eng.close()
