"""Executor interface shared by the HIP (gfx950) and CPU-reference backends."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from .plan import Plan


@dataclass
class DeviceData:
    """A dataset resident on the executor's device (whole set, uploaded once)."""
    x: torch.Tensor          # executor-specific layout
    y: torch.Tensor          # [N, C] fp32 targets (one-hot for categorical)
    n: int
    w: Optional[torch.Tensor] = None   # [N] fp32 per-sample loss weights (None = unweighted)


def prepare_targets(y: np.ndarray, plan: Plan) -> np.ndarray:
    y = np.asarray(y)
    head = plan.head
    if head.loss == "sparse_categorical_crossentropy":
        yi = y.reshape(-1).astype(np.int64)
        out = np.zeros((yi.shape[0], head.N), np.float32)
        out[np.arange(yi.shape[0]), yi] = 1.0
        return out
    y = y.astype(np.float32)
    if y.ndim == 1:
        y = y.reshape(-1, 1)
    if y.shape[1] != head.N:
        raise ValueError("targets have %d columns, model outputs %d" % (y.shape[1], head.N))
    return np.ascontiguousarray(y)


def standardize_weights(y, n: int, sample_weight=None, class_weight=None) -> Optional[np.ndarray]:
    """Per-sample loss weights [n] fp32 from Keras' ``sample_weight`` / ``class_weight``
    (Keras 2.2.4 ``standardize_weights``), or None when neither is given.

    ``sample_weight``: 1-D, one entry per sample.  ``class_weight``: dict class -> weight; a
    row's class is the argmax of a multi-column target or int(y) of a one-column one, and every
    class present in ``y`` must be in the dict.  Both given: the product."""
    w = None
    if sample_weight is not None:
        w = np.asarray(sample_weight, dtype=np.float32)
        if w.ndim != 1:
            raise ValueError("sample_weight must be 1-D (one weight per sample), got shape %s" % (w.shape,))
        if w.shape[0] != n:
            raise ValueError("sample_weight has %d entries for %d samples" % (w.shape[0], n))
    if class_weight is not None:
        if not isinstance(class_weight, dict):
            raise ValueError("class_weight must be a dict {class: weight}")
        if y is None:
            raise ValueError("class_weight needs targets")
        ya = np.asarray(y)
        if ya.ndim > 2:
            raise ValueError("class_weight not supported for %d-D targets" % ya.ndim)
        cls = ya.argmax(axis=1) if (ya.ndim == 2 and ya.shape[1] > 1) else ya.reshape(-1).astype(np.int64)
        if cls.shape[0] != n:
            raise ValueError("targets have %d rows for %d samples" % (cls.shape[0], n))
        missing = set(np.unique(cls).tolist()) - set(int(k) for k in class_weight.keys())
        if missing:
            raise ValueError("class_weight must contain all classes in the data; the classes %s exist in the "
                             "data but not in class_weight" % sorted(missing))
        lut = {int(k): float(v) for k, v in class_weight.items()}
        cw = np.asarray([lut[int(c)] for c in cls], dtype=np.float32)
        w = cw if w is None else w * cw
    return None if w is None else np.ascontiguousarray(w, dtype=np.float32)


def warmup_lr(g: int, spe: int, size: int, epochs: float, base: float) -> float:
    """LR of 0-based warmup step g: ramps linearly from ~base/size to base over
    ``epochs * spe`` steps (Goyal et al. 2017 gradual warmup; the same schedule the device
    bookkeeping computes, misc.hip step_bookkeeping)."""
    return base / size * ((g + 1) / spe * (size - 1) / epochs + 1.0)


class Executor:
    """Runs training / evaluation steps of a compiled Plan on one device."""

    device: torch.device

    def __init__(self, plan: Plan, store, optimizer, seed: int):
        self.plan = plan
        self.store = store
        self.optimizer = optimizer
        self.seed = int(seed) & 0xFFFFFFFF
        self.reducer = None          # data-parallel gradient reducer (parallel.dist)
        self.lr_warmup = None        # (t0, steps, spe, size, epochs, base) device LR schedule
        # the ROC metrics (metrics.py): off unless configure_metrics asks for one
        self.roc_on = False          # auc / purity / efficiency or a weighted metric is compiled in
        self.roc_weighted = False    # ... a weighted one: weighted data feeds the weighted set too

    # learning-rate schedule ---------------------------------------------------------------
    def set_lr_warmup(self, t0: int, steps: int, spe: int, size: int, epochs: float, base: float) -> None:
        """Gradual LR warmup evaluated per step by the executor itself (no per-batch host
        write): optimizer step g = iterations - t0 - 1 < steps uses
        ``warmup_lr(g, ...)`` as its base LR (``parallel.callbacks.LearningRateWarmupCallback``)."""
        self.lr_warmup = (int(t0), int(steps), int(spe), int(size), float(epochs), float(base)) if steps > 0 else None

    def base_lr_for_step(self, t: int, host_lr: float) -> float:
        """Base LR of optimizer iteration ``t`` (1-based), before Keras ``decay``."""
        w = self.lr_warmup
        if w is not None:
            t0, steps, spe, size, epochs, base = w
            g = t - t0 - 1
            if 0 <= g < steps:
                return warmup_lr(g, spe, size, epochs, base)
        return host_lr

    # data ---------------------------------------------------------------------------------
    def upload(self, x: np.ndarray, y: Optional[np.ndarray], w: Optional[np.ndarray] = None) -> DeviceData:
        """``w``: per-sample loss weights [N] (standardize_weights), None = unweighted."""
        raise NotImplementedError

    # steps --------------------------------------------------------------------------------
    def train_step(self, data: DeviceData, perm: torch.Tensor, pos: int, bs: int) -> None:
        raise NotImplementedError

    def train_steps(self, data: DeviceData, perm: torch.Tensor, pos: int, bs: int, k: int) -> None:
        """``k`` consecutive full batches starting at ``pos`` (backends may fuse them)."""
        for i in range(k):
            self.train_step(data, perm, pos + i * bs, bs)

    def eval_step(self, data: DeviceData, pos: int, bs: int) -> None:
        raise NotImplementedError

    def predict_step(self, data: DeviceData, pos: int, bs: int) -> torch.Tensor:
        raise NotImplementedError

    # metrics ------------------------------------------------------------------------------
    def reset_metrics(self) -> None:
        raise NotImplementedError

    def read_metrics(self):
        """(mean_loss, mean_acc, count) since the last reset; synchronises."""
        raise NotImplementedError

    def last_batch_metrics(self):
        raise NotImplementedError

    def configure_metrics(self, names, weighted_names) -> None:
        """The canonical metric names of Model.compile (``metrics`` / ``weighted_metrics``), before the
        first step.  Anything beyond the plain accuracy turns the ROC state on: the steps then
        accumulate the score histograms and confusion sums of metrics.py."""
        self.roc_weighted = bool(weighted_names)
        self.roc_on = self.roc_weighted or any(n != "acc" for n in names)
        if self.roc_on:
            self._init_roc()

    def _init_roc(self) -> None:
        raise NotImplementedError

    def roc_shift(self, data: DeviceData) -> int:
        """The fixed-point shift k of a weighted data set (sum(w) * 2^k <= 2^61), found once per set;
        ValueError for negative or non-finite weights."""
        k = getattr(data, "_roc_k", None)
        if k is None:
            from ..metrics import BAD_WEIGHTS, weight_shift
            w = data.w.detach()
            if w.numel() and (not bool(torch.isfinite(w).all()) or bool((w < 0).any())):
                raise ValueError(BAD_WEIGHTS)
            k = data._roc_k = weight_shift(float(w.double().sum()))
        return k

    def extra_metrics(self) -> dict:
        """{name: value} of the ROC metrics since the last reset ('acc', 'auc', 'purity', 'efficiency'
        and their 'weighted_' twins, as far as the head defines them); synchronises."""
        raise NotImplementedError

    # params -------------------------------------------------------------------------------
    def params_changed(self) -> None:
        """Called after the host overwrote master weights (set_weights/load/broadcast)."""

    def optimizer_state(self):
        """List of flat fp32 slot tensors (Keras optimizer weights, minus iterations)."""
        raise NotImplementedError

    def set_optimizer_state(self, iterations: int, slots) -> None:
        raise NotImplementedError

    def synchronize(self) -> None:
        pass
