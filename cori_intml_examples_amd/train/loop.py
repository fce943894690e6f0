"""``Model.fit`` driver (Keras 2.2 ``fit_loop`` semantics, GPU-friendly).

Differences from a naive port: the dataset is uploaded to the device once, the
per-epoch shuffle is a device permutation, the per-batch step is one HIP-graph
replay on GPU, and epoch metrics accumulate on the device (one D2H per epoch).
Per-batch host syncs happen only when a callback actually consumes batch logs; without
per-batch callbacks, runs of full batches are replayed ``INTML_STEPS_PER_GRAPH`` (8) steps
per graph launch.

Reference behaviour reproduced: ``validation_split`` takes the *last* fraction
before shuffling (``DistHPO_mnist.ipynb:188,293``: 60000 -> 49800/10200), the final
partial batch is processed, ``Train on N samples, validate on M samples`` banner,
History keys ``loss, acc, val_loss, val_acc`` (+ ``lr`` from ReduceLROnPlateau; + the ROC and weighted
metrics the model was compiled with, epoch logs only).
"""
from __future__ import annotations

import os
from typing import Optional

import numpy as np
import torch

from . import callbacks as cbks


def _split_validation(x, y, validation_split, validation_data, w=None):
    """(x, y, w, vx, vy, vw): ``w`` / ``vw`` are per-sample loss weights or None.  The
    validation split slices the weights with x and y (last fraction, before shuffling)."""
    from ..models.executor_base import DeviceData
    if isinstance(x, DeviceData) and validation_data is None and validation_split and 0.0 < validation_split < 1.0:
        from ..io.synth import split
        tr, va = split(x, validation_split)
        return tr, None, None, va, None, None
    if validation_data is not None:
        vw = None
        if len(validation_data) == 3:
            vx, vy, vw = validation_data
        else:
            vx, vy = validation_data
        return x, y, w, vx, vy, vw
    if validation_split and 0.0 < validation_split < 1.0:
        n = len(x)
        split_at = int(n * (1.0 - validation_split))
        return (x[:split_at], y[:split_at], None if w is None else w[:split_at],
                x[split_at:], y[split_at:], None if w is None else w[split_at:])
    return x, y, w, None, None, None


def shard_indices(n: int, rank: int, size: int, shuffle: bool, seed: int, epoch: int) -> torch.Tensor:
    """Rank ``rank``'s sample indices for ``epoch``: its disjoint ``n // size`` slice of a
    permutation every rank draws identically (``seed`` is rank 0's, broadcast; the epoch is
    mixed in, so the shards change every epoch).  Unshuffled: the contiguous block
    ``[rank * per, (rank + 1) * per)``, the fixed-shard layout."""
    per = n // size
    if shuffle:
        g = torch.Generator(device="cpu")
        g.manual_seed((seed * 1000003 + 7919 * (epoch + 1)) & 0x7FFFFFFFFFFF)
        order = torch.randperm(n, generator=g)
    else:
        order = torch.arange(n)
    return order[rank * per:(rank + 1) * per]


def fit_loop(model, x, y, batch_size, epochs, verbose, callbacks, validation_split, validation_data,
             shuffle, initial_epoch, sample_weight=None, class_weight=None):
    from ..models.executor_base import DeviceData, standardize_weights
    from ..parallel import state as dp_state
    ex = model._executor
    if isinstance(x, DeviceData):
        x = model._upload_weighted(x, None, sample_weight, class_weight)   # (weights attached to the set)
        w = None
    else:
        w = standardize_weights(y, len(x), sample_weight, class_weight)
    x, y, w, vx, vy, vw = _split_validation(x, y, validation_split, validation_data, w)
    if vw is not None and not isinstance(vx, DeviceData):
        vw = standardize_weights(vy, len(vx), vw, None)

    # data-parallel sharding (default) or the reference's replicated semantics.  Sharded: every
    # rank keeps the WHOLE training set resident (HBM is not the constraint for these data
    # sets) and takes its disjoint 1/size slice of an epoch permutation that all ranks draw
    # from the same seed -- a distributed sampler that reshards every epoch, so the n % size
    # samples left out differ from epoch to epoch instead of being dropped for good.
    dp = dp_state.current()
    shard = None
    if dp is not None and dp.size > 1 and dp.shard_data and getattr(model.optimizer, "distributed", False):
        from ..parallel import dist as _dist
        shard = (dp.rank, dp.size, int(_dist.broadcast_object(int(model._seed) & 0x7FFFFFFF, 0)))

    # (a DeviceData -- e.g. io.synth.for_model, generated on the device -- is used as is)
    train = x if isinstance(x, DeviceData) else (ex.upload(x, y, w) if w is not None else ex.upload(x, y))
    n_local = train.n // shard[1] if shard else train.n
    if isinstance(vx, DeviceData):
        val = model._upload_weighted(vx, None, vw, None)
    elif vx is not None:
        val = ex.upload(vx, vy, vw) if vw is not None else ex.upload(vx, vy)
    else:
        val = None
    do_val = val is not None

    model.history = cbks.History()
    # DP consistency guard (the reference's own multi-rank check is identical test loss on every
    # rank, DistTrain_mnist.ipynb:526-527): a cross-rank digest of the weights at every epoch end
    check_dp = (shard is not None or (dp is not None and dp.size > 1
                                       and getattr(model.optimizer, "distributed", False)))
    check_dp = check_dp and os.environ.get("INTML_DP_CHECK", "1") not in ("0", "false", "False")
    model.history.dp_consistency = [] if check_dp else None
    progbar = cbks.ProgbarLogger() if verbose else None
    cb_list = ([progbar] if progbar else []) + list(callbacks or []) + [model.history]
    cb = cbks.CallbackList(cb_list)
    out_labels = model.metrics_names
    metrics = list(out_labels) + (["val_" + n for n in out_labels] if do_val else [])
    cb.set_model(model)
    cb.set_params({"batch_size": batch_size, "epochs": epochs, "steps": None,
                   "samples": n_local, "verbose": verbose, "do_validation": do_val,
                   "metrics": metrics, "initial_epoch": initial_epoch})
    for c in cb:
        c.validation_data = (vx, vy) if do_val else None
    model.stop_training = False
    need_batch_logs = cb.batch_logs_needed
    need_batch_begin = cb.batch_begin_needed
    steps_per_replay = max(1, int(os.environ.get("INTML_STEPS_PER_GRAPH", "8")))

    if do_val and verbose:
        print("Train on %d samples, validate on %d samples" % (n_local, val.n))
    elif verbose:
        print("Train on %d samples" % n_local)

    from ..farm.engine import should_stop as farm_should_stop
    gen = torch.Generator(device="cpu")
    gen.manual_seed((model._seed + 7919 * (dp.rank if dp is not None else 0)) & 0x7FFFFFFF)
    cb.on_train_begin()
    for epoch in range(initial_epoch, epochs):
        cb.on_epoch_begin(epoch, {})
        if shard:
            perm = shard_indices(train.n, shard[0], shard[1], shuffle, shard[2], epoch).to(ex.device)
        elif shuffle:
            perm = torch.randperm(train.n, generator=gen).to(ex.device)
        else:
            perm = torch.arange(train.n, device=ex.device)
        ex.reset_metrics()
        nb = (n_local + batch_size - 1) // batch_size
        # Without per-batch callbacks, runs of full batches go to the device as chunks of
        # `chunk` steps (one HIP-graph replay each); the partial tail batch runs alone.
        chunk = 1 if (need_batch_logs or need_batch_begin) else steps_per_replay
        b = 0
        while b < nb:
            pos = b * batch_size
            bs = min(batch_size, n_local - pos)
            k = 1
            if chunk > 1 and bs == batch_size:
                k = max(1, min(chunk, (n_local - pos) // batch_size))
            if k > 1:
                ex.train_steps(train, perm, pos, bs, k)
                b += k
                if progbar is not None and verbose == 1:
                    progbar.progress(pos + k * bs, [])
            else:
                if need_batch_begin:
                    cb.on_batch_begin(b, {"batch": b, "size": bs})
                ex.train_step(train, perm, pos, bs)
                if need_batch_logs:
                    l, a = ex.last_batch_metrics()
                    logs = {"batch": b, "size": bs, "loss": l}
                    if "acc" in out_labels:        # (batch logs stay loss / acc: no per-batch ROC metrics)
                        logs["acc"] = a
                    cb.on_batch_end(b, logs)
                if progbar is not None and verbose == 1:
                    if need_batch_logs or b == nb - 1 or b % 50 == 0:
                        progbar.progress(pos + bs, [])
                b += 1
            if farm_should_stop():      # Stop button / AsyncResult.abort on a farm engine
                model.stop_training = True
            if model.stop_training:
                break
        loss, acc, _ = ex.read_metrics()
        epoch_logs = dict(zip(out_labels, model._metric_values(loss, acc)))
        if do_val:
            model._run_eval(val, batch_size)
            vloss, vacc, _ = ex.read_metrics()
            epoch_logs.update(zip(["val_" + n for n in out_labels], model._metric_values(vloss, vacc)))
        if check_dp:
            # before the callbacks: a checkpoint / early-stop decision never sees diverged ranks
            model.history.dp_consistency.append(dp_consistency_check(model, epoch))
        cb.on_epoch_end(epoch, epoch_logs)
        if model.stop_training:
            break
    cb.on_train_end()
    model.history.data_plane = data_plane_of(ex, dp)
    return model.history


def weight_digest(model) -> list:
    """(sum, sum |w|, sum w^2) of the flat fp32 master weights, accumulated in fp64: equal on
    every rank iff (to fp64 rounding of identical inputs, i.e. exactly) the ranks agree."""
    m = model.store.master[:model.store.numel].detach().double()
    return [float(m.sum()), float(m.abs().sum()), float((m * m).sum())]


def dp_consistency_check(model, epoch: int) -> dict:
    """One allgather of 3 doubles per epoch: every rank's weight digest.  Raises
    ``DataParallelDivergence`` on EVERY rank (they all see the same gathered list) if any rank
    differs -- a data-plane ordering bug, a dropped bucket or a rank that skipped a step would
    otherwise train on silently, diverged.  Returns the History record."""
    from ..parallel import dist as _dist
    d = weight_digest(model)
    digests = _dist.allgather(d)
    ok = all(x == digests[0] for x in digests)
    rec = {"epoch": int(epoch), "digest": d, "identical": ok}
    if not ok:
        bad = [i for i, x in enumerate(digests) if x != digests[0]]
        rec["ranks_differing"] = bad
        model.history.dp_consistency.append(rec)
        raise _dist.DataParallelDivergence(
            "data-parallel ranks diverged at the end of epoch %d: weight digests of ranks %s differ "
            "from rank 0's (%s vs %s); data plane %s" % (epoch, bad, digests[bad[0]], digests[0],
                                                           data_plane_of(model._executor, _dp_state())))
    return rec


def _dp_state():
    from ..parallel import state as dp_state
    return dp_state.current()


def data_plane_of(ex, dp) -> Optional[str]:
    """Which gradient data plane a distributed fit() ran on (recorded on its History):
    "rccl" / "xgmi" / "hybrid" for the native captured reducer (NativeGradReducer), "gloo" /
    "nccl" for the torch.distributed reducer, None without data parallelism; plus how
    dist.init chose it."""
    red = getattr(ex, "reducer", None)
    if red is None or dp is None:
        return None
    if type(red).__name__ == "NativeGradReducer":
        plane = "xgmi" if (red.xgmi is not None and len(red.buckets) == 1) else red.plane
        kind = "NativeGradReducer:%s" % plane
    else:
        kind = "GradReducer:%s" % dp.backend
    return kind + (" [%s]" % dp.plane if dp.plane else "")
