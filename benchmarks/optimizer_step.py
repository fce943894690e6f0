"""Step time of the RPV CNN ([16,32,64]/[128], 64x64x3, B=128) per optimizer on one GPU.

    python benchmarks/optimizer_step.py [--opts Adam,Adagrad,Adamax,AMSGrad] [--rounds 6] [--steps 256]
                                        [--clipnorm C] [--l2 X] [--activation NAME[,NAME..]] [--batch-norm]
                                        [--pool avg] [--global-pool avg|max]
                                        [--metrics a,b] [--weighted-metrics a,b] [--eval-samples N]
                                        [--loss NAME[,NAME..]]

Method (the README's sample-weight measurement): one model per optimizer, all alive at once;
``rounds`` interleaved rounds, in each of which every model runs ``steps`` training steps as
32-step graph replays, timed with device events after a settle run; the figure is the median of a
model's rounds.  Prints one JSON line.

``--clipnorm C`` adds two more models per optimizer: ``<name>/unfused`` (the same optimizer built
under ``INTML_TUNE=fuse_optim=0,early_reduce=0``: every slab reduction, then one optimizer launch
-- the structure of a clipping step without the clip) and ``<name>/clipnorm`` (``clipnorm=C``: that
structure plus the norm launch and the clipped load).  The difference between the two is the cost
of gradient clipping.

``--l2 X`` likewise adds ``<name>/unfused`` and ``<name>/l2`` (an l2 kernel regularizer ``X`` on
every Conv2D / Dense: that structure plus the one ``weight_reg`` launch).  The difference between
the two is the cost of the weight regularizers.

``--activation NAME[,NAME..]`` adds ``<name>/perlayer`` (the relu model built under
``INTML_TUNE=conv_stack=0,fuse_head=0``: the per-layer structure a model with hidden activations
takes, without the activation launches) and one ``<name>/<activation>`` model per name (that
structure plus one ``act_fwd`` and one ``act_bwd`` launch per hidden stage).  The difference between
those is the cost of the activation launches; the difference between ``<name>`` and
``<name>/perlayer`` is the cost of leaving the fused conv stack.

``--batch-norm`` adds ``<name>/perlayer`` likewise and ``<name>/bn`` (a BatchNormalization between
every hidden Conv2D / Dense and its relu: that structure plus ``bn_stats``, ``bn_apply_fwd``,
``bn_bwd_reduce`` and ``bn_bwd_apply`` per hidden stage, whose conv kernels run un-pooled).

``--pool avg`` adds ``<name>/unstacked`` (the relu model built under ``INTML_TUNE=conv_stack=0``: the
per-layer conv structure an average-pooled or globally pooled model takes, the head still running the
last dense's epilogue) and ``<name>/pool-avg`` (AveragePooling2D in every conv block: that structure
plus ``pool_fwd`` and ``pool_bwd`` per conv stage, whose conv kernels run un-pooled);
``--global-pool avg|max`` adds ``<name>/unstacked`` likewise and ``<name>/gpool-<kind>`` (a global
pooling layer in the Flatten's place: ``gpool_fwd`` and ``gpool_bwd``, and a Dense(128) over 64
inputs instead of 4096).

``--loss NAME[,NAME..]`` adds ``<name>/unfused-head`` (the default model built under
``INTML_TUNE=fuse_head=0``: ``dense_epi`` as a launch of its own, then the first head kernel) and one
``<name>/loss-<NAME>`` model per name (that structure with the ``loss_head`` launch in the head's
place; ``NAME@N`` puts the loss on a sigmoid output of N columns, ``binary_crossentropy@8`` being the
multi-label head).  The difference between those is the cost of the second head kernel.

``--metrics a,b`` adds ``<name>/metrics`` (the model compiled with these metrics: with a ROC metric among
them the step has one more launch, ``roc_accum`` behind the head); ``--weighted-metrics a,b`` adds
``<name>/weighted-data`` (the default model on sample-weighted data: the weighted head instances, no new
launch) and ``<name>/metrics+weighted`` (both lists compiled in, on that data: ``roc_accum`` feeds the
weighted set too).  ``--eval-samples N`` also times, for every model, an evaluation pass over N samples at
the batch size (eval-step graph replays between two device events, the epoch's metric read included)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from cori_intml_examples_amd import optim  # noqa: E402
from cori_intml_examples_amd.apps import zoo  # noqa: E402
from cori_intml_examples_amd.utils import set_random_seed  # noqa: E402

REPLAY = 32


UNFUSED = "fuse_optim=0,early_reduce=0"
PERLAYER = "conv_stack=0,fuse_head=0"
UNSTACKED = "conv_stack=0"
UNFUSED_HEAD = "fuse_head=0"


def make_opt(name, **kw):
    return optim.Adam(amsgrad=True, **kw) if name == "AMSGrad" else getattr(optim, name)(**kw)


def variants(names, clipnorm, l2=None, activations=(), batch_norm=False, pool="max", global_pool=None,
             metrics=None, weighted_metrics=None, losses=()):
    """[(label, optimizer name, optimizer keywords, INTML_TUNE while its plan is built, model l2,
    hidden activation -- or "relu+bn": relu behind a BatchNormalization, "relu+pool=avg" /
    "relu+gpool=<kind>": relu with that builder keyword; a 7th entry, where present: the builder's
    metric keywords, "weighted_data": True for sample-weighted data)]"""
    out = []
    for nm in names:
        out.append((nm, nm, {}, None, 0.0, "relu"))
        if metrics:
            out.append((nm + "/metrics", nm, {}, None, 0.0, "relu", {"metrics": metrics}))
        if weighted_metrics:
            out.append((nm + "/weighted-data", nm, {}, None, 0.0, "relu", {"weighted_data": True}))
            out.append((nm + "/metrics+weighted", nm, {}, None, 0.0, "relu",
                        {"metrics": metrics or ["accuracy"], "weighted_metrics": weighted_metrics, "weighted_data": True}))
        if clipnorm is not None or l2:
            out.append((nm + "/unfused", nm, {}, UNFUSED, 0.0, "relu"))
        if clipnorm is not None:
            out.append((nm + "/clipnorm", nm, {"clipnorm": clipnorm}, None, 0.0, "relu"))
        if l2:
            out.append((nm + "/l2", nm, {}, None, l2, "relu"))
        if activations or batch_norm:
            out.append((nm + "/perlayer", nm, {}, PERLAYER, 0.0, "relu"))
        if pool != "max" or global_pool:
            out.append((nm + "/unstacked", nm, {}, UNSTACKED, 0.0, "relu"))
        if pool != "max":
            out.append((nm + "/pool-" + pool, nm, {}, None, 0.0, "relu+pool=" + pool))
        if global_pool:
            out.append((nm + "/gpool-" + global_pool, nm, {}, None, 0.0, "relu+gpool=" + global_pool))
        if batch_norm:
            out.append((nm + "/bn", nm, {}, None, 0.0, "relu+bn"))
        for act in activations:
            out.append((nm + "/" + act, nm, {}, None, 0.0, act))
        if losses:
            # the loss head's structure with the first head kernel: the default model under fuse_head=0
            out.append((nm + "/unfused-head", nm, {}, UNFUSED_HEAD, 0.0, "relu"))
        for ls in losses:
            # NAME@N: the loss on a sigmoid output of N columns (binary_crossentropy@8: the multi-label head)
            name, _, cols = ls.partition("@")
            out.append((nm + "/loss-" + ls, nm, {}, None, 0.0, "relu",
                        dict({"loss": name}, **({"outputs": int(cols)} if cols else {}))))
    return out


class tuned:
    """INTML_TUNE set while a model's plan is built and captured (the knobs are read then)."""

    def __init__(self, tv):
        self.tv = tv

    def __enter__(self):
        self.old = os.environ.get("INTML_TUNE")
        if self.tv is not None:
            os.environ["INTML_TUNE"] = self.tv

    def __exit__(self, *exc):
        if self.tv is not None:
            if self.old is None:
                os.environ.pop("INTML_TUNE", None)
            else:
                os.environ["INTML_TUNE"] = self.old


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--opts", default="Adam,Adagrad,Adamax,AMSGrad")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--clipnorm", type=float, default=None)
    ap.add_argument("--l2", type=float, default=None)
    ap.add_argument("--activation", default="", help="comma-separated hidden activations to time")
    ap.add_argument("--batch-norm", action="store_true", help="time the model with BatchNormalization layers")
    ap.add_argument("--pool", choices=["max", "avg"], default="max", help="time the model with AveragePooling2D layers")
    ap.add_argument("--global-pool", choices=["avg", "max"], default=None,
                    help="time the model with a global pooling layer in the Flatten's place")
    ap.add_argument("--loss", default="", metavar="NAME[,NAME]",
                    help="time the model with these Keras losses in binary_crossentropy's place (the loss head), "
                         "and the default model under fuse_head=0 (the same structure with the first head kernel)")
    ap.add_argument("--metrics", default="", help="comma-separated compile metrics to time (e.g. accuracy,auc)")
    ap.add_argument("--weighted-metrics", default="", help="comma-separated weighted_metrics to time, on weighted data")
    ap.add_argument("--eval-samples", type=int, default=0, help="also time an evaluation pass over this many samples")
    a = ap.parse_args()
    split = lambda t: [n for n in t.split(",") if n]
    var = [v if len(v) == 7 else v + ({},) for v in
           variants(a.opts.split(","), a.clipnorm, a.l2, split(a.activation), a.batch_norm, a.pool, a.global_pool,
                    split(a.metrics), split(a.weighted_metrics), split(a.loss))]
    names = [v[0] for v in var]
    tunes = {v[0]: v[3] for v in var}
    bs, reps = a.batch, max(1, a.steps // REPLAY)
    rs = np.random.RandomState(0)
    x = rs.rand(bs * REPLAY, 64, 64, 3).astype(np.float32)
    y = (rs.rand(bs * REPLAY) > 0.5).astype(np.float32)
    w = rs.uniform(0.5, 2.0, bs * REPLAY).astype(np.float32)
    runs, keys = {}, {}
    for nm, oname, kw, tv, l2, act, extra in var:
        set_random_seed(1)
        with tuned(tv):
            m = zoo.rpv_cnn((64, 64, 3), conv_sizes=[16, 32, 64], fc_sizes=[128], dropout=0.2,
                            optimizer=make_opt(oname, **kw), lr=None, device="cuda:0", **({"l2": l2} if l2 else {}),
                            **({"batch_norm": True} if act == "relu+bn" else {}),
                            **({"pool": act.split("=")[1]} if act.startswith("relu+pool=") else {}),
                            **({"global_pool": act.split("=")[1]} if act.startswith("relu+gpool=") else {}),
                            **({"activation": act} if not act.startswith("relu") else {}),
                            **{k: v for k, v in extra.items() if k != "weighted_data"})
        ex = m._executor
        yv = y if extra.get("outputs", 1) == 1 else (rs.rand(bs * REPLAY, extra["outputs"]) > 0.5).astype(np.float32)
        d = ex.upload(x, yv, w) if extra.get("weighted_data") else ex.upload(x, yv)
        keys[nm] = (bs, "train", "w") if extra.get("weighted_data") else (bs, "train")
        perm = torch.arange(d.n, device=ex.device)
        runs[nm] = (m, ex, d, perm)

    def timed(nm, n):
        _, ex, d, perm = runs[nm]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            ex.train_steps(d, perm, 0, bs, REPLAY)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / (n * REPLAY)      # us per step

    for nm in names:                    # plan + graph capture (under the model's knobs) + clock settle
        with tuned(tunes[nm]):
            timed(nm, 4)
    us = {nm: [] for nm in names}
    for _ in range(a.rounds):
        for nm in names:
            timed(nm, 2)                # back under load after the other models' turn
            us[nm].append(timed(nm, reps))
    ev = {}
    if a.eval_samples:
        # an evaluation pass: eval_samples / bs eval-step replays over the resident set, then the metric read
        nb = max(1, a.eval_samples // bs)

        def eval_pass(nm):
            m, ex, d, _ = runs[nm]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ex.reset_metrics()
            for b in range(nb):
                ex.eval_step(d, (b % REPLAY) * bs, bs)
            m._metric_values(*ex.read_metrics()[:2])
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3

        ev = {nm: [] for nm in names}
        for nm in names:
            eval_pass(nm)
        for _ in range(a.rounds):
            for nm in names:
                ev[nm].append(eval_pass(nm))
    out = {"workload": "rpv_cnn 64x64x3 [16,32,64]/[128] B=%d" % bs, "steps_per_run": reps * REPLAY, "rounds": a.rounds,
           "us_per_step_median": {nm: round(statistics.median(v), 2) for nm, v in us.items()},
           "us_per_step_runs": {nm: [round(t, 2) for t in v] for nm, v in us.items()},
           "optim_fused": {nm: bool(runs[nm][1]._plans[keys[nm]].optim_fused) for nm in names},
           "launches": {nm: [it[0] for it in runs[nm][1]._plans[keys[nm]].launches] for nm in names},
           "finite": {nm: bool(np.isfinite(runs[nm][0].store.master[:runs[nm][0].store.numel].sum().item()))
                      for nm in names}}
    if ev:
        out["eval_samples"] = max(1, a.eval_samples // bs) * bs
        out["eval_pass_us_median"] = {nm: round(statistics.median(v), 1) for nm, v in ev.items()}
        out["eval_pass_us_runs"] = {nm: [round(t, 1) for t in v] for nm, v in ev.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
