"""Model zoo: the three CNN families the reference trains.

  M1 ``mnist_cnn``      Conv(h1,valid)-Conv(h2)-MaxPool-Dropout-Flatten-Dense(h3)-Dropout-
                         Dense(10,softmax)  (mnist.py:44-59, DistTrain_mnist.ipynb:294-304)
  M2 ``rpv_cnn``        [Conv(c,same)+ReLU, MaxPool] x n - Dropout - Flatten -
                         [Dense(f)+ReLU, Dropout] x m - Dense(1, sigmoid)   (rpv.py:38-72)
  M3 ``rpv_legacy_cnn`` strided 4-conv + Dense(512) RPV model (Train_rpv.ipynb:205-219)
"""
from __future__ import annotations

from ..models import (Activation, AveragePooling2D, BatchNormalization, Conv2D, Dense, Dropout, Flatten,
                      GlobalAveragePooling2D, GlobalMaxPooling2D, Input, MaxPooling2D, Model, Sequential)
from .. import optim as optimizers
from .. import regularizers


def _kernel_l2(l2):
    """Layer keywords of the builders' ``l2=``: an l2 kernel regularizer on every Conv2D / Dense
    (not on biases); nothing at all for 0 -- exactly the unregularized model."""
    return {"kernel_regularizer": regularizers.l2(l2)} if l2 else {}


def _hidden(layer_cls, *args, activation="relu", batch_norm=False, **kw):
    """The layers of one hidden Conv2D / Dense: the layer itself, or with ``batch_norm`` its linear
    form, a BatchNormalization and the activation as a layer (ahead of the stage's pool / dropout)."""
    if not batch_norm:
        return [layer_cls(*args, activation=activation, **kw)]
    return [layer_cls(*args, **kw), BatchNormalization(), Activation(activation)]


def _pool(pool):
    """The builders' ``pool=``: the 2x2 pooling layer of a conv block, "max" (the reference's) | "avg"."""
    if pool not in ("max", "avg"):
        raise ValueError("pool = %r (\"max\" or \"avg\")" % (pool,))
    return (MaxPooling2D if pool == "max" else AveragePooling2D)(pool_size=(2, 2))


def _bridge(global_pool):
    """The builders' ``global_pool=``: the layer between the conv part and the dense part, Flatten
    (None, the reference's) | GlobalAveragePooling2D ("avg") | GlobalMaxPooling2D ("max")."""
    if global_pool not in (None, "avg", "max"):
        raise ValueError("global_pool = %r (None, \"avg\" or \"max\")" % (global_pool,))
    return {None: Flatten, "avg": GlobalAveragePooling2D, "max": GlobalMaxPooling2D}[global_pool]()


def _chain(h, layers):
    for layer in layers:
        h = layer(h)
    return h


def clipped_optimizer(optimizer: str, lr=None, clipnorm=None, clipvalue=None):
    """The training CLIs' ``--clipnorm`` / ``--clipvalue``: the optimizer name itself when neither
    is given (nothing changes), else the optimizer object built with them (Keras keywords)."""
    kw = {k: v for k, v in (("clipnorm", clipnorm), ("clipvalue", clipvalue)) if v is not None}
    if not kw:
        return optimizer
    if lr is not None:
        kw["lr"] = lr
    return type(optimizers.get(optimizer))(**kw)      # (any name optimizers.get knows: "Adam", "adam")


def _opt(optimizer, lr, use_horovod):
    if isinstance(optimizer, str):
        opt = getattr(optimizers, optimizer)(lr=lr) if lr is not None else optimizers.get(optimizer)
    else:
        opt = optimizer
    if use_horovod:
        from ..parallel import hvd
        opt = hvd.DistributedOptimizer(opt)
    return opt


def _metric_lists(metrics, weighted_metrics):
    """compile()'s metric arguments: the builders' defaults compile what they always compiled."""
    kw = {"metrics": ["accuracy"] if metrics is None else list(metrics)}
    if weighted_metrics:
        kw["weighted_metrics"] = list(weighted_metrics)
    return kw


def parse_metric_list(text):
    """'a,b' of a CLI flag -> ['a', 'b'] (None / '' -> None: the builder's default)."""
    return [t.strip() for t in text.split(",") if t.strip()] if text else None


def fom_from_history(history, name: str, mode: str) -> float:
    """The FoM a training CLI prints for logged name ``name`` (a ``val_`` key of the History): the
    best or last epoch's value; for the larger-is-better names (acc and the ROC family) 1 - value,
    so the evaluators keep minimising ("best" is then the best epoch by that metric)."""
    from ..hpo.evaluator import figure_of_merit
    from ..metrics import larger_is_better
    if name not in history:
        raise ValueError("--fom-metric %s: not a logged metric (logged: %s)" % (name, ", ".join(sorted(history))))
    vals = [float(v) for v in history[name]]
    return figure_of_merit([1.0 - v for v in vals] if larger_is_better(name) else vals, mode)


def mnist_cnn(h1=4, h2=8, h3=32, dropout=0.5, dropout2=None, optimizer="Adadelta", lr=None,
              n_classes=10, input_shape=(28, 28, 1), use_horovod=False, device=None, activation="relu",
              batch_norm=False, pool="max", global_pool=None, metrics=None, weighted_metrics=None, loss=None, l2=0.0):
    """``activation``: the hidden activation of every Conv2D / Dense ("relu": the reference's model).
    ``metrics`` / ``weighted_metrics``: Model.compile's lists (None: ["accuracy"] and none).
    ``batch_norm``: every hidden Conv2D / Dense becomes layer(linear) -> BatchNormalization ->
    Activation(activation).  ``pool``: "max" | "avg", the 2x2 pooling layer.  ``global_pool``: None |
    "avg" | "max", a global pooling layer in the Flatten's place (behind the Dropout: the plan wants
    the conv stage's dropout ahead of it).  ``loss``: a Keras loss name of the README's "Losses"
    table in categorical_crossentropy's place (None: the reference's loss)."""
    reg = _kernel_l2(l2)
    hid = dict(activation=activation, batch_norm=batch_norm, **reg)
    m = Sequential(device=device)
    for layer in (_hidden(Conv2D, h1, (3, 3), input_shape=input_shape, **hid) + _hidden(Conv2D, h2, (3, 3), **hid)):
        m.add(layer)
    m.add(_pool(pool))
    m.add(Dropout(dropout))
    m.add(_bridge(global_pool))
    for layer in _hidden(Dense, h3, **hid):
        m.add(layer)
    m.add(Dropout(dropout if dropout2 is None else dropout2))
    m.add(Dense(n_classes, activation="softmax", **reg))
    m.compile(optimizer=_opt(optimizer, lr, use_horovod), loss=loss or "categorical_crossentropy", **_metric_lists(metrics, weighted_metrics))
    return m


def rpv_cnn(input_shape, conv_sizes=(8, 16, 32), fc_sizes=(64,), dropout=0.5, optimizer="Adam", lr=0.001,
            use_horovod=False, device=None, activation="relu", batch_norm=False, pool="max", global_pool=None,
            metrics=None, weighted_metrics=None, loss=None, outputs=1, l2=0.0):
    """``activation``: the hidden activation of every Conv2D / Dense ("relu": the reference's model).
    ``metrics`` / ``weighted_metrics``: Model.compile's lists (None: ["accuracy"] and none).
    ``batch_norm``: every hidden Conv2D / Dense becomes layer(linear) -> BatchNormalization ->
    Activation(activation).  ``pool``: "max" | "avg", the 2x2 pooling layer of every conv block.
    ``global_pool``: None | "avg" | "max", a global pooling layer in the Flatten's place.
    ``loss``: a Keras loss name of the README's "Losses" table in binary_crossentropy's place
    (None: the reference's loss).  ``outputs``: the sigmoid output's columns (1: the reference's
    model; more: a multi-label head)."""
    reg = _kernel_l2(l2)
    hid = dict(activation=activation, batch_norm=batch_norm, **reg)
    inputs = Input(shape=input_shape)
    h = inputs
    for c in conv_sizes:
        h = _chain(h, _hidden(Conv2D, c, kernel_size=(3, 3), padding="same", **hid))
        h = _pool(pool)(h)
    h = Dropout(dropout)(h)
    h = _bridge(global_pool)(h)
    for f in fc_sizes:
        h = _chain(h, _hidden(Dense, f, **hid))
        h = Dropout(dropout)(h)
    outputs = Dense(outputs, activation="sigmoid", **reg)(h)
    model = Model(inputs=inputs, outputs=outputs, name="RPVClassifier", device=device)
    model.compile(optimizer=_opt(optimizer, lr, use_horovod), loss=loss or "binary_crossentropy",
                  **_metric_lists(metrics, weighted_metrics))
    return model


def rpv_legacy_cnn(input_shape=(64, 64, 1), optimizer="Adam", lr=None, h1=64, h2=128, h3=256, h4=256, h5=512,
                   use_horovod=False, device=None, activation="relu", batch_norm=False, pool="max",
                   global_pool=None, metrics=None, weighted_metrics=None, loss=None):
    """``activation``: the hidden activation of every Conv2D / Dense ("relu": the reference's model).
    ``metrics`` / ``weighted_metrics``: Model.compile's lists (None: ["accuracy"] and none).
    ``batch_norm``: every hidden Conv2D / Dense becomes layer(linear) -> BatchNormalization ->
    Activation(activation).  ``pool``: accepted for symmetry with the other builders (this model's
    convs are strided, it has no 2x2 pooling layer).  ``global_pool``: None | "avg" | "max", a
    global pooling layer in the Flatten's place: "avg" removes the 65,536-row Dense kernel.
    ``loss``: a Keras loss name in binary_crossentropy's place (None: the reference's loss)."""
    _pool(pool)
    hid = dict(activation=activation, batch_norm=batch_norm)
    h = inputs = Input(shape=input_shape)
    for c, st in ((h1, 1), (h2, 2), (h3, 1), (h4, 2)):
        h = _chain(h, _hidden(Conv2D, c, kernel_size=(3, 3), strides=st, padding="same", **hid))
    h = _bridge(global_pool)(h)
    h = _chain(h, _hidden(Dense, h5, **hid))
    outputs = Dense(1, activation="sigmoid")(h)
    model = Model(inputs=inputs, outputs=outputs, name="RPVClassifier", device=device)
    model.compile(optimizer=_opt(optimizer, lr, use_horovod), loss=loss or "binary_crossentropy",
                  **_metric_lists(metrics, weighted_metrics))
    return model
