"""Keras-2.2.4-shaped ``keras.activations``: the element-wise activations by name.

``relu`` / ``linear`` run inside the fused epilogues of the conv and dense kernels, ``softmax``
and an output ``sigmoid`` inside the head kernel; the other names are the hidden activations of
``ops/reference.py: ACTIVATIONS`` (``act.hip`` on the GPU).  The functions here work on NumPy
arrays and torch tensors (for callers that pass ``activation=activations.tanh`` or evaluate one
by hand); a layer only records the NAME, the executors do the math.
"""
from __future__ import annotations

import numpy as np
import torch

from .ops import reference as _R

# hidden activations as Conv2D / Dense / Activation strings (LeakyReLU is a layer, not a string)
HIDDEN = tuple(n for n in _R.ACTIVATIONS if n != "leaky_relu")
NAMES = ("linear", "relu", "softmax") + HIDDEN


def _apply(fn, x):
    if isinstance(x, torch.Tensor):
        return fn(x)
    return fn(torch.as_tensor(np.asarray(x, dtype=np.float32))).numpy()


def linear(x):
    return x


def relu(x, alpha=0.0, max_value=None, threshold=0.0):
    if alpha != 0.0 or max_value is not None or threshold != 0.0:
        raise NotImplementedError("relu with alpha / max_value / threshold (use the LeakyReLU layer)")
    return _apply(torch.relu, x)


def softmax(x, axis=-1):
    return _apply(lambda t: torch.softmax(t, axis), x)


def elu(x, alpha=1.0):
    return _apply(lambda t: _R.act("elu", float(alpha), t), x)


def _named(name):
    def fn(x):
        return _apply(lambda t: _R.act(name, 0.0, t), x)
    fn.__name__ = fn.__qualname__ = name
    fn.__doc__ = "Keras ``%s`` (formula: ops/reference.py act)." % name
    return fn


tanh, sigmoid, hard_sigmoid, selu, softplus, softsign = (
    _named(n) for n in ("tanh", "sigmoid", "hard_sigmoid", "selu", "softplus", "softsign"))


def serialize(activation):
    if activation is None:
        return "linear"
    name = activation if isinstance(activation, str) else getattr(activation, "__name__", None)
    if name not in NAMES:
        raise ValueError("unknown activation %r (known: %s)" % (activation, ", ".join(NAMES)))
    return name


def deserialize(name, custom_objects=None):
    if custom_objects and name in custom_objects:
        return custom_objects[name]
    if name not in NAMES:
        raise ValueError("unknown activation %r (known: %s)" % (name, ", ".join(NAMES)))
    return globals()[name]


def get(identifier):
    if identifier is None:
        return linear
    if isinstance(identifier, str):
        return deserialize(identifier)
    if callable(identifier):
        return identifier
    raise ValueError("could not interpret activation identifier %r" % (identifier,))
