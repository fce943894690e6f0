"""Keras-2.2.4 weight regularizers (``keras/regularizers.py``): L1 / L2 penalties on a layer's
kernel or bias.

For a weight tensor ``w`` with ``L1L2(l1, l2)`` the penalty is ``l1 * sum(|w|) + l2 * sum(w*w)``;
the model penalty P is the sum over every regularized tensor, computed from the weights the
step's forward used.  Every reported loss (train and test batches, epoch ``loss`` / ``val_loss``,
``evaluate``) is ``L_data + P``; the penalty is not multiplied by sample weights.  Every step's
update sees ``g + l1 * sgn(w) + 2 * l2 * w`` with ``sgn(0) = 0``, added before gradient clipping.

The objects here are symbolic (no math): the executors read ``Model.regularized_ranges()`` --
``ops/reference.py`` on the CPU, ``weight_reg_kernel`` (``csrc/kernels/reg.hip``) inside the
captured step on a GPU.  The coefficients are fp32 values, as Keras casts them to ``floatx``.
"""
from __future__ import annotations

import math

import numpy as np


def _coef(v, what: str) -> float:
    """A coefficient as Keras holds it: cast to float32, kept as the Python float of that value."""
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError("regularizer coefficient %s=%r is not a number" % (what, v))
    if not math.isfinite(f) or f < 0:
        raise ValueError("regularizer coefficient %s=%r must be finite and >= 0" % (what, v))
    with np.errstate(over="ignore"):
        f32 = float(np.float32(f))
    if not math.isfinite(f32):
        raise ValueError("regularizer coefficient %s=%r does not fit float32" % (what, v))
    return f32


class Regularizer:
    """Regularizer base class."""

    def get_config(self) -> dict:
        return {}

    @classmethod
    def from_config(cls, config: dict) -> "Regularizer":
        return cls(**config)


class L1L2(Regularizer):
    """Regularizer for L1 and L2 regularization: ``l1 * sum(|w|) + l2 * sum(w*w)``."""

    def __init__(self, l1=0., l2=0.):
        self.l1 = _coef(l1, "l1")
        self.l2 = _coef(l2, "l2")

    def __bool__(self):
        """False for ``L1L2(0, 0)``: it counts as "no regularizer"."""
        return self.l1 > 0 or self.l2 > 0

    def get_config(self) -> dict:
        return {"l1": self.l1, "l2": self.l2}

    def __eq__(self, other):
        return isinstance(other, L1L2) and (self.l1, self.l2) == (other.l1, other.l2)

    def __hash__(self):
        return hash((self.l1, self.l2))

    def __repr__(self):
        return "L1L2(l1=%r, l2=%r)" % (self.l1, self.l2)


def l1(l=0.01) -> L1L2:
    return L1L2(l1=l)


def l2(l=0.01) -> L1L2:
    return L1L2(l2=l)


def l1_l2(l1=0.01, l2=0.01) -> L1L2:
    return L1L2(l1=l1, l2=l2)


_NAMES = {"l1": l1, "l2": l2, "l1_l2": l1_l2}


def serialize(regularizer):
    """The Keras config dict ``{"class_name": "L1L2", "config": {"l1": .., "l2": ..}}``; None for
    no regularizer (``None`` or ``L1L2(0, 0)``)."""
    if regularizer is None or not regularizer:
        return None
    return {"class_name": type(regularizer).__name__, "config": regularizer.get_config()}


def deserialize(config, custom_objects=None):
    if not isinstance(config, dict) or "class_name" not in config:
        raise ValueError("Could not interpret regularizer config: %r" % (config,))
    name = config["class_name"]
    if name != "L1L2":
        raise ValueError("Unknown regularizer class %r (only L1L2 is implemented)" % (name,))
    cfg = dict(config.get("config") or {})
    unknown = sorted(set(cfg) - {"l1", "l2"})
    if unknown:
        raise ValueError("Unknown L1L2 config keys %s" % unknown)
    return L1L2(**cfg)


def get(identifier):
    """None, an instance, a name ("l1" / "l2" / "l1_l2": that constructor's defaults) or a Keras
    config dict -> the regularizer (None stays None)."""
    if identifier is None:
        return None
    if isinstance(identifier, L1L2):
        return identifier
    if isinstance(identifier, Regularizer):
        raise ValueError("Unknown regularizer class %r (only L1L2 is implemented)" % type(identifier).__name__)
    if isinstance(identifier, dict):
        return deserialize(identifier)
    if isinstance(identifier, str):
        if identifier in _NAMES:
            return _NAMES[identifier]()
        raise ValueError("Unknown regularizer %r (known: l1, l2, l1_l2)" % (identifier,))
    raise ValueError("Could not interpret regularizer identifier: %r" % (identifier,))
