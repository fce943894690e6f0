"""Keras-2.2.4 weight constraints (``keras/constraints.py``): a projection applied to a layer's
kernel or bias directly after its optimizer update, ``w <- C(update(w))``; optimizer slots are
untouched.  With ``norms = sqrt(sum(w * w, axis, keepdims=True))`` and ``K.epsilon() = 1e-7``:

    MaxNorm(max_value, axis)        w *= clip(norms, 0, max_value) / (1e-7 + norms)
    NonNeg()                        w *= (w >= 0)
    UnitNorm(axis)                  w /= (1e-7 + norms)
    MinMaxNorm(min, max, rate, axis) w *= (rate * clip(norms, min, max) + (1 - rate) * norms) / (1e-7 + norms)

As in Keras the factor is applied also when the norm lies inside its bound (it is then
``norms / (1e-7 + norms)``, not 1), and a group of norm 0 stays 0.

The objects here are symbolic (no math): the executors read ``ParamStore.constrained_tensors()``
-- ``ops/reference.py`` on the CPU, the column-norm kernels of ``csrc/kernels/constraint.hip`` at the
end of the captured step on a GPU.  ``axis`` must be a prefix of the tensor's axes (``0``, ``[0, 1]``,
``[0, 1, 2]`` of a Conv2D kernel; ``0`` of a Dense kernel or a bias): the tensor is then a row-major
``[R, M]`` matrix and a group is one column.  The parameters are fp32 values, as Keras casts them to
``floatx``.
"""
from __future__ import annotations

import math

import numpy as np

# the kind codes of the kernels' descriptor table (args.h CON_*)
KIND_MAX_NORM, KIND_NON_NEG, KIND_UNIT_NORM, KIND_MIN_MAX_NORM = 0, 1, 2, 3
EPSILON = float(np.float32(1e-7))


def _f32(v, what: str) -> float:
    """A parameter as Keras holds it: cast to float32, kept as the Python float of that value."""
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError("constraint parameter %s=%r is not a number" % (what, v))
    with np.errstate(over="ignore"):
        f32 = float(np.float32(f))
    if not math.isfinite(f32) or f32 < 0:
        raise ValueError("constraint parameter %s=%r must be finite in float32 and >= 0" % (what, v))
    return f32


def _axis(axis):
    """Keras' ``axis``: an int stays an int, a sequence becomes a list of ints (its config form)."""
    if isinstance(axis, (int, np.integer)) and not isinstance(axis, bool):
        return int(axis)
    try:
        return [int(a) for a in axis]
    except (TypeError, ValueError):
        raise ValueError("constraint axis=%r is neither an integer nor a sequence of integers" % (axis,))


class Constraint:
    """Constraint base class."""
    kind = None                    # KIND_* of the kernels' table
    axis = 0

    def params(self):
        """The kind's fp32 parameters, as the descriptor table takes them (three words)."""
        return (0.0, 0.0, 0.0)

    def get_config(self) -> dict:
        return {}

    @classmethod
    def from_config(cls, config: dict) -> "Constraint":
        return cls(**config)

    def rows(self, shape, layer_name: str) -> int:
        """R of the row-major [R, M] view of a tensor of ``shape`` this constraint's axis set gives:
        the axes (negative ones normalised) must be a prefix of the tensor's; anything else is a
        NotImplementedError naming the layer."""
        nd = len(shape)
        raw = self.axis if isinstance(self.axis, list) else [self.axis]
        axes = sorted(a + nd if a < 0 else a for a in raw)
        if not axes or axes != list(range(len(axes))) or len(axes) > nd:
            raise NotImplementedError("layer %s: %s with axis=%r on a weight of shape %r is not implemented (the axes "
                                      "must be a prefix of the weight's: 0, [0, 1], ...)"
                                      % (layer_name, type(self).__name__, self.axis, tuple(shape)))
        return int(np.prod(shape[:len(axes)]))

    def __eq__(self, other):
        return type(other) is type(self) and self.get_config() == other.get_config()

    def __hash__(self):
        return hash((type(self).__name__, repr(self.get_config())))

    def __repr__(self):
        return "%s(%s)" % (type(self).__name__, ", ".join("%s=%r" % kv for kv in self.get_config().items()))


class MaxNorm(Constraint):
    """``w *= clip(norms, 0, max_value) / (1e-7 + norms)``."""
    kind = KIND_MAX_NORM

    def __init__(self, max_value=2, axis=0):
        self.max_value = _f32(max_value, "max_value")
        self.axis = _axis(axis)

    def params(self):
        return (0.0, self.max_value, 1.0)

    def get_config(self):
        return {"max_value": self.max_value, "axis": self.axis}


class NonNeg(Constraint):
    """``w *= (w >= 0)``."""
    kind = KIND_NON_NEG


class UnitNorm(Constraint):
    """``w /= (1e-7 + norms)``."""
    kind = KIND_UNIT_NORM

    def __init__(self, axis=0):
        self.axis = _axis(axis)

    def get_config(self):
        return {"axis": self.axis}


class MinMaxNorm(Constraint):
    """``w *= (rate * clip(norms, min_value, max_value) + (1 - rate) * norms) / (1e-7 + norms)``."""
    kind = KIND_MIN_MAX_NORM

    def __init__(self, min_value=0.0, max_value=1.0, rate=1.0, axis=0):
        self.min_value = _f32(min_value, "min_value")
        self.max_value = _f32(max_value, "max_value")
        self.rate = _f32(rate, "rate")
        self.axis = _axis(axis)

    def params(self):
        return (self.min_value, self.max_value, self.rate)

    def get_config(self):
        return {"min_value": self.min_value, "max_value": self.max_value, "rate": self.rate, "axis": self.axis}


# Keras' aliases
max_norm = maxnorm = MaxNorm
non_neg = nonneg = NonNeg
unit_norm = unitnorm = UnitNorm
min_max_norm = MinMaxNorm

_CLASSES = {c.__name__: c for c in (MaxNorm, NonNeg, UnitNorm, MinMaxNorm)}
_NAMES = dict(_CLASSES, max_norm=MaxNorm, maxnorm=MaxNorm, non_neg=NonNeg, nonneg=NonNeg, unit_norm=UnitNorm,
              unitnorm=UnitNorm, min_max_norm=MinMaxNorm)


def serialize(constraint):
    """The Keras config dict ``{"class_name": "MaxNorm", "config": {..}}``; None for no constraint."""
    if constraint is None:
        return None
    return {"class_name": type(constraint).__name__, "config": constraint.get_config()}


def deserialize(config, custom_objects=None):
    if not isinstance(config, dict) or "class_name" not in config:
        raise ValueError("Could not interpret constraint config: %r" % (config,))
    cls = _CLASSES.get(config["class_name"])
    if cls is None:
        raise ValueError("Unknown constraint class %r (known: %s)" % (config["class_name"], ", ".join(_CLASSES)))
    return cls.from_config(dict(config.get("config") or {}))


def get(identifier):
    """None, an instance, a class or alias name (that constructor's defaults) or a Keras config dict
    -> the constraint (None stays None)."""
    if identifier is None:
        return None
    if isinstance(identifier, Constraint):
        if identifier.kind is None:
            raise ValueError("Unknown constraint class %r (known: %s)" % (type(identifier).__name__, ", ".join(_CLASSES)))
        return identifier
    if isinstance(identifier, dict):
        return deserialize(identifier)
    if isinstance(identifier, str):
        if identifier in _NAMES:
            return _NAMES[identifier]()
        raise ValueError("Unknown constraint %r (known: %s)" % (identifier, ", ".join(sorted(_NAMES))))
    raise ValueError("Could not interpret constraint identifier: %r" % (identifier,))
