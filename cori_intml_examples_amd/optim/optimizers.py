"""Keras-2.2 optimizers (hyper-parameters + state layout).

The update math runs in ONE fused multi-tensor HIP launch over the flat parameter
buffer (``csrc/kernels/optim.hip``) on GPU, or in ``ops/reference.py`` on CPU.
Name lookup by string mirrors ``getattr(optimizers, optimizer)(lr=lr)`` at
``rpv.py:62`` and ``model.compile(optimizer='Adadelta')`` at ``mnist.py:58``.
"""
from __future__ import annotations

from ..ops.reference import EPS


class KVariable:
    """Mutable scalar standing in for a Keras backend variable (``optimizer.lr``)."""

    def __init__(self, value: float, name: str = "var"):
        self._v = float(value)
        self.name = name

    def get(self) -> float:
        return self._v

    def set(self, v) -> None:
        self._v = float(v)

    def __float__(self):
        return self._v

    def __repr__(self):
        return "<KVariable %s=%g>" % (self.name, self._v)

    # arithmetic convenience (keeps user code like ``lr * 0.5`` working)
    def __mul__(self, o): return self._v * float(o)
    __rmul__ = __mul__
    def __truediv__(self, o): return self._v / float(o)
    def __add__(self, o): return self._v + float(o)
    __radd__ = __add__
    def __sub__(self, o): return self._v - float(o)
    def __lt__(self, o): return self._v < float(o)
    def __gt__(self, o): return self._v > float(o)
    def __le__(self, o): return self._v <= float(o)
    def __ge__(self, o): return self._v >= float(o)
    def __eq__(self, o):
        try:
            return self._v == float(o)
        except (TypeError, ValueError):
            return False
    __hash__ = object.__hash__


# The optimizer kinds of the fused update kernels, kind -> (id, state buffers the kernels touch
# unconditionally, True if the kernels that choose the optimizer at run time have an instance):
# the Python copy of csrc/kernels/common.h's OPT_KIND_TABLE, which the extension exports as
# OPT_KINDS (tests/test_optimizer_kinds.py compares the two).  A kind without the run-time
# instance runs no early reduction, no fused dense update and no xGMI data plane.
KINDS = {"sgd": (0, 0, True), "rmsprop": (1, 0, True), "adadelta": (2, 0, True), "adam": (3, 0, True),
         "nadam": (4, 0, True), "adagrad": (5, 1, False), "adamax": (6, 2, False), "amsgrad": (7, 3, False)}
KIND_IDS = {k: v[0] for k, v in KINDS.items()}
STANDALONE_KINDS = frozenset(k for k, v in KINDS.items() if not v[2])

# hyper-parameters of the kernel argument structs: (optimizer attribute, struct field, default
# when the optimizer has none, conversion)
_HYPER = (("beta_1", "beta1", 0.9, float), ("beta_2", "beta2", 0.999, float), ("epsilon", "eps", 1e-7, float),
          ("rho", "rho", 0.95, float), ("momentum", "momentum", 0.0, float), ("nesterov", "nesterov", False, int),
          ("initial_decay", "decay", 0.0, float), ("schedule_decay", "schedule_decay", 0.004, float))


def fill_kernel_args(opt, args, kind_field: str = "kind"):
    """Write ``opt``'s kind id and hyper-parameters into the fields ``args`` has (OptimArgs:
    kind, beta1, beta2, eps, rho, momentum, nesterov; StepBeginArgs: opt_kind, beta1, beta2,
    decay, schedule_decay)."""
    setattr(args, kind_field, KIND_IDS[opt.kind])
    for attr, field, default, conv in _HYPER:
        if hasattr(args, field):
            setattr(args, field, conv(getattr(opt, attr, default)))
    return args


def fill_clip_args(opt, args, clip_state_ptr: int):
    """Write ``opt``'s gradient clipping into OptimArgs ``args``: the clip-state buffer the norm
    launch writes its factor to (clipnorm) and the clamp bound (clipvalue).  Nothing is written
    for an optimizer without clipping (the fields' defaults mean off)."""
    cn, cv = clip_pair(opt)
    if cn:
        args.clip = clip_state_ptr
    if cv:
        args.clipvalue = cv
    return args


def _clip_arg(v) -> float:
    """A clipnorm / clipvalue argument as the kernels take it: None or <= 0 means off (0.0)."""
    if v is None:
        return 0.0
    v = float(v)
    return v if v > 0 else 0.0


def clip_pair(opt):
    """(clipnorm, clipvalue) of an optimizer or its DistributedOptimizer wrapper, 0.0 = off."""
    base = getattr(opt, "_base_optimizer", opt)
    return _clip_arg(getattr(base, "clipnorm", None)), _clip_arg(getattr(base, "clipvalue", None))


def get_value(x) -> float:
    return x.get() if isinstance(x, KVariable) else float(x)


def set_value(x, v) -> None:
    if not isinstance(x, KVariable):
        raise TypeError("set_value needs a KVariable")
    x.set(v)


class Optimizer:
    kind = "base"
    n_slots = 0          # number of flat fp32 state buffers
    default_lr = 0.01

    def __init__(self, lr=None, decay=0.0, learning_rate=None, **kw):
        # Keras 2.2.4 Optimizer.get_gradients: clipnorm = c > 0 scales every gradient by c / n
        # when the GLOBAL norm n (over all trainable parameters) is >= c; clipvalue = v > 0 then
        # clamps every element to [-v, v].  Kept only when given (get_config); <= 0 / None = off.
        # (other unknown keywords are accepted and ignored, as before)
        for key in ("clipnorm", "clipvalue"):
            if key in kw:
                v = kw[key]
                setattr(self, key, None if v is None else float(v))
        if lr is None:
            lr = learning_rate if learning_rate is not None else self.default_lr
        self.lr = KVariable(lr, "lr")
        self.decay = float(decay)
        self.initial_decay = self.decay
        self.iterations = 0          # host mirror of the device step counter
        self.distributed = False
        self.compression = None
        self._extra = {}

    def current_lr(self) -> float:
        lr = self.lr.get()
        if self.initial_decay > 0:
            lr = lr / (1.0 + self.initial_decay * self.iterations)
        return lr

    def hparams(self) -> dict:
        return {}

    @property
    def clips(self) -> bool:
        """True when clipnorm or clipvalue is on (the step then runs the clipping plan)."""
        return any(clip_pair(self))

    def _clip_config(self) -> dict:
        return {k: getattr(self, k) for k in ("clipnorm", "clipvalue") if hasattr(self, k)}

    def get_config(self) -> dict:
        cfg = {"lr": self.lr.get(), "decay": self.decay}
        cfg.update(self.hparams())
        cfg.update(self._clip_config())
        return cfg

    @classmethod
    def from_config(cls, cfg):
        return cls(**cfg)

    @property
    def class_name(self) -> str:
        return type(self).__name__


class SGD(Optimizer):
    kind = "sgd"
    default_lr = 0.01

    def __init__(self, lr=None, momentum=0.0, decay=0.0, nesterov=False, **kw):
        super().__init__(lr=lr, decay=decay, **kw)
        self.momentum = float(momentum)
        self.nesterov = bool(nesterov)
        self.n_slots = 1 if self.momentum else 0

    def hparams(self):
        return {"momentum": self.momentum, "nesterov": self.nesterov}


class RMSprop(Optimizer):
    kind = "rmsprop"
    n_slots = 1
    default_lr = 0.001

    def __init__(self, lr=None, rho=0.9, epsilon=None, decay=0.0, **kw):
        super().__init__(lr=lr, decay=decay, **kw)
        self.rho = float(rho)
        self.epsilon = EPS if epsilon is None else float(epsilon)

    def hparams(self):
        return {"rho": self.rho, "epsilon": self.epsilon}


class Adagrad(Optimizer):
    kind = "adagrad"
    n_slots = 1
    default_lr = 0.01

    def __init__(self, lr=None, epsilon=None, decay=0.0, **kw):
        super().__init__(lr=lr, decay=decay, **kw)
        self.epsilon = EPS if epsilon is None else float(epsilon)

    def hparams(self):
        return {"epsilon": self.epsilon}


class Adadelta(Optimizer):
    kind = "adadelta"
    n_slots = 2
    default_lr = 1.0

    def __init__(self, lr=None, rho=0.95, epsilon=None, decay=0.0, **kw):
        super().__init__(lr=lr, decay=decay, **kw)
        self.rho = float(rho)
        self.epsilon = EPS if epsilon is None else float(epsilon)

    def hparams(self):
        return {"rho": self.rho, "epsilon": self.epsilon}


class Adam(Optimizer):
    kind = "adam"
    n_slots = 2
    default_lr = 0.001

    def __init__(self, lr=None, beta_1=0.9, beta_2=0.999, epsilon=None, decay=0.0, amsgrad=False, **kw):
        super().__init__(lr=lr, decay=decay, **kw)
        self.beta_1, self.beta_2 = float(beta_1), float(beta_2)
        self.epsilon = EPS if epsilon is None else float(epsilon)
        self.amsgrad = bool(amsgrad)
        if self.amsgrad:             # third slot: the running maximum of v
            self.kind, self.n_slots = "amsgrad", 3

    def hparams(self):
        return {"beta_1": self.beta_1, "beta_2": self.beta_2, "epsilon": self.epsilon,
                "amsgrad": self.amsgrad}


class Adamax(Optimizer):
    kind = "adamax"
    n_slots = 2
    default_lr = 0.002

    def __init__(self, lr=None, beta_1=0.9, beta_2=0.999, epsilon=None, decay=0.0, **kw):
        super().__init__(lr=lr, decay=decay, **kw)
        self.beta_1, self.beta_2 = float(beta_1), float(beta_2)
        self.epsilon = EPS if epsilon is None else float(epsilon)

    def hparams(self):
        return {"beta_1": self.beta_1, "beta_2": self.beta_2, "epsilon": self.epsilon}


class Nadam(Optimizer):
    kind = "nadam"
    n_slots = 2
    default_lr = 0.002

    def __init__(self, lr=None, beta_1=0.9, beta_2=0.999, epsilon=None, schedule_decay=0.004, **kw):
        kw.pop("decay", None)
        super().__init__(lr=lr, **kw)
        self.beta_1, self.beta_2 = float(beta_1), float(beta_2)
        self.epsilon = EPS if epsilon is None else float(epsilon)
        self.schedule_decay = float(schedule_decay)
        self.m_schedule = 1.0        # host mirror (device keeps its own copy)

    def hparams(self):
        return {"beta_1": self.beta_1, "beta_2": self.beta_2, "epsilon": self.epsilon,
                "schedule_decay": self.schedule_decay}

    def get_config(self):
        cfg = {"lr": self.lr.get()}
        cfg.update(self.hparams())
        cfg.update(self._clip_config())
        return cfg


# lowercase aliases as accepted by keras.optimizers.get
_BY_NAME = {"sgd": SGD, "rmsprop": RMSprop, "adagrad": Adagrad, "adadelta": Adadelta, "adam": Adam,
            "adamax": Adamax, "nadam": Nadam}


def get(identifier) -> Optimizer:
    if isinstance(identifier, Optimizer):
        return identifier
    if hasattr(identifier, "_base_optimizer"):      # DistributedOptimizer wrapper
        return identifier
    if isinstance(identifier, type) and issubclass(identifier, Optimizer):
        return identifier()
    if isinstance(identifier, str):
        cls = _BY_NAME.get(identifier.lower())
        if cls is None:
            raise ValueError("unknown optimizer %r" % identifier)
        return cls()
    if isinstance(identifier, dict):
        return deserialize(identifier)
    raise ValueError("cannot interpret optimizer %r" % (identifier,))


def deserialize(cfg: dict) -> Optimizer:
    cls = _BY_NAME[cfg["class_name"].lower()]
    return cls.from_config(cfg.get("config", {}))


def serialize(opt: Optimizer) -> dict:
    base = getattr(opt, "_base_optimizer", opt)
    return {"class_name": type(base).__name__, "config": base.get_config()}
