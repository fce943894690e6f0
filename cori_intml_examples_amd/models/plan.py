"""Fused stage plan: groups a Keras layer chain into the kernels that execute it.

The reference runs every Keras layer as separate TF ops.  Here a
model is compiled into *stages*, each of which maps onto one fused HIP kernel
family on gfx950:

  ConvStage   Conv2D(+ReLU) [+MaxPool 2x2] [+Dropout]   -> conv_mm (fwd epilogue)
  DenseStage  Dense(+ReLU) [+Dropout]                   -> dense split-K + epilogue
  HeadStage   final Dense + softmax/sigmoid + loss      -> head_fused (fwd+loss+bwd)

A hidden activation other than relu / linear (``act``: a name of ops/reference.py ACTIVATIONS,
from the layer's ``activation=`` or from an Activation / LeakyReLU / ELU layer directly behind a
linear Conv2D / Dense) makes the stage ``dropout(A(maxpool(conv)))``: its kernels run in their
linear form and one element-wise launch per direction follows them (act.hip).  A is
non-decreasing, so this equals Keras' ``maxpool(A(conv))``.

A BatchNormalization directly behind a linear Conv2D / hidden Dense (``bn``) makes the stage
``dropout(maxpool(A(BN(conv))))``: the linear kernels store the un-pooled pre-activation, and the
bn.hip launches normalise, activate (relu), pool and drop.  gamma may be negative, so the pool is
never taken before BN.

An AveragePooling2D in MaxPooling2D's place (``pool_kind`` 'avg') makes the stage
``dropout(avgpool(A(conv)))``, Keras' own order: averaging does not commute with A, so the conv
kernel (with its relu) and the activation launch run un-pooled, and the pool.hip launches average
and drop.  A GlobalAveragePooling2D / GlobalMaxPooling2D in Flatten's place is a stage of its own
without weights (``Plan.gpool``), with the Dropout behind it.

The plan is backend-agnostic; executors (``executor_ref`` / ``executor_hip``)
interpret it.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Tuple

from .layers import (ELU, Activation, AveragePooling2D, BatchNormalization, Conv2D, Dense, Dropout, Flatten,
                     GlobalAveragePooling2D, GlobalMaxPooling2D, InputLayer, Layer, LeakyReLU, MaxPooling2D, activation_of)
from ..ops.reference import conv_pads


@dataclass
class ConvStage:
    conv: Conv2D
    in_shape: Tuple[int, int, int]          # H, W, Cin
    conv_shape: Tuple[int, int, int]        # Ho, Wo, Cout (pre-pool)
    out_shape: Tuple[int, int, int]         # post-pool shape
    relu: bool
    pool: Optional[MaxPooling2D] = None
    dropout: Optional[Dropout] = None
    stream: int = 0                         # RNG stream id of the dropout
    act: Optional[str] = None               # hidden activation other than relu / linear (None for those)
    act_alpha: float = 0.0
    bn: Optional[BatchNormalization] = None  # dropout(maxpool(A(BN(conv)))): the pool is NOT taken before BN

    @property
    def pool_kind(self) -> Optional[str]:
        """'max' | 'avg' | None: what ``pool`` is."""
        return None if self.pool is None else "avg" if isinstance(self.pool, AveragePooling2D) else "max"

    @property
    def rate(self) -> float:
        return self.dropout.rate if self.dropout is not None else 0.0

    @property
    def stride(self) -> int:
        return self.conv.strides[0]

    @property
    def pads(self):
        H, W, _ = self.in_shape
        kh, kw = self.conv.kernel_size
        return conv_pads(H, W, kh, kw, self.stride, self.conv.padding)


@dataclass
class DenseStage:
    dense: Dense
    K: int
    N: int
    relu: bool
    dropout: Optional[Dropout] = None
    stream: int = 0
    flat_from: Optional[Tuple[int, int, int]] = None   # (H,W,C) if the input comes from a Flatten
    act: Optional[str] = None               # hidden activation other than relu / linear (None for those)
    act_alpha: float = 0.0
    bn: Optional[BatchNormalization] = None  # dropout(A(BN(dense)))

    @property
    def rate(self) -> float:
        return self.dropout.rate if self.dropout is not None else 0.0


@dataclass
class GlobalPoolStage:
    """GlobalAveragePooling2D / GlobalMaxPooling2D behind the last conv stage [+ Dropout]: a stage
    of its own without weights, (H, W, C) -> (C,)."""
    layer: Layer
    mode: str                               # 'avg' | 'max'
    in_shape: Tuple[int, int, int]          # H, W, C: the last conv stage's output
    dropout: Optional[Dropout] = None
    stream: int = 0
    relu = False
    act = None
    act_alpha = 0.0
    bn = None

    @property
    def rate(self) -> float:
        return self.dropout.rate if self.dropout is not None else 0.0


@dataclass
class HeadStage:
    dense: Dense
    K: int
    N: int
    activation: Optional[str]     # 'softmax' | 'sigmoid' | None
    loss: str                     # canonical loss name
    flat_from: Optional[Tuple[int, int, int]] = None


@dataclass
class Plan:
    input_shape: Tuple[int, ...]
    convs: List[ConvStage] = field(default_factory=list)
    denses: List[DenseStage] = field(default_factory=list)
    head: Optional[HeadStage] = None
    gpool: Optional[GlobalPoolStage] = None

    @property
    def stages(self):
        return (list(self.convs) + ([self.gpool] if self.gpool else []) + list(self.denses)
                + ([self.head] if self.head else []))


# every Keras name (and alias) of a loss -> its canonical name
LOSS_ALIASES = {"categorical_crossentropy": "categorical_crossentropy",
                "binary_crossentropy": "binary_crossentropy",
                "mse": "mse", "MSE": "mse", "mean_squared_error": "mse",
                "sparse_categorical_crossentropy": "sparse_categorical_crossentropy",
                "mae": "mae", "MAE": "mae", "mean_absolute_error": "mae",
                "msle": "msle", "MSLE": "msle", "mean_squared_logarithmic_error": "msle",
                "logcosh": "logcosh", "hinge": "hinge", "squared_hinge": "squared_hinge",
                "categorical_hinge": "categorical_hinge",
                "kld": "kld", "KLD": "kld", "kullback_leibler_divergence": "kld",
                "poisson": "poisson"}
# the losses that go with every output activation (README, "Losses"); the crossentropies keep
# their own activation
TABLE_LOSSES = ("mse", "mae", "msle", "logcosh", "hinge", "squared_hinge", "categorical_hinge", "kld", "poisson")


def canonical_loss(loss) -> str:
    """The canonical name of a Keras loss name, alias, or loss function (by its ``__name__``)."""
    name = loss if isinstance(loss, str) else getattr(loss, "__name__", str(loss))
    if name not in LOSS_ALIASES:
        raise NotImplementedError("loss %r is not implemented" % (name,))
    return LOSS_ALIASES[name]


def classic_head(activation, loss: str, N: int) -> bool:
    """True for the three (activation, loss) pairs of the first head kernel at the widths it
    supports: softmax + (sparse_)categorical_crossentropy, sigmoid + binary_crossentropy
    at N == 1, linear + mse (a linear output with a crossentropy name has always run as mse).
    Every other pair runs the loss head."""
    if activation == "softmax":
        return loss in ("categorical_crossentropy", "sparse_categorical_crossentropy")
    if activation == "sigmoid":
        return loss == "binary_crossentropy" and N == 1
    return loss not in TABLE_LOSSES or loss == "mse"


def binary_accuracy_head(loss: str, N: int) -> bool:
    """Keras' ``compile`` rule for 'acc': binary_accuracy (mean over the columns of
    [rint(p) == y]) for a one-column output or binary_crossentropy, else categorical_accuracy."""
    return N == 1 or loss == "binary_crossentropy"


ACT_LAYERS = (Activation, LeakyReLU, ELU)


def _stage_act(layer, name, alpha, what):
    """(relu, act, act_alpha) of a hidden stage whose activation is ``name``."""
    if name is None:
        return False, None, 0.0
    if name == "relu":
        return True, None, 0.0
    if name == "softmax":
        raise NotImplementedError("%s activation softmax (layer %s): softmax is an output activation" % (what, layer.name))
    return False, name, float(alpha)


def build_plan(layers: List[Layer], loss) -> Plan:
    """``layers`` is the linear chain starting with an InputLayer."""
    if not layers or not isinstance(layers[0], InputLayer):
        raise ValueError("model must start with an input layer")
    loss = canonical_loss(loss)
    plan = Plan(input_shape=tuple(layers[0].output_shape_))
    cur_conv: Optional[ConvStage] = None
    cur_dense: Optional[DenseStage] = None
    flat_from = None
    body = layers[1:]
    stream = 0
    open_stage = None          # (stage, its Conv2D / Dense): an activation layer may still fold into it
    prev = layers[0]
    skip = False
    for i, layer in enumerate(body):
        last = i == len(body) - 1
        before, prev = prev, layer
        if skip:                # the output Activation layer, taken by the head Dense before it
            skip = False
            continue
        if not isinstance(layer, ACT_LAYERS + (Conv2D, Dense, BatchNormalization)):
            open_stage = None
        if isinstance(layer, BatchNormalization):
            if isinstance(before, BatchNormalization):
                raise NotImplementedError("layer %s follows %s: two BatchNormalization layers on one stage"
                                          % (layer.name, before.name))
            if plan.head is not None or (last and isinstance(before, Dense)):
                raise NotImplementedError("layer %s follows %s, the output Dense: BatchNormalization behind the "
                                          "output layer is not implemented"
                                          % (layer.name, (plan.head.dense if plan.head is not None else before).name))
            if isinstance(before, (Conv2D, Dense)) and before.activation is not None:
                raise NotImplementedError("layer %s follows %s, which already has the activation %s: "
                                          "BatchNormalization must follow a linear Conv2D or Dense (put the "
                                          "activation behind it as a layer)"
                                          % (layer.name, before.name, before.activation))
            if open_stage is None or before is not open_stage[1]:
                raise NotImplementedError("layer %s follows %s: BatchNormalization must directly follow a linear "
                                          "Conv2D or hidden Dense (before any activation, pooling, dropout or "
                                          "flatten)" % (layer.name, before.name))
            open_stage[0].bn = layer
        elif isinstance(layer, ACT_LAYERS):
            name, alpha = activation_of(layer)
            if open_stage is None:
                owner = before if isinstance(before, (Conv2D, Dense)) else None
                if owner is not None and owner.activation is not None:
                    raise NotImplementedError("layer %s follows %s, which already has the activation %s: two "
                                              "activations on one stage" % (layer.name, owner.name, owner.activation))
                raise NotImplementedError("layer %s follows %s: an activation layer must directly follow a Conv2D "
                                          "or Dense (before any pooling, dropout or flatten)"
                                          % (layer.name, before.name))
            stage, owner = open_stage
            if stage.relu or stage.act is not None:
                raise NotImplementedError("layer %s follows %s and %s: two activations on one stage"
                                          % (layer.name, owner.name, before.name))
            stage.relu, stage.act, stage.act_alpha = _stage_act(layer, name, alpha, "hidden")
            if name is not None:
                open_stage = None
        elif isinstance(layer, Conv2D):
            if plan.gpool is not None:
                raise NotImplementedError("layer %s follows %s: Conv2D after a global pooling layer"
                                          % (layer.name, plan.gpool.layer.name))
            if plan.denses or flat_from is not None:
                raise NotImplementedError("Conv2D after Flatten/Dense")
            relu, act, alpha = _stage_act(layer, layer.activation, 1.0 if layer.activation == "elu" else 0.0, "conv")
            cur_conv = ConvStage(conv=layer, in_shape=tuple(layer.input_shape),
                                 conv_shape=tuple(layer.output_shape_),
                                 out_shape=tuple(layer.output_shape_), relu=relu, act=act, act_alpha=alpha)
            plan.convs.append(cur_conv)
            cur_dense = None
            open_stage = (cur_conv, layer) if layer.activation is None else None
        elif isinstance(layer, MaxPooling2D):       # (AveragePooling2D too)
            if cur_conv is None or cur_conv.pool is not None or cur_conv.dropout is not None or plan.gpool is not None:
                raise NotImplementedError("%s must directly follow a Conv2D" % type(layer).__name__)
            if isinstance(layer, AveragePooling2D) and cur_conv.bn is not None:
                raise NotImplementedError("layer %s follows %s on the stage of %s: AveragePooling2D on a "
                                          "BatchNormalization stage is not implemented"
                                          % (layer.name, cur_conv.bn.name, cur_conv.conv.name))
            cur_conv.pool = layer
            cur_conv.out_shape = tuple(layer.output_shape_)
        elif isinstance(layer, (GlobalAveragePooling2D, GlobalMaxPooling2D)):
            what = type(layer).__name__
            if plan.gpool is not None:
                raise NotImplementedError("layer %s follows %s: two global pooling layers"
                                          % (layer.name, plan.gpool.layer.name))
            if flat_from is not None or plan.denses:
                raise NotImplementedError("layer %s follows %s: %s behind a Flatten or Dense"
                                          % (layer.name, before.name, what))
            if cur_conv is None:
                raise NotImplementedError("layer %s follows %s: %s must follow the last conv stage (not the "
                                          "model input)" % (layer.name, before.name, what))
            plan.gpool = GlobalPoolStage(layer=layer, mode=layer.mode, in_shape=tuple(layer.input_shape))
            cur_conv = None
        elif isinstance(layer, Dropout):
            stream += 1
            tgt = cur_dense if cur_dense is not None else cur_conv
            if tgt is None and plan.gpool is not None and not plan.denses and plan.head is None:
                tgt = plan.gpool
            if tgt is None:
                raise NotImplementedError("Dropout directly on the model input")
            if tgt.dropout is not None:
                raise NotImplementedError("two consecutive Dropout layers")
            tgt.dropout = layer
            tgt.stream = stream
        elif isinstance(layer, Flatten):
            if plan.gpool is not None:
                raise NotImplementedError("layer %s follows %s: Flatten behind a global pooling layer"
                                          % (layer.name, plan.gpool.layer.name))
            if flat_from is not None or plan.denses:
                raise NotImplementedError("Flatten after Dense")
            flat_from = tuple(layer.input_shape)
        elif isinstance(layer, Dense):
            if len(layer.input_shape) != 1:
                raise ValueError("Dense on non-flat input")
            ff = flat_from if not plan.denses else None
            open_stage = None
            out_act = body[i + 1] if i == len(body) - 2 and isinstance(body[i + 1], ACT_LAYERS) else None
            if last or out_act is not None:
                act = layer.activation
                if out_act is not None:
                    # Dense(n) + Activation("softmax" | "sigmoid") as the last two layers: the head
                    if act is not None:
                        raise NotImplementedError("layer %s follows %s, which already has the activation %s: two "
                                                  "activations on one stage" % (out_act.name, layer.name, act))
                    act, skip = activation_of(out_act)[0], True
                if act not in (None, "softmax", "sigmoid"):
                    raise NotImplementedError("output activation %s" % act)
                plan.head = HeadStage(dense=layer, K=layer.input_shape[0], N=layer.units,
                                      activation=act, loss=loss, flat_from=ff)
            else:
                relu, act, alpha = _stage_act(layer, layer.activation, 1.0 if layer.activation == "elu" else 0.0,
                                              "hidden Dense")
                cur_dense = DenseStage(dense=layer, K=layer.input_shape[0], N=layer.units,
                                       relu=relu, flat_from=ff, act=act, act_alpha=alpha)
                plan.denses.append(cur_dense)
                open_stage = (cur_dense, layer) if layer.activation is None else None
            cur_conv = None
        else:
            raise NotImplementedError("layer type %s" % type(layer).__name__)
    if plan.head is None:
        raise NotImplementedError("the model must end with a Dense layer")
    if plan.head.activation == "softmax" and loss not in ("categorical_crossentropy",
                                                          "sparse_categorical_crossentropy") + TABLE_LOSSES:
        raise NotImplementedError("softmax output with loss %s" % loss)
    if plan.head.activation == "sigmoid" and loss not in ("binary_crossentropy",) + TABLE_LOSSES:
        raise NotImplementedError("sigmoid output with loss %s" % loss)
    return plan
