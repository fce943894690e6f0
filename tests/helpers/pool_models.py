"""Small models with AveragePooling2D / GlobalAveragePooling2D / GlobalMaxPooling2D layers, and
``torch_forward``: tests/helpers/act_models.py's independent autograd model of a layer chain in
Keras' order, extended by the three pooling layers and BatchNormalization (training statistics)."""
import numpy as np
import torch
import torch.nn.functional as F

from cori_intml_examples_amd.models import (Activation, AveragePooling2D, BatchNormalization, Conv2D, Dense, Dropout,
                                            Flatten, GlobalAveragePooling2D, GlobalMaxPooling2D, Input,
                                            MaxPooling2D, Model)
from cori_intml_examples_amd.ops.rng import dropout_keep

from helpers.act_models import _torch_act

KINDS = ("avg_tiny", "avg_odd_gap", "max_gmp", "tanh_avg", "bn_gap")


def _finish(inp, out, opt, device, dp=False):
    m = Model(inp, out, device=device)
    if dp:
        from cori_intml_examples_amd.parallel import hvd
        opt = hvd.DistributedOptimizer(opt)
    loss = "binary_crossentropy" if out.shape[-1] == 1 else "categorical_crossentropy"
    m.compile(optimizer=opt, loss=loss, metrics=["accuracy"])
    return m


def avg_tiny(opt, device="cpu", drop=0.0, dp=False):
    """16x16x3, three Conv(relu) + AveragePooling2D, Dense(16), sigmoid head."""
    h = inp = Input(shape=(16, 16, 3))
    for c in (4, 8, 8):
        h = AveragePooling2D((2, 2))(Conv2D(c, (3, 3), activation="relu", padding="same")(h))
    h = Flatten()(Dropout(drop)(h))
    h = Dropout(drop)(Dense(16, activation="relu")(h))
    return _finish(inp, Dense(1, activation="sigmoid")(h), opt, device, dp)


def avg_odd_gap(opt, device="cpu", drop=0.0):
    """19x17x2 odd sizes: avg pools (one over an odd grid, with a dropout), then
    GlobalAveragePooling2D -> Dropout -> Dense(20) -> softmax(3)."""
    inp = Input(shape=(19, 17, 2))
    h = AveragePooling2D()(Conv2D(5, (3, 3), activation="relu", padding="same")(inp))     # 19x17 -> 9x8
    h = Dropout(drop)(h)
    h = AveragePooling2D()(Conv2D(12, (3, 3), activation="relu")(h))                      # 7x6 -> 3x3
    h = Dropout(drop)(GlobalAveragePooling2D()(h))
    h = Dense(20, activation="relu")(h)
    return _finish(inp, Dense(3, activation="softmax")(h), opt, device)


def max_gmp(opt, device="cpu", drop=0.0):
    """max-pooled convs -> GlobalMaxPooling2D -> softmax(3) head directly."""
    inp = Input(shape=(16, 16, 3))
    h = MaxPooling2D()(Conv2D(6, (3, 3), activation="relu", padding="same")(inp))
    h = Dropout(drop)(MaxPooling2D()(Conv2D(12, (3, 3), activation="relu", padding="same")(h)))
    h = GlobalMaxPooling2D()(h)
    return _finish(inp, Dense(3, activation="softmax")(h), opt, device)


def tanh_avg(opt, device="cpu", drop=0.0):
    """tanh convs (one as a layer) with average pools, Flatten, a tanh Dense."""
    inp = Input(shape=(16, 16, 3))
    h = AveragePooling2D()(Conv2D(4, (3, 3), activation="tanh", padding="same")(inp))
    h = Dropout(drop)(AveragePooling2D()(Activation("tanh")(Conv2D(8, (3, 3), padding="same")(h))))
    h = Dense(16, activation="tanh")(Flatten()(h))
    return _finish(inp, Dense(1, activation="sigmoid")(h), opt, device)


def bn_gap(opt, device="cpu", drop=0.0):
    """BN conv stages (one max-pooled) -> GlobalAveragePooling2D -> Dropout -> Dense -> sigmoid.  The
    convs have no bias: ahead of a BatchNormalization its gradient is zero analytically, and what a
    backend computes there is its own rounding noise."""
    inp = Input(shape=(16, 16, 3))
    h = MaxPooling2D()(Activation("relu")(BatchNormalization()(Conv2D(6, (3, 3), padding="same", use_bias=False)(inp))))
    h = Activation("relu")(BatchNormalization()(Conv2D(8, (3, 3), padding="same", use_bias=False)(h)))
    h = Dropout(drop)(GlobalAveragePooling2D()(h))
    h = Dense(16, activation="relu")(h)
    return _finish(inp, Dense(1, activation="sigmoid")(h), opt, device)


def build(kind, opt, device="cpu", drop=0.0):
    return globals()[kind](opt, device=device, drop=drop)


# ------------------------------------------------------------------------------------ independent autograd model
def torch_forward(model, weights, x, step=None):
    """Logits of ``model``'s layer chain on x [B, H, W, C] with ``weights`` (tensors in get_weights()
    order), layer by layer in Keras' order; ``step``: the dropout counter of a training step (None:
    no dropout).  BatchNormalization uses the batch statistics (a training step)."""
    it = iter(weights)
    h = torch.as_tensor(x)
    stream = 0
    layers = model.layers[1:]
    for k, layer in enumerate(layers):
        cls = type(layer).__name__
        if cls == "Conv2D":
            w = next(it)
            b = next(it) if layer.use_bias else None
            hn = h.permute(0, 3, 1, 2)
            if layer.padding == "same":
                kh, kw = layer.kernel_size
                H, W = h.shape[1], h.shape[2]
                th, tw = max(kh - 1, 0), max(kw - 1, 0)          # (stride 1)
                hn = F.pad(hn, (tw // 2, tw - tw // 2, th // 2, th - th // 2))
            hn = F.conv2d(hn, w.permute(3, 2, 0, 1), b, stride=layer.strides[0])
            h = _torch_act(layer.activation, 1.0, hn.permute(0, 2, 3, 1))
        elif cls == "Dense":
            w = next(it)
            h = h @ w
            if layer.use_bias:
                h = h + next(it)
            if k < len(layers) - 1:
                h = _torch_act(layer.activation, 1.0, h)       # (the output activation lives in the loss)
        elif cls == "Activation":
            h = _torch_act(layer.activation, 1.0, h)
        elif cls == "BatchNormalization":
            gamma, beta = next(it), next(it)
            next(it), next(it)                                  # moving mean / variance: not used in training
            ax = tuple(range(h.dim() - 1))
            mean = h.mean(ax)
            var = ((h - mean) ** 2).mean(ax)
            h = gamma * (h - mean) / torch.sqrt(var + layer.epsilon) + beta
        elif cls == "MaxPooling2D":
            h = F.max_pool2d(h.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
        elif cls == "AveragePooling2D":
            h = F.avg_pool2d(h.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
        elif cls == "GlobalAveragePooling2D":
            h = h.mean((1, 2))
        elif cls == "GlobalMaxPooling2D":
            h = h.reshape(h.shape[0], -1, h.shape[-1]).max(1).values
        elif cls == "Dropout":
            stream += 1
            if step is not None and layer.rate > 0:
                keep = dropout_keep(h.numel(), layer.rate, model._seed, stream, step).view(h.shape)
                h = h * keep.to(h.dtype) / (1.0 - layer.rate)
        elif cls == "Flatten":
            h = h.reshape(h.shape[0], -1)
        else:
            raise ValueError(cls)
    return h


def torch_loss_grads(model, x, y, step=1):
    """(mean batch loss, [gradient per TRAINABLE weight tensor, in get_weights() order]) of one
    training batch, by autograd in fp32."""
    ws = [torch.tensor(np.asarray(w), dtype=torch.float32, requires_grad=True) for w in model.get_weights()]
    z = torch_forward(model, ws, torch.as_tensor(x, dtype=torch.float32), step)
    yt = torch.as_tensor(np.asarray(y, np.float32))
    if z.shape[-1] == 1:
        loss = F.binary_cross_entropy_with_logits(z.reshape(-1), yt.reshape(-1))
    else:
        loss = -(yt * torch.log_softmax(z, -1)).sum(-1).mean()
    loss.backward()
    return float(loss.detach()), [None if w.grad is None else w.grad.numpy() for w in ws]
