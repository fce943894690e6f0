"""The tiny and odd models of tests/helpers/reg_models.py with a choice of hidden activation.

``act``: a string (the ``activation=`` of every hidden Conv2D / Dense), or ("LeakyReLU", alpha) /
("ELU", alpha) / ("Activation", name): linear layers, each followed by that layer (before the
pooling, as Keras wants it).  ``torch_forward`` is an independent autograd model of the same layer
chain in Keras' order (activate, then pool), for the tests that need a reference of their own."""
import numpy as np
import torch
import torch.nn.functional as F

from cori_intml_examples_amd.models import (ELU, Activation, Conv2D, Dense, Dropout, Flatten, Input, LeakyReLU,
                                            MaxPooling2D, Model)
from cori_intml_examples_amd.ops.rng import dropout_keep


def _hidden(h, layer_of, act):
    """layer_of(activation) builds the Conv2D / Dense; returns the activated tensor."""
    if isinstance(act, str) or act is None:
        return layer_of(act)(h)
    kind, arg = act
    h = layer_of(None)(h)
    return {"LeakyReLU": LeakyReLU, "ELU": ELU, "Activation": Activation}[kind](arg)(h)


def tiny(opt, device="cpu", channels=3, drop=0.0, act="relu", dp=False):
    inp = Input(shape=(16, 16, channels))
    h = inp
    for c in (4, 8, 8):
        h = _hidden(h, lambda a, c=c: Conv2D(c, kernel_size=(3, 3), activation=a, padding="same"), act)
        h = MaxPooling2D(pool_size=(2, 2))(h)
    h = Dropout(drop)(h)
    h = Flatten()(h)
    h = _hidden(h, lambda a: Dense(16, activation=a), act)
    h = Dropout(drop)(h)
    out = Dense(1, activation="sigmoid")(h)
    m = Model(inputs=inp, outputs=out, name="RPVClassifier", device=device)
    if dp:
        from cori_intml_examples_amd.parallel import hvd
        opt = hvd.DistributedOptimizer(opt)
    m.compile(optimizer=opt, loss="binary_crossentropy", metrics=["accuracy"])
    return m


def odd(opt, device="cpu", drop=0.0, act="relu"):
    inp = Input(shape=(19, 17, 2))
    h = _hidden(inp, lambda a: Conv2D(5, (3, 3), activation=a, padding="same"), act)
    h = MaxPooling2D((2, 2))(h)
    h = _hidden(h, lambda a: Conv2D(12, (3, 3), activation=a), act)
    h = MaxPooling2D((2, 2))(h)
    h = Flatten()(h)
    h = _hidden(h, lambda a: Dense(20, activation=a), act)
    h = Dropout(drop)(h)
    h = _hidden(h, lambda a: Dense(9, activation=a), act)
    out = Dense(3, activation="softmax")(h)
    m = Model(inp, out, device=device)
    m.compile(optimizer=opt, loss="categorical_crossentropy", metrics=["accuracy"])
    return m


def build(kind, opt, device="cpu", drop=0.0, act="relu"):
    return (tiny if kind == "tiny" else odd)(opt, device=device, drop=drop, act=act)


# ------------------------------------------------------------------------------------ independent autograd model
def _torch_act(name, alpha, x):
    if name in (None, "linear"):
        return x
    if name == "relu":
        return torch.relu(x)
    if name == "tanh":
        return torch.tanh(x)
    if name == "sigmoid":
        return torch.sigmoid(x)
    if name == "hard_sigmoid":
        return torch.clamp(0.2 * x + 0.5, 0.0, 1.0)
    if name == "elu":
        return F.elu(x, alpha)
    if name == "selu":
        return F.selu(x)
    if name == "softplus":
        return F.softplus(x)
    if name == "softsign":
        return F.softsign(x)
    if name == "leaky_relu":
        return F.leaky_relu(x, alpha)
    raise ValueError(name)


def torch_forward(model, weights, x, step=None):
    """Logits of ``model``'s layer chain on x [B, H, W, C] with ``weights`` (tensors in
    get_weights() order; give them requires_grad for autograd), layer by layer in Keras' order.
    ``step``: the dropout counter of a training step (None: inference, no dropout)."""
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
                s = layer.strides[0]
                th = max((-(-H // s) - 1) * s + kh - H, 0)
                tw = max((-(-W // s) - 1) * s + kw - W, 0)
                hn = F.pad(hn, (tw // 2, tw - tw // 2, th // 2, th - th // 2))
            hn = F.conv2d(hn, w.permute(3, 2, 0, 1), b, stride=layer.strides[0])
            h = _torch_act(layer.activation, 1.0, hn.permute(0, 2, 3, 1))
        elif cls == "Dense":
            w = next(it)
            h = h @ w
            if layer.use_bias:
                h = h + next(it)
            if k < len(layers) - 1 and not (k == len(layers) - 2 and type(layers[-1]).__name__ == "Activation"):
                h = _torch_act(layer.activation, 1.0, h)       # (the output activation lives in the loss)
        elif cls == "Activation":
            if k < len(layers) - 1:
                h = _torch_act(layer.activation, 1.0, h)
        elif cls == "LeakyReLU":
            h = _torch_act("leaky_relu", layer.alpha, h)
        elif cls == "ELU":
            h = _torch_act("elu", layer.alpha, h)
        elif cls == "MaxPooling2D":
            h = F.max_pool2d(h.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
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
    """(mean batch loss, [gradient per weight tensor]) of one training batch, by autograd in fp32."""
    ws = [torch.tensor(np.asarray(w), dtype=torch.float32, requires_grad=True) for w in model.get_weights()]
    z = torch_forward(model, ws, torch.as_tensor(x, dtype=torch.float32), step)
    yt = torch.as_tensor(np.asarray(y, np.float32))
    if z.shape[-1] == 1:
        loss = F.binary_cross_entropy_with_logits(z.reshape(-1), yt.reshape(-1))
    else:
        loss = -(yt * torch.log_softmax(z, -1)).sum(-1).mean()
    loss.backward()
    return float(loss.detach()), [w.grad.numpy() for w in ws]
