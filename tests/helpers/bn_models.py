"""Small models with BatchNormalization stages, and an independently written autograd model of the
same layer chain in Keras' order: layer(linear) -> BatchNormalization -> activation -> pool -> dropout.

``act``: "relu" / a table activation string (an ``Activation`` layer behind each BN), or
("LeakyReLU", alpha) / ("ELU", alpha), or None (no activation layer)."""
import numpy as np
import torch
import torch.nn.functional as F

from cori_intml_examples_amd.models import (ELU, Activation, BatchNormalization, Conv2D, Dense, Dropout, Flatten,
                                            Input, LeakyReLU, MaxPooling2D, Model)
from cori_intml_examples_amd.ops.rng import dropout_keep

from helpers.act_models import _torch_act


def _act_layer(act):
    if act is None:
        return None
    if isinstance(act, str):
        return Activation(act)
    return {"LeakyReLU": LeakyReLU, "ELU": ELU}[act[0]](act[1])


def bn_stage(h, layer, act, **bn_kw):
    h = BatchNormalization(**bn_kw)(layer(h))
    a = _act_layer(act)
    return a(h) if a is not None else h


def _compile(m, opt, loss, dp=False):
    if dp:
        from cori_intml_examples_amd.parallel import hvd
        opt = hvd.DistributedOptimizer(opt)
    m.compile(optimizer=opt, loss=loss, metrics=["accuracy"])
    return m


def tiny(opt, device="cpu", channels=3, drop=0.0, act="relu", dp=False, **bn_kw):
    """Three pooled conv + BN stages and one dense + BN (16x16 inputs)."""
    inp = Input(shape=(16, 16, channels))
    h = inp
    for c in (4, 8, 8):
        h = bn_stage(h, Conv2D(c, kernel_size=(3, 3), padding="same"), act, **bn_kw)
        h = MaxPooling2D(pool_size=(2, 2))(h)
    h = Dropout(drop)(h)
    h = Flatten()(h)
    h = bn_stage(h, Dense(16), act, **bn_kw)
    h = Dropout(drop)(h)
    out = Dense(1, activation="sigmoid")(h)
    return _compile(Model(inputs=inp, outputs=out, name="RPVClassifier", device=device), opt, "binary_crossentropy", dp)


def odd(opt, device="cpu", drop=0.0, act="relu", **bn_kw):
    """Odd sizes (19x17: the last row / column outside every window), an un-pooled BN conv with 12
    filters (channel stride 16), two denses of which one has no BN.  The dropout sits on a dense
    stage, as in helpers/act_models.py (tiny has the one on a pooled conv stage)."""
    inp = Input(shape=(19, 17, 2))
    h = bn_stage(inp, Conv2D(5, (3, 3), padding="same"), act, **bn_kw)
    h = MaxPooling2D((2, 2))(h)
    h = bn_stage(h, Conv2D(12, (3, 3)), act, **bn_kw)          # un-pooled, 7 x 6
    h = Flatten()(h)
    h = bn_stage(h, Dense(20), act, **bn_kw)
    h = Dropout(drop)(h)
    h = Dense(9, activation="relu")(h)
    out = Dense(3, activation="softmax")(h)
    return _compile(Model(inp, out, device=device), opt, "categorical_crossentropy")


def build(kind, opt, device="cpu", drop=0.0, act="relu", **bn_kw):
    return (tiny if kind == "tiny" else odd)(opt, device=device, drop=drop, act=act, **bn_kw)


# ------------------------------------------------------------------------------------ independent autograd model
def torch_forward(model, weights, x, step=None, stats=None):
    """Logits of ``model``'s layer chain on x [B, H, W, C] with ``weights`` (tensors in
    get_weights() order), layer by layer in Keras' order.  ``step``: the dropout counter of a
    training step -- BN then uses the batch statistics (appended to ``stats`` as (layer name, mean,
    biased var, m)); None: inference with the moving statistics and no dropout."""
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
                th, tw = max(kh - 1, 0), max(kw - 1, 0)          # stride 1
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
        elif cls == "BatchNormalization":
            C = h.shape[-1]
            gamma = next(it) if layer.scale else torch.ones(C, dtype=h.dtype)
            beta = next(it) if layer.center else torch.zeros(C, dtype=h.dtype)
            mm, mv = next(it), next(it)
            if step is None:
                h = gamma * (h - mm) / torch.sqrt(mv + layer.epsilon) + beta
            else:
                h2 = h.reshape(-1, C)
                mean = h2.mean(0)
                var = ((h2 - mean) ** 2).mean(0)
                if stats is not None:
                    stats.append((layer.name, mean.detach().numpy().copy(), var.detach().numpy().copy(), h2.shape[0]))
                h = gamma * (h - mean) / torch.sqrt(var + layer.epsilon) + beta
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


def torch_loss_grads(model, x, y, step=1, dtype=torch.float32):
    """(mean batch loss, [gradient per weight tensor or None for the moving statistics], BN batch
    statistics) of one training batch, by autograd."""
    specs = model.store.specs
    ws = [torch.tensor(np.asarray(w), dtype=dtype, requires_grad=s.trainable)
          for w, s in zip(model.get_weights(), specs)]
    stats = []
    z = torch_forward(model, ws, torch.as_tensor(np.asarray(x), dtype=dtype), step, stats)
    yt = torch.as_tensor(np.asarray(y), dtype=dtype)
    if z.shape[-1] == 1:
        loss = F.binary_cross_entropy_with_logits(z.reshape(-1), yt.reshape(-1))
    else:
        loss = -(yt * torch.log_softmax(z, -1)).sum(-1).mean()
    loss.backward()
    return float(loss.detach()), [w.grad.numpy() if w.grad is not None else None for w in ws], stats
