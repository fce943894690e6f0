"""DepthwiseConv2D / SeparableConv2D without a GPU: configs, weights, rejected arguments and positions,
the CPU executor against an independent float64 autograd model, the HDF5 round trip, the compat names
and the builders' ``separable=``."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cori_intml_examples_amd import Conv2D, Dense, Dropout, Flatten, Input, MaxPooling2D, Model, optim
from cori_intml_examples_amd.models import BatchNormalization, DepthwiseConv2D, SeparableConv2D
from cori_intml_examples_amd.models.layers import LAYER_CLASSES
from cori_intml_examples_amd.utils import set_random_seed

CPU = torch.device("cpu")


def _model(layers, shape, out=1):
    h = inp = Input(shape=shape)
    for l in layers:
        h = l(h)
    m = Model(inp, Dense(out, activation="sigmoid")(h), device=CPU)
    m.compile(optimizer=optim.SGD(lr=0.0), loss="binary_crossentropy", metrics=["accuracy"])
    return m


def test_weights_names_shapes_counts_and_configs():
    m = _model([SeparableConv2D(32, 3, activation="relu", depthwise_regularizer="l2"), DepthwiseConv2D((3, 3), strides=2),
                Flatten()], (9, 9, 16))
    sep, dw = m.layers[1], m.layers[2]
    assert sep.name.startswith("separable_conv2d_") and dw.name.startswith("depthwise_conv2d_")
    assert [(s[0], s[1]) for s in sep.weight_specs()] == [("depthwise_kernel", (3, 3, 16, 1)),
                                                           ("pointwise_kernel", (1, 1, 16, 32)), ("bias", (32,))]
    assert [(s[0], s[1]) for s in dw.weight_specs()] == [("depthwise_kernel", (3, 3, 32, 1)), ("bias", (32,))]
    assert sep.count_params() == 144 + 512 + 32 and dw.count_params() == 288 + 32
    assert sep.output_shape_ == (7, 7, 32) and dw.output_shape_ == (3, 3, 32)
    assert list(sep.weight_regularizers()) == ["depthwise_kernel"]
    for l in (sep, dw):
        cfg = l.get_config()
        assert cfg["depth_multiplier"] == 1 and "depthwise_initializer" in cfg and cfg["depthwise_constraint"] is None
        back = LAYER_CLASSES[type(l).__name__].from_config(cfg)
        assert back.get_config() == cfg
    assert "pointwise_regularizer" in sep.get_config() and sep.get_config()["filters"] == 32


@pytest.mark.parametrize("cls,args", [(DepthwiseConv2D, (3,)), (SeparableConv2D, (8, 3))])
@pytest.mark.parametrize("kw,word", [({"depth_multiplier": 2}, "depth_multiplier"), ({"strides": (1, 2)}, "anisotropic"),
                                     ({"dilation_rate": 2}, "dilation_rate"), ({"data_format": "channels_first"}, "channels_last"),
                                     ({"activity_regularizer": "l2"}, "activity_regularizer"),
                                     ({"depthwise_constraint": "max_norm"}, "depthwise_constraint"),
                                     ({"bias_constraint": "non_neg"}, "bias_constraint")])
def test_rejected_arguments_name_the_layer(cls, args, kw, word):
    with pytest.raises(NotImplementedError, match=word) as e:
        cls(*args, name="the_layer", **kw)
    assert "the_layer" in str(e.value)


@pytest.mark.parametrize("behind", [lambda: MaxPooling2D((2, 2)), BatchNormalization, lambda: Dropout(0.2)])
def test_layers_that_may_not_follow_a_depthwise_conv(behind):
    nxt = behind()
    with pytest.raises(NotImplementedError, match="directly behind a DepthwiseConv2D") as e:
        _model([DepthwiseConv2D(3, name="dwl"), nxt, Flatten()], (8, 8, 4))
    assert "dwl" in str(e.value) and nxt.name in str(e.value)


def test_plan_stages():
    m = _model([SeparableConv2D(8, 3, strides=2, padding="same", activation="relu"), MaxPooling2D((2, 2)), Dropout(0.1),
                DepthwiseConv2D(3, activation="relu"), Flatten()], (16, 16, 3))
    a, b, c = m._plan.convs
    assert (a.depthwise, a.relu, a.use_bias, a.stride, a.out_shape, a.pool, a.wname) == \
        (True, False, False, 2, (8, 8, 3), None, "depthwise_kernel")
    assert (b.pointwise, b.relu, b.use_bias, b.stride, b.kernel_size, b.in_shape, b.out_shape, b.wname) == \
        (True, True, True, 1, (1, 1), (8, 8, 3), (4, 4, 8), "pointwise_kernel")
    assert b.pool is not None and b.rate == 0.1 and a.conv is b.conv
    assert (c.depthwise, c.relu, c.use_bias, c.out_shape) == (True, True, True, (2, 2, 8))


def _torch_forward(m, x, mask_of):
    """The model in float64 torch autograd, written from the Keras definitions: returns (loss, weights)."""
    ws = [torch.tensor(w, dtype=torch.float64, requires_grad=True) for w in m.get_weights()]
    it = iter(ws)
    h = torch.tensor(x, dtype=torch.float64).permute(0, 3, 1, 2)

    def conv(h, w, l, groups=1):
        if l.padding == "same":
            from cori_intml_examples_amd.ops.reference import conv_pads
            pt, pb, pl, pr = conv_pads(h.shape[2], h.shape[3], w.shape[2], w.shape[3], l.strides[0], "same")
            h = F.pad(h, (pl, pr, pt, pb))
        return F.conv2d(h, w, stride=l.strides[0], groups=groups)
    for l in m.layers[1:]:
        kind = type(l).__name__
        if kind in ("SeparableConv2D", "DepthwiseConv2D"):
            h = conv(h, next(it).permute(2, 3, 0, 1), l, groups=h.shape[1])
            if kind == "SeparableConv2D":
                h = F.conv2d(h, next(it).permute(3, 2, 0, 1))
        elif kind == "Conv2D":
            h = conv(h, next(it).permute(3, 2, 0, 1), l)
        elif kind == "MaxPooling2D":
            h = F.max_pool2d(h, 2)
        elif kind == "Dropout":
            h = h * mask_of(l, tuple(h.permute(0, 2, 3, 1).shape)).permute(0, 3, 1, 2)
        elif kind == "Flatten":
            h = h.permute(0, 2, 3, 1).reshape(h.shape[0], -1)
        elif kind == "Dense":
            h = h @ next(it)
        if kind in ("SeparableConv2D", "DepthwiseConv2D", "Conv2D", "Dense") and l.use_bias:
            b = next(it)
            h = h + (b.view(1, -1, 1, 1) if h.dim() == 4 else b)
        if getattr(l, "activation", None) == "relu":
            h = torch.relu(h)
    return h, ws


MODELS = {
    "sep_pool_drop": lambda: ([Conv2D(6, 3, activation="relu"), SeparableConv2D(8, 3, padding="same", activation="relu"),
                               MaxPooling2D((2, 2)), Dropout(0.25), Flatten()], (10, 9, 2)),
    "dw_between_convs": lambda: ([Conv2D(5, 3, activation="relu"), DepthwiseConv2D(3, strides=2, padding="same", activation="relu"),
                                  Conv2D(4, 3, activation="relu"), Flatten()], (12, 12, 1)),
    "sep_first": lambda: ([SeparableConv2D(8, 5, strides=2, activation="relu"), Flatten()], (11, 11, 3)),
}


@pytest.mark.parametrize("kind", sorted(MODELS))
def test_cpu_executor_matches_float64_autograd(kind):
    from cori_intml_examples_amd.ops.rng import dropout_keep
    set_random_seed(11)
    layers, shape = MODELS[kind]()
    m = _model(layers, shape)
    rs = np.random.RandomState(0)
    x, y = rs.rand(5, *shape).astype(np.float32), (rs.rand(5) > 0.5).astype(np.float32)
    ex = m._executor
    d = ex.upload(x, y)
    ex.train_step(d, torch.arange(5), 0, 5)
    streams = iter(range(1, 9))

    def mask_of(layer, shp):
        keep = dropout_keep(int(np.prod(shp)), layer.rate, m._seed, next(streams), 1)
        return keep.double().view(shp) / (1.0 - layer.rate)
    z, ws = _torch_forward(m, x, mask_of)
    loss = F.binary_cross_entropy_with_logits(z.reshape(-1), torch.tensor(y, dtype=torch.float64))
    # (the model's last Dense has a sigmoid: _torch_forward leaves it linear for the logits form)
    loss.backward()
    for s, w in zip(m.store.specs, ws):
        got = m.store.view(s.layer, s.short, grad=True).double()
        assert torch.allclose(got, w.grad.reshape(got.shape), rtol=2e-4, atol=1e-6), s.name


def test_hdf5_round_trip_with_optimizer_slots(tmp_path):
    from cori_intml_examples_amd.io.keras_h5 import load_model
    set_random_seed(3)
    layers, shape = MODELS["dw_between_convs"]()
    layers.insert(1, SeparableConv2D(5, 3, padding="same", activation="relu"))
    h = inp = Input(shape=shape)
    for l in layers:
        h = l(h)
    m = Model(inp, Dense(1, activation="sigmoid")(h), device=CPU)
    m.compile(optimizer=optim.Adam(), loss="binary_crossentropy", metrics=["accuracy"])
    rs = np.random.RandomState(1)
    x, y = rs.rand(6, *shape).astype(np.float32), (rs.rand(6) > 0.5).astype(np.float32)
    m.train_on_batch(x, y)
    path = str(tmp_path / "m.h5")
    m.save(path)
    back = load_model(path)
    assert [l.get_config() for l in back.layers] == [l.get_config() for l in m.layers]
    assert [s.name for s in back.store.specs] == [s.name for s in m.store.specs]
    for a, b in zip(m.get_weights(), back.get_weights()):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(m._executor.optimizer_state(), back._executor.optimizer_state()):
        assert torch.equal(a, b) and float(a.abs().sum()) > 0
    assert m.train_on_batch(x, y) == back.train_on_batch(x, y)


def test_compat_names_and_builders():
    from cori_intml_examples_amd import compat
    from cori_intml_examples_amd.apps import zoo
    compat.install()
    import keras.layers as KL
    assert KL.SeparableConv2D is SeparableConv2D and KL.DepthwiseConv2D is DepthwiseConv2D
    kinds = lambda m: [type(l).__name__ for l in m.layers if "Conv" in type(l).__name__]
    from cori_intml_examples_amd.apps import mnist as mnist_app, rpv as rpv_app
    for build in (lambda **kw: zoo.rpv_cnn((16, 16, 3), device=CPU, **kw), lambda **kw: zoo.mnist_cnn(device=CPU, **kw),
                  lambda **kw: rpv_app.build_model((16, 16, 3), device=CPU, **kw),
                  lambda **kw: mnist_app.build_model(device=CPU, **kw),
                  lambda **kw: zoo.rpv_legacy_cnn((16, 16, 1), h1=4, h2=4, h3=4, h4=4, h5=8, device=CPU, **kw)):
        plain, sep = build(), build(separable=True)
        assert set(kinds(plain)) == {"Conv2D"} and kinds(build(separable=False)) == kinds(plain)
        assert kinds(sep) == ["Conv2D"] + ["SeparableConv2D"] * (len(kinds(plain)) - 1)
        assert sep.count_params() < plain.count_params()


def test_cli_separable_flag(monkeypatch):
    """``train_rpv --separable`` through main(): the model it builds, and the default without the flag."""
    from cori_intml_examples_amd.apps import rpv as rpv_app, train_rpv
    from cori_intml_examples_amd.parallel import hvd
    monkeypatch.setenv("INTML_DEVICE", "cpu")
    built, orig = [], rpv_app.build_model

    class Built(Exception):
        pass

    def capture(*a, **kw):
        built.append(orig(*a, **kw))
        raise Built()
    monkeypatch.setattr(rpv_app, "build_model", capture)
    base = ["--synthetic", "--n-train", "32", "--n-valid", "16", "--h1", "4", "--h2", "4", "--h3", "4", "--h4", "8"]
    assert train_rpv.build_parser().parse_args(base).separable is False
    for argv in (base, base + ["--separable"]):
        try:
            with pytest.raises(Built):
                train_rpv.main(argv)
        finally:
            hvd.shutdown()
    kinds = [[type(l).__name__ for l in m.layers if "Conv" in type(l).__name__] for m in built]
    assert kinds == [["Conv2D"] * 3, ["Conv2D", "SeparableConv2D", "SeparableConv2D"]]


@pytest.mark.parametrize("plane", ["xgmi", "hybrid"])
def test_separable_models_stay_on_the_rccl_plane(plane):
    """The xGMI planes are gated like BatchNormalization: forced is a ValueError naming the layers and the
    plane, auto falls back to rccl; the names come from the plan's depthwise stages."""
    from cori_intml_examples_amd.parallel.dist import dw_layer_names, plane_for_optimizer
    m = _model([SeparableConv2D(4, 3, name="sep_a"), DepthwiseConv2D(3, name="dw_b"), Flatten()], (8, 8, 2))
    names = dw_layer_names(m._plan)
    assert names == ("sep_a", "dw_b")
    opt = optim.Adam()
    assert plane_for_optimizer(plane, opt, forced=False) == plane
    assert plane_for_optimizer(plane, opt, forced=False, dw_layers=names) == "rccl"
    assert plane_for_optimizer("rccl", opt, forced=True, dw_layers=names) == "rccl"
    with pytest.raises(ValueError, match="SeparableConv2D layers \\(sep_a, dw_b\\).*%r data plane" % plane):
        plane_for_optimizer(plane, opt, forced=True, dw_layers=names)
