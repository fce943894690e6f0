"""Dilated Conv2D without a GPU: config round trip, output shapes, the refused combinations, the CPU
executor's gradients against float64 autograd, and an HDF5 save / load that keeps dilation_rate."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cori_intml_examples_amd import (AveragePooling2D, BatchNormalization, Conv2D, Dense, Dropout, Flatten, Input,
                                     MaxPooling2D, Model, Sequential, optim)
from cori_intml_examples_amd.apps import zoo
from cori_intml_examples_amd.models import DepthwiseConv2D, SeparableConv2D
from cori_intml_examples_amd.utils import set_random_seed


def test_config_round_trip_keeps_the_dilation_rate():
    c = Conv2D(4, (3, 3), dilation_rate=2, padding="same", name="ctx")
    cfg = c.get_config()
    assert cfg["dilation_rate"] == [2, 2]
    assert Conv2D.from_config(cfg).dilation_rate == (2, 2)
    # an undilated layer's config is what it always was
    plain = Conv2D(4, (3, 3), name="p").get_config()
    assert plain["dilation_rate"] == [1, 1] and Conv2D.from_config(plain).get_config() == plain
    assert Conv2D.from_config({k: v for k, v in plain.items() if k != "dilation_rate"}).dilation_rate == (1, 1)


@pytest.mark.parametrize("k,d,padding,want", [((3, 3), 2, "valid", (7, 5)), ((3, 3), 2, "same", (11, 9)),
                                              ((2, 2), 3, "valid", (8, 6)), ((2, 2), 3, "same", (11, 9)),
                                              ((1, 3), 4, "valid", (11, 1))])
def test_output_shapes(k, d, padding, want):
    c = Conv2D(6, k, dilation_rate=d, padding=padding)
    c.build((11, 9, 3))
    assert c.output_shape_ == want + (6,)


def test_even_kernel_pads_asymmetrically_like_tf():
    m = Sequential(device="cpu")
    m.add(Conv2D(4, (2, 2), dilation_rate=3, padding="same", input_shape=(8, 8, 2)))
    m.add(Flatten())
    m.add(Dense(1, activation="sigmoid"))
    m.compile(optimizer="Adam", loss="binary_crossentropy")
    assert m._plan.convs[0].pads == (1, 2, 1, 2) and m._plan.convs[0].dilated


def _model(layers):
    m = Sequential(device="cpu")
    for l in layers:
        m.add(l)
    m.add(Flatten())
    m.add(Dense(1, activation="sigmoid"))
    m.compile(optimizer="Adam", loss="binary_crossentropy")
    return m


def test_refused_combinations():
    with pytest.raises(ValueError, match=r"bad \(Conv2D\): strides = \(2, 2\) with dilation_rate = \(2, 2\)"):
        Conv2D(4, (3, 3), strides=2, dilation_rate=2, name="bad")
    with pytest.raises(NotImplementedError, match=r"bad \(Conv2D\): anisotropic dilation_rate = \(1, 2\)"):
        Conv2D(4, (3, 3), dilation_rate=(1, 2), name="bad")
    with pytest.raises(ValueError, match="small.*spans 7x7 pixels"):
        Conv2D(4, (3, 3), dilation_rate=3, name="small").build((6, 9, 1))
    for cls in (DepthwiseConv2D, lambda *a, **k: SeparableConv2D(4, *a, **k)):
        with pytest.raises(NotImplementedError, match="dilat"):
            cls((3, 3), dilation_rate=2)
    for behind in (MaxPooling2D((2, 2), name="nxt"), AveragePooling2D((2, 2), name="nxt"), BatchNormalization(name="nxt"),
                   Dropout(0.2, name="nxt")):
        with pytest.raises(NotImplementedError, match="nxt follows dil: %s directly behind a dilated Conv2D" % type(behind).__name__):
            _model([Conv2D(4, (3, 3), dilation_rate=2, padding="same", name="dil", input_shape=(8, 8, 2)), behind])
    # a Conv2D, SeparableConv2D, Flatten or global pooling layer may follow
    _model([Conv2D(4, (3, 3), dilation_rate=2, input_shape=(12, 12, 2)), SeparableConv2D(4, (3, 3)), Conv2D(4, (2, 2), dilation_rate=2)])


def test_cpu_executor_gradients_match_float64_autograd():
    set_random_seed(3)
    inp = Input(shape=(9, 8, 3))
    h = Conv2D(5, (3, 3), dilation_rate=2, padding="same", activation="relu")(inp)
    h = Conv2D(4, (2, 2), dilation_rate=3, activation="tanh")(h)
    m = Model(inp, Dense(1, activation="sigmoid")(Flatten()(h)), device="cpu")
    m.compile(optimizer=optim.SGD(lr=0.0), loss="binary_crossentropy")
    rs = np.random.RandomState(0)
    x, y = rs.randn(6, 9, 8, 3).astype(np.float32), (rs.rand(6, 1) > 0.5).astype(np.float32)
    m.train_on_batch(x, y)
    w = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in m.get_weights()]
    t = torch.tensor(x, dtype=torch.float64).permute(0, 3, 1, 2)
    t = torch.relu(F.conv2d(F.pad(t, (2, 2, 2, 2)), w[0].permute(3, 2, 0, 1), w[1], dilation=2))
    t = torch.tanh(F.conv2d(t, w[2].permute(3, 2, 0, 1), w[3], dilation=3))
    p = torch.sigmoid(t.permute(0, 2, 3, 1).reshape(6, -1) @ w[4] + w[5])
    F.binary_cross_entropy(p, torch.tensor(y, dtype=torch.float64)).backward()
    got = m.store.grad[:m.store.numel].numpy()
    want = np.concatenate([v.grad.numpy().ravel() for v in w])
    assert np.abs(got - want).max() <= 1e-5 * max(1.0, np.abs(want).max()) and np.abs(want).max() > 1e-3


def test_hdf5_save_and_load_keep_the_dilation(tmp_path):
    from cori_intml_examples_amd.io.keras_h5 import load_model
    set_random_seed(5)
    m = zoo.rpv_context_cnn((12, 12, 3), dilations=(1, 2, 3), filters=(4, 6, 8), dense=(8,), device="cpu")
    path = str(tmp_path / "ctx.h5")
    m.save(path)
    c = load_model(path)
    assert [getattr(l, "dilation_rate", None) for l in c.layers] == [getattr(l, "dilation_rate", None) for l in m.layers]
    assert [s.dilation for s in c._plan.convs] == [1, 2, 3]
    x = np.random.RandomState(1).rand(5, 12, 12, 3).astype(np.float32)
    np.testing.assert_array_equal(m.predict(x, batch_size=5), c.predict(x, batch_size=5))
