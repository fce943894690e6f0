"""Conv2DTranspose without a GPU: config / name / weight round trip, output shapes, the refused arguments and
combinations, the CPU executor's forward and gradients against float64 loops of the formulas (exact on small
integers), and an HDF5 save / load."""
import numpy as np
import pytest
import torch

from cori_intml_examples_amd import (AveragePooling2D, BatchNormalization, Conv2DTranspose, Dense, Dropout, Flatten,
                                     MaxPooling2D, Sequential, regularizers)
from cori_intml_examples_amd.apps import zoo
from cori_intml_examples_amd.models.layers import LAYER_CLASSES, reset_names
from cori_intml_examples_amd.ops import reference as R
from cori_intml_examples_amd.utils import set_random_seed

# (kernel, stride, padding) -> output grid of a 4x5 map
SHAPES = [(3, 2, "same", (8, 10)), (3, 2, "valid", (9, 11)), (2, 2, "valid", (8, 10)), (4, 2, "same", (8, 10)),
          (1, 2, "valid", (8, 10)), (3, 1, "same", (4, 5)), (5, 3, "same", (12, 15))]


def test_config_names_weights_and_fans_round_trip():
    reset_names()
    c = Conv2DTranspose(6, (3, 2), strides=2, padding="same", activation="relu", kernel_regularizer=regularizers.l2(1e-3))
    assert c.name == "conv2d_transpose_1" and LAYER_CLASSES["Conv2DTranspose"] is Conv2DTranspose
    c.build((4, 5, 3))
    assert [(n, s) for n, s, _ in c.weight_specs()] == [("kernel", (3, 2, 6, 3)), ("bias", (6,))]
    cfg = c.get_config()
    assert cfg["output_padding"] is None and cfg["strides"] == [2, 2] and cfg["dilation_rate"] == [1, 1]
    assert Conv2DTranspose.from_config(cfg).get_config() == cfg
    # Keras' _compute_fans on (kh, kw, filters, Cin): fan_in = filters * kh * kw (he_uniform uses fan_in alone, so
    # the conventional order, Cin * kh * kw = 18, would give a limit five times as large)
    set_random_seed(7)
    m = Sequential(device="cpu")
    m.add(Conv2DTranspose(50, (3, 3), use_bias=False, kernel_initializer="he_uniform", input_shape=(4, 4, 2)))
    m.add(Flatten())
    m.add(Dense(1, activation="sigmoid"))
    m.compile(optimizer="Adam", loss="binary_crossentropy")
    w = m.get_weights()[0]
    limit = np.sqrt(6.0 / (50 * 9))
    assert w.shape == (3, 3, 50, 2) and 0.9 * limit < np.abs(w).max() <= limit


@pytest.mark.parametrize("k,s,padding,want", SHAPES)
def test_output_shapes(k, s, padding, want):
    c = Conv2DTranspose(6, k, strides=s, padding=padding)
    c.build((4, 5, 3))
    assert c.output_shape_ == want + (6,)


def _model(layers):
    m = Sequential(device="cpu")
    for l in layers:
        m.add(l)
    m.add(Flatten())
    m.add(Dense(1, activation="sigmoid"))
    m.compile(optimizer="Adam", loss="binary_crossentropy")
    return m


@pytest.mark.parametrize("kw,match", [({"strides": (1, 2)}, r"strides = \(1, 2\)"), ({"strides": 5}, r"strides = \(5, 5\)"),
                                      ({"output_padding": 1}, "output_padding"), ({"dilation_rate": 2}, "dilation_rate"),
                                      ({"data_format": "channels_first"}, "data_format"),
                                      ({"activity_regularizer": regularizers.l2(0.1)}, "activity_regularizer"),
                                      ({"kernel_constraint": "max_norm"}, "kernel_constraint"),
                                      ({"bias_constraint": "non_neg"}, "bias_constraint")])
def test_refused_arguments(kw, match):
    with pytest.raises(NotImplementedError, match=r"bad \(Conv2DTranspose\): " + match):
        Conv2DTranspose(4, (3, 3), name="bad", **kw)


@pytest.mark.parametrize("behind", [MaxPooling2D, AveragePooling2D, BatchNormalization, lambda **kw: Dropout(0.2, **kw)])
def test_refused_behind_a_transposed_layer(behind):
    with pytest.raises(NotImplementedError, match="nxt follows up: .* directly behind a Conv2DTranspose"):
        _model([Conv2DTranspose(4, (3, 3), strides=2, name="up", input_shape=(4, 4, 2)), behind(name="nxt")])


@pytest.mark.parametrize("k,s,padding,want", SHAPES)
def test_cpu_ops_equal_the_float64_loops(k, s, padding, want):
    B, H, W, Cin, Cout = 2, 4, 5, 3, 5
    rs = np.random.RandomState(k * 10 + s)
    x, w = rs.randint(-2, 3, (B, H, W, Cin)).astype(np.float64), rs.randint(-2, 3, (k, k, Cout, Cin)).astype(np.float64)
    b, dz = rs.randint(-2, 3, (Cout,)).astype(np.float64), rs.randint(-2, 3, (B,) + want + (Cout,)).astype(np.float64)
    pt, _, pl, _ = R.tconv_pads(k, k, s, padding)
    z, dx, dw = np.zeros_like(dz) + b, np.zeros_like(x), np.zeros_like(w)
    for i in range(H):
        for j in range(W):
            for ky in range(k):
                for kx in range(k):
                    Y, X = i * s + ky - pt, j * s + kx - pl
                    if 0 <= Y < want[0] and 0 <= X < want[1]:
                        z[:, Y, X] += x[:, i, j] @ w[ky, kx].T
                        dx[:, i, j] += dz[:, Y, X] @ w[ky, kx]
                        dw[ky, kx] += dz[:, Y, X].T @ x[:, i, j]
    t = lambda v: torch.tensor(v, dtype=torch.float32)
    np.testing.assert_array_equal(R.conv2d_transpose(t(x), t(w), t(b), s, padding).numpy(), z)
    gx, gw, gb = R.conv2d_transpose_backward(t(x), t(w), t(dz), s, padding)
    np.testing.assert_array_equal(gx.numpy(), dx)
    np.testing.assert_array_equal(gw.numpy(), dw)
    np.testing.assert_array_equal(gb.numpy(), dz.sum((0, 1, 2)))


def test_hdf5_save_and_load(tmp_path):
    from cori_intml_examples_amd.io.keras_h5 import load_model
    set_random_seed(5)
    m = zoo.rpv_hourglass_cnn((8, 8, 3), filters=(4, 6), up=(5, 4), dense=(8,), device="cpu", l2=1e-3)
    x = np.random.RandomState(1).rand(6, 8, 8, 3).astype(np.float32)
    m.train_on_batch(x, (x.mean((1, 2, 3)) > 0.5).astype(np.float32))
    path = str(tmp_path / "hourglass.h5")
    m.save(path)
    c = load_model(path)
    assert [type(l).__name__ for l in c.layers] == [type(l).__name__ for l in m.layers]
    assert [s.transposed for s in c._plan.convs] == [False, False, True, False, True, False]
    np.testing.assert_array_equal(m.predict(x, batch_size=6), c.predict(x, batch_size=6))
