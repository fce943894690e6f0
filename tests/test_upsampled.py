"""UpSampling2D without a GPU: config / name / compat, shapes, refusals, the fold into the ConvStage behind it, the CPU
ops, an HDF5 save / load, the hourglass builder's default."""
import numpy as np
import pytest
import torch

from cori_intml_examples_amd import (AveragePooling2D, BatchNormalization, Conv2D, Conv2DTranspose, Dense, Dropout, Flatten,
                                     GlobalAveragePooling2D, MaxPooling2D, Sequential, UpSampling2D, compat)
from cori_intml_examples_amd.apps import zoo
from cori_intml_examples_amd.models.layers import LAYER_CLASSES, DepthwiseConv2D, SeparableConv2D, reset_names
from cori_intml_examples_amd.ops import reference as R
from cori_intml_examples_amd.utils import set_random_seed


def upconv_oracle(x, w, b, dt, s, pt, pl):
    """(z, dx, dW, db) and the sums of |terms| of z, dx, dW by the three formulas, in float64 loops."""
    (B, H, W, _), (KH, KW, _, Cout), (Ho, Wo) = x.shape, w.shape, dt.shape[1:3]
    z, zm = np.zeros((B, Ho, Wo, Cout)) + b, np.zeros((B, Ho, Wo, Cout)) + np.abs(b)
    dx, dxm, dw, dwm = np.zeros(x.shape), np.zeros(x.shape), np.zeros(w.shape), np.zeros(w.shape)
    for Y, X, ky, kx in np.ndindex(Ho, Wo, KH, KW):
        u, v = Y + ky - pt, X + kx - pl
        if 0 <= u < H * s and 0 <= v < W * s:
            i, j = u // s, v // s
            z[:, Y, X] += x[:, i, j] @ w[ky, kx]
            zm[:, Y, X] += np.abs(x[:, i, j]) @ np.abs(w[ky, kx])
            dx[:, i, j] += dt[:, Y, X] @ w[ky, kx].T
            dxm[:, i, j] += np.abs(dt[:, Y, X]) @ np.abs(w[ky, kx]).T
            dw[ky, kx] += x[:, i, j].T @ dt[:, Y, X]
            dwm[ky, kx] += np.abs(x[:, i, j]).T @ np.abs(dt[:, Y, X])
    return z, dx, dw, dt.sum((0, 1, 2)), zm, dxm, dwm


def _model(layers, tail=True):
    m = Sequential(device="cpu")
    for l in layers + ([Flatten(), Dense(1, activation="sigmoid")] if tail else []):
        m.add(l)
    m.compile(optimizer="Adam", loss="binary_crossentropy")
    return m


def test_config_name_shapes_and_compat():
    reset_names()
    u = UpSampling2D(3)
    assert u.name == "up_sampling2d_1" and LAYER_CLASSES["UpSampling2D"] is UpSampling2D and u.weight_specs() == []
    u.build((4, 5, 3))
    cfg = u.get_config()
    assert u.output_shape_ == (12, 15, 3) and UpSampling2D().size == (2, 2)
    assert cfg == {"name": "up_sampling2d_1", "trainable": True, "size": [3, 3], "data_format": "channels_last",
                   "interpolation": "nearest"} and UpSampling2D.from_config(cfg).get_config() == cfg
    compat.install()
    assert __import__("keras").layers.UpSampling2D is UpSampling2D


@pytest.mark.parametrize("kw,exc,match", [({"size": (1, 2)}, NotImplementedError, r"size = \(1, 2\)"),
                                          ({"size": 5}, NotImplementedError, r"size = \(5, 5\)"),
                                          ({"interpolation": "bilinear"}, NotImplementedError, "interpolation"),
                                          ({"data_format": "channels_first"}, NotImplementedError, "data_format"),
                                          ({"size": 0}, ValueError, r"size = \(0, 0\)")])
def test_refused_arguments(kw, exc, match):
    with pytest.raises(exc, match=r"bad \(UpSampling2D\): " + match):
        UpSampling2D(name="bad", **kw)


@pytest.mark.parametrize("nxt", [None, Flatten, MaxPooling2D, GlobalAveragePooling2D, lambda **k: UpSampling2D(2, **k),
                                 lambda **k: Conv2D(4, 3, strides=2, **k), lambda **k: Conv2D(4, 3, dilation_rate=2, **k),
                                 lambda **k: SeparableConv2D(4, 3, **k), lambda **k: DepthwiseConv2D(3, **k),
                                 lambda **k: Conv2DTranspose(4, 3, **k)])
def test_refused_behind_an_upsampling_layer(nxt):
    layers = [Conv2D(4, 3, input_shape=(8, 8, 2)), UpSampling2D(2, name="ups")] + ([nxt(name="nxt")] if nxt else [])
    with pytest.raises(NotImplementedError, match=r"ups \(UpSampling2D\) is followed by " + ("layer nxt" if nxt else "the model output")):
        _model(layers, tail=nxt is not None)


@pytest.mark.parametrize("behind", [MaxPooling2D, AveragePooling2D, BatchNormalization, lambda **kw: Dropout(0.2, **kw)])
def test_refused_behind_an_upsampled_conv_and_a_valid_conv_larger_than_the_grid(behind):
    with pytest.raises(NotImplementedError, match="nxt follows cv: .* directly behind an up-sampled Conv2D"):
        _model([UpSampling2D(2, input_shape=(4, 4, 2)), Conv2D(4, 3, name="cv"), behind(name="nxt")])
    with pytest.raises(ValueError, match=r"cv \(Conv2D\): .* larger than the 4x4 grid that ups"):
        _model([UpSampling2D(2, name="ups", input_shape=(2, 2, 2)), Conv2D(4, 5, name="cv")])


def test_fold_into_the_conv_stage():
    m = _model([Conv2D(4, 3, padding="same", input_shape=(4, 5, 3)), UpSampling2D(3), Conv2D(6, (2, 3), padding="same"),
                UpSampling2D(1), Conv2D(2, 3)])
    c0, c1, c2 = m._plan.convs
    assert (c0.upsample, c1.upsample, c2.upsample) == (1, 3, 1) and c1.unfused == "up-sampled Conv2D" and c2.unfused is None
    assert c1.in_shape == (4, 5, 4) and c1.conv_shape == c1.out_shape == (12, 15, 6) and c1.pads == (0, 1, 1, 1)
    assert c2.in_shape == (12, 15, 6) and c2.up_layer is None
    v = _model([UpSampling2D(2, input_shape=(4, 5, 3)), Conv2D(6, 3)])._plan.convs[0]      # stage 0, valid
    assert v.in_shape == (4, 5, 3) and v.conv_shape == (6, 8, 6) and v.pads == (0, 0, 0, 0)


@pytest.mark.parametrize("k,s,padding", [((3, 3), 2, "same"), ((3, 3), 3, "valid"), ((2, 2), 2, "same"), ((1, 3), 4, "valid"),
                                         ((5, 5), 2, "same")])
def test_cpu_ops_equal_the_float64_loops(k, s, padding):
    B, H, W, Cin, Cout = 2, 4, 5, 3, 5
    rs = np.random.RandomState(k[0] * 10 + s)
    pt, pb, pl, pr = R.conv_pads(H * s, W * s, k[0], k[1], 1, padding)
    draw = lambda *shape: rs.randint(-2, 3, shape).astype(np.float64)
    x, w, b, dz = draw(B, H, W, Cin), draw(*k, Cin, Cout), draw(Cout), draw(B, H * s + pt + pb - k[0] + 1, W * s + pl + pr - k[1] + 1, Cout)
    z, dx, dw, db = upconv_oracle(x, w, b, dz, s, pt, pl)[:4]
    t = lambda v: torch.tensor(v, dtype=torch.float32)
    np.testing.assert_array_equal(R.conv2d(t(x), t(w), t(b), 1, padding, 1, s).numpy(), z)
    for got, want in zip(R.conv2d_backward(t(x), t(w), t(dz), 1, padding, upsample=s), (dx, dw, db)):
        np.testing.assert_array_equal(got.numpy(), want)


def test_hdf5_save_and_load_and_default_up_mode(tmp_path):
    from cori_intml_examples_amd.io.keras_h5 import load_model
    set_random_seed(5)
    d = zoo.rpv_hourglass_cnn((8, 8, 3), filters=(4, 6), up=(5,), dense=(8,), device="cpu")
    assert [type(l).__name__ for l in d.layers].count("Conv2DTranspose") == 1 and not any(s.upsample > 1 for s in d._plan.convs)
    m = zoo.rpv_hourglass_cnn((8, 8, 3), filters=(4, 6), up=(5, 4), dense=(8,), device="cpu", l2=1e-3, up_mode="upsample")
    x = np.random.RandomState(1).rand(6, 8, 8, 3).astype(np.float32)
    m.train_on_batch(x, (x.mean((1, 2, 3)) > 0.5).astype(np.float32))
    m.save(str(tmp_path / "hourglass.h5"))
    c = load_model(str(tmp_path / "hourglass.h5"))
    assert [type(l).__name__ for l in c.layers] == [type(l).__name__ for l in m.layers] and [s.upsample for s in c._plan.convs] == [1, 1, 2, 1, 2, 1]
    np.testing.assert_array_equal(m.predict(x, batch_size=6), c.predict(x, batch_size=6))
    lines = []
    c.summary(print_fn=lines.append)
    assert any("up_sampling2d_" in l and "(None, 4, 4, 6)" in l for l in lines)
