"""AveragePooling2D, GlobalAveragePooling2D and GlobalMaxPooling2D without a GPU: the float64
oracle against float64 autograd, the fp32 reference ops against the oracle, the layer classes,
the plan's position rules and their errors, the CPU executor against an independently written
autograd model, its bf16 rounding points, checkpoints, the compat names, the builders and CLIs."""
import io
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cori_intml_examples_amd import optim
from cori_intml_examples_amd.apps import mnist as mnist_app
from cori_intml_examples_amd.apps import rpv as rpv_app
from cori_intml_examples_amd.apps import train_mnist, train_rpv, zoo
from cori_intml_examples_amd.io.keras_h5 import load_model
from cori_intml_examples_amd.models import (Activation, AveragePooling2D, BatchNormalization, Conv2D, Dense, Dropout,
                                            Flatten, GlobalAveragePooling2D, GlobalMaxPooling2D, Input, MaxPooling2D,
                                            Model, Sequential, reset_names)
from cori_intml_examples_amd.models.layers import LAYER_CLASSES
from cori_intml_examples_amd.models.step_program import stage_geometry
from cori_intml_examples_amd.ops import reference as R
from cori_intml_examples_amd.utils import set_random_seed

from helpers import pool_models as M
from helpers import pool_oracle as O


# ------------------------------------------------------------------------------------ 1. the oracle
@pytest.mark.parametrize("shape", [(2, 2, 2, 3), (3, 5, 7, 4), (2, 8, 6, 5), (1, 1, 1, 2), (2, 16, 16, 3)])
def test_oracle_matches_float64_autograd(shape):
    rs = np.random.RandomState(sum(shape))
    x = rs.randn(*shape)                                  # continuous draws: no ties
    B, H, W, C = shape
    xt = torch.tensor(x, requires_grad=True)
    if H >= 2 and W >= 2:
        y = F.avg_pool2d(xt.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
        np.testing.assert_allclose(O.avg2_fwd(x), y.detach().numpy(), rtol=1e-14, atol=1e-15)
        dy = rs.randn(*y.shape)
        y.backward(torch.tensor(dy))
        got = O.avg2_bwd(dy, (H, W))
        np.testing.assert_allclose(got, xt.grad.numpy(), rtol=1e-14, atol=1e-15)
        assert np.all(got[:, 2 * (H // 2):] == 0) and np.all(got[:, :, 2 * (W // 2):] == 0)
        xt.grad = None
    inv = O.inv_n(H, W) * (H * W)                         # the oracle multiplies by fp32(1 / n), autograd divides by n
    y = xt.mean((1, 2))
    np.testing.assert_allclose(O.gavg_fwd(x), y.detach().numpy() * inv, rtol=1e-13, atol=1e-15)
    dy = rs.randn(B, C)
    y.backward(torch.tensor(dy))
    np.testing.assert_allclose(O.gavg_bwd(dy, (H, W)), xt.grad.numpy() * inv, rtol=1e-13, atol=1e-15)
    xt.grad = None
    y, idx = xt.reshape(B, H * W, C).max(1)
    val, at = O.gmax_fwd(x)
    assert np.array_equal(val, y.detach().numpy()) and np.array_equal(at, idx.numpy())
    y.backward(torch.tensor(dy))
    assert np.array_equal(O.gmax_bwd(dy, at, (H, W)), xt.grad.numpy())


def test_oracle_takes_the_first_maximum_and_true_negative_maxima():
    x = -np.ones((1, 2, 3, 4)) * 5.0
    x[0, 0, 2, 0] = x[0, 1, 1, 0] = -1.0                  # a duplicated maximum of an all-negative channel
    x[0, :, :, 1] = -7.0                                  # all equal
    x[0, 1, 2, 2] = -0.5
    val, at = O.gmax_fwd(x)
    assert val.tolist() == [[-1.0, -7.0, -0.5, -5.0]] and at.tolist() == [[2, 0, 5, 0]]
    g = O.gmax_bwd(np.ones((1, 4)), at, (2, 3))
    assert g.sum() == 4 and g[0, 0, 2, 0] == 1 and g[0, 1, 1, 0] == 0 and g[0, 0, 0, 1] == 1


@pytest.mark.parametrize("shape", [(3, 5, 7, 4), (2, 8, 6, 5), (2, 16, 16, 3)])
def test_reference_ops_match_the_oracle(shape):
    rs = np.random.RandomState(5)
    x = rs.randn(*shape).astype(np.float32)
    x[0, 0, 1, 0] = x[0, 1, 0, 0] = 9.0                   # a tie: first maximum in row-major order
    B, H, W, C = shape
    xt = torch.tensor(x)
    np.testing.assert_allclose(R.avgpool2x2(xt).numpy(), O.avg2_fwd(x), rtol=1e-6, atol=1e-7)
    dp = rs.randn(B, H // 2, W // 2, C).astype(np.float32)
    np.testing.assert_array_equal(R.avgpool2x2_backward(torch.tensor(dp), (H, W)).numpy(), O.avg2_bwd(dp, (H, W)))
    np.testing.assert_allclose(R.global_avgpool(xt).numpy(), O.gavg_fwd(x), rtol=1e-5, atol=1e-6)
    dg = rs.randn(B, C).astype(np.float32)
    np.testing.assert_allclose(R.global_avgpool_backward(torch.tensor(dg), (H, W)).numpy(), O.gavg_bwd(dg, (H, W)),
                               rtol=1e-6)
    val, idx = R.global_maxpool(xt)
    oval, oidx = O.gmax_fwd(x)
    assert np.array_equal(val.numpy(), oval) and np.array_equal(idx.numpy(), oidx) and oidx[0, 0] == 1
    np.testing.assert_array_equal(R.global_maxpool_backward(torch.tensor(dg), idx, (H, W)).numpy(),
                                  O.gmax_bwd(dg, oidx, (H, W)))


# ------------------------------------------------------------------------------------ 2. layers
def test_layer_configs_and_names():
    a, g, m = AveragePooling2D(), GlobalAveragePooling2D(), GlobalMaxPooling2D()
    assert (a.name, g.name, m.name) == ("average_pooling2d_1", "global_average_pooling2d_1", "global_max_pooling2d_1")
    assert AveragePooling2D().name == "average_pooling2d_2" and MaxPooling2D().name == "max_pooling2d_1"
    assert a.get_config() == {"name": "average_pooling2d_1", "trainable": True, "pool_size": [2, 2], "padding": "valid",
                              "strides": [2, 2], "data_format": "channels_last"}
    assert g.get_config() == {"name": "global_average_pooling2d_1", "trainable": True, "data_format": "channels_last"}
    assert m.get_config() == {"name": "global_max_pooling2d_1", "trainable": True, "data_format": "channels_last"}
    for layer in (a, g, m):
        assert layer.weight_specs() == [] and layer.count_params() == 0
        twin = type(layer).from_config(layer.get_config())
        assert type(twin) is type(layer) and twin.get_config() == layer.get_config()
        assert LAYER_CLASSES[type(layer).__name__] is type(layer)
    assert AveragePooling2D(pool_size=2, strides=(2, 2), padding="valid", data_format="channels_last").pool_size == (2, 2)


@pytest.mark.parametrize("kw", [{"pool_size": (3, 3)}, {"pool_size": (2, 2), "strides": (1, 1)}, {"padding": "same"},
                                {"pool_size": 4}])
def test_average_pooling_rejects_what_max_pooling_rejects(kw):
    with pytest.raises(NotImplementedError) as ea:
        AveragePooling2D(**kw)
    with pytest.raises(NotImplementedError) as em:
        MaxPooling2D(**kw)
    assert str(ea.value) == str(em.value)


def test_global_pooling_rejects_channels_first():
    for cls in (GlobalAveragePooling2D, GlobalMaxPooling2D):
        with pytest.raises(NotImplementedError):
            cls(data_format="channels_first")


@pytest.mark.parametrize("hw", [(2, 2), (5, 7), (8, 6), (19, 17), (3, 2)])
def test_output_shapes(hw):
    H, W = hw
    inp = Input(shape=(H, W, 5))
    assert AveragePooling2D()(inp).shape == (H // 2, W // 2, 5)
    assert GlobalAveragePooling2D()(inp).shape == (5,) and GlobalMaxPooling2D()(inp).shape == (5,)


# ------------------------------------------------------------------------------------ 3. the plan
def _compile(out_of):
    reset_names()
    inp = Input(shape=(12, 10, 3))
    out = out_of(inp)
    m = Model(inp, out, device="cpu")
    m.compile(optimizer="SGD", loss="binary_crossentropy" if out.shape[-1] == 1 else "categorical_crossentropy")
    return m


def test_average_pooling_takes_max_poolings_place():
    m = _compile(lambda i: Dense(1, activation="sigmoid")(Flatten()(Dropout(0.3)(AveragePooling2D()(
        Activation("tanh")(Conv2D(4, (3, 3))(Dropout(0.1)(AveragePooling2D()(Conv2D(5, (3, 3), activation="relu")(i))))))))))
    p = m._executor.plan
    assert [c.pool_kind for c in p.convs] == ["avg", "avg"] and p.gpool is None
    assert [(c.relu, c.act, c.rate, c.stream) for c in p.convs] == [(True, None, 0.1, 1), (False, "tanh", 0.3, 2)]
    assert [c.out_shape for c in p.convs] == [(5, 4, 5), (1, 1, 4)]
    _, convs, _, _, _ = stage_geometry(p)
    g = convs[0]
    assert g.avg and not g.pool and not g.plain and g.dropout_in == "pool" and (g.Hp, g.Wp) == (5, 4)
    lin = g.linear
    assert (lin.relu, lin.pool, lin.avg, lin.rate, lin.Hp, lin.Wp) == (True, False, False, 0.0, 10, 8) and lin.plain
    assert convs[1].linear.relu is False and convs[1].act == "tanh"
    mx = _compile(lambda i: Dense(1, activation="sigmoid")(Flatten()(MaxPooling2D()(Conv2D(5, (3, 3), activation="relu")(i)))))
    assert [c.pool_kind for c in mx._executor.plan.convs] == ["max"]
    gm = stage_geometry(mx._executor.plan)[1][0]
    assert gm.pool and not gm.avg and gm.plain and gm.linear is gm


def test_global_pooling_is_a_stage_of_its_own():
    m = _compile(lambda i: Dense(3, activation="softmax")(Dense(7, activation="relu")(Dropout(0.25)(
        GlobalAveragePooling2D()(Dropout(0.5)(MaxPooling2D()(Conv2D(6, (3, 3), activation="relu")(i))))))))
    p = m._executor.plan
    gp = p.gpool
    assert gp.mode == "avg" and gp.in_shape == (5, 4, 6) and gp.rate == 0.25 and gp.stream == 2
    assert p.convs[0].rate == 0.5 and p.convs[0].stream == 1 and p.denses[0].K == 6 and p.denses[0].flat_from is None
    assert p.stages == [p.convs[0], gp, p.denses[0], p.head]
    _, convs, denses, head_src, _ = stage_geometry(p)
    s = denses[0].src
    assert (s.kind, s.idx, s.C, s.Cs, s.H, s.W) == ("gpool", 0, 6, 8, 1, 1) and head_src.kind == "dense"
    # straight into the head, and without a Dropout
    m = _compile(lambda i: Dense(3, activation="softmax")(GlobalMaxPooling2D()(Conv2D(6, (3, 3))(i))))
    p = m._executor.plan
    assert p.gpool.mode == "max" and p.gpool.rate == 0.0 and not p.denses and p.head.K == 6
    src = stage_geometry(p)[3]
    assert (src.kind, src.C, src.Cs, src.width) == ("gpool", 6, 8, 8)


def _raises(out_of, *words):
    with pytest.raises(NotImplementedError) as e:
        _compile(out_of)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_position_rules_and_their_errors():
    head = lambda h: Dense(1, activation="sigmoid")(h)
    # AveragePooling2D on a BatchNormalization stage: names both layers
    _raises(lambda i: head(Flatten()(AveragePooling2D()(Activation("relu")(BatchNormalization()(Conv2D(4, (3, 3))(i)))))),
            "average_pooling2d_1", "batch_normalization_1", "AveragePooling2D on a BatchNormalization stage")
    # a second pooling layer on one stage, a pooling layer behind the dropout or on the input
    _raises(lambda i: head(Flatten()(AveragePooling2D()(MaxPooling2D()(Conv2D(4, (3, 3))(i))))),
            "AveragePooling2D must directly follow a Conv2D")
    _raises(lambda i: head(Flatten()(MaxPooling2D()(AveragePooling2D()(Conv2D(4, (3, 3))(i))))),
            "MaxPooling2D must directly follow a Conv2D")
    _raises(lambda i: head(Flatten()(AveragePooling2D()(Dropout(0.1)(Conv2D(4, (3, 3))(i))))),
            "AveragePooling2D must directly follow a Conv2D")
    _raises(lambda i: head(Flatten()(AveragePooling2D()(i))), "AveragePooling2D must directly follow a Conv2D")
    # global pooling: on the input, behind Flatten / Dense, followed by Flatten, twice, ahead of a conv
    _raises(lambda i: head(GlobalAveragePooling2D()(i)), "global_average_pooling2d_1", "input_1", "model input")
    _raises(lambda i: head(GlobalMaxPooling2D()(Flatten()(Conv2D(4, (3, 3))(i)))),
            "global_max_pooling2d_1", "flatten_1", "behind a Flatten or Dense")
    _raises(lambda i: head(GlobalAveragePooling2D()(Dense(4)(Flatten()(Conv2D(4, (3, 3))(i))))),
            "global_average_pooling2d_1", "dense_1", "behind a Flatten or Dense")
    _raises(lambda i: head(Flatten()(GlobalAveragePooling2D()(Conv2D(4, (3, 3))(i)))),
            "flatten_1", "global_average_pooling2d_1", "Flatten behind a global pooling layer")
    _raises(lambda i: head(GlobalMaxPooling2D()(GlobalAveragePooling2D()(Conv2D(4, (3, 3))(i)))),
            "global_max_pooling2d_1", "global_average_pooling2d_1", "two global pooling layers")
    _raises(lambda i: head(Dropout(0.1)(Dropout(0.1)(GlobalAveragePooling2D()(Conv2D(4, (3, 3))(i))))),
            "two consecutive Dropout layers")
    # a pooling layer behind the global one keeps the pooling error
    with pytest.raises(NotImplementedError):
        reset_names()
        m = Sequential(device="cpu")
        m.add(Conv2D(4, (3, 3), input_shape=(8, 8, 1)))
        m.add(GlobalAveragePooling2D())
        m.add(Dense(4))
        m.add(GlobalAveragePooling2D())
        m.add(Dense(1, activation="sigmoid"))
        m.compile(optimizer="SGD", loss="binary_crossentropy")


# ------------------------------------------------------------------------------------ 4. the CPU executor
def _grads(m):
    return [m.store.view(l, n, grad=True).numpy().copy() if n not in l.non_trainable_weights_ else None
            for l in m.layers for n, _, _ in l.weight_specs()]


def _xy(m, n, seed=1):
    rs = np.random.RandomState(seed)
    x = rs.rand(n, *m.input_shape[1:]).astype(np.float32)
    nout = m.output_shape[-1]
    y = (rs.rand(n) > 0.5).astype(np.float32) if nout == 1 else np.eye(nout, dtype=np.float32)[rs.randint(0, nout, n)]
    return x, y


@pytest.mark.parametrize("kind", M.KINDS)
def test_cpu_executor_gradients_match_autograd(kind):
    """One training step (dropout 0.25) of the CPU executor's hand-written backward against autograd
    of an independently written model in Keras' order.  fp32 on both sides."""
    set_random_seed(3)
    m = M.build(kind, optim.SGD(lr=0.0), "cpu", drop=0.25)
    x, y = _xy(m, 24)
    loss, want = M.torch_loss_grads(m, x, y, step=1)
    ex = m._executor
    d = ex.upload(x, y)
    ex.reset_metrics()
    ex.train_step(d, torch.arange(d.n), 0, d.n)
    got = _grads(m)
    assert abs(ex.read_metrics()[0] - loss) < 1e-5 * max(1.0, loss)
    seen = 0
    for g, w in zip(got, want):
        if g is None:
            continue
        seen += 1
        assert np.linalg.norm(g - w) <= 1e-4 * np.linalg.norm(w) + 1e-7, (kind, g.shape, np.linalg.norm(g - w),
                                                                          np.linalg.norm(w))
        assert np.linalg.norm(w) > 0
    assert seen >= 4


def test_odd_leftover_row_and_column_get_no_gradient():
    """A 5x7 map: the last row and column lie outside every window, so the input pixels that only
    they see get no gradient through an identity-like 1x1 conv."""
    set_random_seed(2)
    inp = Input(shape=(5, 7, 1))
    h = AveragePooling2D()(Conv2D(2, (1, 1))(inp))
    m = Model(inp, Dense(1, activation="sigmoid")(Flatten()(h)), device="cpu")
    m.compile(optimizer=optim.SGD(lr=0.0), loss="binary_crossentropy")
    x, y = _xy(m, 4)
    x2 = x.copy()
    x2[:, 4, :, :] += 3.0
    x2[:, :, 6, :] -= 2.0
    np.testing.assert_array_equal(m.predict(x), m.predict(x2))


def _bf(t):
    return t.to(torch.bfloat16).to(torch.float32)


@pytest.mark.parametrize("mode", ["avg", "max"])
def test_ref_bf16_rounding_points(mode, monkeypatch):
    """ref_bf16=1: the un-pooled activation is rounded before the averaging and the pooled output
    once; the global stage reads the stored conv output (GlobalMaxPooling2D takes its index there)
    and stores its own output and gradient rounded."""
    monkeypatch.setenv("INTML_TUNE", "ref_bf16=1")
    set_random_seed(4)
    inp = Input(shape=(9, 8, 2))
    h = AveragePooling2D()(Conv2D(5, (3, 3), activation="relu", padding="same")(inp))
    h = (GlobalAveragePooling2D if mode == "avg" else GlobalMaxPooling2D)()(h)
    m = Model(inp, Dense(3, activation="softmax")(h), device="cpu")
    m.compile(optimizer=optim.SGD(lr=0.0), loss="categorical_crossentropy")
    ex = m._executor
    assert ex.emulate_bf16
    x, y = _xy(m, 6)
    x = _bf(torch.tensor(x)).numpy()
    with torch.no_grad():
        z, a_head, saved = ex._forward(torch.tensor(x), True, 1)
    conv = m.layers[1]
    lin = _bf(torch.relu(R.conv2d(torch.tensor(x), _bf(m.store.view(conv, "kernel")), m.store.view(conv, "bias"), 1,
                                  "same")))
    a_in, r, code, mask, out = saved[0]
    assert torch.equal(r, lin) and code is None and mask is None          # rounded before the averaging
    pooled = _bf(R.avgpool2x2(lin))
    assert torch.equal(out, pooled) and out.shape == (6, 4, 4, 5)          # ... and the pooled output once
    assert not torch.equal(pooled, R.avgpool2x2(lin))                      # (the rounding is not a no-op here)
    hw, idx, gmask = ex._gp_ctx
    assert hw == (4, 4) and gmask is None
    if mode == "avg":
        assert idx is None and torch.equal(a_head, _bf(R.global_avgpool(pooled)))
    else:
        val, want = R.global_maxpool(pooled)                               # on the STORED values
        assert torch.equal(idx, want) and torch.equal(a_head, val)
    # the backward stores the global stage's gradient, the pooled dP and dz rounded
    d = ex.upload(x, y)
    ex.train_step(d, torch.arange(6), 0, 6)
    _, dlog, _ = ex._head_loss(z, torch.tensor(y))
    head = m.layers[-1]
    dg = _bf((dlog / 6) @ m.store.view(head, "kernel").t())
    dmap = R.global_avgpool_backward(dg, hw) if mode == "avg" else R.global_maxpool_backward(dg, idx, hw)
    dz = _bf(R.avgpool2x2_backward(_bf(dmap), (9, 8)) * (lin > 0))
    _, dw, db = R.conv2d_backward(torch.tensor(x), _bf(m.store.view(conv, "kernel")), dz, 1, "same", need_dx=False)
    np.testing.assert_array_equal(m.store.view(conv, "kernel", grad=True).numpy(), dw.numpy())
    np.testing.assert_array_equal(m.store.view(conv, "bias", grad=True).numpy(), db.numpy())
    assert float(dz[:, 8].abs().sum()) == 0.0                              # the leftover odd row


# ------------------------------------------------------------------------------------ 5. checkpoints, compat
def test_three_steps_checkpoint_and_summary(tmp_path):
    set_random_seed(5)
    m = M.avg_odd_gap(optim.Adam(lr=0.01), "cpu", drop=0.1)
    x, y = _xy(m, 48, seed=0)
    w0 = [w.copy() for w in m.get_weights()]
    losses = [m.train_on_batch(x[16 * k:16 * k + 16], y[16 * k:16 * k + 16])[0] for k in range(3)]
    assert np.all(np.isfinite(losses)) and m.optimizer.iterations == 3
    assert all(np.abs(a - b).max() > 1e-5 for a, b in zip(w0, m.get_weights()))
    p = str(tmp_path / "m.h5")
    m.save(p)
    c = load_model(p, device="cpu")
    assert [type(l).__name__ for l in c.layers] == [type(l).__name__ for l in m.layers]
    assert [l.get_config() for l in c.layers] == [l.get_config() for l in m.layers]
    assert c.get_config() == m.get_config()
    assert [s.pool_kind for s in c._executor.plan.convs] == ["avg", "avg"] and c._executor.plan.gpool.mode == "avg"
    np.testing.assert_array_equal(c.predict(x, batch_size=16), m.predict(x, batch_size=16))
    assert c.test_on_batch(x[:16], y[:16]) == m.test_on_batch(x[:16], y[:16])
    assert np.isfinite(c.train_on_batch(x[:16], y[:16])[0]) and c.optimizer.iterations == 4
    buf = io.StringIO()
    with redirect_stdout(buf):
        m.summary()
    s = buf.getvalue()
    assert "average_pooling2d_1 (Average" in s and "global_average_pooling2d_1 (" in s and "(None, 12)" in s
    g = M.max_gmp(optim.SGD(), "cpu")
    q = str(tmp_path / "g.h5")
    g.save(q)
    c = load_model(q, device="cpu")
    assert c._executor.plan.gpool.mode == "max" and c.get_config() == g.get_config()
    np.testing.assert_array_equal(c.predict(x[:8, :16, :16, :1].repeat(3, -1)), g.predict(x[:8, :16, :16, :1].repeat(3, -1)))


def test_sequential_and_compat_names():
    from cori_intml_examples_amd import compat
    saved = {k: v for k, v in sys.modules.items() if k == "keras" or k.startswith("keras.")}
    try:
        compat.install(force=True, groups=("keras",))
        import keras
        from keras.layers import AveragePooling2D as KA
        from keras.layers import GlobalAveragePooling2D as KG
        from keras.layers import GlobalMaxPooling2D as KM
        assert (KA, KG, KM) == (AveragePooling2D, GlobalAveragePooling2D, GlobalMaxPooling2D)
        m = keras.models.Sequential(device="cpu")
        m.add(keras.layers.Conv2D(4, (3, 3), activation="relu", input_shape=(8, 8, 1)))
        m.add(KA(pool_size=(2, 2)))
        m.add(KG())
        m.add(keras.layers.Dense(3, activation="softmax"))
        m.compile(optimizer="SGD", loss="categorical_crossentropy")
        assert m._executor.plan.convs[0].pool_kind == "avg" and m._executor.plan.gpool.mode == "avg"
        assert [l.name for l in m.layers[1:3]] == ["average_pooling2d_1", "global_average_pooling2d_1"]
    finally:
        for k in [k for k in sys.modules if k == "keras" or k.startswith("keras.")]:
            del sys.modules[k]
        sys.modules.update(saved)


# ------------------------------------------------------------------------------------ 6. builders and CLIs
def _types(m):
    return [type(l).__name__ for l in m.layers]


def test_builders_take_pool_and_global_pool():
    builds = [lambda **kw: zoo.rpv_cnn((16, 16, 1), conv_sizes=[4, 8], fc_sizes=[8], device="cpu", **kw),
              lambda **kw: rpv_app.build_model((16, 16, 1), conv_sizes=[4, 8], fc_sizes=[8], device="cpu", **kw),
              lambda **kw: zoo.mnist_cnn(device="cpu", **kw), lambda **kw: mnist_app.build_model(device="cpu", **kw),
              lambda **kw: zoo.rpv_legacy_cnn((16, 16, 1), h1=4, h2=4, h3=4, h4=4, h5=8, device="cpu", **kw)]
    for k, build in enumerate(builds):
        reset_names()
        a = build()
        reset_names()
        b = build(pool="max", global_pool=None)
        assert [l.get_config() for l in a.layers] == [l.get_config() for l in b.layers] and _types(a) == _types(b)
        assert not {"AveragePooling2D", "GlobalAveragePooling2D", "GlobalMaxPooling2D"} & set(_types(a))
        assert "Flatten" in _types(a)
        t = build(pool="avg", global_pool="avg")
        want = [{"MaxPooling2D": "AveragePooling2D", "Flatten": "GlobalAveragePooling2D"}.get(n, n) for n in _types(a)]
        assert _types(t) == want
        assert t._executor.plan.gpool.mode == "avg" and all(c.pool_kind in (None, "avg") for c in t._executor.plan.convs)
        u = build(global_pool="max")
        assert _types(u) == [{"Flatten": "GlobalMaxPooling2D"}.get(n, n) for n in _types(a)]
        for bad in ({"pool": "min"}, {"global_pool": "sum"}):
            with pytest.raises(ValueError):
                build(**bad)


def test_legacy_parameter_counts():
    reset_names()
    assert zoo.rpv_legacy_cnn(device="cpu").count_params() == 34515201
    assert zoo.rpv_legacy_cnn(device="cpu", global_pool="avg").count_params() == 1091841


class _Built(Exception):
    pass


@pytest.mark.parametrize("cli", ["rpv", "mnist"])
@pytest.mark.parametrize("pool,gpool", [(None, None), ("avg", None), ("max", "avg"), ("avg", "max")])
def test_cli_pool_arguments(cli, pool, gpool, monkeypatch):
    from cori_intml_examples_amd.parallel import hvd
    monkeypatch.setenv("INTML_DEVICE", "cpu")
    got = {}
    mod, attr = (rpv_app, "build_model") if cli == "rpv" else (zoo, "mnist_cnn")
    orig = getattr(mod, attr)

    def capture(*a, **kw):
        got["model"] = orig(*a, **kw)
        raise _Built()
    monkeypatch.setattr(mod, attr, capture)
    argv = (["--pool", pool] if pool else []) + (["--global-pool", gpool] if gpool else [])
    if cli == "rpv":
        argv += ["--synthetic", "--n-train", "32", "--n-valid", "16", "--h1", "4", "--h2", "4", "--h3", "4", "--h4", "8"]
        ns = train_rpv.build_parser().parse_args(argv)
    else:
        argv += ["--n-train", "32", "--h1", "2", "--h2", "2", "--h3", "4"]
        ns = train_mnist.build_parser().parse_args(argv)
    assert ns.pool == (pool or "max") and ns.global_pool == gpool
    try:
        with pytest.raises(_Built):
            (train_rpv if cli == "rpv" else train_mnist).main(argv)
    finally:
        hvd.shutdown()
    types = _types(got["model"])
    assert ("AveragePooling2D" in types) == (pool == "avg") and ("MaxPooling2D" in types) == (pool != "avg")
    bridge = {None: "Flatten", "avg": "GlobalAveragePooling2D", "max": "GlobalMaxPooling2D"}[gpool]
    assert bridge in types and len(set(types) & {"Flatten", "GlobalAveragePooling2D", "GlobalMaxPooling2D"}) == 1


def test_benchmark_script_variants():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("optimizer_step_bench", os.path.join(root, "benchmarks",
                                                                                        "optimizer_step.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    v = mod.variants(["Adam"], None, pool="avg", global_pool="avg")
    assert [(x[0], x[3], x[5]) for x in v] == [("Adam", None, "relu"), ("Adam/unstacked", "conv_stack=0", "relu"),
                                               ("Adam/pool-avg", None, "relu+pool=avg"),
                                               ("Adam/gpool-avg", None, "relu+gpool=avg")]
    assert [x[0] for x in mod.variants(["Adam"], None)] == ["Adam"]
