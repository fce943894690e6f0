"""BatchNormalization on the CPU: the float64 oracle pinned by autograd and by
torch.nn.functional.batch_norm, the layer (config, rejected arguments, weights, summary), the
position rules of the plan, the parameter store, the CPU reference executor against an independent
autograd model, moving statistics, eval mode, HDF5, two gloo ranks, compat names, builders and CLIs."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cori_intml_examples_amd import optim
from cori_intml_examples_amd.apps import mnist as mnist_app
from cori_intml_examples_amd.apps import rpv as rpv_app
from cori_intml_examples_amd.apps import train_mnist, train_rpv, zoo
from cori_intml_examples_amd.io.datasets import synthetic_rpv
from cori_intml_examples_amd.io.h5 import H5File
from cori_intml_examples_amd.models import (ELU, Activation, BatchNormalization, Conv2D, Dense, Dropout, Flatten, Input,
                                            LeakyReLU, MaxPooling2D, Model, Sequential, load_model)
from cori_intml_examples_amd.models.layers import reset_names
from cori_intml_examples_amd.models.params import ParamStore
from cori_intml_examples_amd.models.plan import build_plan
from cori_intml_examples_amd.utils import set_random_seed

from helpers import bn_models as M
from helpers import bn_oracle as O
from test_dp import _torchrun

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-3


# ------------------------------------------------------------------------------------ 1. the oracle
def _case(seed=0, shape=(3, 7, 5, 4)):
    rng = np.random.default_rng(seed)
    z = rng.normal(0.5, 2.0, shape)
    C = shape[-1]
    return z, rng.normal(0.3, 1.0, C), rng.normal(0, 1, C), rng.normal(0, 1, shape[:1] + (shape[1] // 2, shape[2] // 2, C))


def test_oracle_is_pinned_by_float64_autograd():
    z, gamma, beta, dp = _case()
    zt, gt, bt = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (z, gamma, beta))
    z2 = zt.reshape(-1, z.shape[-1])
    mean = z2.mean(0)
    var = ((z2 - mean) ** 2).mean(0)
    u = gt * (zt - mean) / torch.sqrt(var + EPS) + bt
    p = F.max_pool2d(u.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    (p * torch.tensor(dp)).sum().backward()
    uo, xhat, mo, vo, m = O.forward_train(z, gamma, beta, EPS)
    po, code = O.maxpool2x2(uo)
    assert np.allclose(uo, u.detach().numpy(), rtol=1e-12, atol=1e-12) and np.allclose(po, p.detach().numpy(), rtol=1e-12)
    du = O.route(dp, code, z.shape[1:3])
    assert np.all(du[:, 6:, :, :] == 0) and np.all(du[:, :, 4:, :] == 0)        # 7 x 5: outside every window
    dz, dgamma, dbeta = O.backward(du, xhat, gamma, vo, EPS)
    assert np.allclose(dz, zt.grad.numpy(), rtol=1e-10, atol=1e-12)
    assert np.allclose(dgamma, gt.grad.numpy(), rtol=1e-10) and np.allclose(dbeta, bt.grad.numpy(), rtol=1e-10)
    assert np.abs(dz[:, 6, :, :]).max() > 0                   # the mean terms reach every element


def test_oracle_against_torch_batch_norm():
    """An independent implementation: the normalised output and the input gradient agree; only
    the running variance differs, by the documented factor (torch: m / (m - 1), Keras 2.2.4:
    m / (m - (1 + eps)))."""
    z, gamma, beta, _ = _case(1)
    C = z.shape[-1]
    mom = 0.9
    zt = torch.tensor(z, requires_grad=True)
    rm, rv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    out = F.batch_norm(zt.permute(0, 3, 1, 2), rm, rv, torch.tensor(gamma), torch.tensor(beta), training=True,
                       momentum=1 - mom, eps=EPS).permute(0, 2, 3, 1)
    g = np.random.default_rng(2).normal(0, 1, z.shape)
    (out * torch.tensor(g)).sum().backward()
    u, xhat, mean, var, m = O.forward_train(z, gamma, beta, EPS)
    assert np.allclose(u, out.detach().numpy(), rtol=1e-11, atol=1e-12)
    assert np.allclose(O.backward(g, xhat, gamma, var, EPS)[0], zt.grad.numpy(), rtol=1e-9, atol=1e-12)
    mm, mv = O.moving_update(np.zeros(C), np.ones(C), mean, var, m, mom, EPS)
    assert np.allclose(mm, rm.numpy(), rtol=1e-12)
    assert np.allclose((mv - mom) / (m / (m - (1 + EPS))), (rv.numpy() - mom) / (m / (m - 1.0)), rtol=1e-10)
    assert not np.allclose(mv, rv.numpy(), rtol=1e-7)
    # m = 1: var = 0 exactly, u = beta, the moving variance receives 0
    u1, x1, _, v1, m1 = O.forward_train(z[:1, :1, :1], gamma, beta, EPS)
    assert m1 == 1 and np.all(v1 == 0) and np.all(x1 == 0) and np.array_equal(u1.reshape(-1), beta)
    assert np.array_equal(O.moving_update(np.zeros(C), np.ones(C), z[0, 0, 0], v1, 1, mom, EPS)[1], np.full(C, mom))
    # ties: the first maximum in row-major window order
    t = np.zeros((1, 2, 2, 1))
    assert O.maxpool2x2(t)[1].item() == 0
    t[0, 1, 0, 0] = t[0, 1, 1, 0] = 1.0
    assert O.maxpool2x2(t)[1].item() == 2


# ------------------------------------------------------------------------------------ 2. the layer
def test_config_round_trip_and_naming():
    bn = BatchNormalization(momentum=0.9, epsilon=1e-5, center=False)
    assert bn.name == "batch_normalization_1" and BatchNormalization().name == "batch_normalization_2"
    cfg = bn.get_config()
    assert cfg == {"name": "batch_normalization_1", "trainable": True, "axis": -1, "momentum": 0.9, "epsilon": 1e-5,
                   "center": False, "scale": True, "beta_initializer": {"class_name": "Zeros", "config": {}},
                   "gamma_initializer": {"class_name": "Ones", "config": {}},
                   "moving_mean_initializer": {"class_name": "Zeros", "config": {}},
                   "moving_variance_initializer": {"class_name": "Ones", "config": {}},
                   "beta_regularizer": None, "gamma_regularizer": None, "beta_constraint": None, "gamma_constraint": None}
    assert BatchNormalization.from_config(cfg).get_config() == cfg
    d = BatchNormalization()
    assert (d.axis, d.momentum, d.epsilon, d.center, d.scale) == (-1, 0.99, 1e-3, True, True)


@pytest.mark.parametrize("kw,exc", [
    (dict(axis=1), NotImplementedError), (dict(axis=3), NotImplementedError), (dict(axis=[3]), NotImplementedError),
    (dict(beta_initializer="ones"), NotImplementedError), (dict(gamma_initializer="zeros"), NotImplementedError),
    (dict(moving_mean_initializer="ones"), NotImplementedError),
    (dict(moving_variance_initializer="glorot_uniform"), NotImplementedError),
    (dict(gamma_initializer={"class_name": "Constant", "config": {"value": 2}}), NotImplementedError),
    (dict(beta_regularizer="l2"), NotImplementedError), (dict(gamma_regularizer="l1"), NotImplementedError),
    (dict(beta_constraint="non_neg"), NotImplementedError), (dict(gamma_constraint="max_norm"), NotImplementedError),
    (dict(momentum=1.0), ValueError), (dict(momentum=-0.1), ValueError), (dict(epsilon=0.0), ValueError),
    (dict(epsilon=-1e-3), ValueError), (dict(trainable=False), NotImplementedError)])
def test_rejected_arguments_name_the_layer(kw, exc):
    with pytest.raises(exc, match="batch_normalization_1"):
        BatchNormalization(**kw)


def _chain(*layers, shape=(8, 8, 2)):
    m = Sequential(device="cpu")
    first = layers[0]
    first.batch_input_shape = (None,) + tuple(shape)
    for l in layers:
        m.add(l)
    return m


def test_weight_order_names_and_summary():
    m = _chain(Conv2D(5, (3, 3)), BatchNormalization(), Flatten(), Dense(4), BatchNormalization(scale=False),
               Dense(3), BatchNormalization(center=False), Dense(2, activation="softmax"))
    names = [s.name for s in m.store.specs]
    assert names[2:6] == ["batch_normalization_1/%s:0" % n for n in ("gamma", "beta", "moving_mean", "moving_variance")]
    assert names[8:11] == ["batch_normalization_2/%s:0" % n for n in ("beta", "moving_mean", "moving_variance")]
    assert names[13:16] == ["batch_normalization_3/%s:0" % n for n in ("gamma", "moving_mean", "moving_variance")]
    bn = m.layers[1]
    ws = bn.get_weights()
    assert [w.shape for w in ws] == [(5,)] * 4
    assert [w.tolist() for w in ws] == [[1.0] * 5, [0.0] * 5, [0.0] * 5, [1.0] * 5]
    bn.set_weights([np.full(5, v, np.float32) for v in (2, 3, 4, 5)])
    assert [w[0] for w in m.get_weights()[2:6]] == [2, 3, 4, 5]
    assert [w[0] for w in m.layers[1].get_weights()] == [2, 3, 4, 5]
    with pytest.raises(ValueError):
        bn.set_weights([np.zeros(5)] * 3)
    lines = []
    m.summary(print_fn=lines.append)
    total = m.count_params()
    assert "Non-trainable params: %d" % (2 * 5 + 2 * 4 + 2 * 3) in lines
    assert "Trainable params: {:,}".format(total - 24) in lines and "Total params: {:,}".format(total) in lines
    assert any(l.startswith("batch_normalization_1 (Batch") and l.rstrip().endswith("20") for l in lines)
    m.compile("adam", "categorical_crossentropy")
    assert all(len(s) == m.store.numel for s in m._executor.optimizer_state())      # no slots for moving statistics


# ------------------------------------------------------------------------------------ 3. the plan
def _plan(*layers, shape=(8, 8, 2), loss="categorical_crossentropy"):
    return build_plan(_chain(*layers, shape=shape)._chain, loss)


def test_positions_the_plan_accepts():
    p = _plan(Conv2D(4, (3, 3)), BatchNormalization(), Activation("relu"), MaxPooling2D(), Dropout(0.1),
              Conv2D(4, (3, 3), padding="same"), BatchNormalization(), LeakyReLU(0.2),
              Flatten(), Dense(6), BatchNormalization(), ELU(0.5), Dropout(0.2), Dense(5), BatchNormalization(),
              Dense(4, activation="tanh"), Dense(3, activation="softmax"))
    assert [(s.bn.name, s.relu, s.act, s.pool is not None, s.rate) for s in p.convs] == [
        ("batch_normalization_1", True, None, True, 0.1), ("batch_normalization_2", False, "leaky_relu", False, 0.0)]
    assert [(s.bn.name if s.bn else None, s.relu, s.act, s.rate) for s in p.denses] == [
        ("batch_normalization_3", False, "elu", 0.2), ("batch_normalization_4", False, None, 0.0), (None, False, "tanh", 0.0)]
    # a plan without BN compares equal to what it is today: the new field defaults to None
    q = _plan(Conv2D(4, (3, 3), activation="relu"), MaxPooling2D(), Flatten(), Dense(3, activation="softmax"))
    assert q.convs[0].bn is None and "bn" in type(q.convs[0]).__dataclass_fields__
    assert type(q.convs[0]).__dataclass_fields__["bn"].default is None


@pytest.mark.parametrize("layers,match", [
    (lambda: (Conv2D(4, (3, 3), activation="relu"), BatchNormalization(), Flatten(), Dense(3)),
     "batch_normalization_1 follows conv2d_1, which already has the activation relu"),
    (lambda: (Conv2D(4, (3, 3)), Activation("relu"), BatchNormalization(), Flatten(), Dense(3)),
     "batch_normalization_1 follows activation_1: BatchNormalization must directly follow"),
    (lambda: (Conv2D(4, (3, 3)), MaxPooling2D(), BatchNormalization(), Flatten(), Dense(3)),
     "batch_normalization_1 follows max_pooling2d_1"),
    (lambda: (Conv2D(4, (3, 3)), Dropout(0.1), BatchNormalization(), Flatten(), Dense(3)),
     "batch_normalization_1 follows dropout_1"),
    (lambda: (Conv2D(4, (3, 3)), Flatten(), BatchNormalization(), Dense(3)),
     "batch_normalization_1 follows flatten_1"),
    (lambda: (BatchNormalization(), Conv2D(4, (3, 3)), Flatten(), Dense(3)),
     "batch_normalization_1 follows batch_normalization_1_input"),
    (lambda: (Flatten(), Dense(4), Dense(3), BatchNormalization()),
     "batch_normalization_1 follows dense_2, the output Dense"),
    (lambda: (Conv2D(4, (3, 3)), BatchNormalization(), BatchNormalization(), Flatten(), Dense(3)),
     "batch_normalization_2 follows batch_normalization_1: two BatchNormalization layers on one stage"),
    (lambda: (Conv2D(4, (3, 3)), BatchNormalization(), Activation("relu"), Activation("tanh"), Flatten(), Dense(3)),
     "activation_2 follows"),
    (lambda: (Conv2D(4, (3, 3)), BatchNormalization(), MaxPooling2D(), Activation("relu"), Flatten(), Dense(3)),
     "activation_1 follows max_pooling2d_1"),
    (lambda: (Flatten(), Dense(4, activation="tanh"), BatchNormalization(), Dense(3)),
     "batch_normalization_1 follows dense_1, which already has the activation tanh"),
])
def test_position_rules_and_their_errors(layers, match):
    with pytest.raises(NotImplementedError, match=match):
        _plan(*layers())


# ------------------------------------------------------------------------------------ 4. the store
def test_store_without_batchnorm_is_unchanged_and_with_it_keeps_the_trainable_range():
    def layout(m):
        st = m.store
        return [(s.name, s.offset, s.numel, s.trainable) for s in st.specs], st.numel, st.capacity, st.master.numel()

    reset_names()
    plain = zoo.rpv_cnn((16, 16, 3), conv_sizes=[4, 8], fc_sizes=[8], device="cpu")
    specs, numel, cap, size = layout(plain)
    off = 0
    for name, o, n, tr in specs:                       # Keras order, packed, all trainable: as before
        assert o == off and tr
        off += n
    assert numel == off and cap == max(64, (off + 63) // 64 * 64) == size == plain.store.grad.numel()
    reset_names()
    bn = zoo.rpv_cnn((16, 16, 3), conv_sizes=[4, 8], fc_sizes=[8], device="cpu", batch_norm=True)
    st = bn.store
    train = [s for s in st.specs if s.trainable]
    frozen = [s for s in st.specs if not s.trainable]
    assert [s.short for s in frozen] == ["moving_mean", "moving_variance"] * 3
    off = 0
    for s in train:
        assert s.offset == off
        off += s.numel
    assert st.numel == off == numel + 2 * (4 + 8 + 8) and st.capacity == (off + 63) // 64 * 64 == st.grad.numel()
    off = st.capacity
    for s in frozen:
        assert s.offset == off
        off += s.numel
    assert st.master.numel() == st.total >= off
    assert set(st.layer_ranges()) == {l.name for l in bn.layers if l.count_params(trainable=True)}
    assert max(hi for _, hi in st.layer_ranges().values()) == st.numel
    with pytest.raises(KeyError):
        st.view(frozen[0].layer, "moving_mean", grad=True)
    for s in st.specs:                                 # ones / zeros through the constant kinds
        v = st.view(s.layer, s.short)
        if s.short in ("gamma", "moving_variance"):
            assert torch.all(v == 1)
        if s.short in ("beta", "moving_mean"):
            assert torch.all(v == 0)
    assert isinstance(st, ParamStore)


# ------------------------------------------------------------------------------------ 5. the CPU executor
def _randomise_bn(m, seed=3):
    rng = np.random.default_rng(seed)
    ws = []
    for w, s in zip(m.get_weights(), m.store.specs):
        if s.short == "gamma":
            w = rng.normal(0.8, 0.5, w.shape).astype(np.float32)
            w[0] = -abs(w[0]) - 0.2
        elif s.short == "beta":
            w = rng.normal(0, 0.3, w.shape).astype(np.float32)
        elif s.short == "moving_mean":
            w = rng.normal(0, 0.2, w.shape).astype(np.float32)
        elif s.short == "moving_variance":
            w = rng.uniform(0.5, 1.5, w.shape).astype(np.float32)
        ws.append(w)
    m.set_weights(ws)


CASES = [("tiny", "relu", {}), ("tiny", ("LeakyReLU", 0.3), {}), ("odd", "tanh", {}), ("odd", "relu", {"center": False}),
         ("tiny", "tanh", {"scale": False}), ("odd", None, {"momentum": 0.5, "epsilon": 1e-2})]


@pytest.mark.parametrize("kind,act,kw", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_cpu_executor_against_the_autograd_model(kind, act, kw):
    """One training step of the CPU executor (fp32) against an independently written autograd model
    in Keras' order -- conv+BN+relu+pool, conv+BN+LeakyReLU, dense+BN+tanh, center=False,
    scale=False -- gradients of every trainable tensor, and the moving statistics against the
    float64 oracle's update from the autograd model's batch statistics."""
    set_random_seed(5)
    m = M.build(kind, optim.SGD(lr=0.0), "cpu", drop=0.2, act=act, **kw)
    _randomise_bn(m)
    x, y, _ = synthetic_rpv(6, channels=m.input_shape[-1], size=16, seed=1) if kind == "tiny" else (None, None, None)
    if kind == "odd":
        rs = np.random.RandomState(2)
        x, y = rs.rand(6, 19, 17, 2).astype(np.float32), np.eye(3, dtype=np.float32)[rs.randint(0, 3, 6)]
    w0 = m.get_weights()
    ex = m._executor
    d = ex.upload(x, y)
    ex.reset_metrics()
    ex.train_step(d, torch.arange(d.n), 0, d.n)
    loss, want, stats = M.torch_loss_grads(m.__class__ and _clone(kind, act, kw, w0, m._seed), x, y, step=1)
    assert abs(ex.read_metrics()[0] - loss) < 1e-5 * max(1.0, abs(loss))
    assert len(stats) == sum(type(l).__name__ == "BatchNormalization" for l in m.layers)
    for s, g in zip(m.store.specs, want):
        if not s.trainable:
            assert g is None
            continue
        got = m.store.view(s.layer, s.short, grad=True).numpy()
        # (the bias ahead of a BN has the exact gradient 0: both sides hold rounding noise there)
        ahead_of_bn = s.short == "bias" and any(
            st.bn is not None and s.layer in (getattr(st, "conv", None), getattr(st, "dense", None))
            for st in m._plan.convs + m._plan.denses)
        tol = 1e-4 * np.linalg.norm(g) + 1e-6
        assert np.linalg.norm(got - g) <= (2e-5 if ahead_of_bn else tol), (s.name, np.linalg.norm(got - g), np.linalg.norm(g))
    k = 0
    frozen = [(s, w) for s, w in zip(m.store.specs, w0) if not s.trainable]
    bns = [l for l in m.layers if type(l).__name__ == "BatchNormalization"]
    for layer, (_, mean, var, rows) in zip(bns, stats):      # (the twin's layers have names of their own)
        wm, wv = O.moving_update(frozen[k][1], frozen[k + 1][1], mean, var, rows, layer.momentum, layer.epsilon)
        mm, mv = layer.get_weights()[-2:]
        assert np.allclose(mm, wm, rtol=1e-5, atol=1e-6) and np.allclose(mv, wv, rtol=1e-5, atol=1e-6), layer.name
        k += 2


def _clone(kind, act, kw, weights, seed):
    m = M.build(kind, optim.SGD(lr=0.0), "cpu", drop=0.2, act=act, **kw)
    m.set_weights(weights)
    m._seed = seed
    return m


def test_moving_statistics_after_k_steps_and_eval_mode():
    set_random_seed(9)
    m = M.tiny(optim.SGD(lr=0.0), drop=0.0, act="relu", momentum=0.8)        # lr 0: the weights stay, the statistics move
    _randomise_bn(m)
    x, y, _ = synthetic_rpv(24, channels=3, size=16, seed=2)
    w0 = m.get_weights()
    want = {s.name: w.astype(np.float64) for s, w in zip(m.store.specs, w0) if not s.trainable}
    for k in range(4):
        xb, yb = x[6 * k:6 * k + 6], y[6 * k:6 * k + 6]
        _, _, stats = M.torch_loss_grads(m, xb, yb, step=k + 1, dtype=torch.float64)
        for name, mean, var, rows in stats:
            a, b = name + "/moving_mean:0", name + "/moving_variance:0"
            want[a], want[b] = O.moving_update(want[a], want[b], mean, var, rows, 0.8, EPS)
        before = m.predict(x[:5])
        m.train_on_batch(xb, yb)
    for s, w in zip(m.store.specs, m.get_weights()):
        if s.trainable:
            assert np.array_equal(w, w0[m.store.specs.index(s)])
        else:
            assert np.allclose(w, want[s.name], rtol=1e-4, atol=1e-5), s.name
    # evaluation, test_on_batch and predict use the moving statistics and update nothing
    snap = m.store.master.clone()
    p = m.predict(x)
    ev = m.evaluate(x, y, batch_size=7, verbose=0)
    tb = m.test_on_batch(x[:6], y[:6])
    assert torch.equal(snap, m.store.master)
    ws = [torch.tensor(w) for w in m.get_weights()]
    ref = torch.sigmoid(M.torch_forward(m, ws, torch.tensor(x), step=None)).numpy()
    assert np.allclose(p, ref, rtol=1e-4, atol=1e-5)
    assert not np.allclose(p[:5], before, atol=1e-6)         # the last step moved the statistics predict uses
    assert np.array_equal(m.predict(x[:3], batch_size=3), p[:3])             # no batch dependence
    # train mode differs from eval mode on the same batch
    ztrain = torch.sigmoid(M.torch_forward(m, ws, torch.tensor(x[:6]), step=99)).detach().numpy()
    assert np.abs(ztrain - p[:6]).max() > 1e-3 and np.isfinite(ev[0]) and np.isfinite(tb[0])


def test_ref_bf16_rounds_at_the_storage_points(monkeypatch):
    monkeypatch.setenv("INTML_TUNE", "ref_bf16=1")
    set_random_seed(4)
    m = M.odd(optim.SGD(lr=0.0), act="relu")
    assert m._executor.emulate_bf16
    x = np.random.RandomState(0).rand(6, 19, 17, 2).astype(np.float32)
    y = np.eye(3, dtype=np.float32)[[0, 1, 2, 0, 1, 2]]
    seen = {}
    orig = type(m._executor)._bn_backward

    def spy(self, bn, du, ctx):
        dz = orig(self, bn, du, ctx)
        seen[bn.name] = (du.clone(), dz.clone())
        return dz
    monkeypatch.setattr(type(m._executor), "_bn_backward", spy)
    m.train_on_batch(x, y)
    q = lambda t: t.to(torch.bfloat16).to(torch.float32)
    assert len(seen) == 3
    for du, dz in seen.values():
        assert torch.equal(q(du), du) and torch.equal(q(dz), dz)        # the gradient buffer and dz are bf16 values
    du0 = seen["batch_normalization_1"][0]
    assert torch.all(du0[:, 18, :, :] == 0) and torch.all(du0[:, :, 16, :] == 0)
    assert seen["batch_normalization_1"][1][:, 18].abs().max() > 0


# ------------------------------------------------------------------------------------ 6. HDF5
def test_hdf5_round_trip_and_optimizer_weights(tmp_path):
    set_random_seed(3)
    m = M.tiny(optim.Adam(lr=0.01), drop=0.1, act="relu", momentum=0.9)
    x, y, _ = synthetic_rpv(32, channels=3, size=16, seed=1)
    m.fit(x, y, batch_size=8, epochs=1, verbose=0, shuffle=False)
    p = str(tmp_path / "m.h5")
    m.save(p)
    with H5File(p, "r") as f:
        names = [str(n) for n in f.attrs("model_weights/batch_normalization_1")["weight_names"]]
        assert names == ["batch_normalization_1/%s:0" % n for n in ("gamma", "beta", "moving_mean", "moving_variance")]
        opt_names = [str(n) for n in f.attrs("optimizer_weights")["weight_names"]]
        n_train = sum(s.trainable for s in m.store.specs)
        assert len(m.store.specs) == n_train + 8
        # Adam: iterations, then m and v per TRAINABLE tensor, then Keras' vhat placeholders
        assert len(opt_names) == 1 + 3 * n_train
        shapes = [tuple(f.read_dataset("optimizer_weights/" + n).shape) for n in opt_names[1:1 + n_train]]
        assert shapes == [s.shape for s in m.store.specs if s.trainable]
    m2 = load_model(p)
    assert [l.get_config() for l in m2.layers] == [l.get_config() for l in m.layers]
    for a, b in zip(m.get_weights(), m2.get_weights()):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(m._executor.optimizer_state(), m2._executor.optimizer_state()):
        assert torch.equal(a, b)
    assert m2.optimizer.iterations == 4
    assert np.array_equal(m.predict(x), m2.predict(x))
    w = str(tmp_path / "w.h5")
    m.save_weights(w)
    m3 = M.tiny(optim.Adam(), act="relu")
    assert not np.array_equal(m3.get_weights()[4], m.get_weights()[4])
    m3.load_weights(w)
    for a, b in zip(m.get_weights(), m3.get_weights()):
        np.testing.assert_array_equal(a, b)
    # functional and Sequential configs know the layer
    s = _chain(Conv2D(4, (3, 3)), BatchNormalization(momentum=0.7), Flatten(), Dense(2, activation="softmax"))
    s.compile("sgd", "categorical_crossentropy")
    ps = str(tmp_path / "s.h5")
    s.save(ps)
    assert load_model(ps).layers[1].momentum == 0.7


# ------------------------------------------------------------------------------------ 7. data parallel
def test_two_ranks_keep_their_own_statistics(tmp_path):
    r = _torchrun(2, [os.path.join(ROOT, "tests", "bn_dp_worker.py"), str(tmp_path)])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    reps = [json.load(open(tmp_path / ("rank%d.json" % i))) for i in range(2)]
    print(json.dumps(reps, indent=1))
    assert reps[0]["trainable_digest"] == reps[1]["trainable_digest"]          # identical trainable weights
    assert reps[0]["moving_digest"] != reps[1]["moving_digest"]                # each rank's own statistics
    for rep in reps:
        assert rep["size"] == 2 and rep["moved"] > 1e-4, rep
        assert rep["moving_err_vs_local_oracle"] < 1e-5, rep
        assert rep["digest_check_identical"], rep
        # the broadcast carried rank 0's moving statistics (0 + 0.25 and 1 + 0.25)
        assert rep["moving_after_broadcast"] == pytest.approx([0.25, 1.25] * 4), rep


# ------------------------------------------------------------------------------------ 8. compat, builders, CLIs
def test_compat_names():
    from cori_intml_examples_amd import compat
    compat.install()
    import keras
    from keras.layers import BatchNormalization as KBN
    assert KBN is BatchNormalization and keras.layers.BatchNormalization is BatchNormalization
    import cori_intml_examples_amd as pkg
    assert pkg.BatchNormalization is BatchNormalization and pkg.models.layers.BatchNormalization is BatchNormalization


def _kinds(m):
    return [type(l).__name__ for l in m.layers if type(l).__name__ != "InputLayer"]


def test_builders_take_batch_norm():
    for build in (lambda **kw: zoo.rpv_cnn((16, 16, 1), conv_sizes=[4, 8], fc_sizes=[8], device="cpu", **kw),
                  lambda **kw: rpv_app.build_model((16, 16, 1), conv_sizes=[4, 8], fc_sizes=[8], device="cpu", **kw),
                  lambda **kw: zoo.mnist_cnn(device="cpu", **kw), lambda **kw: mnist_app.build_model(device="cpu", **kw),
                  lambda **kw: zoo.rpv_legacy_cnn((16, 16, 1), h1=4, h2=4, h3=4, h4=4, h5=8, device="cpu", **kw)):
        reset_names()
        a = build()
        reset_names()
        b = build(batch_norm=False)
        assert [l.get_config() for l in a.layers] == [l.get_config() for l in b.layers]
        assert "BatchNormalization" not in _kinds(a) and a.store.total == a.store.capacity
        m = build(batch_norm=True, activation="tanh")
        kinds = _kinds(m)
        hidden = [i for i, k in enumerate(kinds[:-1]) if k in ("Conv2D", "Dense")]
        assert hidden and all(kinds[i + 1:i + 3] == ["BatchNormalization", "Activation"] for i in hidden)
        assert all(l.activation is None for l in m.layers[:-1] if isinstance(l, (Conv2D, Dense)))
        assert all(l.activation == "tanh" for l in m.layers[:-1] if isinstance(l, Activation))
        stages = m._plan.convs + m._plan.denses
        assert all(s.bn is not None and s.act == "tanh" for s in stages) and len(stages) == len(hidden)


class _Built(Exception):
    pass


@pytest.mark.parametrize("mod,name", [(train_rpv, "build_model"), (train_mnist, "mnist_cnn")])
def test_clis_take_batch_norm(mod, name, monkeypatch):
    p = mod.build_parser()
    assert p.parse_args([]).batch_norm is False and p.parse_args(["--batch-norm"]).batch_norm is True
