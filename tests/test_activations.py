"""Hidden activations beyond relu / linear (tanh, sigmoid, hard_sigmoid, elu, selu, softplus,
softsign, the LeakyReLU / ELU / Activation layers) on the CPU: the fp32 twins against the
float64 oracle, the layers, the plan's folding rules, the CPU executor against an independent
autograd model, checkpoints, the compat names, the builders and the CLIs."""
import sys

import numpy as np
import pytest
import torch

from cori_intml_examples_amd import activations, optim
from cori_intml_examples_amd.apps import mnist as mnist_app
from cori_intml_examples_amd.apps import rpv as rpv_app
from cori_intml_examples_amd.apps import train_mnist, train_rpv, zoo
from cori_intml_examples_amd.io.keras_h5 import load_model
from cori_intml_examples_amd.models import (ELU, Activation, Conv2D, Dense, Dropout, Flatten, Input, LeakyReLU,
                                            MaxPooling2D, Model, Sequential, reset_names)
from cori_intml_examples_amd.models.layers import LAYER_CLASSES, Layer
from cori_intml_examples_amd.models.plan import build_plan
from cori_intml_examples_amd.ops import reference as R
from cori_intml_examples_amd.utils import set_random_seed

from helpers import act_models as M
from helpers import act_oracle as O

A03 = float(np.float32(0.3))


# ------------------------------------------------------------------------------------ 1. the fp32 twins
def _grid():
    g = np.concatenate([np.linspace(-20, 20, 4001), np.linspace(-1e-3, 1e-3, 201), [-88.0, -30.0, 30.0, 88.0]])
    return np.unique(g.astype(np.float32))


@pytest.mark.parametrize("name,alpha", O.CASES)
def test_fp32_twins_match_the_float64_oracle(name, alpha):
    """fp32 evaluation of O(1)-sized expressions: a few fp32 roundings, relative to the value or
    (where 0.2 x + 0.5 or 1 + e^-x cancel) to the O(1) intermediate."""
    x = _grid()
    got = R.act(name, alpha, torch.tensor(x)).numpy().astype(np.float64)
    want = O.act(name, alpha, x)
    tol = 8 * 2.0 ** -24
    assert np.all(np.abs(got - want) <= tol * np.abs(want) + tol), np.abs(got - want).max()
    y = want.astype(np.float32)
    gg = R.act_grad_from_output(name, alpha, torch.tensor(y)).numpy().astype(np.float64)
    gw = O.act_grad_from_output(name, alpha, y)
    assert np.all(np.abs(gg - gw) <= tol * np.abs(gw) + tol), np.abs(gg - gw).max()
    assert np.all(gg >= 0) and np.all(gw >= 0)
    assert np.all(np.diff(want) >= 0)                            # non-decreasing


@pytest.mark.parametrize("name,alpha", O.CASES)
def test_derivative_from_output_is_the_derivative(name, alpha):
    """A'(A(x)) == dA/dx: float64 autograd through the twin's formula (which equals the oracle's
    to 1e-14) against the oracle's derivative-from-output, away from the kinks."""
    x = np.linspace(-12, 12, 2401) + 1e-3
    if name == "hard_sigmoid":
        x = x[np.abs(np.abs(x) - 2.5) > 1e-2]
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    yt = R.act(name, alpha, xt)
    assert np.abs(yt.detach().numpy() - O.act(name, alpha, x)).max() < 1e-14 * max(1.0, np.abs(x).max())
    yt.sum().backward()
    want = xt.grad.numpy()
    got = O.act_grad_from_output(name, alpha, O.act(name, alpha, x))
    # (y carries a float64 rounding of its own: 1 - y^2 near saturation loses relative accuracy)
    assert np.all(np.abs(got - want) <= 1e-6 * np.abs(want) + 1e-12), np.abs(got - want).max()


def test_limits_and_nan():
    inf, nan = float("inf"), float("nan")
    x = torch.tensor([-inf, inf, nan])
    lim = {"tanh": (-1, 1), "sigmoid": (0, 1), "hard_sigmoid": (0, 1), "elu": (-1, inf), "softplus": (0, inf),
           "softsign": (-1, 1), "selu": (-O.SELU_S * O.SELU_A, inf)}
    for name, (lo, hi) in lim.items():
        for fn in (lambda v: R.act(name, 1.0, v).numpy(), lambda v: O.act(name, 1.0, v.numpy())):
            v = fn(x)
            assert abs(v[0] - lo) < 1e-6 and (v[1] == hi or abs(v[1] - hi) < 1e-6) and np.isnan(v[2]), (name, v)
    for alpha, lo in ((0.0, 0.0), (A03, -inf)):
        for v in (R.act("leaky_relu", alpha, x).numpy(), O.act("leaky_relu", alpha, x.numpy())):
            assert v[0] == lo and v[1] == inf and np.isnan(v[2])


def test_activations_module():
    assert set(activations.NAMES) == {"linear", "relu", "softmax"} | set(O.STRINGS)
    for n in activations.NAMES:
        fn = activations.get(n)
        assert activations.serialize(fn) == n and activations.deserialize(n) is fn
    assert activations.get(None) is activations.linear and activations.serialize(None) == "linear"
    x = np.linspace(-3, 3, 13).astype(np.float32)
    for n in O.STRINGS:
        np.testing.assert_allclose(activations.get(n)(x), O.act(n, 1.0, x), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(activations.elu(x, 0.5), O.act("elu", 0.5, x), rtol=1e-5, atol=1e-6)
    with pytest.raises(ValueError):
        activations.get("swish")
    # a function as the layer argument records its name
    assert Dense(3, activation=activations.tanh).activation == "tanh"


# ------------------------------------------------------------------------------------ 2. the layers
def test_layer_configs_and_names():
    reset_names()
    a, l, e, l2 = Activation("tanh"), LeakyReLU(), ELU(), LeakyReLU(alpha=0.1)
    assert [x.name for x in (a, l, e, l2)] == ["activation_1", "leaky_re_lu_1", "elu_1", "leaky_re_lu_2"]
    assert a.get_config() == {"name": "activation_1", "trainable": True, "activation": "tanh"}
    assert l.get_config() == {"name": "leaky_re_lu_1", "trainable": True, "alpha": 0.30000001192092896}
    assert e.get_config() == {"name": "elu_1", "trainable": True, "alpha": 1.0}
    assert l2.get_config()["alpha"] == float(np.float32(0.1))
    for x in (a, l, e):
        assert x.weight_specs() == [] and x.count_params() == 0
        y = LAYER_CLASSES[type(x).__name__].from_config(x.get_config())
        assert y.get_config() == x.get_config()
    assert Activation("linear").activation is None and Activation("linear").get_config()["activation"] == "linear"
    for n in O.STRINGS:
        assert n in Layer.activation_names
        assert Conv2D(2, (3, 3), activation=n).get_config()["activation"] == n
        assert Dense(2, activation=n).get_config()["activation"] == n


def test_negative_alpha_is_a_value_error():
    for cls in (LeakyReLU, ELU):
        with pytest.raises(ValueError, match="neg_layer"):
            cls(alpha=-0.1, name="neg_layer")
        assert cls(alpha=0.0).alpha == 0.0
    with pytest.raises(ValueError):
        Dense(3, activation="swish")


# ------------------------------------------------------------------------------------ 3. the plan
def _chain(*layers):
    t = Input(shape=(8, 8, 2))
    first = t
    for l in layers:
        t = l(t)
    m = Model(first, t, device="cpu")
    return [first.layer] + list(layers)


def _plan(*layers, loss="binary_crossentropy"):
    return build_plan(_chain(*layers), loss)


def test_strings_and_layers_become_stage_activations():
    p = _plan(Conv2D(4, (3, 3), activation="tanh"), MaxPooling2D(), Conv2D(4, (3, 3)), ELU(0.5), Flatten(),
              Dense(8, activation="elu"), Dense(8), LeakyReLU(), Dropout(0.1), Dense(8, activation="sigmoid"),
              Dense(1, activation="sigmoid"))
    assert [(c.relu, c.act, c.act_alpha) for c in p.convs] == [(False, "tanh", 0.0), (False, "elu", 0.5)]
    assert [(d.relu, d.act, d.act_alpha) for d in p.denses] == [(False, "elu", 1.0), (False, "leaky_relu", A03),
                                                                 (False, "sigmoid", 0.0)]
    assert p.denses[1].dropout is not None and p.head.activation == "sigmoid"
    # relu / linear stages keep act = None
    q = _plan(Conv2D(4, (3, 3), activation="relu"), Conv2D(4, (3, 3)), Flatten(), Dense(1, activation="sigmoid"))
    assert [(c.relu, c.act) for c in q.convs] == [(True, None), (False, None)]


def test_activation_relu_folds_to_the_relu_stage():
    reset_names()
    a = _plan(Conv2D(4, (3, 3)), Activation("relu"), MaxPooling2D(), Dropout(0.2), Flatten(), Dense(8),
              Activation("relu"), Dense(4), Activation("linear"), Dense(1, activation="sigmoid"))
    b = _plan(Conv2D(4, (3, 3), activation="relu"), MaxPooling2D(), Dropout(0.2), Flatten(),
              Dense(8, activation="relu"), Dense(4), Dense(1, activation="sigmoid"))
    key = lambda p: ([(c.relu, c.act, c.act_alpha, c.pool is not None, c.rate, c.stream, c.out_shape) for c in p.convs],
                     [(d.relu, d.act, d.act_alpha, d.K, d.N, d.rate, d.stream) for d in p.denses],
                     (p.head.K, p.head.N, p.head.activation, p.head.loss))
    assert key(a) == key(b)


def test_dense_plus_activation_softmax_is_the_head():
    p = _plan(Flatten(), Dense(8, activation="tanh"), Dense(3), Activation("softmax"), loss="categorical_crossentropy")
    assert len(p.denses) == 1 and p.head.N == 3 and p.head.activation == "softmax"
    p = _plan(Flatten(), Dense(1), Activation("sigmoid"))
    assert not p.denses and p.head.activation == "sigmoid"
    with pytest.raises(NotImplementedError, match="output activation tanh"):
        _plan(Flatten(), Dense(1), Activation("tanh"))
    with pytest.raises(NotImplementedError):
        _plan(Flatten(), Dense(1), LeakyReLU())


def test_unsupported_placements_name_both_layers():
    with pytest.raises(NotImplementedError, match=r"(?s)act_x.*conv_x|conv_x.*act_x"):
        _plan(Conv2D(4, (3, 3), activation="relu", name="conv_x"), Activation("tanh", name="act_x"), Flatten(), Dense(1))
    with pytest.raises(NotImplementedError, match=r"(?s)act_y.*dense_y|dense_y.*act_y"):
        _plan(Flatten(), Dense(4, activation="tanh", name="dense_y"), LeakyReLU(name="act_y"), Dense(1))
    for before in (MaxPooling2D(name="blocker"), Dropout(0.1, name="blocker")):
        with pytest.raises(NotImplementedError, match=r"(?s)act_z.*blocker"):
            _plan(Conv2D(4, (3, 3)), before, Activation("tanh", name="act_z"), Flatten(), Dense(1))
    with pytest.raises(NotImplementedError, match=r"(?s)act_z.*blocker"):
        _plan(Conv2D(4, (3, 3)), Flatten(name="blocker"), ELU(name="act_z"), Dense(1))
    with pytest.raises(NotImplementedError, match="act_in"):
        _plan(Activation("tanh", name="act_in"), Flatten(), Dense(1))
    with pytest.raises(NotImplementedError, match="softmax"):
        _plan(Flatten(), Dense(4, activation="softmax"), Dense(1))
    with pytest.raises(NotImplementedError, match="softmax"):
        _plan(Flatten(), Dense(4), Activation("softmax"), Dense(1))


# ------------------------------------------------------------------------------------ 4. the CPU executor
def _grads(m):
    return [m.store.view(l, n, grad=True).numpy().copy() for l in m.layers for n, _, _ in l.weight_specs()]


@pytest.mark.parametrize("kind,act", [("tiny", "tanh"), ("odd", ("LeakyReLU", 0.3)), ("odd", ("ELU", 0.5)),
                                      ("tiny", "softplus"), ("odd", "selu")])
def test_cpu_executor_gradients_match_autograd(kind, act):
    """One training step (dropout 0.25) of the CPU executor's hand-written backward -- A' from
    the stored, dropout-scaled output -- against autograd of an independently written model in
    Keras' order (activate, then pool).  fp32 on both sides."""
    set_random_seed(3)
    m = M.build(kind, optim.SGD(lr=0.0), "cpu", drop=0.25, act=act)
    rs = np.random.RandomState(1)
    x = rs.rand(24, *m.input_shape[1:]).astype(np.float32)
    nout = m.output_shape[-1]
    y = (rs.rand(24) > 0.5).astype(np.float32) if nout == 1 else np.eye(nout, dtype=np.float32)[rs.randint(0, nout, 24)]
    loss, want = M.torch_loss_grads(m, x, y, step=1)
    ex = m._executor
    d = ex.upload(x, y)
    ex.reset_metrics()
    ex.train_step(d, torch.arange(d.n), 0, d.n)
    got = _grads(m)
    assert abs(ex.read_metrics()[0] - loss) < 1e-5 * max(1.0, loss)
    for g, w in zip(got, want):
        assert np.linalg.norm(g - w) <= 1e-4 * np.linalg.norm(w) + 1e-7, (kind, act, g.shape)
    assert all(np.linalg.norm(w) > 0 for w in want)


def test_three_steps_checkpoint_and_predictions(tmp_path):
    set_random_seed(5)
    inp = Input(shape=(16, 16, 3))
    h = Conv2D(4, (3, 3), padding="same")(inp)
    h = LeakyReLU(alpha=0.2)(h)
    h = MaxPooling2D()(h)
    h = Conv2D(6, (3, 3), activation="elu")(h)
    h = Flatten()(Dropout(0.1)(h))
    h = ELU(0.7)(Dense(8)(h))
    h = Dense(5, activation="softsign")(h)
    out = Activation("softmax")(Dense(3)(h))
    m = Model(inp, out, device="cpu")
    m.compile(optimizer=optim.Adam(lr=0.01), loss="categorical_crossentropy", metrics=["accuracy"])
    rs = np.random.RandomState(0)
    x = rs.rand(48, 16, 16, 3).astype(np.float32)
    y = np.eye(3, dtype=np.float32)[rs.randint(0, 3, 48)]
    w0 = [w.copy() for w in m.get_weights()]
    losses = [m.train_on_batch(x[16 * k:16 * k + 16], y[16 * k:16 * k + 16])[0] for k in range(3)]
    assert np.all(np.isfinite(losses)) and m.optimizer.iterations == 3
    assert all(np.abs(a - b).max() > 1e-4 for a, b in zip(w0, m.get_weights()))
    p = str(tmp_path / "m.h5")
    m.save(p)
    c = load_model(p, device="cpu")
    assert [type(l).__name__ for l in c.layers] == [type(l).__name__ for l in m.layers]
    assert [l.get_config() for l in c.layers] == [l.get_config() for l in m.layers]
    assert c.get_config() == m.get_config()
    np.testing.assert_array_equal(c.predict(x, batch_size=16), m.predict(x, batch_size=16))
    assert c.test_on_batch(x[:16], y[:16]) == m.test_on_batch(x[:16], y[:16])
    assert np.isfinite(c.train_on_batch(x[:16], y[:16])[0]) and c.optimizer.iterations == 4      # it continues
    import io
    from contextlib import redirect_stdout
    buf = io.StringIO()
    with redirect_stdout(buf):
        m.summary()
    assert "leaky_re_lu" in buf.getvalue() and "(LeakyReLU)" in buf.getvalue() and "(Activation)" in buf.getvalue()


def test_sequential_and_compat_names():
    from cori_intml_examples_amd import compat
    saved = {k: v for k, v in sys.modules.items() if k == "keras" or k.startswith("keras.")}
    try:
        compat.install(force=True, groups=("keras",))
        import keras
        from keras import activations as ka
        from keras.layers import ELU as KE
        from keras.layers import Activation as KA
        from keras.layers import LeakyReLU as KL
        assert (KA, KL, KE) == (Activation, LeakyReLU, ELU) and ka is activations and keras.activations is activations
        m = keras.models.Sequential(device="cpu")
        m.add(keras.layers.Dense(4, input_shape=(6,)))
        m.add(KL(0.1))
        m.add(keras.layers.Dense(3))
        m.add(KA("softmax"))
        m.compile(optimizer="SGD", loss="categorical_crossentropy")
        assert m._executor.plan.denses[0].act == "leaky_relu" and m._executor.plan.head.activation == "softmax"
    finally:
        for k in [k for k in sys.modules if k == "keras" or k.startswith("keras.")]:
            del sys.modules[k]
        sys.modules.update(saved)


# ------------------------------------------------------------------------------------ 5. builders and CLIs
def _acts(m):
    return [l.get_config()["activation"] for l in m.layers if isinstance(l, (Conv2D, Dense))]


def test_builders_take_activation():
    builds = [lambda **kw: zoo.rpv_cnn((16, 16, 1), conv_sizes=[4, 8], fc_sizes=[8], device="cpu", **kw),
              lambda **kw: rpv_app.build_model((16, 16, 1), conv_sizes=[4, 8], fc_sizes=[8], device="cpu", **kw),
              lambda **kw: zoo.mnist_cnn(device="cpu", **kw), lambda **kw: mnist_app.build_model(device="cpu", **kw),
              lambda **kw: zoo.rpv_legacy_cnn((16, 16, 1), h1=4, h2=4, h3=4, h4=4, h5=8, device="cpu", **kw)]
    for build in builds:
        reset_names()
        a = build()
        reset_names()
        b = build(activation="relu")
        assert [l.get_config() for l in a.layers] == [l.get_config() for l in b.layers]
        assert [type(l) for l in a.layers] == [type(l) for l in b.layers]
        assert set(_acts(a)[:-1]) == {"relu"}
        t = build(activation="tanh")
        assert set(_acts(t)[:-1]) == {"tanh"} and _acts(t)[-1] == _acts(a)[-1]
        p = t._executor.plan
        assert all(s.act == "tanh" and not s.relu for s in p.convs + p.denses)


class _Built(Exception):
    pass


@pytest.mark.parametrize("cli", ["rpv", "mnist"])
@pytest.mark.parametrize("act", [None, "relu", "elu"])
def test_cli_activation(cli, act, monkeypatch):
    from cori_intml_examples_amd.parallel import hvd
    monkeypatch.setenv("INTML_DEVICE", "cpu")
    got = {}
    mod, attr = (rpv_app, "build_model") if cli == "rpv" else (zoo, "mnist_cnn")
    orig = getattr(mod, attr)

    def capture(*a, **kw):
        got["model"] = orig(*a, **kw)
        raise _Built()
    monkeypatch.setattr(mod, attr, capture)
    argv = ["--activation", act] if act is not None else []
    if cli == "rpv":
        argv += ["--synthetic", "--n-train", "32", "--n-valid", "16", "--h1", "4", "--h2", "4", "--h3", "4", "--h4", "8"]
        assert train_rpv.build_parser().parse_args(argv).activation == (act or "relu")
    else:
        argv += ["--n-train", "32", "--h1", "2", "--h2", "2", "--h3", "4"]
        assert train_mnist.build_parser().parse_args(argv).activation == (act or "relu")
    try:
        with pytest.raises(_Built):
            (train_rpv if cli == "rpv" else train_mnist).main(argv)
    finally:
        hvd.shutdown()
    assert set(_acts(got["model"])[:-1]) == {act or "relu"}


def test_benchmark_script_variants():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("optimizer_step_bench", os.path.join(root, "benchmarks",
                                                                                        "optimizer_step.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    v = mod.variants(["Adam"], None, None, ["tanh", "elu"])
    assert [(x[0], x[3], x[5]) for x in v] == [("Adam", None, "relu"), ("Adam/perlayer", "conv_stack=0,fuse_head=0", "relu"),
                                               ("Adam/tanh", None, "tanh"), ("Adam/elu", None, "elu")]
    assert [x[0] for x in mod.variants(["Adam"], None)] == ["Adam"]
