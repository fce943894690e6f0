"""Keras L1 / L2 weight regularizers on the CPU: the public module (get / serialize / the three
constructors, float32-rounded coefficients, errors), the layers' config surface, the float64
oracle of tests/helpers/reg_oracle.py pinned by autograd, the CPU executor's regularized steps,
losses and clipping against that oracle, HDF5 round trips, two gloo ranks and the builders' /
CLIs' ``l2``."""
import json
import os

import numpy as np
import pytest
import torch

import cori_intml_examples_amd as pkg
from cori_intml_examples_amd import optim, regularizers
from cori_intml_examples_amd.apps import mnist as mnist_app
from cori_intml_examples_amd.apps import rpv as rpv_app
from cori_intml_examples_amd.apps import train_mnist, train_rpv, zoo
from cori_intml_examples_amd.io.datasets import synthetic_rpv
from cori_intml_examples_amd.io.h5 import H5File
from cori_intml_examples_amd.models import Conv2D, Dense, Flatten, MaxPooling2D, Sequential, load_model
from cori_intml_examples_amd.models import executor_ref as ER
from cori_intml_examples_amd.models.layers import reset_names
from cori_intml_examples_amd.ops import reference as R
from cori_intml_examples_amd.utils import set_random_seed

from helpers import clip_oracle as C
from helpers import reg_models as M
from helpers import reg_oracle as G
from test_dp import _torchrun

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L2_001 = 0.009999999776482582          # float32(0.01) as a Python float


# ------------------------------------------------------------------------------------ 1. the module
def test_constructors_and_float32_config():
    assert pkg.regularizers is regularizers
    assert regularizers.serialize(regularizers.l2(0.01)) == {"class_name": "L1L2", "config": {"l1": 0.0, "l2": L2_001}}
    assert regularizers.l1(0.01).get_config() == {"l1": L2_001, "l2": 0.0}
    assert regularizers.l1_l2().get_config() == {"l1": L2_001, "l2": L2_001}
    assert regularizers.l1().l1 == L2_001 and regularizers.l2().l2 == L2_001
    r = regularizers.L1L2(l1=0.5, l2=0.25)           # exact in float32
    assert (r.l1, r.l2) == (0.5, 0.25) and isinstance(r, regularizers.Regularizer)
    assert regularizers.L1L2().get_config() == {"l1": 0.0, "l2": 0.0}
    assert regularizers.serialize(None) is None and regularizers.serialize(regularizers.L1L2(0, 0)) is None


def test_get_and_deserialize():
    assert regularizers.get(None) is None
    r = regularizers.l1_l2(0.5, 0.25)
    assert regularizers.get(r) is r
    for name, cfg in (("l1", {"l1": L2_001, "l2": 0.0}), ("l2", {"l1": 0.0, "l2": L2_001}),
                      ("l1_l2", {"l1": L2_001, "l2": L2_001})):
        assert regularizers.get(name).get_config() == cfg
    ser = regularizers.serialize(r)
    for back in (regularizers.get(ser), regularizers.deserialize(ser), regularizers.L1L2.from_config(ser["config"])):
        assert back == r and back.get_config() == {"l1": 0.5, "l2": 0.25}
    assert regularizers.get({"class_name": "L1L2", "config": {"l2": 0.01}}).get_config() == {"l1": 0.0, "l2": L2_001}
    assert json.loads(json.dumps(ser)) == ser


@pytest.mark.parametrize("bad", [-1e-3, float("nan"), float("inf"), -float("inf"), 1e39, "x"])
def test_bad_coefficients_raise(bad):
    for mk in (lambda: regularizers.l1(bad), lambda: regularizers.l2(bad), lambda: regularizers.L1L2(l2=bad),
               lambda: regularizers.l1_l2(0.1, bad), lambda: regularizers.get({"class_name": "L1L2", "config": {"l1": bad}})):
        with pytest.raises(ValueError):
            mk()


def test_unknown_identifiers_raise():
    with pytest.raises(ValueError, match="Orthogonal"):
        regularizers.get({"class_name": "Orthogonal", "config": {}})
    with pytest.raises(ValueError, match="l3"):
        regularizers.get("l3")
    with pytest.raises(ValueError):
        regularizers.get(3.0)
    with pytest.raises(ValueError):
        regularizers.deserialize({"config": {}})
    with pytest.raises(ValueError, match="l3"):
        regularizers.get({"class_name": "L1L2", "config": {"l3": 1.0}})

    class Mine(regularizers.Regularizer):
        pass
    with pytest.raises(ValueError, match="Mine"):
        regularizers.get(Mine())


def test_compat_exposes_keras_regularizers():
    import sys
    from cori_intml_examples_amd import compat
    saved = {k: v for k, v in sys.modules.items() if k == "keras" or k.startswith("keras.")}
    try:
        compat.install(force=True, groups=("keras",))
        import keras
        from keras.regularizers import l2
        assert l2 is regularizers.l2 and keras.regularizers.l1_l2 is regularizers.l1_l2
        d = keras.layers.Dense(4, kernel_regularizer=l2(0.01))
        assert d.get_config()["kernel_regularizer"]["config"]["l2"] == L2_001
    finally:
        for k in [k for k in sys.modules if k == "keras" or k.startswith("keras.")]:
            del sys.modules[k]
        sys.modules.update(saved)


# ------------------------------------------------------------------------------------ 2. layers
VS = {"class_name": "VarianceScaling", "config": {"scale": 1.0, "mode": "fan_avg", "distribution": "uniform",
                                                  "seed": None}}


def test_default_layer_config_is_todays_literal():
    d = Dense(7, activation="relu", name="d")
    assert d.get_config() == {
        "name": "d", "trainable": True, "units": 7, "activation": "relu", "use_bias": True,
        "kernel_initializer": VS, "bias_initializer": {"class_name": "Zeros", "config": {}},
        "kernel_regularizer": None, "bias_regularizer": None, "activity_regularizer": None,
        "kernel_constraint": None, "bias_constraint": None}
    c = Conv2D(3, (3, 3), padding="same", name="c", input_shape=(8, 8, 1))
    assert c.get_config() == {
        "name": "c", "trainable": True, "batch_input_shape": [None, 8, 8, 1], "dtype": "float32", "filters": 3,
        "kernel_size": [3, 3], "strides": [1, 1], "padding": "same", "data_format": "channels_last",
        "dilation_rate": [1, 1], "activation": "linear", "use_bias": True, "kernel_initializer": VS,
        "bias_initializer": {"class_name": "Zeros", "config": {}}, "kernel_regularizer": None,
        "bias_regularizer": None, "activity_regularizer": None, "kernel_constraint": None, "bias_constraint": None}
    assert list(d.get_config()) == list(Dense(7, name="d", kernel_regularizer="l2").get_config())   # same key order
    assert d.kernel_regularizer is None and d.weight_regularizers() == {}
    # L1L2(0, 0) counts as no regularizer
    z = Dense(7, name="z", kernel_regularizer=regularizers.L1L2(0, 0), bias_regularizer=regularizers.l2(0.0))
    assert z.kernel_regularizer is None and z.get_config()["kernel_regularizer"] is None and z.weight_regularizers() == {}


@pytest.mark.parametrize("cls,args", [(Dense, (5,)), (Conv2D, (5, (3, 3)))])
def test_layer_config_round_trips_regularizers(cls, args):
    ser = {"class_name": "L1L2", "config": {"l1": 0.5, "l2": L2_001}}
    layer = cls(*args, name="x", kernel_regularizer=regularizers.l1_l2(0.5, 0.01), bias_regularizer="l2")
    cfg = layer.get_config()
    assert cfg["kernel_regularizer"] == ser and cfg["activity_regularizer"] is None
    assert cfg["bias_regularizer"] == {"class_name": "L1L2", "config": {"l1": 0.0, "l2": L2_001}}
    back = cls.from_config(json.loads(json.dumps(cfg)))
    assert back.get_config() == cfg and back.kernel_regularizer == layer.kernel_regularizer
    assert set(back.weight_regularizers()) == {"kernel", "bias"}
    assert set(cls(*args, use_bias=False, bias_regularizer="l2").weight_regularizers()) == set()
    plain = cls.from_config(cls(*args, name="p").get_config())     # None passes through
    assert plain.kernel_regularizer is None and plain.bias_regularizer is None
    with pytest.raises(ValueError):
        cls(*args, kernel_regularizer={"class_name": "Nope", "config": {}})


@pytest.mark.parametrize("cls,args", [(Dense, (5,)), (Conv2D, (5, (3, 3)))])
def test_activity_regularizer_raises(cls, args):
    with pytest.raises(NotImplementedError, match="my_layer"):
        cls(*args, name="my_layer", activity_regularizer=regularizers.l2(0.01))
    with pytest.raises(NotImplementedError, match="act"):
        cls.from_config(dict(cls(*args, name="act").get_config(), activity_regularizer={"class_name": "L1L2",
                                                                                         "config": {"l1": 0.1, "l2": 0.0}}))
    cls(*args, activity_regularizer=None)


def test_regularized_ranges_follow_the_store():
    m = M.tiny(optim.SGD(lr=0.1))
    ranges = m.regularized_ranges()
    specs = {(s.layer.name, s.short): s for s in m.store.specs}
    want = []
    for s in m.store.specs:
        if s.short == "kernel":
            want.append((s.offset, s.offset + s.numel, float(np.float32(M.L1)), float(np.float32(M.L2))))
        elif s.layer is m.layers[3]:                      # the second conv's bias
            want.append((s.offset, s.offset + s.numel, 0.0, float(np.float32(M.BIAS_L2))))
    assert ranges == want and len(ranges) == 6 and len(specs) == 10
    assert ranges == sorted(ranges) and all(a[1] <= b[0] for a, b in zip(ranges, ranges[1:]))
    assert M.tiny(optim.SGD(lr=0.1), reg=False).regularized_ranges() == []


# ------------------------------------------------------------------------------------ 3. the oracle
def test_oracle_is_pinned_by_autograd():
    rs = np.random.RandomState(4)
    w = rs.randn(300) * 10.0 ** rs.uniform(-3, 1, 300)
    w[[0, 17, 99, 100, 255]] = 0.0                       # exact zeros: sgn(0) = 0
    w[18] = -0.0
    ranges = [(0, 100, 0.25, 0.0), (100, 101, 0.0, 0.5), (120, 256, 1e-3, 3e-2)]
    t = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    p = sum(l1 * t[lo:hi].abs().sum() + l2 * (t[lo:hi] * t[lo:hi]).sum() for lo, hi, l1, l2 in ranges)
    p.backward()
    np.testing.assert_allclose(G.penalty(ranges, w), float(p.detach()), rtol=1e-14)
    np.testing.assert_allclose(G.grad_term(ranges, w), t.grad.numpy(), rtol=1e-14, atol=0)
    term = G.grad_term(ranges, w)
    assert np.all(term[[0, 17, 18, 99]] == 0.0) and np.all(term[101:120] == 0.0) and np.all(term[256:] == 0.0)
    g = rs.randn(300)
    np.testing.assert_array_equal(G.add_grad(ranges, w, g), g + term)
    assert G.batch_loss(0.5, ranges, w) == 0.5 + G.penalty(ranges, w)
    assert G.epoch_loss([(16, 1.0, 0.5), (8, 4.0, 0.25)]) == (16 * 1.5 + 8 * 4.25) / 24
    # the float32 form agrees with the float64 one to float32 rounding, and leaves the rest alone
    f = G.grad_f32(ranges, w, g)
    # (three roundings -- two products' sum and the final sum -- each at most 2^-24 of |g| + |term|)
    w32, g32 = w.astype(np.float32), g.astype(np.float32)
    assert np.all(np.abs(f - G.add_grad(ranges, w32, g32)) <= 2.0 ** -22 * (np.abs(g32) + np.abs(G.grad_term(ranges, w32))))
    np.testing.assert_array_equal(f[256:], g[256:].astype(np.float32))


def test_reference_ops_match_the_oracle():
    rs = np.random.RandomState(5)
    w = (rs.randn(500) * 10.0 ** rs.uniform(-3, 0, 500)).astype(np.float32)
    w[[3, 250]] = 0.0
    g = rs.randn(500).astype(np.float32)
    ranges = [(1, 130, float(np.float32(1e-3)), float(np.float32(0.01))), (130, 135, 0.0, 0.5), (301, 499, 0.25, 0.0)]
    pen = float(R.regularization_penalty(ranges, torch.tensor(w)))
    assert abs(pen - G.penalty(ranges, w)) <= 1e-5 * G.penalty(ranges, w)
    gt = torch.tensor(g.copy())
    R.add_regularization_grad(ranges, torch.tensor(w), gt)
    np.testing.assert_array_equal(gt.numpy(), G.grad_f32(ranges, w, g))       # the same fp32 operation order
    np.testing.assert_allclose(gt.numpy(), G.add_grad(ranges, w, g), rtol=1e-6, atol=1e-7)
    assert float(R.regularization_penalty([], torch.tensor(w))) == 0.0


# ------------------------------------------------------------------------------------ 4. CPU executor
@pytest.fixture
def unregularized(monkeypatch):
    """The data gradients the CPU executor hands to add_regularization_grad, before it adds the term."""
    rec = []
    orig = R.add_regularization_grad

    def spy(ranges, master, g):
        rec.append(g.detach().clone().double().numpy()[:max(hi for _, hi, _, _ in ranges) + 1])
        return orig(ranges, master, g)
    monkeypatch.setattr(ER.R, "add_regularization_grad", spy)
    return rec


OPTS = {"SGD": lambda **kw: optim.SGD(lr=0.05, **kw), "Adam": lambda **kw: optim.Adam(lr=0.01, **kw)}


def _twin_of(m):
    """The same model without regularizers, at m's current weights (its losses are L_data)."""
    t = M.tiny(optim.SGD(lr=0.0), reg=False)
    t.set_weights(m.get_weights())
    return t


@pytest.mark.parametrize("name", sorted(OPTS))
@pytest.mark.parametrize("steps", [1, 3])
def test_cpu_executor_matches_oracle(name, steps, unregularized):
    """train_on_batch steps of the tiny model with l1_l2 on every kernel and l2 on one bias: every
    reported loss is L_data + P of the pre-update weights, and the weights and slots follow the
    oracle's update of g_data + dP/dw.  Bound: the project's 2e-5 * max(1, 100 lr) on the weights,
    1e-5 relative on the losses (fp32 sums)."""
    set_random_seed(5)
    opt = OPTS[name]()
    m = M.tiny(opt)
    ranges = m.regularized_ranges()
    x, y, _ = synthetic_rpv(96, size=16, channels=3, seed=3)
    n = m.store.numel
    p = m.store.master[:n].double().numpy().copy()
    slots = [np.zeros(n) for _ in range(opt.n_slots)]
    bound = 2e-5 * max(1.0, 100 * float(opt.lr))
    for t in range(1, steps + 1):
        xb, yb = x[32 * (t - 1):32 * t], y[32 * (t - 1):32 * t]
        data_loss = _twin_of(m).test_on_batch(xb, yb)[0]
        pen = G.penalty(ranges, m.store.master[:n].double().numpy())
        assert pen > 0.05 * data_loss                    # the penalty is no rounding matter here
        loss, acc = m.train_on_batch(xb, yb)
        assert abs(loss - G.batch_loss(data_loss, ranges, p)) <= 1e-5 * loss, (t, loss, data_loss, pen)
        assert len(unregularized) == t
        p, slots, _ = C.step(opt.kind, p, G.add_grad(ranges, p, unregularized[-1]), slots, t, opt)
        errs = [float(np.abs(m.store.master[:n].double().numpy() - p).max())]
        errs += [float(np.abs(s.double().numpy() - r).max()) for s, r in zip(m._executor.optimizer_state(), slots)]
        print("%s step %d: loss %.6f = %.6f + %.6f, max |err| %s (bound %.3g)" % (name, t, loss, data_loss, pen, errs, bound))
        assert max(errs) < bound, (name, t, errs)
    # and the term mattered: the unregularized update from the same gradient is somewhere else
    plain, _, _ = C.step(opt.kind, m.store.master[:n].double().numpy(), unregularized[-1],
                         [np.zeros(n) for _ in range(opt.n_slots)], 1, opt)
    with_term, _, _ = C.step(opt.kind, m.store.master[:n].double().numpy(),
                             G.add_grad(ranges, m.store.master[:n].double().numpy(), unregularized[-1]),
                             [np.zeros(n) for _ in range(opt.n_slots)], 1, opt)
    assert np.abs(plain - with_term).max() > 3 * bound


def test_every_reported_loss_contains_the_penalty():
    """test_on_batch, evaluate (ragged last batch), fit's epoch loss and val_loss, and sample
    weights: the penalty joins every loss once per row, unweighted; acc is untouched."""
    set_random_seed(6)
    m = M.tiny(optim.SGD(lr=0.0))                        # lr = 0: the weights (and P) never move
    twin = _twin_of(m)
    x, y, _ = synthetic_rpv(40, size=16, channels=3, seed=8)
    pen = G.penalty(m.regularized_ranges(), m.store.master[:m.store.numel].double().numpy())
    tol = 1e-5
    a, b = m.test_on_batch(x[:16], y[:16]), twin.test_on_batch(x[:16], y[:16])
    assert abs(a[0] - (b[0] + pen)) <= tol * a[0] and a[1] == b[1]
    a, b = m.evaluate(x, y, batch_size=16, verbose=0), twin.evaluate(x, y, batch_size=16, verbose=0)   # 16 + 16 + 8
    assert abs(a[0] - (b[0] + pen)) <= tol * a[0] and a[1] == b[1]
    sw = np.linspace(0.0, 3.0, 16).astype(np.float32)
    a, b = m.test_on_batch(x[:16], y[:16], sample_weight=sw), twin.test_on_batch(x[:16], y[:16], sample_weight=sw)
    assert abs(a[0] - (b[0] + pen)) <= tol * a[0]        # ... not (weighted loss + weighted penalty)
    a, b = m.train_on_batch(x[:16], y[:16], sample_weight=sw), twin.train_on_batch(x[:16], y[:16], sample_weight=sw)
    assert abs(a[0] - (b[0] + pen)) <= tol * a[0] and a[1] == b[1]
    h = m.fit(x, y, batch_size=16, epochs=1, verbose=0, shuffle=False, validation_data=(x[:24], y[:24]))
    ht = twin.fit(x, y, batch_size=16, epochs=1, verbose=0, shuffle=False, validation_data=(x[:24], y[:24]))
    for key in ("loss", "val_loss"):
        assert abs(h.history[key][0] - (ht.history[key][0] + pen)) <= tol * h.history[key][0], key
    assert h.history["acc"] == ht.history["acc"] and h.history["val_acc"] == ht.history["val_acc"]


def test_val_loss_uses_the_weights_of_its_own_forward():
    set_random_seed(7)
    m = M.tiny(optim.SGD(lr=0.05))
    x, y, _ = synthetic_rpv(48, size=16, channels=3, seed=9)
    h = m.fit(x[:32], y[:32], batch_size=16, epochs=1, verbose=0, shuffle=False, validation_data=(x[32:], y[32:]))
    pen = G.penalty(m.regularized_ranges(), m.store.master[:m.store.numel].double().numpy())     # after the epoch
    want = _twin_of(m).evaluate(x[32:], y[32:], verbose=0)[0] + pen
    assert abs(h.history["val_loss"][0] - want) <= 1e-5 * want


def test_clipnorm_sees_the_regularized_gradient(unregularized, monkeypatch):
    seen = []
    orig = R.clip_gradients

    def spy(g, cn, cv):
        seen.append(g.detach().clone().double().numpy())
        return orig(g, cn, cv)
    monkeypatch.setattr(ER.R, "clip_gradients", spy)
    set_random_seed(5)
    c = 0.05
    opt = optim.SGD(lr=0.05, clipnorm=c)
    m = M.tiny(opt)
    ranges = m.regularized_ranges()
    x, y, _ = synthetic_rpv(32, size=16, channels=3, seed=3)
    n = m.store.numel
    p = m.store.master[:n].double().numpy().copy()
    m.train_on_batch(x, y)
    greg = G.add_grad(ranges, p, unregularized[0])
    np.testing.assert_allclose(seen[0], greg, rtol=1e-5, atol=1e-8)          # the clip's input: regularized
    want, _, info = C.step(opt.kind, p, greg, [], 1, opt, clipnorm=c)
    assert info["fired"] and info["norm"] > 2 * c
    assert abs(info["norm"] - C.global_norm(unregularized[0])) > 1e-3 * info["norm"]   # not the data gradient's norm
    assert float(np.abs(m.store.master[:n].double().numpy() - want).max()) < 2e-5 * max(1.0, 100 * 0.05)
    assert abs(C.global_norm(m.store.grad[:n].double().numpy()) - c) < 1e-6 * c


# ------------------------------------------------------------------------------------ 5. checkpoints
def _sequential(device="cpu"):
    m = Sequential(device=device)
    m.add(Conv2D(4, (3, 3), activation="relu", input_shape=(12, 12, 1), kernel_regularizer=regularizers.l2(0.01)))
    m.add(MaxPooling2D((2, 2)))
    m.add(Flatten())
    m.add(Dense(8, activation="relu", kernel_regularizer=regularizers.l1_l2(1e-4, 1e-3), bias_regularizer="l1"))
    m.add(Dense(3, activation="softmax"))
    m.compile(optimizer=optim.Adam(lr=0.01), loss="categorical_crossentropy", metrics=["accuracy"])
    return m


@pytest.mark.parametrize("kind", ["sequential", "functional"])
def test_hdf5_round_trip_keeps_the_regularizers(kind, tmp_path):
    set_random_seed(3)
    rs = np.random.RandomState(0)
    if kind == "sequential":
        m = _sequential()
        x = rs.rand(48, 12, 12, 1).astype(np.float32)
        y = np.eye(3, dtype=np.float32)[rs.randint(0, 3, 48)]
    else:
        m = M.tiny(optim.Adam(lr=0.01))
        x, y, _ = synthetic_rpv(48, size=16, channels=3, seed=1)
    m.fit(x[:32], y[:32], batch_size=16, epochs=1, verbose=0, shuffle=False)
    p = str(tmp_path / "m.h5")
    m.save(p)
    with H5File(p) as f:
        mc = json.loads(f.attrs("/")["model_config"])
    layers = mc["config"]["layers"] if isinstance(mc["config"], dict) else mc["config"]
    sers = [lc["config"].get("kernel_regularizer") for lc in layers if lc["class_name"] in ("Conv2D", "Dense")]
    assert sum(s is not None for s in sers) >= 2 and all(s is None or s["class_name"] == "L1L2" for s in sers)
    m2 = load_model(p)
    assert type(m2) is type(m)
    assert m2.regularized_ranges() == m.regularized_ranges() and len(m.regularized_ranges()) >= 3
    assert [l.get_config() for l in m2.layers] == [l.get_config() for l in m.layers]
    m2._executor.seed = m._executor.seed
    la, lb = m.train_on_batch(x[32:], y[32:]), m2.train_on_batch(x[32:], y[32:])
    assert la == lb                                   # the reloaded model's next step is bit-identical
    for a, b in zip(m.get_weights(), m2.get_weights()):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(m._executor.optimizer_state(), m2._executor.optimizer_state()):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------ 6. data parallel
def test_two_ranks_match_the_global_batch(tmp_path):
    """Each rank adds the term to its local gradient, then the gradients are averaged: the weights
    equal the single-process step at the global batch within the bound of the clipping two-rank
    test (1e-5), and every rank's loss is its own data loss plus P."""
    r = _torchrun(2, [os.path.join(ROOT, "tests", "reg_dp_worker.py"), str(tmp_path)])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    reps = [json.load(open(tmp_path / ("rank%d.json" % i))) for i in range(2)]
    print(json.dumps(reps, indent=1))
    assert reps[0]["w1_digest"] == reps[1]["w1_digest"]
    assert reps[0]["data_loss"] != reps[1]["data_loss"]
    for rep in reps:
        assert rep["size"] == 2 and rep["w0_equal"] and rep["ranges"] == 6 and rep["buckets"] == 1, rep
        assert rep["err_vs_single"] < 1e-5 and rep["moved"] > 1e-3, rep
        assert rep["diff_vs_unregularized"] > 1e-4, rep
        assert rep["penalty"] > 0.01 and abs(rep["loss"] - (rep["data_loss"] + rep["penalty"])) <= 1e-5 * rep["loss"], rep


# ------------------------------------------------------------------------------------ 7. builders and CLIs
def _regs(m):
    return [(l.get_config()["kernel_regularizer"], l.get_config()["bias_regularizer"])
            for l in m.layers if isinstance(l, (Conv2D, Dense))]


def test_builders_take_l2():
    ser = {"class_name": "L1L2", "config": {"l1": 0.0, "l2": L2_001}}
    for build in (lambda **kw: zoo.rpv_cnn((16, 16, 1), conv_sizes=[4, 8], fc_sizes=[8], device="cpu", **kw),
                  lambda **kw: rpv_app.build_model((16, 16, 1), conv_sizes=[4, 8], fc_sizes=[8], device="cpu", **kw),
                  lambda **kw: zoo.mnist_cnn(device="cpu", **kw), lambda **kw: mnist_app.build_model(device="cpu", **kw)):
        m = build(l2=0.01)
        assert _regs(m) == [(ser, None)] * len(_regs(m)) and len(_regs(m)) == 4
        assert len(m.regularized_ranges()) == 4 and all(r[2] == 0.0 and r[3] == L2_001 for r in m.regularized_ranges())
        for plain in (build(), build(l2=0.0)):         # 0.0 builds exactly today's model
            assert _regs(plain) == [(None, None)] * 4 and plain.regularized_ranges() == []
        reset_names()
        a = [l.get_config() for l in build().layers]
        reset_names()
        b = [l.get_config() for l in build(l2=0.0).layers]
        assert a == b
    import inspect
    assert list(inspect.signature(zoo.rpv_cnn).parameters)[-1] == "l2"
    assert list(inspect.signature(zoo.mnist_cnn).parameters)[-1] == "l2"
    assert list(inspect.signature(rpv_app.build_model).parameters)[:6] == ["input_shape", "conv_sizes", "fc_sizes",
                                                                         "dropout", "optimizer", "lr"]
    assert list(inspect.signature(mnist_app.build_model).parameters)[:5] == ["h1", "h2", "h3", "dropout", "optimizer"]


class _Built(Exception):
    pass


@pytest.mark.parametrize("cli", ["rpv", "mnist"])
@pytest.mark.parametrize("l2", [None, "0", "0.01"])
def test_cli_l2(cli, l2, monkeypatch):
    """--l2 reaches the model the CLI builds; --l2 0 (and no --l2) builds the unregularized one.
    The run is stopped once the model exists."""
    from cori_intml_examples_amd.parallel import hvd
    monkeypatch.setenv("INTML_DEVICE", "cpu")
    got = {}
    mod, attr = (rpv_app, "build_model") if cli == "rpv" else (zoo, "mnist_cnn")
    orig = getattr(mod, attr)

    def capture(*a, **kw):
        got["model"] = orig(*a, **kw)
        raise _Built()
    monkeypatch.setattr(mod, attr, capture)
    argv = ["--l2", l2] if l2 is not None else []
    if cli == "rpv":
        argv += ["--synthetic", "--n-train", "32", "--n-valid", "16", "--h1", "4", "--h2", "4", "--h3", "4", "--h4", "8"]
        assert train_rpv.build_parser().parse_args(argv).l2 == float(l2 or 0)
    else:
        argv += ["--n-train", "32", "--h1", "2", "--h2", "2", "--h3", "4"]
        assert train_mnist.build_parser().parse_args(argv).l2 == float(l2 or 0)
    try:
        with pytest.raises(_Built):
            (train_rpv if cli == "rpv" else train_mnist).main(argv)
    finally:
        hvd.shutdown()
    want = {"class_name": "L1L2", "config": {"l1": 0.0, "l2": L2_001}} if l2 == "0.01" else None
    assert _regs(got["model"]) == [(want, None)] * (5 if cli == "rpv" else 4)
    assert bool(got["model"].regularized_ranges()) == (want is not None)
