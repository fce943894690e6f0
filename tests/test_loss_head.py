"""The loss table and the multi-label sigmoid head on the CPU: the float64 oracle
(tests/helpers/loss_oracle.py) against autograd and at exact ties, the proof that the oracle's
derived bounds hold for a float32 evaluation (ops/reference.py) on every input set of the GPU
kernel test and flag localised mutations, the plan's names / pairs / messages, the CPU executor
against an independently written autograd model, HDF5, compat names, builders and CLIs."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cori_intml_examples_amd import losses, optim
from cori_intml_examples_amd.io.keras_h5 import load_model
from cori_intml_examples_amd.models import Dense, Input, Model, Sequential
from cori_intml_examples_amd.models.plan import LOSS_ALIASES, binary_accuracy_head, canonical_loss, classic_head
from cori_intml_examples_amd.ops import reference as R
from cori_intml_examples_amd.utils import set_random_seed

from helpers import loss_models as LM
from helpers import loss_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINK_CAP = 0.01            # the share of elements a case may leave to the kink allowance


# ----------------------------------------------------------------------------- 1. oracle vs autograd
def _torch_loss(act, loss, z, y):
    """The table's formulas written directly in torch float64 (autograd gives d loss / d z)."""
    eps = torch.tensor(O.EPS, dtype=torch.float64)
    p = torch.softmax(z, -1) if act == "softmax" else torch.sigmoid(z) if act == "sigmoid" else z
    if loss == "binary_crossentropy":
        pc = p.clamp(O.H.LO, O.H.HI)
        lg = torch.log(pc / (1 - pc))
        return (lg.clamp(min=0) - lg * y + torch.log1p(torch.exp(-lg.abs()))).mean(-1)
    if loss == "mse":
        return ((p - y) ** 2).mean(-1)
    if loss == "mae":
        return (p - y).abs().mean(-1)
    if loss == "msle":
        return ((torch.log(torch.maximum(p, eps) + 1) - torch.log(torch.maximum(y, eps) + 1)) ** 2).mean(-1)
    if loss == "logcosh":
        x = p - y
        return (x.abs() + torch.log1p(torch.exp(-2 * x.abs())) - np.log(2.0)).mean(-1)
    if loss == "hinge":
        return torch.clamp(1 - y * p, min=0).mean(-1)
    if loss == "squared_hinge":
        return (torch.clamp(1 - y * p, min=0) ** 2).mean(-1)
    if loss == "categorical_hinge":
        return torch.clamp(((1 - y) * p).max(-1).values - (y * p).sum(-1) + 1, min=0)
    if loss == "kld":
        yc, pc = y.clamp(O.EPS, 1.0), p.clamp(O.EPS, 1.0)
        return (yc * torch.log(yc / pc)).sum(-1)
    if loss == "poisson":
        return (p - y * torch.log(p + eps)).mean(-1)
    raise KeyError(loss)


# (the one-column sigmoid + binary_crossentropy pair is the first head kernel's: tests/test_head_edges.py)
@pytest.mark.parametrize("act,loss,N", [(a, l, N) for a, l in O.PAIRS for N in (1, 3, 16)
                                        if (l, N) != ("binary_crossentropy", 1)])
def test_oracle_gradient_is_autograd(act, loss, N):
    """Away from kinks (continuous draws; a row near one is left out and must be rare) the oracle's
    dz is float64 autograd of its loss through the activation, and its loss is the formula."""
    Zs, y = O.draw(loss, act, 40, N, seed=5)
    ev = O.evaluate(act, loss, Zs, y)
    z = torch.tensor(Zs, requires_grad=True)
    l = _torch_loss(act, loss, z, torch.tensor(y, dtype=torch.float64))
    l.sum().backward()
    np.testing.assert_allclose(ev.loss, l.detach().numpy(), rtol=1e-12, atol=1e-13)
    near = O.bounds(ev, 1e-9).near_kink.any(1)
    assert near.mean() <= 0.05
    np.testing.assert_allclose(ev.dz[~near], z.grad.numpy()[~near], rtol=1e-9, atol=1e-12)
    # losses.py evaluates the same formulas on the output
    np.testing.assert_allclose(getattr(losses, loss)(y, ev.probs), ev.loss, rtol=2e-6, atol=1e-7)


# ----------------------------------------------------------------------------- 2. exact ties
@pytest.mark.parametrize("case", O.tie_cases(), ids=lambda c: c[1])
def test_subgradient_conventions_at_exact_ties(case):
    name, loss, z, y, want = case
    ev = O.evaluate(None, loss, z, y)
    np.testing.assert_allclose(ev.dz, np.asarray(want), rtol=1e-12, atol=0, err_msg=name)
    l, dz, _ = R.table_loss(None, loss, torch.tensor(z, dtype=torch.float32), torch.tensor(y, dtype=torch.float32))
    np.testing.assert_allclose(dz.double().numpy(), np.asarray(want), rtol=1e-6, atol=0, err_msg=name + " (ops/reference.py)")


def test_accuracy_rule_and_first_maximum():
    # rint is round-half-even: p = 0.5 is 0, p = 1.5 is 2; binary accuracy counts ELEMENTS
    ev = O.evaluate(None, "mse", [[0.5], [1.5], [0.49]], [[0.0], [2.0], [1.0]])
    assert ev.binary and ev.correct.tolist() == [1.0, 1.0, 0.0]
    ev = O.evaluate("sigmoid", "binary_crossentropy", [[3.0, -3.0, 3.0]], [[1.0, 0.0, 0.0]])
    assert ev.binary and ev.correct.tolist() == [2.0]
    # categorical: first argmax of p against first argmax of y, ties included
    ev = O.evaluate(None, "mae", [[0.2, 0.2, 0.1], [0.1, 0.3, 0.3]], [[0.5, 0.5, 0.0], [0.0, 0.0, 1.0]])
    assert not ev.binary and ev.correct.tolist() == [1.0, 0.0]
    _, _, c = R.table_loss(None, "mae", torch.tensor([[0.2, 0.2, 0.1], [0.1, 0.3, 0.3]]), torch.tensor([[0.5, 0.5, 0.0], [0.0, 0.0, 1.0]]))
    assert c.tolist() == [1.0, 0.0]
    assert binary_accuracy_head("hinge", 1) and binary_accuracy_head("binary_crossentropy", 5) and not binary_accuracy_head("hinge", 2)


# ----------------------------------------------------------------------------- 3. the proof of the checker
def _ref32(act, loss, a, W, b, y, mutate=None):
    """ops/reference.py in float32 on the head's input (logits by a float32 matmul)."""
    z = torch.tensor(a, dtype=torch.float32) @ torch.tensor(np.asarray(W, np.float32)) + torch.tensor(np.asarray(b, np.float32))
    y = torch.tensor(np.asarray(y, np.float32))
    if mutate is not None:
        l, dz, c = mutate(act, loss, z, y)
    elif loss == "binary_crossentropy":
        l, dz, c = R.sigmoid_bce(z, y)
    else:
        l, dz, c = R.table_loss(act, loss, z, y)
    d = lambda t: t.double().numpy()
    return d(l), d(dz), d(c), d(R.head_probs(act, z))


def _check(act, loss, a, W, b, y, got, exact=False):
    """[names of the quantities outside the oracle's bounds], the near-kink share, the oracle."""
    z = a @ np.asarray(W, np.float64) + np.asarray(b, np.float64)
    ev = O.evaluate(act, loss, z, y)
    bd = O.bounds(ev, 0.0 if exact else O.logit_error_bound(a, W, b))
    l, dz, c, p = got
    bad = []
    if not (np.abs(l - ev.loss) <= bd.loss + 1e-300).all():
        bad.append("loss")
    tol = bd.dz + (0.0 if exact else bd.dz_jump)
    if not (np.abs(dz - ev.dz) <= tol + 1e-300).all():
        bad.append("dz")
    if not (np.abs(c - ev.correct) <= (0 if exact else bd.acc_ambiguous)).all():
        bad.append("correct")
    if not (np.abs(p - ev.probs) <= bd.dp + 2 * O.U * np.abs(ev.probs)).all():
        bad.append("probs")
    return bad, float(bd.near_kink.mean()), ev


def _problem(act, loss, M, N, K, seed=0):
    a = O.synthetic_input(M, K, seed)
    Zs, y = O.draw(loss, act, M, N, seed)
    b = (0.5 * np.random.RandomState(11).randn(N)).astype(np.float32)
    return a, O.place(a, Zs, b), b, y


@pytest.mark.parametrize("case", O.kernel_cases(), ids=lambda c: "%s-%s-M%d-N%d-K%d-%s" % c)
def test_float32_reference_stays_inside_the_derived_bounds(case):
    act, loss, M, N, K, arch = case
    a, W, b, y = _problem(act, loss, M, N, K)
    bad, share, ev = _check(act, loss, a, W, b, y, _ref32(act, loss, a, W, b, y))
    assert not bad, (case, bad)
    assert share <= KINK_CAP, (case, share)
    assert np.isfinite(ev.loss).all() and np.isfinite(ev.dz).all()


def test_case_list_covers_what_it_must():
    cases = O.kernel_cases()
    assert {(c[0], c[1]) for c in cases} == set(O.KERNEL_PAIRS)
    for loss in O.LOSSES:
        assert {c[3] for c in cases if c[1] == loss and c[0] == O.NATURAL[loss]} == set(O.NS)
    assert {c[3] for c in cases if c[1] == "binary_crossentropy"} == set(O.NS) - {1}
    assert {c[2] for c in cases} == set(O.MS) and {c[4] for c in cases if c[5] == "dense"} == set(O.KS)
    assert {c[5] for c in cases} == {"dense", "conv"}
    kn = {c[4] * c[3] for c in cases}
    assert 1950 in kn and 2080 in kn            # both sides of HEAD_W_LDS = 2048


# localised mutations of the float32 evaluation: each must be flagged on some input set
def _mut_drop_1_over_n(act, loss, z, y):
    l, dz, c = R.table_loss(act, loss, z, y)
    return l, dz * z.shape[-1], c


def _mut_no_sigmoid_slope(act, loss, z, y):
    p = torch.sigmoid(z)
    l, g = R.TABLE_LOSSES[loss](p, y)
    return l, g, R.table_loss(act, loss, z, y)[2]


def _mut_no_softmax_sum(act, loss, z, y):
    p = torch.softmax(z, -1)
    l, g = R.TABLE_LOSSES[loss](p, y)
    return l, p * g, R.table_loss(act, loss, z, y)[2]


def _mut_no_clip_mask(act, loss, z, y):
    l, dz, c = R.table_loss(act, loss, z, y)
    yc, pc = y.clamp(R.EPS, 1.0), z.clamp(R.EPS, 1.0)
    return l, -yc / pc, c


def _mut_hinge_strict(act, loss, z, y):
    l, dz, c = R.table_loss(act, loss, z, y)
    return l, torch.where(1 - y * z > 0, -y, torch.zeros_like(z)) / z.shape[-1], c


def _mut_last_maximum(act, loss, z, y):
    l, dz, c = R.table_loss(act, loss, z, y)
    negs = (1 - y) * z
    last = z.shape[-1] - 1 - torch.flip(negs, [-1]).argmax(-1)
    g = -y + torch.nn.functional.one_hot(last, z.shape[-1]).to(z.dtype) * (1 - y)
    return l, torch.where((l > 0).unsqueeze(-1), g, torch.zeros_like(z)), c


def _mut_bce_flattened(act, loss, z, y):
    # what the executors did before: column 0 only
    l, dz, c = R.sigmoid_bce(z[:, 0], y[:, 0])
    out = torch.zeros_like(z)
    out[:, 0] = dz
    return l, out, c


MUTATIONS = [("a dropped 1/N", _mut_drop_1_over_n, (None, "mae", 26, 15, 130)),
             ("p (1 - p) left out", _mut_no_sigmoid_slope, ("sigmoid", "poisson", 5, 3, 64)),
             ("the softmax Jacobian's sum left out", _mut_no_softmax_sum, ("softmax", "kld", 5, 3, 64)),
             ("a missing clip mask", _mut_no_clip_mask, (None, "kld", 26, 3, 65)),
             ("multi-label BCE trains column 0 only", _mut_bce_flattened, ("sigmoid", "binary_crossentropy", 5, 3, 64))]
TIE_MUTATIONS = [("'>' in place of '>=' in hinge", _mut_hinge_strict, "hinge"),
                 ("the last maximum in place of the first", _mut_last_maximum, "categorical_hinge")]


@pytest.mark.parametrize("name,mut,case", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_mutations_are_flagged(name, mut, case):
    act, loss, M, N, K = case
    a, W, b, y = _problem(act, loss, M, N, K)
    assert not _check(act, loss, a, W, b, y, _ref32(act, loss, a, W, b, y))[0]
    bad = _check(act, loss, a, W, b, y, _ref32(act, loss, a, W, b, y, mutate=mut))[0]
    assert "dz" in bad, (name, bad)


@pytest.mark.parametrize("name,mut,loss", TIE_MUTATIONS, ids=[m[0] for m in TIE_MUTATIONS])
def test_tie_mutations_are_flagged(name, mut, loss):
    """The conventions only differ at exact ties: the tie inputs (exact logits: zero weights, the
    bias is the logit) are compared without the kink allowance."""
    _, _, z, y, _ = [c for c in O.tie_cases() if c[1] == loss][0]
    z, y = np.asarray(z), np.asarray(y)
    a, W = np.ones((1, 4)), np.zeros((4, z.shape[1]), np.float32)
    assert not _check(None, loss, a, W, z[0], y, _ref32(None, loss, a, W, z[0], y), exact=True)[0]
    assert "dz" in _check(None, loss, a, W, z[0], y, _ref32(None, loss, a, W, z[0], y, mutate=mut), exact=True)[0]


# ----------------------------------------------------------------------------- 4. names and pairs
def test_canonical_loss_names_and_aliases():
    want = {"mean_absolute_error": "mae", "MAE": "mae", "mae": "mae", "mean_squared_logarithmic_error": "msle",
            "MSLE": "msle", "msle": "msle", "logcosh": "logcosh", "hinge": "hinge", "squared_hinge": "squared_hinge",
            "categorical_hinge": "categorical_hinge", "kullback_leibler_divergence": "kld", "KLD": "kld", "kld": "kld",
            "poisson": "poisson", "MSE": "mse", "mse": "mse", "mean_squared_error": "mse",
            "binary_crossentropy": "binary_crossentropy", "categorical_crossentropy": "categorical_crossentropy",
            "sparse_categorical_crossentropy": "sparse_categorical_crossentropy"}
    assert LOSS_ALIASES == want
    for k, v in want.items():
        assert canonical_loss(k) == v
        assert canonical_loss(getattr(losses, k)) == v        # the callables of losses.py by __name__
    for bad in ("cosine_proximity", "mape", "mean_absolute_percentage_error"):
        with pytest.raises(NotImplementedError, match="loss %r is not implemented" % bad):
            canonical_loss(bad)


def _dense_model(act, loss, N, device="cpu", opt="Adam", hidden=12):
    m = Sequential([Dense(hidden, activation="relu", input_shape=(7,)), Dense(N, activation=act)], device=device)
    m.compile(optimizer=opt, loss=loss, metrics=["accuracy"])
    return m


def test_allowed_and_refused_pairs():
    for act, loss in O.PAIRS:
        for N in (1, 3):
            hd = _dense_model(act, loss, N)._plan.head
            assert (hd.activation, hd.loss, hd.N) == (act, loss, N)
            assert classic_head(act, loss, N) == ((act, loss, N) == ("sigmoid", "binary_crossentropy", 1) or (act, loss) == (None, "mse"))
    assert classic_head("softmax", "categorical_crossentropy", 10) and classic_head("softmax", "sparse_categorical_crossentropy", 2)
    with pytest.raises(NotImplementedError, match="softmax output with loss binary_crossentropy"):
        _dense_model("softmax", "binary_crossentropy", 3)
    for loss in ("categorical_crossentropy", "sparse_categorical_crossentropy"):
        with pytest.raises(NotImplementedError, match="sigmoid output with loss " + loss):
            _dense_model("sigmoid", loss, 3)


# ----------------------------------------------------------------------------- 5. the CPU executor
def _autograd_step(m, x, y, loss, w=None):
    """Loss, accuracy and all gradients of one batch by an independently written float32 autograd
    model of a Dense(relu) -> Dense(act) network."""
    ws = [torch.tensor(v, requires_grad=True) for v in m.get_weights()]
    h = torch.relu(torch.tensor(x) @ ws[0] + ws[1])
    z = h @ ws[2] + ws[3]
    act = m._plan.head.activation
    yt = torch.tensor(y)
    rows = _torch_loss(act, loss, z.double(), yt.double()).float()
    if w is not None:
        wt = torch.tensor(w)
        batch = (rows * wt).sum() / max(int((wt != 0).sum()), 1)
    else:
        batch = rows.mean()
    batch.backward()
    p = torch.softmax(z, -1) if act == "softmax" else torch.sigmoid(z) if act == "sigmoid" else z
    if y.shape[1] == 1 or loss == "binary_crossentropy":
        acc = float((torch.round(p) == yt).double().mean())
    else:
        acc = float((p.argmax(-1) == yt.argmax(-1)).double().mean())
    return float(batch.detach()), acc, [t.grad.numpy() for t in ws], p.detach().numpy()


CPU_MODELS = [("sigmoid", "binary_crossentropy", 3)] + [(O.NATURAL[l], l, 1 if l in ("hinge", "mae") else 3) for l in O.LOSSES
                                                          if l != "mse"] + [("sigmoid", "mse", 3), ("softmax", "mse", 3)]


@pytest.mark.parametrize("act,loss,N", CPU_MODELS, ids=["%s-%s-%d" % c for c in CPU_MODELS])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_cpu_executor_against_autograd(act, loss, N, weighted):
    """7 -> 12 -> N at batch 6 (the shape at which Dense(3, sigmoid) + binary_crossentropy used to
    die in _backward): loss, accuracy over elements, every gradient, evaluate / predict."""
    set_random_seed(3)
    m = _dense_model(act, loss, N, opt=optim.SGD(lr=0.0))
    rs = np.random.RandomState(4)
    x = rs.rand(6, 7).astype(np.float32)
    y = LM.data(m, 6, loss, seed=9)[1]
    w = np.array([0.5, 0.0, 2.0, 1.0, 3.0, 0.0], np.float32) if weighted else None
    want_l, want_acc, want_g, want_p = _autograd_step(m, x, y, loss, w)
    got = m.train_on_batch(x, y, sample_weight=w)
    assert abs(got[0] - want_l) <= 1e-5 * max(1.0, abs(want_l)) and abs(got[1] - want_acc) < 1e-9, (got, want_l, want_acc)
    st = m.store
    for layer, gi in ((m.layers[-2], 0), (m.layers[-1], 2)):
        np.testing.assert_allclose(st.view(layer, "kernel", grad=True).numpy(), want_g[gi], rtol=2e-4, atol=2e-6)
        np.testing.assert_allclose(st.view(layer, "bias", grad=True).numpy(), want_g[gi + 1], rtol=2e-4, atol=2e-6)
    ev = m.evaluate(x, y, batch_size=4, verbose=0, sample_weight=w)
    assert len(ev) == 2 and abs(ev[1] - want_acc) < 1e-9
    if not weighted:
        assert abs(ev[0] - want_l) <= 1e-5 * max(1.0, abs(want_l))
    p = m.predict(x, batch_size=4)
    assert p.shape == (6, N)
    np.testing.assert_allclose(p, want_p, rtol=1e-5, atol=1e-6)


def test_multilabel_head_trains_every_column():
    set_random_seed(5)
    m = _dense_model("sigmoid", "binary_crossentropy", 3, opt=optim.Adam(lr=0.05))
    rs = np.random.RandomState(0)
    x = rs.rand(64, 7).astype(np.float32)
    y = np.stack([x[:, 0] > 0.5, x[:, 1] > 0.5, x[:, 2] + x[:, 3] > 1.0], 1).astype(np.float32)
    w0 = m.get_weights()[-2].copy()
    h = m.fit(x, y, batch_size=6, epochs=30, verbose=0, validation_data=(x, y))
    assert (np.abs(m.get_weights()[-2] - w0).max(0) > 1e-2).all()          # every column moved
    assert h.history["loss"][-1] < 0.8 * h.history["loss"][0] and h.history["val_acc"][-1] > 0.7
    assert abs(h.history["val_acc"][-1] - ((m.predict(x) > 0.5) == (y > 0.5)).mean()) < 1e-6


# ----------------------------------------------------------------------------- 6. HDF5, compat, builders, CLIs
@pytest.mark.parametrize("loss", ["hinge", losses.mean_absolute_error, losses.KLD])
def test_hdf5_round_trip_keeps_the_loss(loss, tmp_path):
    set_random_seed(6)
    m = _dense_model(None, loss, 3)
    x, y = np.random.RandomState(1).rand(12, 7).astype(np.float32), np.random.RandomState(2).rand(12, 3).astype(np.float32)
    m.fit(x, y, batch_size=6, epochs=1, verbose=0)
    p = str(tmp_path / "m.h5")
    m.save(p)
    c = load_model(p, device="cpu")
    assert c._plan.head.loss == canonical_loss(loss) and isinstance(c.loss, str)
    np.testing.assert_array_equal(c.predict(x), m.predict(x))
    assert c.evaluate(x, y, verbose=0) == m.evaluate(x, y, verbose=0)


def test_compat_keras_names():
    code = r'''
import cori_intml_examples_amd.compat as c
c.install()
import numpy as np
import keras
from keras import losses
from keras.models import Sequential
from keras.layers import Dense
for name in ("mean_absolute_error", "mae", "MAE", "mean_squared_logarithmic_error", "msle", "logcosh", "hinge",
             "squared_hinge", "categorical_hinge", "kullback_leibler_divergence", "kld", "KLD", "poisson", "MSE"):
    assert callable(getattr(keras.losses, name)), name
m = Sequential([Dense(5, activation="relu", input_shape=(4,)), Dense(3, activation="sigmoid")])
m.compile(optimizer="Adam", loss=losses.binary_crossentropy, metrics=["accuracy"])
x = np.random.RandomState(0).rand(12, 4).astype("float32")
y = (np.random.RandomState(1).rand(12, 3) > 0.5).astype("float32")
h = m.fit(x, y, batch_size=6, epochs=1, verbose=0)
m2 = Sequential([Dense(5, activation="relu", input_shape=(4,)), Dense(3)])
m2.compile(optimizer="Adam", loss=losses.squared_hinge, metrics=["accuracy"])
h2 = m2.fit(x, 2 * y - 1, batch_size=6, epochs=1, verbose=0)
print("ok", sorted(h.history), sorted(h2.history), float(losses.hinge(2 * y - 1, m2.predict(x)).mean()) > 0)
'''
    env = dict(os.environ, INTML_DEVICE="cpu", OMP_NUM_THREADS="2", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ok ['acc', 'loss'] ['acc', 'loss'] True" in r.stdout


def test_builders_take_a_loss():
    from cori_intml_examples_amd.apps import mnist, rpv, zoo
    set_random_seed(7)
    kw = dict(conv_sizes=[2, 2], fc_sizes=[4], device="cpu")
    assert zoo.rpv_cnn((8, 8, 1), **kw)._plan.head.loss == "binary_crossentropy"
    assert zoo.rpv_cnn((8, 8, 1), loss=None, **kw)._plan.head.loss == "binary_crossentropy"
    assert zoo.rpv_cnn((8, 8, 1), loss="hinge", **kw)._plan.head.loss == "hinge"
    assert rpv.build_model((8, 8, 1), loss="mean_absolute_error", **kw)._plan.head.loss == "mae"
    assert zoo.mnist_cnn(2, 2, 4, input_shape=(8, 8, 1), device="cpu", loss="kld")._plan.head.loss == "kld"
    assert zoo.mnist_cnn(2, 2, 4, input_shape=(8, 8, 1), device="cpu")._plan.head.loss == "categorical_crossentropy"
    assert mnist.build_model(2, 2, 4, device="cpu", loss="categorical_hinge")._plan.head.loss == "categorical_hinge"
    assert zoo.rpv_legacy_cnn((8, 8, 1), h1=2, h2=2, h3=2, h4=2, h5=4, device="cpu", loss="logcosh")._plan.head.loss == "logcosh"
    assert zoo.rpv_cnn((8, 8, 1), loss="binary_crossentropy", outputs=8, **kw)._plan.head.N == 8
    assert '"--loss"' in open(os.path.join(ROOT, "benchmarks", "optimizer_step.py")).read()


class _Built(Exception):
    pass


@pytest.mark.parametrize("cli,loss,want", [("rpv", "hinge", "hinge"), ("rpv", None, "binary_crossentropy"),
                                           ("mnist", "kullback_leibler_divergence", "kld"),
                                           ("mnist", None, "categorical_crossentropy")])
def test_cli_loss_argument(cli, loss, want, monkeypatch):
    """--loss reaches the compiled model: the CLI's own main() runs up to the built model."""
    from cori_intml_examples_amd.apps import rpv as rpv_app
    from cori_intml_examples_amd.apps import train_mnist, train_rpv, zoo
    from cori_intml_examples_amd.parallel import hvd
    monkeypatch.setenv("INTML_DEVICE", "cpu")
    got = {}
    mod, attr = (rpv_app, "build_model") if cli == "rpv" else (zoo, "mnist_cnn")
    orig = getattr(mod, attr)

    def capture(*a, **kw):
        got["model"] = orig(*a, **kw)
        raise _Built()
    monkeypatch.setattr(mod, attr, capture)
    argv = ["--loss", loss] if loss else []
    if cli == "rpv":
        argv += ["--synthetic", "--n-train", "32", "--n-valid", "16", "--h1", "4", "--h2", "4", "--h3", "4", "--h4", "8"]
        ns = train_rpv.build_parser().parse_args(argv)
    else:
        argv += ["--n-train", "32", "--h1", "2", "--h2", "2", "--h3", "4"]
        ns = train_mnist.build_parser().parse_args(argv)
    assert ns.loss == loss
    try:
        with pytest.raises(_Built):
            (train_rpv if cli == "rpv" else train_mnist).main(argv)
    finally:
        hvd.shutdown()
    assert got["model"]._plan.head.loss == want
