"""ROC / AUC, purity, efficiency and weighted metrics on the CPU: the public interface (compile names,
return values, History keys, callbacks, the CLIs' FoM), the rejected combinations, the key function,
the numpy twin against the float64 oracle, the reference executor against metrics.roc_curve on its
own predict output, and checkpoints."""
import math
import os

import numpy as np
import pytest

from cori_intml_examples_amd import metrics as MT
from cori_intml_examples_amd import optim
from cori_intml_examples_amd.apps import train_rpv
from cori_intml_examples_amd.apps.rpv import classification_report
from cori_intml_examples_amd.io.keras_h5 import load_model
from cori_intml_examples_amd.models import Conv2D, Dense, Dropout, Flatten, MaxPooling2D, Sequential
from cori_intml_examples_amd.parallel import hvd
from cori_intml_examples_amd.train.callbacks import Callback, EarlyStopping, ModelCheckpoint, ReduceLROnPlateau
from cori_intml_examples_amd.utils import set_random_seed

from helpers import roc_oracle as O

H = MT.ROC_H
F32 = np.float32


def _model(n_out=1, metrics=None, weighted_metrics=None, seed=11, head=None, loss=None):
    set_random_seed(seed)
    m = Sequential(device="cpu")
    m.add(Conv2D(4, (3, 3), activation="relu", input_shape=(8, 8, 1)))
    m.add(MaxPooling2D((2, 2)))
    m.add(Dropout(0.2))
    m.add(Flatten())
    m.add(Dense(8, activation="relu"))
    act = head if head is not None else ("sigmoid" if n_out == 1 else "softmax")
    m.add(Dense(n_out, activation=None if act == "linear" else act))
    loss = loss or {"sigmoid": "binary_crossentropy", "softmax": "categorical_crossentropy", "linear": "mse"}[act]
    m.compile(optimizer=optim.Adam(lr=0.01), loss=loss, metrics=metrics, weighted_metrics=weighted_metrics)
    return m


def _data(n, n_out=1, seed=0):
    rs = np.random.RandomState(seed)
    x = rs.rand(n, 8, 8, 1).astype(F32)
    y = (rs.rand(n) > 0.5).astype(F32) if n_out == 1 else np.eye(n_out, dtype=F32)[rs.randint(0, n_out, n)]
    w = rs.uniform(0.1, 4.0, n).astype(F32)
    w[::7] = 0.0
    return x, y, w


def _same(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


# ------------------------------------------------------------------------------------ interface
def test_compile_names_and_return_values():
    m = _model(metrics=["accuracy", "auc"], weighted_metrics=["acc", "auc", "precision", "recall"])
    assert m.metrics_names == ["loss", "acc", "auc", "weighted_acc", "weighted_auc", "weighted_purity",
                               "weighted_efficiency"]
    assert _model(metrics=["efficiency", "purity", "acc"]).metrics_names == ["loss", "efficiency", "purity", "acc"]
    assert _model(metrics=["accuracy"]).metrics_names == ["loss", "acc"]
    assert _model().metrics_names == ["loss"]
    x, y, w = _data(20)
    ev = m.evaluate(x, y, batch_size=6, verbose=0, sample_weight=w)
    assert len(ev) == 7 and all(isinstance(v, float) for v in ev)
    assert len(m.test_on_batch(x, y, sample_weight=w)) == 7 and len(m.train_on_batch(x, y, sample_weight=w)) == 7
    # without weights the weighted set equals its unweighted twin
    ev = dict(zip(m.metrics_names, m.evaluate(x, y, batch_size=6, verbose=0)))
    assert ev["weighted_acc"] == ev["acc"] and _same(ev["weighted_auc"], ev["auc"])
    assert isinstance(_model().evaluate(x, y, verbose=0), float)


def test_history_keys_callbacks_and_batch_logs(tmp_path):
    m = _model(metrics=["accuracy", "auc"], weighted_metrics=["auc"])
    x, y, w = _data(40)
    seen = []

    class Batches(Callback):
        def on_batch_end(self, batch, logs=None):
            seen.append(sorted(k for k in logs if k not in ("batch", "size")))

    ck = ModelCheckpoint(str(tmp_path / "best.h5"), monitor="val_auc", save_best_only=True)
    assert ck.monitor_op is np.greater
    for cb in (EarlyStopping(monitor="val_weighted_auc"), EarlyStopping(monitor="val_purity"),
               EarlyStopping(monitor="val_efficiency"), EarlyStopping(monitor="val_acc")):
        assert cb.monitor_op is np.greater
    assert EarlyStopping(monitor="val_loss").monitor_op is np.less
    rl = ReduceLROnPlateau(monitor="val_auc")
    h = m.fit(x[:24], y[:24], batch_size=8, epochs=3, verbose=0, sample_weight=w[:24],
              validation_data=(x[24:], y[24:], w[24:]), callbacks=[ck, rl, Batches()])
    names = m.metrics_names
    assert sorted(k for k in h.history if k != "lr") == sorted(names + ["val_" + n for n in names])
    assert all(len(h.history[k]) == 3 for k in names)
    assert seen and all(s == ["acc", "loss"] for s in seen)      # batch logs stay loss / acc
    assert os.path.exists(str(tmp_path / "best.h5")) and ck.best == max(h.history["val_auc"])
    assert rl.monitor_op(1.0, 0.5)                               # max mode


def test_train_rpv_fom_metric_prints_one_minus_auc(capsys):
    argv = ["--synthetic", "--n-train", "64", "--n-valid", "32", "--n-epochs", "2", "--batch-size", "16", "--h1", "2",
            "--h2", "2", "--h3", "2", "--h4", "4", "--verbose", "0", "--seed", "3", "--metrics", "accuracy,auc",
            "--fom", "best", "--fom-metric", "val_auc"]
    try:
        h = train_rpv.main(argv)
    finally:
        hvd.shutdown()
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("FoM:")]
    assert len(lines) == 1
    aucs = h.history["val_auc"]
    assert len(aucs) == 2 and float(lines[0].split()[1]) == 1.0 - max(aucs)
    args = train_rpv.build_parser().parse_args([])
    assert args.fom_metric == "val_loss" and args.metrics is None and args.weighted_metrics is None
    with pytest.raises(SystemExit):
        train_rpv.main(["--synthetic", "--weighted-metrics", "auc"])     # needs --use-weights


def test_rejected_combinations():
    with pytest.raises(NotImplementedError) as e:
        _model(3, metrics=["accuracy", "purity"])
    assert "purity" in str(e.value) and "dense_" in str(e.value)
    with pytest.raises(NotImplementedError) as e:
        _model(3, weighted_metrics=["recall"])
    assert "weighted_efficiency" in str(e.value)
    with pytest.raises(NotImplementedError) as e:
        _model(2, metrics=["auc"], head="linear")
    assert "auc" in str(e.value) and "linear" in str(e.value)
    with pytest.raises(NotImplementedError):
        _model(2, weighted_metrics=["accuracy"], head="linear")
    with pytest.raises(NotImplementedError):
        _model(3, metrics=["auc"], head="sigmoid", loss="binary_crossentropy")     # multi-label sigmoid
    with pytest.raises(NotImplementedError) as e:
        _model(metrics=["accuracy", "f1"])                                        # unknown: as before
    assert str(e.value) == "metric 'f1'"
    _model(2, metrics=["accuracy"], head="linear")                                # the plain accuracy still compiles
    m = _model(metrics=["auc"], weighted_metrics=["auc"])
    x, y, w = _data(12)
    for bad in (-1.0, np.nan, np.inf):
        wb = w.copy()
        wb[3] = bad
        with pytest.raises(ValueError, match="finite and non-negative"):
            m.evaluate(x, y, sample_weight=wb, verbose=0)
        with pytest.raises(ValueError, match="finite and non-negative"):
            m.fit(x, y, sample_weight=wb, verbose=0)
        with pytest.raises(ValueError, match="finite and non-negative"):
            MT.roc_curve(y, np.full(12, 0.5, F32), wb)
    _model(metrics=["auc"]).evaluate(x, y, sample_weight=-w, verbose=0)           # (no weighted metric: Keras' rule)


# ------------------------------------------------------------------------------------ the key
def _reachable():
    """The bins some fp32 score reaches: all of the lower half; of the upper half those of the 2^23 + 1
    scores in [0.5, 1] (a grid of 2^-24: towards 1 most bins of 128 per octave hold no fp32 score)."""
    s = (np.arange(2 ** 23, 2 ** 24 + 1) / 2.0 ** 24).astype(F32)
    r = np.zeros(MT.ROC_BINS, bool)
    r[:H] = True
    r[MT.score_bin(s)] = True
    return r


def test_key_edges_round_trip():
    """score_bin(bin_lower_edge(i)) == i for every bin an fp32 score can reach, and the next fp32 below
    the edge falls into a lower bin; the edge of an unreachable bin is the next reachable bin's."""
    assert MT.ROC_BINS == 2 * H + 1 == 32257
    i = np.arange(MT.ROC_BINS)
    e = MT.bin_lower_edge(i)
    k = MT.score_bin(e)
    reach = _reachable()
    assert reach.sum() > H + 2000
    assert np.array_equal(k[reach], i[reach]) and np.array_equal(k == i, reach) and np.all(k >= i)
    below = np.nextafter(e[1:], F32(-1), dtype=F32)
    kb = MT.score_bin(below)
    assert np.all(kb < i[1:])
    prev = np.maximum.accumulate(np.where(reach, i, 0))         # the last reachable bin at or below i
    assert np.array_equal(kb, prev[i[1:] - 1])
    assert np.all(np.diff(e.astype(np.float64)) >= 0) and e[0] == 0 and e[H] == 0.5 and e[2 * H] == 1.0
    with pytest.raises(ValueError):
        MT.bin_lower_edge(MT.ROC_BINS)


def test_key_edge_values_invalid_scores_and_monotony():
    one = F32(1)
    s = np.array([0.0, -0.0, 1e-45, np.nextafter(F32(0.5), F32(0)), 0.5, np.nextafter(F32(0.5), one),
                  np.nextafter(one, F32(0)), 1.0], F32)
    k = MT.score_bin(s)
    assert k.tolist() == [0, 0, 0, H - 1, H, H + 1, 2 * H - (0x33800000 >> 16), 2 * H]
    assert MT.score_bin(np.array([np.nan, -1e-9, np.nextafter(one, F32(2)), np.inf, -np.inf], F32)).tolist() == [-1] * 5
    rs = np.random.RandomState(0)
    draws = np.concatenate([rs.rand(200000), 1 - 10.0 ** rs.uniform(-8, 0, 200000), 10.0 ** rs.uniform(-40, 0, 200000), s])
    draws = np.sort(np.clip(draws, 0, 1).astype(F32))
    assert np.all(np.diff(MT.score_bin(draws)) >= 0)
    up = draws[draws >= 0.5]
    assert np.array_equal((one - up).astype(np.float64), 1.0 - up.astype(np.float64))      # 1 - s is exact
    r = MT.roc_curve([1, 0, 1, 0], np.array([0.9, np.nan, 0.2, 0.1], F32))
    assert r.n_invalid == 1 and all(math.isnan(v) for v in (r.auc, r.accuracy, r.purity, r.efficiency))


# ------------------------------------------------------------------------------------ the numpy twin
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kind", ["weak", "strong", "rpv", "saturated"])
def test_twin_against_the_oracle(kind, weighted):
    n = 4096
    y, s = O.synthetic(kind, n, seed=1)
    w = np.random.RandomState(2).uniform(0.0, 3.0, n).astype(F32) if weighted else None
    r = MT.roc_curve(y, s, w)
    exact, bound = O.exact_auc(y, s, w), O.hist_bound(y, s, MT.score_bin(s), w)
    print("%s weighted=%s: auc %.9f exact %.9f |diff| %.3g bound %.3g" % (kind, weighted, r.auc, exact,
                                                                        abs(r.auc - exact), bound))
    assert bound <= 1e-3                                    # (of the oracle alone)
    # (the weighted histogram holds llrint(w 2^k): each weight is off by at most 2^-(k+1), n 2^-61 of the total)
    assert abs(r.auc - exact) <= bound + 1e-12
    if kind == "saturated":
        assert O.hist_bound(y, s, MT.score_bin(s)) == 0.0
        assert abs(MT.roc_curve(y, s).auc - O.exact_auc(y, s)) <= 2.0 ** -50
    rep, orc = classification_report(y, s, w), O.summary(y, s, w)
    tol = n * 2.0 ** -50
    for got, a, b in ((r.accuracy, rep["accuracy"], orc["acc"]), (r.purity, rep["purity"], orc["purity"]),
                      (r.efficiency, rep["efficiency"], orc["efficiency"])):
        assert abs(got - a) <= tol * a and abs(got - b) <= tol * b
    conf = O.confusion(y, s, w)
    assert all(abs(g - c) <= tol * max(c, 1.0) for g, c in zip(r.confusion, conf))
    # the curve: from (0, 0) at threshold inf to (1, 1), one point per non-empty bin, monotone
    assert r.fpr[0] == r.tpr[0] == 0.0 and np.isinf(r.thresholds[0]) and r.fpr[-1] == r.tpr[-1] == 1.0
    assert np.all(np.diff(r.fpr) >= 0) and np.all(np.diff(r.tpr) >= 0) and np.all(np.diff(r.thresholds) < 0)
    assert len(r.fpr) == len(np.unique(MT.score_bin(s[w > 0] if weighted else s))) + 1
    assert abs(np.trapezoid(r.tpr, r.fpr) - r.auc) <= 1e-12
    assert MT.roc_auc_score(y, s, w) == r.auc


def test_oracle_against_sklearn():
    sk = pytest.importorskip("sklearn.metrics")
    for kind in ("weak", "rpv", "saturated"):
        y, s = O.synthetic(kind, 2000, seed=4)
        w = np.random.RandomState(5).uniform(0.0, 3.0, 2000)
        for ww in (None, w):
            assert abs(O.exact_auc(y, s, ww) - sk.roc_auc_score(y, s, sample_weight=ww)) <= 1e-12
            fpr, tpr, _ = sk.roc_curve(y, s, sample_weight=ww)
            assert abs(np.trapezoid(tpr, fpr) - O.exact_auc(y, s, ww)) <= 1e-12
            o = O.summary(y, s, ww)
            pred = s > 0.5
            assert abs(o["acc"] - sk.accuracy_score(y, pred, sample_weight=ww)) <= 1e-12
            assert abs(o["purity"] - sk.precision_score(y, pred, sample_weight=ww)) <= 1e-12
            assert abs(o["efficiency"] - sk.recall_score(y, pred, sample_weight=ww)) <= 1e-12


def test_degenerate_inputs():
    assert math.isnan(MT.roc_auc_score([1, 1, 1], np.array([0.2, 0.5, 0.9], F32)))          # no negatives
    assert math.isnan(MT.roc_auc_score([1, 0], np.array([0.2, 0.9], F32), [0.0, 1.0]))       # ... of any weight
    r = MT.roc_curve([0, 0, 1], np.array([0.1, 0.2, 0.3], F32))
    assert r.auc == 1.0 and r.purity == 0.0 and r.efficiency == 0.0 and r.accuracy == 2 / 3   # nothing predicted
    assert MT.weight_shift(1.0) == 60 and MT.weight_shift(2.0 ** 61) == -1 and MT.weight_shift(0.0) == 0
    w = np.array([1e-6, 1.0, 1e8], F32)
    k = MT.weight_shift(float(w.astype(np.float64).sum()))
    assert int(MT.fixed_weights(w, k).sum()) <= 2 ** 61


# ------------------------------------------------------------------------------------ RefExecutor
@pytest.mark.parametrize("n_out", [1, 3])
def test_reference_executor_equals_roc_curve_of_its_predict(n_out):
    """The integers are the same, so in eval mode the values are exactly equal."""
    names = dict(metrics=["accuracy", "auc", "purity", "efficiency"], weighted_metrics=["acc", "auc", "purity", "efficiency"]) \
        if n_out == 1 else dict(metrics=["accuracy", "auc"], weighted_metrics=["accuracy", "auc"])
    m = _model(n_out, **names)
    x, y, w = _data(40, n_out, seed=3)
    h = m.fit(x[:24], y[:24], batch_size=6, epochs=2, verbose=0, sample_weight=w[:24],
              validation_data=(x[24:], y[24:], w[24:]))
    p = m.predict(x[24:], batch_size=6)
    ev = dict(zip(m.metrics_names, m.evaluate(x[24:], y[24:], batch_size=6, verbose=0, sample_weight=w[24:])))
    for k, v in ev.items():
        assert _same(v, h.history["val_" + k][-1]), k
    for prefix, ww in (("", None), ("weighted_", w[24:])):
        if n_out == 1:
            r = MT.roc_curve(y[24:], p[:, 0], ww)
            assert r.n_invalid == 0 and not math.isnan(r.auc)
            assert ev[prefix + "auc"] == r.auc and ev[prefix + "acc"] == r.accuracy
            assert ev[prefix + "purity"] == r.purity and ev[prefix + "efficiency"] == r.efficiency
        else:
            curves = MT.per_class_curves(y[24:], p, ww)
            aucs = [c.auc for c in curves if not math.isnan(c.auc)]
            assert len(curves) == 3 and aucs and ev[prefix + "auc"] == sum(aucs) / len(aucs)
            wv = np.ones(16) if ww is None else ww.astype(np.float64)
            acc = float((wv * (MT.first_argmax(p) == y[24:].argmax(1))).sum() / wv.sum())
            assert abs(ev[prefix + "acc"] - acc) <= 16 * 2.0 ** -50
    er = m.evaluate_roc(x[24:], y[24:], sample_weight=w[24:], batch_size=6)
    if n_out == 1:
        assert er.auc == ev["weighted_auc"] and sum(er.confusion) > 0
    else:
        assert [c.auc for c in er] == [c.auc for c in MT.per_class_curves(y[24:], p, w[24:])]
    # ... whether or not the metrics were compiled in
    plain = _model(n_out, metrics=["accuracy"])
    plain.set_weights(m.get_weights())
    er2 = plain.evaluate_roc(x[24:], y[24:], sample_weight=w[24:], batch_size=6)
    assert (er2.auc == er.auc) if n_out == 1 else ([c.auc for c in er2] == [c.auc for c in er])


# ------------------------------------------------------------------------------------ checkpoints
def test_checkpoint_round_trip_and_unchanged_bytes(tmp_path):
    m = _model(metrics=["accuracy", "auc"], weighted_metrics=["auc", "recall"])
    x, y, w = _data(16)
    m.fit(x, y, batch_size=8, epochs=1, verbose=0, sample_weight=w)
    p = str(tmp_path / "m.h5")
    m.save(p)
    c = load_model(p, device="cpu")
    assert c.metrics == ["accuracy", "auc"] and c.weighted_metrics == ["auc", "recall"]
    assert c.metrics_names == m.metrics_names == ["loss", "acc", "auc", "weighted_auc", "weighted_efficiency"]
    a, b = (mm.evaluate(x, y, verbose=0, sample_weight=w) for mm in (m, c))
    assert all(_same(u, v) for u, v in zip(a, b))
    # a model without the new metrics: no weighted_metrics key, the training_config it always wrote
    import json
    from cori_intml_examples_amd.io import h5
    plain = _model(metrics=["accuracy"])
    q = str(tmp_path / "p.h5")
    plain.save(q)
    with h5.H5File(q, "r") as f:
        tc = json.loads(f.attrs("/")["training_config"])
    assert list(tc) == ["optimizer_config", "loss", "metrics", "sample_weight_mode", "loss_weights"]
    assert tc["metrics"] == ["accuracy"]
    with h5.H5File(p, "r") as f:
        assert json.loads(f.attrs("/")["training_config"])["weighted_metrics"] == ["auc", "recall"]
