"""Per-sample and per-class loss weights (Keras 2.2 ``weighted_masked_objective`` /
``standardize_weights``) on the CPU reference backend: fit / evaluate / validation / the
batch calls, the epoch-loss normalisation, the host rules, data parallelism with 2 gloo ranks,
and the compiler's resource report of the weighted head kernel instances.

For a batch of M rows with weights w and nnz = #(w != 0):  L_batch = sum(w l) / nnz, and the
epoch loss is Keras' BaseLogger mean sum_b(M_b L_b) / N.  ``acc`` stays unweighted."""
import json
import os
import shutil
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from cori_intml_examples_amd.apps import zoo
from cori_intml_examples_amd.io.datasets import synthetic_mnist, synthetic_rpv
from cori_intml_examples_amd.models.executor_base import standardize_weights
from cori_intml_examples_amd.ops import reference as R
from cori_intml_examples_amd.utils import set_random_seed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _torchrun(nproc, args, timeout=300):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.update({"INTML_DEVICE": "cpu", "PYTHONPATH": ROOT, "OMP_NUM_THREADS": "2"})
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
           "--master-addr", "127.0.0.1", "--master-port", str(port)] + args
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout, cwd=ROOT)


def make_weights(n, seed=0):
    """The test weights: 0.25 + 3.75 * rand, every fifth entry exactly 0."""
    w = (0.25 + 3.75 * np.random.RandomState(seed).rand(n)).astype(np.float32)
    w[::5] = 0.0
    return w


def _rpv(opt="Adam", lr=0.01, seed=3, size=8):
    set_random_seed(seed)
    return zoo.rpv_cnn((size, size, 1), [2, 2, 2], [4], dropout=0.0, optimizer=opt, lr=lr, device="cpu")


def _bce64(p, y):
    p = np.clip(np.asarray(p, np.float64).reshape(-1), 1e-7, 1 - 1e-7)
    y = np.asarray(y, np.float64).reshape(-1)
    return -(y * np.log(p) + (1 - y) * np.log(1 - p))


def _epoch_loss64(l, w, bs):
    """sum_b(M_b * L_b) / N with L_b = sum(w l) / nnz_b over consecutive batches of bs rows."""
    n, tot = len(l), 0.0
    for s in range(0, n, bs):
        lb, wb = l[s:s + bs], np.asarray(w[s:s + bs], np.float64)
        tot += len(lb) * float((wb * lb).sum()) / max(int((wb != 0).sum()), 1)
    return tot / n


def test_weighted_calls_run():
    """The calls that raised NotImplementedError (or ignored the weights) before."""
    x, y, _ = synthetic_rpv(48, size=8, seed=4)
    w = make_weights(48)
    m = _rpv()
    h = m.fit(x, y, batch_size=16, epochs=1, verbose=0, sample_weight=w)
    assert np.isfinite(h.history["loss"][0])
    h = m.fit(x, y, batch_size=16, epochs=1, verbose=0, class_weight={0: 1., 1: 3.})
    assert np.isfinite(h.history["loss"][0])
    h = m.fit(x, y, batch_size=16, epochs=1, verbose=0, validation_data=(x, y, w))
    assert np.isfinite(h.history["val_loss"][0])
    ew = m.evaluate(x, y, batch_size=16, verbose=0, sample_weight=w)
    eu = m.evaluate(x, y, batch_size=16, verbose=0)
    assert np.isfinite(ew[0]) and ew[0] != eu[0] and ew[1] == eu[1]
    assert h.history["val_loss"][0] == pytest.approx(ew[0], rel=1e-6)
    assert m.test_on_batch(x, y, sample_weight=w)[0] != m.test_on_batch(x, y)[0]
    assert np.isfinite(m.train_on_batch(x, y, sample_weight=w, class_weight={0: 1., 1: 3.})[0])


def test_weighted_training_matches_closed_form_adam():
    """Two Adam steps on the CPU backend == Keras Adam math on fp64 autograd gradients of an
    independently written weighted loss sum(w l) / nnz (model, data and bounds of
    test_framework.py::test_model_training_matches_closed_form_adam)."""
    x, y, _ = synthetic_rpv(32, size=8, seed=4)
    w = make_weights(32)
    m = zoo.rpv_cnn((8, 8, 1), [2, 2, 2], [4], dropout=0.0, optimizer="Adam", lr=0.01, device="cpu")
    ws = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in m.get_weights()]
    mom = [torch.zeros_like(v) for v in ws]
    vel = [torch.zeros_like(v) for v in ws]
    wt = torch.tensor(w, dtype=torch.float64)
    nnz = int((w != 0).sum())
    assert 0 < nnz < 32

    def loss_fn(ws):
        a = torch.tensor(x, dtype=torch.float64)
        for i in range(3):
            a = R.conv2d(a, ws[2 * i], ws[2 * i + 1], 1, "same").relu()
            a = torch.nn.functional.max_pool2d(a.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
        a = a.reshape(a.shape[0], -1)
        a = (a @ ws[6] + ws[7]).relu()
        z = (a @ ws[8] + ws[9]).reshape(-1)
        p = torch.sigmoid(z).clamp(1e-7, 1 - 1e-7)
        yt = torch.tensor(y, dtype=torch.float64)
        l = -(yt * torch.log(p) + (1 - yt) * torch.log(1 - p))
        return (wt * l).sum() / nnz

    for t in (1, 2):
        ws_ = [v.detach().clone().requires_grad_(True) for v in ws]
        loss = loss_fn(ws_)
        gs = torch.autograd.grad(loss, ws_)
        lr_t = 0.01 * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        new = []
        for v, g, mo, ve in zip(ws_, gs, mom, vel):
            mo.mul_(0.9).add_(0.1 * g)
            ve.mul_(0.999).add_(0.001 * g * g)
            new.append((v - lr_t * mo / (ve.sqrt() + 1e-7)).detach())
        ws = new
        out = m.train_on_batch(x, y, sample_weight=w)
        assert out[0] == pytest.approx(float(loss.detach()), rel=1e-4)
    for a, b in zip(m.get_weights(), ws):
        np.testing.assert_allclose(a, b.numpy(), rtol=0, atol=2e-5)


def test_epoch_loss_normalisation():
    """history['loss'] and evaluate(sample_weight=) are sum_b(M_b L_b) / N, with a partial tail
    batch; acc is the unweighted acc."""
    n, bs = 5 * 16 + 7, 16
    x, y, _ = synthetic_rpv(n, size=8, seed=6)
    w = make_weights(n, seed=1)
    m = _rpv(opt="SGD", lr=0.0)
    w0 = [v.copy() for v in m.get_weights()]
    want = _epoch_loss64(_bce64(m.predict(x, batch_size=bs), y), w, bs)
    h = m.fit(x, y, batch_size=bs, epochs=1, verbose=0, shuffle=False, sample_weight=w)
    for a, b in zip(m.get_weights(), w0):
        np.testing.assert_array_equal(a, b)            # lr = 0: the model did not move
    ev = m.evaluate(x, y, batch_size=bs, verbose=0, sample_weight=w)
    eu = m.evaluate(x, y, batch_size=bs, verbose=0)
    assert h.history["loss"][0] == pytest.approx(want, rel=1e-4)
    assert ev[0] == pytest.approx(want, rel=1e-4)
    assert eu[0] == pytest.approx(float(_bce64(m.predict(x, batch_size=bs), y).mean()), rel=1e-4)
    assert abs(want - eu[0]) > 1e-3 * eu[0]            # the weights matter at this bound
    assert h.history["acc"][0] == eu[1] and ev[1] == eu[1]


def test_host_rules():
    y1 = np.array([0, 1, 1, 0, 1], np.float32)
    cw = {0: 0.5, 1: 2.0}
    np.testing.assert_array_equal(standardize_weights(y1, 5, None, cw), [0.5, 2, 2, 0.5, 2])
    np.testing.assert_array_equal(standardize_weights(y1.reshape(-1, 1), 5, None, cw), [0.5, 2, 2, 0.5, 2])
    yh = np.eye(3, dtype=np.float32)[[2, 0, 1, 2]]
    np.testing.assert_array_equal(standardize_weights(yh, 4, None, {0: 1., 1: 2., 2: 4.}), [4, 1, 2, 4])
    sw = np.array([1, 2, 3, 4, 0], np.float32)
    np.testing.assert_array_equal(standardize_weights(y1, 5, sw, cw), [0.5, 4, 6, 2, 0])
    assert standardize_weights(y1, 5, None, None) is None
    with pytest.raises(ValueError):
        standardize_weights(yh, 4, None, {0: 1., 1: 2.})            # class 2 missing
    with pytest.raises(ValueError):
        standardize_weights(y1, 5, np.ones(4, np.float32), None)      # wrong length
    with pytest.raises(ValueError):
        standardize_weights(y1, 5, np.ones((5, 1), np.float32), None)  # 2-D

    # ... and through the public calls
    x, y, _ = synthetic_rpv(40, size=8, seed=4)
    w = make_weights(40)
    m = _rpv(opt="SGD", lr=0.0)
    with pytest.raises(ValueError):
        m.fit(x, y, batch_size=8, epochs=1, verbose=0, class_weight={0: 1.})
    with pytest.raises(ValueError):
        m.fit(x, y, batch_size=8, epochs=1, verbose=0, sample_weight=w[:-1])
    with pytest.raises(ValueError):
        m.evaluate(x, y, verbose=0, sample_weight=w.reshape(-1, 1))
    with pytest.raises(ValueError):
        m.train_on_batch(x, y, sample_weight=np.ones(3, np.float32))
    # class_weight == the equivalent sample_weight; both == their product
    cw = {0: 1., 1: 3.}
    a = m.fit(x, y, batch_size=8, epochs=1, verbose=0, shuffle=False, class_weight=cw, sample_weight=w)
    b = m.fit(x, y, batch_size=8, epochs=1, verbose=0, shuffle=False, sample_weight=w * np.where(y > 0.5, 3., 1.))
    assert a.history["loss"] == b.history["loss"]
    # one-hot targets through fit
    xm, ym, _, _ = synthetic_mnist(40, 1, rows=12, cols=12)
    set_random_seed(2)
    mm = zoo.mnist_cnn(2, 2, 4, dropout=0.0, optimizer="SGD", lr=0.0, input_shape=(12, 12, 1), device="cpu")
    cwm = {k: 1.0 + k for k in range(10)}
    a = mm.fit(xm, ym, batch_size=8, epochs=1, verbose=0, shuffle=False, class_weight=cwm)
    b = mm.fit(xm, ym, batch_size=8, epochs=1, verbose=0, shuffle=False,
               sample_weight=(1.0 + ym.argmax(1)).astype(np.float32))
    assert a.history["loss"] == b.history["loss"]
    # validation_split slices the weights with x and y (the last fraction)
    h = m.fit(x, y, batch_size=8, epochs=1, verbose=0, shuffle=False, validation_split=0.25, sample_weight=w)
    assert h.history["val_loss"][0] == m.evaluate(x[30:], y[30:], batch_size=8, verbose=0, sample_weight=w[30:])[0]
    assert h.history["loss"][0] == m.evaluate(x[:30], y[:30], batch_size=8, verbose=0, sample_weight=w[:30])[0]
    assert h.history["val_loss"][0] != m.evaluate(x[30:], y[30:], batch_size=8, verbose=0)[0]


def test_all_ones_weights_bit_identical():
    x, y, _ = synthetic_rpv(48, size=8, seed=4)
    res = []
    for w in (None, np.ones(16, np.float32)):
        m = _rpv(seed=11)
        outs = [m.train_on_batch(x[16 * k:16 * k + 16], y[16 * k:16 * k + 16], sample_weight=w) for k in range(3)]
        res.append((m.get_weights(), outs))
    for a, b in zip(res[0][0], res[1][0]):
        np.testing.assert_array_equal(a, b)
    assert res[0][1] == res[1][1]


def test_all_zero_batch_is_finite():
    """Keras gives 0/0 here; this project clamps the divisor: zero loss, zero gradient."""
    x, y, _ = synthetic_rpv(16, size=8, seed=4)
    m = _rpv(seed=12)
    w0 = [v.copy() for v in m.get_weights()]
    out = m.train_on_batch(x, y, sample_weight=np.zeros(16, np.float32))
    assert out[0] == 0.0
    for a, b in zip(m.get_weights(), w0):
        assert np.isfinite(a).all()
        np.testing.assert_array_equal(a, b)             # zero gradient: Adam does not move
    assert m.evaluate(x, y, verbose=0, sample_weight=np.zeros(16, np.float32))[0] == 0.0


def test_dp_two_ranks_weighted(tmp_path):
    """2 gloo ranks, strictly positive weights: every rank normalises by its own nnz, the ranks
    end bit-identical and the DP step equals the single-process step on the global batch."""
    r = _torchrun(2, [os.path.join(ROOT, "tests", "dp_weight_worker.py"), str(tmp_path)])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    reps = [json.load(open(tmp_path / ("wrank%d.json" % i))) for i in range(2)]
    assert reps[0]["w1"] == reps[1]["w1"]
    assert reps[0]["wf"] == reps[1]["wf"]
    assert reps[0]["dp_vs_single_maxdiff"] < 1e-5
    assert reps[0]["weighted_differs_from_unweighted"] > 1e-4


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_weighted_head_instances_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources as KR
    rows = KR.report(os.path.join(KR.KDIR, "head.hip"))
    head = [r for r in rows if "head_kernel" in r["name"]]
    wt = [r for r in head if "Lb1E" in r["name"]]
    assert len(head) == 8 and len(wt) == 4, [r["name"] for r in rows]
    assert all(r.get("scratch", 0) == 0 and r.get("vgpr_spill", 0) == 0 for r in head), \
        [(r["name"], r.get("scratch"), r.get("vgpr_spill")) for r in head]


def test_weights_through_compat_keras_names():
    """Reference-style code (``keras`` names registered by compat.install) with weights."""
    code = r'''
import cori_intml_examples_amd.compat as c
c.install()
import numpy as np
from keras.models import Sequential
from keras.layers import Conv2D, MaxPooling2D, Flatten, Dense
model = Sequential()
model.add(Conv2D(2, (3, 3), activation='relu', input_shape=(8, 8, 1)))
model.add(MaxPooling2D(pool_size=(2, 2)))
model.add(Flatten())
model.add(Dense(1, activation='sigmoid'))
model.compile(optimizer='Adam', loss='binary_crossentropy', metrics=['accuracy'])
rs = np.random.RandomState(0)
x = rs.rand(40, 8, 8, 1).astype('float32')
y = (rs.rand(40) > 0.5).astype('float32')
w = (0.25 + 3.75 * rs.rand(40)).astype('float32')
w[::5] = 0
h = model.fit(x, y, batch_size=8, epochs=1, verbose=0, sample_weight=w, class_weight={0: 1., 1: 2.},
              validation_data=(x, y, w))
a = model.evaluate(x, y, batch_size=8, verbose=0, sample_weight=w)
b = model.test_on_batch(x[:8], y[:8], sample_weight=w[:8])
t = model.train_on_batch(x[:8], y[:8], sample_weight=w[:8], class_weight={0: 1., 1: 2.})
print('ok', sorted(h.history), h.history['val_loss'][0] == a[0], len(b), len(t))
'''
    env = dict(os.environ, INTML_DEVICE="cpu", OMP_NUM_THREADS="2", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ok ['acc', 'loss', 'val_acc', 'val_loss'] True 2 2" in r.stdout
