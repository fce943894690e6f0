"""The second output-head kernel (csrc/kernels/loss_head.hip) on the GPU.

1. The kernel alone, steered as tests/test_head_edges.py steers head_kernel: SGD at learning rate
   0, the logits placed by lstsq on the head's saved input, the float64 oracle
   (tests/helpers/loss_oracle.py) evaluated on the logits recomputed in float64 from that saved
   bf16 input and the float32 weights.  Every (activation, loss) pair, every loss on its natural
   activation at N = 1, 2, 3, 15, 16, the multi-label binary_crossentropy at every N > 1,
   M = 1, 3, 4, 5, 26, K = 5, 64, 65, 130 (K N on both sides of HEAD_W_LDS), behind a hidden
   dense and on a flattened conv of 3 channels padded to 8.  Checked against the oracle's DERIVED
   bounds (tests/test_loss_head.py proves them on these same input sets): loss, probs, exact
   integer correct counts, gw / gb, the gradient stored for the previous stage, the train / eval /
   predict plans, the weighted instances, repeated launches, exact ties, the launchers' checks
   and NaN propagation.
2. Whole models against the CPU executor at the project's standing bounds, and the structure
   (launch lists, graph replay, fit, checkpoint, data parallel at one rank).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cori_intml_examples_amd import optim
from cori_intml_examples_amd.io.keras_h5 import load_model
from cori_intml_examples_amd.models import Conv2D, Dense, Flatten, Input, MaxPooling2D, Model
from cori_intml_examples_amd.optim import SGD
from cori_intml_examples_amd.utils import set_random_seed

from helpers import loss_models as LM
from helpers import loss_oracle as O
from test_head_edges import Rig, _inputs
from test_hip_model import _build, _data, _rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
U = O.U
KINK_CAP = 0.01


def _K():
    from cori_intml_examples_amd.ops.hip import kernels
    return kernels()


# ------------------------------------------------------------------------------------ 1. the kernel alone
def _head_model(arch, act, loss, N, K):
    """dense: conv -> pool -> flatten -> Dense(K, relu) -> head; conv: Conv2D(3) (3 channels in a
    stride of 8) -> pool -> flatten (4 * 4 * 3 = 48) -> head."""
    inp = Input(shape=(8, 8, 1))
    h = Conv2D(3 if arch == "conv" else 8, (3, 3), activation="relu", padding="same")(inp)
    h = Flatten()(MaxPooling2D((2, 2))(h))
    if arch == "dense":
        h = Dense(K, activation="relu")(h)
    m = Model(inp, Dense(N, activation=act)(h), device="cuda")
    m.compile(optimizer=SGD(lr=0.0), loss=loss, metrics=["accuracy"])
    return m


def _weights(M, seed):
    """Sample weights over 1e-3 .. 1e3 with zeros."""
    rs = np.random.RandomState(seed)
    w = (10.0 ** rs.uniform(-3, 3, M)).astype(np.float32)
    w[::4] = 0.0
    if M == 1:
        w[0] = 0.37
    return w


def _compare(tag, rig, t, ev, bd, a, wts=None):
    """One training run against the oracle ``ev`` with its bounds ``bd``."""
    M, N = ev.M, ev.N
    W64 = np.asarray(rig.W, np.float64)
    f = O.H.weight_factor(wts) if wts is not None else np.ones(M)
    rows, dz = ev.loss * f, ev.dz * f[:, None]
    tol_dz = (bd.dz + bd.dz_jump) * f[:, None] + 4 * U * np.abs(dz)
    assert t["n"] == M and t["flag"] == 0, (tag, t["n"], t["flag"])
    # loss: the rows' bounds, the float32 sum of up to four rows per workgroup, the 2^-32 fixed point
    lb = float((bd.loss * f).mean() + 8 * U * np.abs(rows).mean() + 2.0 ** -30)
    el = abs(t["loss"] - rows.mean())
    # correct: an exact integer; only elements the logit error may flip are allowed to differ
    div = N if (ev.binary and N > 1) else 1
    cnt = t["acc"] * M * div
    assert abs(cnt - round(cnt)) < 1e-6 and abs(round(cnt) - ev.correct.sum()) <= bd.acc_ambiguous.sum(), (tag, cnt, ev.correct.sum())
    gw, gb = a.T @ dz / M, dz.sum(0) / M
    tw = np.abs(a).T @ tol_dz / M + (M + 2) * U * (np.abs(a).T @ np.abs(dz)) / M
    tb = tol_dz.sum(0) / M + (M + 2) * U * np.abs(dz).sum(0) / M
    ew, eb = np.abs(t["gw"].reshape(gw.shape) - gw), np.abs(t["gb"].reshape(gb.shape) - gb)
    mask = a > 0
    ref = (dz / M) @ W64.T * mask
    tp = 2.0 ** -8 * np.abs(ref) + ((tol_dz / M) @ np.abs(W64).T + (N + 2) * U * (np.abs(dz) / M) @ np.abs(W64).T) * mask
    ep = np.abs(t["dprev"] - ref)
    print("%-44s loss err %.3g (bound %.3g)  gw %.3g (%.3g)  gb %.3g (%.3g)  dprev %.3g (max |ref| %.3g)  near-kink %.4f"
          % (tag, el, lb, ew.max(), tw.max(), eb.max(), tb.max(), ep.max(), np.abs(ref).max(), bd.near_kink.mean()))
    assert el <= lb, (tag, "loss", el, lb)
    assert (ew <= tw + 1e-300).all(), (tag, "gw", float((ew - tw).max()))
    assert (eb <= tb + 1e-300).all(), (tag, "gb", float((eb - tb).max()))
    assert (ep <= tp + 1e-300).all(), (tag, "dprev", float((ep - tp).max()))
    assert t["dpad"] == 0.0
    assert bd.near_kink.mean() <= KINK_CAP, (tag, bd.near_kink.mean())


def _oracle(rig, a, act, loss, y):
    z = a @ np.asarray(rig.W, np.float64) + np.asarray(rig.b, np.float64)
    ev = O.evaluate(act, loss, z, y)
    return ev, O.bounds(ev, O.logit_error_bound(a, rig.W, rig.b))


@pytest.mark.parametrize("case", O.kernel_cases(), ids=lambda c: "%s-%s-M%d-N%d-K%d-%s" % c)
def test_loss_head_kernel_against_the_oracle(case):
    act, loss, M, N, K, arch = case
    set_random_seed(71)
    m = _head_model(arch, act, loss, N, K)
    ex = m._executor
    assert ex.loss_head and ex.plan.head.K == K and (arch == "dense" or (ex.head_src.C, ex.head_src.Cs) == (3, 8))
    rig = Rig(m, _inputs(m, M))
    Zs, y = O.draw(loss, act, M, N)
    b = (0.5 * np.random.RandomState(11).randn(N)).astype(np.float32)
    rig.set_head(rig.w0[-2], b)
    t0 = rig.train(y)                                         # the head's input
    names = [l.name for l in t0["bp"].launches]
    assert "loss_head" in names and "head" not in names and t0["bp"].head_blocks == -(-M // 4)
    assert arch == "conv" or "dense_epi0" in names
    a = t0["a"]
    rig.set_head(O.place(a, Zs, b), b)
    t = rig.train(y)
    assert torch.equal(t["prev"], t0["prev"]), "head input changed between runs"
    tag = "%s %s M=%d N=%d K=%d %s" % case
    ev, bd = _oracle(rig, a, act, loss, y)
    assert np.isfinite(ev.loss).all() and np.isfinite(ev.dz).all()
    _compare(tag, rig, t, ev, bd, a)
    # a repeated launch: bit for bit
    t2 = rig.train(y)
    for k in ("gw", "gb", "dprev", "loss", "acc"):
        assert np.array_equal(t[k], t2[k]), (tag, k)
    # eval and predict plans
    e = rig.evaluate(y)
    assert e["n"] == M and e["flag"] == 0 and e["acc"] == t["acc"]
    assert abs(e["loss"] - ev.loss.mean()) <= float(bd.loss.mean() + 8 * U * np.abs(ev.loss).mean() + 2.0 ** -30)
    assert "loss_head" in [l.name for l in e["bp"].launches]
    p = rig.predict()
    assert p["probs"].shape == (M, N)
    ep = np.abs(p["probs"] - ev.probs)
    assert (ep <= bd.dp + 2 * U * np.abs(ev.probs)).all(), (tag, "probs", float(ep.max()))
    # the weighted instances: all-ones weights bit-identical to unweighted, then real weights
    t1 = rig.train(y, np.ones(M, np.float32))
    assert (M, "train", "w") in ex._plans and t1["bp"].weighted
    for k in ("gw", "gb", "dprev", "loss", "acc"):
        assert np.array_equal(t[k], t1[k]), (tag, "ones", k)
    wts = _weights(M, seed=M + N)
    _compare(tag + " weighted", rig, rig.train(y, wts), ev, bd, a, wts=wts)


TIES = O.tie_cases()


@pytest.mark.parametrize("case", TIES, ids=lambda c: c[1])
def test_exact_ties_take_the_documented_subgradient(case):
    """Zero head weights: the bias IS the logit, exactly, in every row."""
    name, loss, z, y, want = case
    z, y, want = np.asarray(z, np.float64), np.asarray(y, np.float32), np.asarray(want, np.float64)
    N, M = z.shape[1], 5
    set_random_seed(72)
    m = _head_model("dense", None, loss, N, 64)
    rig = Rig(m, _inputs(m, M))
    rig.set_head(np.zeros_like(rig.w0[-2]), z[0])
    t = rig.train(np.repeat(y, M, 0))
    ev = O.evaluate(None, loss, np.repeat(z, M, 0), np.repeat(y, M, 0))
    np.testing.assert_allclose(ev.dz[0], want[0], rtol=1e-12)
    got = t["gb"].reshape(-1)
    print(name, got, want[0])
    assert (np.abs(got - want[0]) <= 16 * U * np.abs(want[0])).all(), (name, got, want[0])
    assert abs(t["loss"] - ev.loss.mean()) <= 16 * U * max(1.0, abs(ev.loss.mean()))
    assert abs(t["acc"] * M - ev.correct.sum()) < 1e-9


def test_launcher_checks():
    K = _K()
    s = torch.cuda.current_stream().cuda_stream
    buf = torch.zeros(4096, device="cuda")

    def args(**kw):
        h = K.HeadArgs()
        h.h = h.w = h.y = h.wslab = buf.data_ptr()
        h.M, h.K, h.Ks, h.N, h.act, h.loss = 4, 8, 8, 3, 0, K.LOSS_HINGE
        for k, v in kw.items():
            setattr(h, k, v)
        return h

    for kw, msg in ((dict(N=0), "N must be in 1..16"), (dict(N=17), "N must be in 1..16"), (dict(loss=-1), "unknown loss code"),
                    (dict(loss=K.LOSS_COUNT), "unknown loss code"), (dict(act=3), "unknown activation code"),
                    (dict(loss=K.LOSS_BCE, act=0), "needs a sigmoid output"), (dict(loss=K.LOSS_BCE, act=2), "needs a sigmoid output"),
                    (dict(M=0), "must be positive"), (dict(h=0), "null input or weight pointer"),
                    (dict(training=1, wslab=0), "needs targets and slabs")):
        with pytest.raises(ValueError, match=msg):
            K.loss_head(args(**kw), s)
    codes = [K.LOSS_MSE, K.LOSS_MAE, K.LOSS_MSLE, K.LOSS_LOGCOSH, K.LOSS_HINGE, K.LOSS_SQ_HINGE, K.LOSS_CAT_HINGE, K.LOSS_KLD,
             K.LOSS_POISSON, K.LOSS_BCE]
    assert codes == list(range(10)) and K.LOSS_COUNT == 10
    torch.cuda.synchronize()


def test_nan_reaches_the_sticky_flag():
    """poisson on a linear output with p + eps <= 0: log of a negative number.  The batch's loss is
    NaN, the non-finite counter is raised and stays raised until reset_metrics."""
    set_random_seed(73)
    m = _head_model("dense", None, "poisson", 3, 64)
    rig = Rig(m, _inputs(m, 5))
    y = np.ones((5, 3), np.float32)
    rig.set_head(np.zeros_like(rig.w0[-2]), np.array([1.0, -1.0, 2.0], np.float32))
    t = rig.train(y)
    assert t["flag"] >= 1 and np.isnan(t["loss"])
    # (only the loss has the logarithm: g = (1 - y / (p + eps)) / N stays finite)
    np.testing.assert_allclose(t["gb"].reshape(-1), [(1 - 1 / q) / 3 for q in (1.0, -1.0, 2.0)], rtol=1e-5, atol=1e-6)
    assert np.isnan(m._executor.read_metrics()[0])            # sticky
    rig.set_head(np.zeros_like(rig.w0[-2]), np.array([1.0, 1.0, 2.0], np.float32))
    t = rig.train(y)                                          # (Rig.train resets the metrics)
    assert t["flag"] == 0 and np.isfinite(t["loss"])


# ------------------------------------------------------------------------------------ 2. whole models
def _pair(spec, mk, drop=0.2, **kw):
    kind, act, loss, N = spec
    set_random_seed(1234)
    g = LM.build(kind, act, loss, N, mk(), "cuda", drop=drop, **kw)
    set_random_seed(1234)
    c = LM.build(kind, act, loss, N, mk(), "cpu", drop=drop, **kw)
    assert g._seed == c._seed and g._executor.loss_head
    for a, b in zip(g.get_weights(), c.get_weights()):
        np.testing.assert_array_equal(a, b)
    return g, c


def _three_steps(g, c, x, y):
    """Batches of 6, 6 and a ragged 4."""
    for m in (g, c):
        ex = m._executor
        d = ex.upload(x, y)
        perm = torch.arange(d.n, device=ex.device)
        for pos, bs in ((0, 6), (6, 6), (12, 4)):
            ex.train_step(d, perm, pos, bs)
    torch.cuda.synchronize()
    n = g.store.numel
    return g.store.master[:n].cpu().numpy(), c.store.master[:n].numpy()


OPTS = {"Adam": optim.Adam, "AMSGrad": lambda: optim.Adam(amsgrad=True), "SGDm": lambda: optim.SGD(lr=0.01, momentum=0.9),
        "Adam+clipnorm": lambda: optim.Adam(clipnorm=0.5)}
STEPS = [(s, "Adam", 0.0) for s in LM.MODELS] + [(LM.MODELS[1], "AMSGrad", 0.0), (LM.MODELS[4], "SGDm", 0.0),
                                                 (LM.MODELS[9], "Adam+clipnorm", 1e-3)]


@pytest.mark.parametrize("spec,opt,l2", STEPS, ids=["%s-%s-%s-%d-%s" % (s + (o,)) for s, o, _ in STEPS])
def test_three_steps_track_the_cpu_reference(spec, opt, l2):
    """The standing bound (relative L2 error of all weights <= 1e-2) after three optimizer steps over
    batches of 6, 6 and 4 rows, dropout 0.2, fp32 CPU executor."""
    g, c = _pair(spec, OPTS[opt], l2=l2)
    x, y = LM.data(g, 16, spec[2], seed=3)
    n = g.store.numel
    w0 = g.store.master[:n].cpu().numpy()
    wg, wc = _three_steps(g, c, x, y)
    print("%s %s: rel err %.3g, moved %.3g" % (spec, opt, _rel(wg, wc), _rel(wg, w0)))
    assert _rel(wg, wc) <= 1e-2 and _rel(wg, w0) > 1e-4
    lg, ag, _ = g._executor.read_metrics()
    lc, ac, _ = c._executor.read_metrics()
    assert abs(lg - lc) < 2e-2 * max(1.0, abs(lc)) and abs(ag - ac) <= 2.0 / 16
    names = [l.name for l in g._executor._plans[(6, "train")].launches]
    assert "loss_head" in names and "head" not in names


@pytest.mark.parametrize("spec", LM.MODELS, ids=["%s-%s-%s-%d" % s for s in LM.MODELS])
def test_grads_match_the_bf16_reference(spec, monkeypatch):
    """The standing one-step standard (per tensor: relative error <= 5e-2, cosine > 0.995) against the
    CPU executor with the GPU's bf16 storage points."""
    monkeypatch.setenv("INTML_TUNE", "ref_bf16=1")
    g, c = _pair(spec, lambda: optim.SGD(lr=0.0))
    assert c._executor.emulate_bf16
    x, y = LM.data(g, 48, spec[2])
    for m in (g, c):
        ex = m._executor
        d = ex.upload(x, y)
        ex.reset_metrics()
        ex.train_step(d, torch.arange(d.n, device=ex.device), 0, d.n)
    torch.cuda.synchronize()
    gg = g.store.grad[:g.store.numel].cpu().numpy()
    cg = c.store.grad[:c.store.numel].numpy()
    worst = []
    for s in g.store.specs:
        a, b = gg[s.offset:s.offset + s.numel], cg[s.offset:s.offset + s.numel]
        worst.append((_rel(a, b), float(np.dot(a, b) / max(np.linalg.norm(a) * np.linalg.norm(b), 1e-30)), s.name))
    print("%s: worst grad rel err %.3g (cos %.6f) at %s" % ((spec,) + max(worst)))
    for err, cos, nm in worst:
        assert err <= 5e-2 and cos > 0.995, "%s: grad rel err %.3g cos %.6f" % (nm, err, cos)
    lg, lc = g._executor.read_metrics()[0], c._executor.read_metrics()[0]
    assert abs(lg - lc) < 1e-3 * max(1.0, abs(lc)), (lg, lc)


# ------------------------------------------------------------------------------------ 3. structure
def _plan_names(m, bs=128, loss=None):
    x, y = _data(m, bs, seed=21) if loss is None else LM.data(m, bs, loss, seed=21)
    ex = m._executor
    d = ex.upload(x, y)
    ex.train_steps(d, torch.arange(d.n, device=ex.device), 0, bs, 1)
    ex.eval_step(d, 0, bs)
    ex.predict_step(d, 0, bs)
    torch.cuda.synchronize()
    assert np.isfinite(m.store.master[:m.store.numel].sum().item())
    return {mode: [l.name for l in ex._plans[(bs, mode)].launches] for mode in ("train", "eval", "predict")}


def _rpv(**kw):
    from cori_intml_examples_amd.apps import zoo
    set_random_seed(57)
    return zoo.rpv_cnn((64, 64, 3), conv_sizes=[16, 32, 64], fc_sizes=[128], dropout=0.2, optimizer="Adam", lr=1e-3,
                       device="cuda", **kw)


# the default steps, as tests/test_pooling_gpu.py::test_plans_without_new_pooling_are_unchanged pins them
RPV_TRAIN = ["conv_stack_fwd", "dense_fwd0", "head", "dense_bwd0", "wgrad_dgrad_conv2", "wgrad_dgrad_conv1",
             "wgrad_conv0", "reduce_b0"]
MNIST_TRAIN = ["conv_stack_fwd", "dense_fwd0", "head", "dense_bwd0", "wgrad_dgrad_conv1", "wgrad_conv0", "reduce_b0"]


def test_old_pairs_record_their_old_launch_lists(monkeypatch):
    monkeypatch.delenv("INTML_TUNE", raising=False)
    set_random_seed(57)
    ref = _plan_names(_build("rpv_bench", "cuda", opt="Adam", drop=0.2, cin=3, hw=64))
    assert ref["train"] == RPV_TRAIN
    assert _plan_names(_rpv(loss=None)) == ref and _plan_names(_rpv(loss="binary_crossentropy")) == ref
    assert _plan_names(_build("mnist_bench", "cuda", opt="Adam", drop=0.4, cin=1, hw=28))["train"] == MNIST_TRAIN
    # linear + mse keeps the first kernel as well (and its 0.0 accuracy)
    set_random_seed(57)
    m = LM.build("tiny", None, "mse", 3, optim.Adam(), "cuda")
    assert not m._executor.loss_head and "head" in _plan_names(m, 8, "mse")["train"]
    assert m._executor.read_metrics()[1] == 0.0


def test_loss_head_takes_the_unfused_head_structure(monkeypatch):
    """The launch list of a loss_head model is the fuse_head=0 list with head replaced by loss_head."""
    monkeypatch.setenv("INTML_TUNE", "fuse_head=0")
    un = _plan_names(_rpv())
    assert "dense_epi0" in un["train"] and "head" in un["train"]
    monkeypatch.delenv("INTML_TUNE")
    for loss in ("hinge", "mae"):
        got = _plan_names(_rpv(loss=loss), loss=loss)
        for mode in un:
            assert got[mode] == ["loss_head" if n == "head" else n for n in un[mode]], (loss, mode, got[mode])


def test_graph_replay_equals_single_steps_and_eager_launches(monkeypatch):
    res = []
    for chunks, graphs in (([1] * 8, "1"), ([8], "1"), ([1] * 8, "0")):
        monkeypatch.setenv("INTML_GRAPHS", graphs)
        set_random_seed(21)
        m = LM.build("odd", "sigmoid", "binary_crossentropy", 3, optim.Adam(decay=0.01), "cuda", drop=0.2)
        x, y = LM.data(m, 64, "binary_crossentropy", seed=4)
        ex = m._executor
        assert ex.use_graphs == (graphs == "1")
        d = ex.upload(x, y)
        perm = torch.randperm(d.n, generator=torch.Generator().manual_seed(3)).to(ex.device)
        ex.reset_metrics()
        pos = 0
        for k in chunks:
            ex.train_steps(d, perm, pos, 8, k)
            pos += 8 * k
        torch.cuda.synchronize()
        n = m.store.numel
        res.append(([m.store.master[:n].clone(), m.store.grad[:n].clone()] + [s.clone() for s in ex.optimizer_state()],
                    ex._metrics(), int(m.optimizer.iterations)))
    for other in res[1:]:
        for a, b in zip(res[0][0], other[0]):
            assert torch.equal(a, b)
        assert res[0][1] == other[1] and other[1][2] == 64 and other[2] == 8
    assert res[0][1][1] * 3 == round(res[0][1][1] * 3)        # element counts: thirds of a row


def test_fit_logs_the_accuracy_rule():
    """binary_accuracy over elements for the multi-label head, categorical_accuracy for a hinge head of
    3 columns: fit's val_acc equals the rule applied to predict()."""
    for act, loss, rule in (("sigmoid", "binary_crossentropy", "binary"), (None, "squared_hinge", "categorical")):
        set_random_seed(9)
        m = LM.build("tiny", act, loss, 3, optim.Adam(lr=0.01), "cuda")
        x, y = LM.data(m, 40, loss, seed=2)
        h = m.fit(x[:32], y[:32], batch_size=8, epochs=2, verbose=0, validation_data=(x[32:], y[32:]))
        assert sorted(h.history) == ["acc", "loss", "val_acc", "val_loss"]
        p = m.predict(x[32:], batch_size=8)
        want = (np.rint(p) == y[32:]).mean() if rule == "binary" else (p.argmax(1) == y[32:].argmax(1)).mean()
        assert abs(h.history["val_acc"][-1] - want) < 1e-6, (loss, h.history["val_acc"], want)
        ev = m.evaluate(x[32:], y[32:], batch_size=8, verbose=0)
        assert abs(ev[1] - h.history["val_acc"][-1]) < 1e-9 and abs(ev[0] - h.history["val_loss"][-1]) < 1e-6


def test_gpu_checkpoint_loads_on_cpu_and_continues(tmp_path):
    set_random_seed(8)
    m = LM.build("odd", "softmax", "kld", 4, optim.Adam(lr=0.01), "cuda", drop=0.1)
    x, y = LM.data(m, 48, "kld", seed=1)
    m.fit(x[:32], y[:32], batch_size=8, epochs=1, verbose=0, shuffle=False)
    p = str(tmp_path / "g.h5")
    m.save(p)
    c = load_model(p, device="cpu")
    assert c._plan.head.loss == "kld" and c.optimizer.iterations == m.optimizer.iterations == 4
    for a, b in zip(m.get_weights(), c.get_weights()):
        np.testing.assert_array_equal(a, b)
    assert np.abs(c.predict(x[32:], batch_size=16) - m.predict(x[32:], batch_size=16)).max() < 2e-2
    n = c.store.numel
    lc, lg = c.train_on_batch(x[32:], y[32:]), m.train_on_batch(x[32:], y[32:])
    torch.cuda.synchronize()
    assert abs(lc[0] - lg[0]) < 2e-2 * max(1.0, lg[0])
    assert _rel(m.store.master[:n].cpu().numpy(), c.store.master[:n].numpy()) < 1e-2


def test_data_parallel_step_at_one_rank(tmp_path):
    out = tmp_path / "dp.json"
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("WORLD_SIZE", "RANK", "INTML_DP_BACKEND", "INTML_COMM", "INTML_XGMI", "INTML_TUNE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "loss_dp_worker_gpu.py"), str(out)],
                       env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rep = json.load(open(out))
    print(json.dumps(rep, indent=1))
    assert rep["native"] and rep["moved"] > 1e-4, rep
    assert "loss_head" in rep["base_launches"] and "head" not in rep["base_launches"]
    for mode in ("captured", "segmented"):
        c = rep[mode]
        assert c["reducer"] == "NativeGradReducer" and c["comm_in_graph"] == (mode == "captured"), c
        assert "loss_head" in c["launches"]
        assert c["iterations"] == 4 and all(c["identical"]), (mode, c)
