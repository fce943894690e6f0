"""ROC / AUC, purity, efficiency and weighted metrics on the GPU: the roc.hip kernels alone against the
numpy twin (bit for bit: histograms, confusion sums, invalid counter; guards; determinism; the
launchers' checks; roc_finish against Python-integer arithmetic), and whole models (evaluate against
metrics.roc_curve on the model's own predict output and against the float64 oracle, fit logs, graph
replay, the prologue-free and prologue plans, unchanged plans and weights, data parallel at one rank)."""
import json
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

from cori_intml_examples_amd import metrics as MT
from cori_intml_examples_amd import optim
from cori_intml_examples_amd.models import Conv2D, Dense, Dropout, Flatten, MaxPooling2D, Sequential
from cori_intml_examples_amd.utils import set_random_seed

from helpers import roc_oracle as O
from test_hip_model import _build, _data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
GUARD = 64
EDGES = np.array([0.0, -0.0, 1e-45, np.nextafter(np.float32(0.5), np.float32(0)), 0.5,
                  np.nextafter(np.float32(0.5), np.float32(1)), np.nextafter(np.float32(1), np.float32(0)), 1.0,
                  np.nan, -1e-9, np.nextafter(np.float32(1), np.float32(2))], np.float32)


def _K():
    from cori_intml_examples_amd.ops.hip import kernels
    return kernels()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Buf:
    """A payload behind and ahead of ``GUARD`` sentinel elements; get() checks both guard regions."""

    def __init__(self, values, dtype):
        v = np.ascontiguousarray(values, dtype=dtype).reshape(-1)
        sent = np.array(-7 if np.issubdtype(np.dtype(dtype), np.integer) else np.nan, dtype)
        self.init = np.concatenate([np.full(GUARD, sent, dtype), v, np.full(GUARD, sent, dtype)])
        self.n = v.size
        self.t = torch.from_numpy(self.init.copy()).cuda()
        self.ptr = self.t.data_ptr() + GUARD * self.init.itemsize

    def refill(self):
        self.t.copy_(torch.from_numpy(self.init.copy()))

    def get(self):
        v = self.t.cpu().numpy()
        ib = self.init.view(np.uint8).reshape(len(self.init), -1)
        vb = v.view(np.uint8).reshape(len(v), -1)
        assert np.array_equal(vb[:GUARD], ib[:GUARD]) and np.array_equal(vb[GUARD + self.n:], ib[GUARD + self.n:])
        return v[GUARD:GUARD + self.n]


class Case:
    """One roc_accum problem on the device: probs [M][N], targets, optional weights, optionally
    addressed through yidx into a data set bound in a StepState."""

    def __init__(self, K, probs, y, w=None, via_yidx=False, seed=0):
        self.K = K
        self.p = np.ascontiguousarray(probs, np.float32)
        self.M, self.N = self.p.shape
        self.softmax = self.N > 1
        self.y, self.w = np.ascontiguousarray(y, np.float32).reshape(self.M, self.N), w
        self.k = MT.weight_shift(float(np.asarray(w, np.float32).astype(np.float64).sum())) if w is not None else 0
        words = K.ROC_HDR + 2 * self.N * K.ROC_BLOCK
        hdr = np.zeros(words, np.int64)
        hdr[0] = self.k
        hdr[1:2].view(np.float64)[0] = np.ldexp(1.0, self.k)
        self.state = Buf(hdr, np.int64)
        self.res = Buf(np.zeros(2 * self.N * K.ROC_RES_WORDS, np.int64), np.int64)
        self.pb = Buf(self.p, np.float32)
        a = self.a = K.RocArgs()
        a.probs, a.M, a.N, a.softmax = self.pb.ptr, self.M, self.N, int(self.softmax)
        a.state, a.res = self.state.ptr, self.res.ptr
        self.keep = []
        if via_yidx:
            # a data set of 2M + 3 rows; the batch's rows are a random selection of them
            rs = np.random.RandomState(seed + 77)
            nd = 2 * self.M + 3
            idx = rs.permutation(nd)[:self.M].astype(np.int32)
            dy = rs.rand(nd, self.N).astype(np.float32)
            dy[idx] = self.y
            dw = rs.rand(nd).astype(np.float32)
            if w is not None:
                dw[idx] = w
            ty, tw, ti = Buf(dy, np.float32), Buf(dw, np.float32), Buf(idx, np.int32)
            st = torch.zeros(K.STEP_STATE_BYTES, dtype=torch.uint8, device="cuda")
            st.view(torch.int64)[K.STEP_STATE_DATA_OFFSET // 8 + 1] = ty.ptr
            st.view(torch.int32)[K.STEP_STATE_DATAN_OFFSET // 4] = nd
            st.view(torch.int32)[K.STEP_STATE_DATAN_OFFSET // 4 + 2] = self.N
            if w is not None:
                st.view(torch.int64)[K.STEP_STATE_DATAW_OFFSET // 8] = tw.ptr
            a.yidx, a.st = ti.ptr, st.data_ptr()
            self.keep += [ty, tw, ti, st]
        else:
            ty = Buf(self.y, np.float32)
            a.y = ty.ptr
            self.keep.append(ty)
            if w is not None:
                tw = Buf(w, np.float32)
                a.wb = tw.ptr
                self.keep.append(tw)
        a.weighted = int(w is not None)

    def launch(self):
        self.K.roc_accum(self.a, _stream())
        torch.cuda.synchronize()

    def blocks(self):
        """(pos, neg, tail) [2][N][..] of the device state, guards and header checked."""
        K = self.K
        v = self.state.get()
        assert v[0] == self.k and np.all(v[2:K.ROC_HDR] == 0)
        b = v[K.ROC_HDR:].reshape(2, self.N, K.ROC_BLOCK)
        for buf in [self.pb] + [k for k in self.keep if isinstance(k, Buf)]:
            buf.get()
        return b[:, :, :K.ROC_BINS], b[:, :, K.ROC_BINS:2 * K.ROC_BINS], b[:, :, 2 * K.ROC_BINS:]

    def twin(self, times=1):
        st = MT.RocState(self.N, self.softmax, self.k)
        for _ in range(times):
            st.accumulate(self.p, self.y, self.w)
        return st.pos, st.neg, st.tail

    def check(self, times=1):
        got, want = self.blocks(), self.twin(times)
        for g, w_, name in zip(got, want, ("pos", "neg", "tail")):
            assert np.array_equal(g, w_), (name, np.argwhere(g != w_)[:5])
        if self.w is None:
            assert not got[0][1].any() and not got[1][1].any() and not got[2][1].any()


def _scores(rs, M, N):
    if N == 1:
        p = rs.rand(M, 1).astype(np.float32)
        p[rs.rand(M) < 0.2] = 1.0                      # a saturated share: lanes that meet in one bin
        y = (rs.rand(M, 1) < 0.4).astype(np.float32)
        return p, y
    z = rs.randn(M, N).astype(np.float32) * 3
    e = np.exp(z - z.max(1, keepdims=True))
    p = (e / e.sum(1, keepdims=True)).astype(np.float32)
    y = np.eye(N, dtype=np.float32)[rs.randint(0, N, M)]
    return p, y


def _weights(rs, M):
    """1e-6 .. 1e8 (log-uniform) with zeros."""
    w = (10.0 ** rs.uniform(-6, 8, M)).astype(np.float32)
    w[rs.rand(M) < 0.15] = 0.0
    return w


# ------------------------------------------------------------------------------------ 1. roc_accum
@pytest.mark.parametrize("N", [1, 2, 3, 16])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 257])
def test_accum_equals_the_numpy_twin(M, N):
    K = _K()
    rs = np.random.RandomState(1000 * M + N)
    p, y = _scores(rs, M, N)
    for w, via in ((None, False), (_weights(rs, M), False), (None, True), (_weights(rs, M), True)):
        c = Case(K, p, y, w, via_yidx=via, seed=M + N)
        c.launch()
        c.check()


@pytest.mark.parametrize("weighted", [False, True])
def test_accum_one_bin_distinct_bins_and_edge_scores(weighted):
    K = _K()
    rs = np.random.RandomState(5)
    M = 257
    y = (rs.rand(M, 1) < 0.5).astype(np.float32)
    w = _weights(rs, M) if weighted else None
    one = Case(K, np.ones((M, 1), np.float32), y, w)                       # every row in bin 2H
    one.launch()
    one.check()
    pos, neg, tail = one.blocks()
    assert pos[0, 0, 2 * MT.ROC_H] + neg[0, 0, 2 * MT.ROC_H] == M and np.count_nonzero(pos[0, 0]) == 1
    low = MT.bin_lower_edge(np.arange(0, MT.ROC_H, 61)[:M])               # every row in a bin of its own
    assert len(np.unique(MT.score_bin(low))) == M
    dist = Case(K, low.reshape(M, 1), y, w)
    dist.launch()
    dist.check()
    pos, neg, _ = dist.blocks()
    assert (pos[0, 0] + neg[0, 0]).max() == 1
    ye = (np.arange(2 * len(EDGES)) % 2).astype(np.float32).reshape(-1, 1)  # every edge score in both classes
    edge = Case(K, np.repeat(EDGES, 2).reshape(-1, 1), ye, None if w is None else np.full(len(ye), 0.75, np.float32))
    edge.launch()
    edge.check()
    pos, neg, tail = edge.blocks()
    assert tail[0, 0, MT.T_INVALID] == 6 and pos[0, 0].sum() + neg[0, 0].sum() == 2 * len(EDGES) - 6
    assert pos[0, 0, 0] == 3 and pos[0, 0, MT.ROC_H] == 1 and pos[0, 0, 2 * MT.ROC_H] == 1


def test_accum_is_deterministic_and_additive():
    K = _K()
    rs = np.random.RandomState(9)
    p, y = _scores(rs, 257, 3)
    w = _weights(rs, 257)
    c = Case(K, p, y, w, via_yidx=True)
    seen = []
    for _ in range(4):
        c.state.refill()
        c.launch()
        seen.append(c.state.get().copy())
    assert all(np.array_equal(seen[0], s) for s in seen[1:])
    c.launch()                       # a second launch into the same state: twice the integers
    c.launch()
    c.check(times=3)
    # several launches over the pieces == one launch over the concatenation (the same k)
    whole = Case(K, p, y, w)
    whole.launch()
    parts = None
    for lo, hi in ((0, 64), (64, 65), (65, 257)):
        part = Case(K, p[lo:hi], y[lo:hi], w[lo:hi])
        if parts is not None:
            part.state.t.copy_(parts.state.t)
        hdr = part.state.t[GUARD:GUARD + 2]
        hdr[0] = whole.k
        hdr[1:2].view(torch.float64)[0] = float(np.ldexp(1.0, whole.k))
        part.launch()
        parts = part
    assert np.array_equal(parts.state.get(), whole.state.get())


def test_launcher_host_checks():
    K = _K()
    rs = np.random.RandomState(2)
    p, y = _scores(rs, 8, 1)
    good = Case(K, p, y)

    def bad(**kw):
        c = Case(K, p, y)
        for k, v in kw.items():
            setattr(c.a, k, v)
        with pytest.raises(ValueError):
            K.roc_accum(c.a, _stream())
        torch.cuda.synchronize()
        assert not c.state.get()[K.ROC_HDR:].any()

    bad(M=0)
    bad(N=0)
    bad(N=17)
    bad(N=2)               # a sigmoid head has one column
    bad(softmax=1)         # a softmax head has at least two
    bad(probs=0)
    bad(state=0)
    bad(y=0)
    bad(yidx=good.pb.ptr)  # yidx without a StepState
    f = Case(K, p, y)
    f.a.res = 0
    with pytest.raises(ValueError):
        K.roc_finish(f.a, _stream())
    f.a.res, f.a.state = f.res.ptr, 0
    with pytest.raises(ValueError):
        K.roc_finish(f.a, _stream())
    good.launch()
    good.check()


# ------------------------------------------------------------------------------------ 2. roc_finish
def test_finish_against_integer_arithmetic():
    """auc = sum_b neg[b] (2 pos_above[b] + pos[b]) / (2 P N): two int-to-double conversions, one product,
    at most ROC_BINS additions of non-negative terms and one division -> 4 * ROC_BINS * 2^-53 relative."""
    K = _K()
    rs = np.random.RandomState(11)
    N = 3
    c = Case(K, *_scores(rs, 4, N))
    words = K.ROC_HDR + 2 * N * K.ROC_BLOCK
    st = np.zeros(words, np.int64)
    blk = st[K.ROC_HDR:].reshape(2, N, K.ROC_BLOCK)
    B = K.ROC_BINS
    blk[0, 0, :B] = rs.randint(0, 1 << 40, B)                # dense, large counts
    blk[0, 0, B:2 * B] = rs.randint(0, 1 << 40, B)
    sparse = rs.rand(2, B) < 0.01                            # sparse
    blk[0, 1, :B] = sparse[0] * rs.randint(1, 1000, B)
    blk[0, 1, B:2 * B] = sparse[1] * rs.randint(1, 1000, B)
    blk[0, 2, :B] = rs.randint(0, 5, B)                      # an empty negative class -> NaN
    blk[1, 0, 100] = 7                                       # perfectly separated: auc 1
    blk[1, 0, B + 50] = 9
    blk[1, 1, 50] = 7                                        # ... and inverted: auc 0
    blk[1, 1, B + 100] = 9
    blk[1, 2, 2 * K.ROC_H] = 1 << 60                         # the largest sums, one shared bin: 0.5
    blk[1, 2, B + 2 * K.ROC_H] = 1 << 60
    blk[:, :, 2 * B:] = rs.randint(0, 1 << 50, (2, N, K.ROC_TAIL))
    c.state.t[GUARD:GUARD + words] = torch.from_numpy(st).cuda()
    K.roc_finish(c.a, _stream())
    torch.cuda.synchronize()
    r = c.res.get().reshape(2, N, K.ROC_RES_WORDS)
    c.state.get()
    tol = 4 * K.ROC_BINS * 2.0 ** -53
    for s in range(2):
        for n in range(N):
            pos, neg = [int(v) for v in blk[s, n, :B]], [int(v) for v in blk[s, n, B:2 * B]]
            P, Nn = sum(pos), sum(neg)
            got = float(r[s, n, :1].view(np.float64)[0])
            assert r[s, n, 1] == P and r[s, n, 2] == Nn
            assert np.array_equal(r[s, n, 3:3 + K.ROC_TAIL], blk[s, n, 2 * B:])
            if P == 0 or Nn == 0:
                assert np.isnan(got)
                continue
            above, num = 0, 0
            for b in range(B - 1, -1, -1):
                num += neg[b] * (2 * above + pos[b])
                above += pos[b]
            want = Fraction(num, 2 * P * Nn)
            err = abs(Fraction(got) - want)
            print("set %d class %d: auc %.17g, |err| %.3g (bound %.3g relative)" % (s, n, got, float(err), tol))
            assert err <= want * Fraction(tol), (s, n, got, float(want))
            assert abs(MT.hist_auc(blk[s, n, :B], blk[s, n, B:2 * B]) - float(want)) <= 2.0 ** -52 * float(want)
    assert float(r[1, 0, :1].view(np.float64)[0]) == 1.0 and float(r[1, 1, :1].view(np.float64)[0]) == 0.0
    assert float(r[1, 2, :1].view(np.float64)[0]) == 0.5


# ------------------------------------------------------------------------------------ 3. models
NEW = dict(metrics=["accuracy", "auc", "purity", "efficiency"], weighted_metrics=["acc", "auc", "precision", "recall"])
NEW3 = dict(metrics=["accuracy", "auc"], weighted_metrics=["accuracy", "auc"])


def _binary(device="cuda", opt=None, seed=31, **metrics):
    """The RPV-shaped tiny model of tests/test_hip_model.py (16x16x3, dropout 0.2), re-compiled with the metrics."""
    set_random_seed(seed)
    m = _build("rpv", device, drop=0.2, cin=3, hw=16)
    m.compile(optimizer=opt or optim.Adam(), loss="binary_crossentropy", **(metrics or dict(metrics=["accuracy"])))
    return m


def _three_class(device="cuda", seed=32, **metrics):
    set_random_seed(seed)
    m = Sequential(device=device)
    m.add(Conv2D(8, (3, 3), activation="relu", input_shape=(16, 16, 1)))
    m.add(MaxPooling2D((2, 2)))
    m.add(Dropout(0.2))
    m.add(Flatten())
    m.add(Dense(32, activation="relu"))
    m.add(Dropout(0.2))
    m.add(Dense(3, activation="softmax"))
    m.compile(optimizer=optim.Adam(), loss="categorical_crossentropy", **(metrics or dict(metrics=["accuracy"])))
    return m


def _sample_weights(n, seed=3):
    w = np.random.RandomState(seed).uniform(0.1, 5.0, n).astype(np.float32)
    w[::5] = 0.0
    return w


def _same(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


@pytest.mark.parametrize("weighted", [False, True])
def test_binary_evaluate_equals_roc_curve_of_predict(weighted):
    """Batches of 6, 6 and a ragged 4: every metric equals metrics.roc_curve on the model's own predict
    output exactly (the same integers), and the float64 oracle within its bound B."""
    m = _binary(**NEW)
    x, y = _data(m, 16, seed=7)
    w = _sample_weights(16) if weighted else None
    vals = dict(zip(m.metrics_names, m.evaluate(x, y, batch_size=6, verbose=0, sample_weight=w)))
    assert list(vals) == ["loss", "acc", "auc", "purity", "efficiency", "weighted_acc", "weighted_auc",
                          "weighted_purity", "weighted_efficiency"]
    p = m.predict(x, batch_size=6)[:, 0]
    for prefix, ww in (("", None), ("weighted_", w)):
        rc = MT.roc_curve(y, p, ww)
        print(prefix, vals[prefix + "auc"], rc)
        assert rc.n_invalid == 0
        assert _same(vals[prefix + "auc"], rc.auc) and vals[prefix + "acc"] == rc.accuracy
        assert vals[prefix + "purity"] == rc.purity and vals[prefix + "efficiency"] == rc.efficiency
        bound = O.hist_bound(y, p, MT.score_bin(p), ww)
        assert abs(rc.auc - O.exact_auc(y, p, ww)) <= bound + 1e-12
        s = O.summary(y, p, ww)
        for k in ("acc", "purity", "efficiency"):
            assert abs(vals[prefix + k] - s[k]) <= 16 * 2.0 ** -50 * max(s[k], 1e-300)
    er = m.evaluate_roc(x, y, sample_weight=w, batch_size=6)
    assert _same(er.auc, vals["weighted_auc"]) and er.fpr[0] == er.tpr[0] == 0.0 and np.isinf(er.thresholds[0])
    assert er.fpr[-1] == er.tpr[-1] == 1.0


@pytest.mark.parametrize("weighted", [False, True])
def test_three_class_evaluate_equals_roc_curve_of_predict(weighted):
    m = _three_class(**NEW3)
    x, y = _data(m, 16, seed=8)
    w = _sample_weights(16) if weighted else None
    vals = dict(zip(m.metrics_names, m.evaluate(x, y, batch_size=6, verbose=0, sample_weight=w)))
    assert list(vals) == ["loss", "acc", "auc", "weighted_acc", "weighted_auc"]
    p = m.predict(x, batch_size=6)
    cls = y.argmax(1)
    for prefix, ww in (("", None), ("weighted_", w)):
        curves = MT.per_class_curves(y, p, ww)
        aucs = [c.auc for c in curves if not np.isnan(c.auc)]
        assert aucs and vals[prefix + "auc"] == sum(aucs) / len(aucs)
        for n, c in enumerate(curves):
            if not np.isnan(c.auc):
                bound = O.hist_bound(cls == n, p[:, n], MT.score_bin(p[:, n]), ww)
                assert abs(c.auc - O.exact_auc(cls == n, p[:, n], ww)) <= bound + 1e-12
        wv = np.ones(16) if ww is None else ww.astype(np.float64)
        acc = float((wv * (MT.first_argmax(p) == cls)).sum() / wv.sum())
        assert abs(vals[prefix + "acc"] - acc) <= 16 * 2.0 ** -50
    assert vals["acc"] == float((MT.first_argmax(p) == cls).mean())
    assert len(m.evaluate_roc(x, y, sample_weight=w)) == 3


def test_fit_logs_every_key_and_weights_are_unchanged_by_the_metrics():
    """Two epochs with validation: every name and its val_ twin; the trained weights are bit-identical
    to the same model compiled without the metrics."""
    res = []
    for metrics in (NEW, {}):
        m = _binary(**metrics)
        x, y = _data(m, 40, seed=9)
        w = _sample_weights(40)
        h = m.fit(x[:24], y[:24], batch_size=8, epochs=2, verbose=0, shuffle=False, sample_weight=w[:24],
                  validation_data=(x[24:], y[24:], w[24:]))
        torch.cuda.synchronize()
        res.append((m.store.master[:m.store.numel].clone(), h.history, m))
    assert torch.equal(res[0][0], res[1][0])
    names = res[0][2].metrics_names
    assert sorted(res[0][1]) == sorted(names + ["val_" + n for n in names])
    assert all(len(v) == 2 for v in res[0][1].values())
    assert res[0][1]["loss"] == res[1][1]["loss"] and res[0][1]["val_acc"] == res[1][1]["val_acc"]
    m = res[0][2]
    p = m.predict(x[24:], batch_size=8)[:, 0]
    assert _same(res[0][1]["val_weighted_auc"][-1], MT.roc_curve(y[24:], p, w[24:]).auc)
    assert _same(res[0][1]["val_auc"][-1], MT.roc_curve(y[24:], p).auc)


def _train_ints(m, chunks, x, y, w):
    ex = m._executor
    d = ex.upload(x, y, w)
    perm = torch.randperm(d.n, generator=torch.Generator().manual_seed(3)).to(ex.device)
    ex.reset_metrics()
    pos = 0
    for k in chunks:
        ex.train_steps(d, perm, pos, 8, k)
        pos += 8 * k
    torch.cuda.synchronize()
    vals = ex.extra_metrics()
    return [a.copy() for a in ex.roc_histograms()], m.store.master[:m.store.numel].clone(), vals


def test_graph_replay_eager_and_single_steps_give_the_same_integers(monkeypatch):
    """8 steps in one graph, 8 single-step replays and eager launches (INTML_GRAPHS=0): the same ROC
    integers and the same weights."""
    res = []
    for graphs, chunks in (("1", [1] * 8), ("1", [8]), ("0", [1] * 8)):
        monkeypatch.setenv("INTML_GRAPHS", graphs)
        m = _binary(**NEW)
        assert m._executor.use_graphs == (graphs == "1")
        x, y = _data(m, 64, seed=4)
        res.append(_train_ints(m, chunks, x, y, _sample_weights(64)))
    for other in res[1:]:
        for a, b in zip(res[0][0], other[0]):
            assert np.array_equal(a, b)
        assert torch.equal(res[0][1], other[1])
        assert all(_same(res[0][2][k], other[2][k]) for k in res[0][2])
    pos, neg, tail = res[0][0]
    assert pos[0].sum() + neg[0].sum() == 64 and tail[0, 0, :4].sum() == 64 and pos[1].sum() > 0


@pytest.mark.parametrize("build", [_binary, _three_class])
def test_prologue_free_and_prologue_plans_agree(build, monkeypatch):
    res = []
    for tv in ("", "pro_free=0"):
        monkeypatch.setenv("INTML_TUNE", tv)
        m = build(**(NEW if build is _binary else NEW3))
        x, y = _data(m, 16, seed=6)
        w = _sample_weights(16)
        ex = m._executor
        vals = m.evaluate(x, y, batch_size=6, verbose=0, sample_weight=w)
        ev = [a.copy() for a in ex.roc_histograms()]
        d = ex.upload(x, y, w)
        ex.reset_metrics()
        ex.train_step(d, torch.arange(16, device=ex.device), 0, 16)
        torch.cuda.synchronize()
        tr = [a.copy() for a in ex.roc_histograms()]
        plan = ex._plans[(16, "train", "w")]
        names = [l.name for l in plan.launches]
        assert not plan.pro_free if tv else (plan.pro_free or build is not _binary)
        assert names.count("roc_accum") == 1 and names[names.index("head") + 1] == "roc_accum"
        roc = plan.launches[names.index("roc_accum")].args["roc"]
        assert (roc.yidx != 0) == plan.pro_free and roc.weighted == 1
        res.append((vals, ev, tr))
    assert res[0][0][1:] == res[1][0][1:]
    for a, b in zip(res[0][1] + res[0][2], res[1][1] + res[1][2]):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------ 4. plans
def _plan_names(m, bs=128):
    x, y = _data(m, bs, seed=21)
    ex = m._executor
    d = ex.upload(x, y)
    ex.train_steps(d, torch.arange(d.n, device=ex.device), 0, bs, 1)
    ex.eval_step(d, 0, bs)
    ex.predict_step(d, 0, bs)
    torch.cuda.synchronize()
    assert np.isfinite(m.store.master[:m.store.numel].sum().item())
    return {mode: [l.name for l in ex._plans[(bs, mode)].launches] for mode in ("train", "eval", "predict")}


# the launch lists recorded without the feature (tests/test_pooling_gpu.py pins the same)
RPV_TRAIN = ["conv_stack_fwd", "dense_fwd0", "head", "dense_bwd0", "wgrad_dgrad_conv2", "wgrad_dgrad_conv1",
             "wgrad_conv0", "reduce_b0"]
MNIST_TRAIN = ["conv_stack_fwd", "dense_fwd0", "head", "dense_bwd0", "wgrad_dgrad_conv1", "wgrad_conv0", "reduce_b0"]


def test_plans_without_roc_metrics_are_unchanged(monkeypatch):
    monkeypatch.delenv("INTML_TUNE", raising=False)
    set_random_seed(57)
    rpv = _build("rpv_bench", "cuda", opt="Adam", drop=0.2, cin=3, hw=64)
    ref = _plan_names(rpv)
    print(ref)
    assert ref["train"] == RPV_TRAIN and len(ref["train"]) == 8
    assert ref["eval"] == ref["predict"] and ref["eval"][0] == "conv_stack_fwd" and ref["eval"][-1] == "head"
    ex = rpv._executor
    assert not ex.roc_on and ex.roc_state is None
    assert all(p.probs is None for k, p in ex._plans.items() if k[1] != "predict")
    mn = _plan_names(_build("mnist_bench", "cuda", opt="Adam", drop=0.4, cin=1, hw=28))
    assert mn["train"] == MNIST_TRAIN and mn["eval"] == mn["predict"]
    assert not [n for names in (ref, mn) for mode in names for n in names[mode] if "roc" in n]
    # with a metric: exactly one roc_accum, directly behind the head; never in a predict plan
    from cori_intml_examples_amd.apps import zoo
    set_random_seed(57)
    on = _plan_names(zoo.rpv_cnn((64, 64, 3), conv_sizes=[16, 32, 64], fc_sizes=[128], dropout=0.2, optimizer="Adam",
                                 lr=1e-3, device="cuda", metrics=["accuracy", "auc"]))
    assert on["train"] == RPV_TRAIN[:3] + ["roc_accum"] + RPV_TRAIN[3:]
    assert on["eval"] == ref["eval"] + ["roc_accum"] and on["predict"] == ref["predict"]
    set_random_seed(57)
    on3 = _plan_names(zoo.mnist_cnn(32, 64, 128, dropout=0.4, optimizer="Adam", lr=1e-3, input_shape=(28, 28, 1),
                                    device="cuda", weighted_metrics=["accuracy"]))
    assert on3["train"] == MNIST_TRAIN[:3] + ["roc_accum"] + MNIST_TRAIN[3:]
    assert on3["eval"] == mn["eval"] + ["roc_accum"] and on3["predict"] == mn["predict"]


# ------------------------------------------------------------------------------------ 5. data parallel
def test_data_parallel_step_at_one_rank(tmp_path):
    out = tmp_path / "dp.json"
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("WORLD_SIZE", "RANK", "INTML_DP_BACKEND", "INTML_COMM", "INTML_XGMI", "INTML_TUNE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "roc_dp_worker_gpu.py"), str(out)],
                       env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rep = json.load(open(out))
    print(json.dumps(rep, indent=1))
    assert rep["native"] and rep["moved"] > 1e-4, rep
    assert rep["base_launches"].count("roc_accum") == 1
    for mode in ("captured", "segmented"):
        c = rep[mode]
        assert c["reducer"] == "NativeGradReducer" and c["comm_in_graph"] == (mode == "captured"), c
        assert c["launches"].count("roc_accum") == 1 and c["launches"][c["launches"].index("head") + 1] == "roc_accum"
        assert c["iterations"] == 4 and all(c["identical"]), (mode, c)
        assert c["val_auc"] == rep["base_val_auc"] and c["val_weighted_auc"] == rep["base_val_weighted_auc"], (mode, c)
        assert c["auc"] == rep["base_auc"]
