"""Keras L1 / L2 weight regularizers on the GPU: weight_reg_kernel alone against the float64
oracle of tests/helpers/reg_oracle.py (NaN-padded buffers, unaligned bases, ragged and adjacent
ranges, gaps, zeros, bit-level gradient, error-bounded penalty, determinism, the metric words),
the regularized step at bit level against an unregularized twin, end to end against the CPU
reference executor, graph replay, plan gating, the data-parallel step at one rank and a
GPU -> CPU checkpoint."""
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from cori_intml_examples_amd import optim
from cori_intml_examples_amd.io.datasets import synthetic_rpv
from cori_intml_examples_amd.io.keras_h5 import load_model
from cori_intml_examples_amd.utils import set_random_seed

from helpers import clip_oracle as C
from helpers import reg_models as M
from helpers import reg_oracle as G
from test_hip_model import _build, _data, _rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

KINDS = {"SGD": lambda **kw: optim.SGD(lr=0.01, momentum=0.9, **kw), "Adam": optim.Adam, "Nadam": optim.Nadam,
         "Adadelta": optim.Adadelta, "Adamax": optim.Adamax, "AMSGrad": lambda **kw: optim.Adam(amsgrad=True, **kw)}
UNFUSED = "fuse_optim=0,early_reduce=0"
# From a dry run of the CPU executor on these models and batches (seed 1234, _data seed 3, dropout
# 0.2): the global norm of the regularized gradient over the three steps is 0.42 .. 0.50 ("tiny")
# and 0.85 .. 2.7 ("odd"), so clipnorm 0.1 fires on every step (the test asserts it from the oracle).
CLIPNORM = 0.1
PAD = 8                                 # floats of NaN padding in front of the buffers' payload


def _K():
    from cori_intml_examples_amd.ops.hip import kernels
    return kernels()


def _f32(v):
    return float(np.float32(v))


# ------------------------------------------------------------------------------------ 1. the kernel alone
def _chain(K, nparts):
    """The longest chain of additions of weight_reg_kernel: the term's own sum l1 |w| + l2 w^2 (1),
    per thread REG_VEC_PER_THREAD groups of ((t0 + t1) + (t2 + t3)) added to the accumulator
    (3 each), the workgroup tree (6 butterfly levels + 3 adds of the 4 wave sums), then the
    finish: ceil(partials / 256) adds per thread and the same tree.  The two products of a term
    (w * w, then l2 * that) are the "+ 2" of the bound."""
    tree = 6 + 3
    return 1 + 3 * K.REG_VEC_PER_THREAD + tree + math.ceil(nparts / K.REG_THREADS) + tree


def _range_sets(K):
    ch = K.REG_CHUNK
    a, b = (_f32(1e-3), _f32(1e-2)), (_f32(0.25), _f32(0.5))
    sets = {"len%d" % n: [(3, 3 + n) + a] for n in (1, 3, 4, 1023, 1024, 1025, ch - 1, ch + 1)}
    sets["len4_aligned"] = [(4, 8) + a]
    # adjacent ranges with different coefficients, borders that are no multiples of 4
    sets["adjacent"] = [(0, 7) + a, (7, 1030) + b, (1030, 1033, _f32(0.125), 0.0), (1033, ch + 50, 0.0, _f32(0.03))]
    # l1 only, l2 only, a gap between them
    sets["gap"] = [(2, 501, _f32(0.01), 0.0), (777, 3 * ch + 5, 0.0, _f32(0.02))]
    # whole chunks that no range touches get no workgroup
    sets["far"] = [(1, 10) + a, (5 * ch + 3, 5 * ch + 900) + b, (9 * ch - 2, 9 * ch + 2, _f32(0.5), _f32(0.5))]
    return sets


def _make(ranges, off, seed=0, zeros=True):
    """(p, g) host buffers: NaN padding around [PAD + off, PAD + off + n); p is NaN outside the
    ranges too (a read there poisons P), g random there (a write there shows)."""
    n = max(hi for _, hi, _, _ in ranges) + 5
    gen = torch.Generator().manual_seed(seed)
    p = torch.full((PAD + off + n + 64,), float("nan"), dtype=torch.float32)
    g = torch.full((PAD + off + n + 64,), float("nan"), dtype=torch.float32)
    g[PAD + off:PAD + off + n] = torch.randn(n, generator=gen)
    for lo, hi, _, _ in ranges:
        m = hi - lo
        w = torch.randn(m, generator=gen) * 10.0 ** torch.empty(m).uniform_(-3, 0.5, generator=gen)
        if zeros and m >= 8:                          # exact zeros and negative zeros in w
            w[0], w[m // 2], w[m - 1] = 0.0, -0.0, 0.0
        p[PAD + off + lo:PAD + off + hi] = w
    return p, g, n


def _args(K, pb, gb, off, n, ranges, state, partials, st=None, rows=0.0, add_grad=1):
    a = K.RegArgs()
    a.p = pb.data_ptr() + 4 * (PAD + off)
    a.g = gb.data_ptr() + 4 * (PAD + off)
    a.n = n
    a.set_ranges([tuple(r) for r in ranges])
    a.rows, a.add_grad = float(rows), int(add_grad)
    a.partials, a.npartials = partials.data_ptr(), partials.numel()
    a.state = state.data_ptr()
    if st is not None:
        a.st = st.data_ptr()
    return a


def _run(K, a, state):
    K.weight_reg(a, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    s = state.cpu()
    assert int(s.view(torch.int32)[K.REG_TICKET]) == 0           # the last workgroup reset the ticket
    return np.float32(s[K.REG_PENALTY].item())


def _chunks(K, ranges, mis):
    return sorted({c for lo, hi, _, _ in ranges for c in range((lo + mis) // K.REG_CHUNK, (hi + mis - 1) // K.REG_CHUNK + 1)})


def _bits(t):
    return t.cpu().view(torch.int32).numpy()


@pytest.mark.parametrize("off", [0, 1, 3])
def test_kernel_matches_the_oracle(off):
    """Gradient bit for bit (NumPy float32, the kernel's operation order), nothing outside the
    ranges read into P or written, P within (L + 2) * 2^-24 relative of float64 (all terms are
    non-negative: the addition-chain bound; L: _chain), add_grad = 0 leaves g alone and gives the
    same P bits."""
    K = _K()
    dev = torch.device("cuda")
    state = torch.zeros(K.REG_STATE_WORDS, dtype=torch.float32, device=dev)
    for name, ranges in _range_sets(K).items():
        p, g, n = _make(ranges, off, seed=len(name))
        pb, gb = p.to(dev), g.to(dev)
        assert pb.data_ptr() % 16 == 0 and gb.data_ptr() % 16 == 0
        chunks = _chunks(K, ranges, (PAD + off) % 4)
        partials = torch.full((len(chunks) + 2,), float("nan"), dtype=torch.float32, device=dev)
        a = _args(K, pb, gb, off, n, ranges, state, partials)
        assert K.reg_blocks(a) == len(chunks), (name, off, chunks)
        assert [r[:2] for r in a.ranges()] == [r[:2] for r in ranges]
        assert all(r[3] == np.float32(2.0) * np.float32(r[4]) for r in a.ranges())         # l2x2, formed on the host
        pen = _run(K, a, state)
        w = p[PAD + off:PAD + off + n].numpy()
        want_g = g.clone()
        want_g[PAD + off:PAD + off + n] = torch.from_numpy(G.grad_f32(ranges, w, g[PAD + off:PAD + off + n].numpy()))
        # every bit of the gradient buffer: the formula inside the ranges, unchanged outside and in the padding
        assert np.array_equal(_bits(gb), _bits(want_g)), (name, off)
        assert np.array_equal(_bits(pb), _bits(p))                                         # p is read only
        ref = G.penalty(ranges, np.where(np.isnan(w), 0.0, w.astype(np.float64)))
        assert ref > 0
        tol = (_chain(K, len(chunks)) + 2) * 2.0 ** -24
        print("%s off %d: %d workgroups, P %.8g (float64 %.8g, rel err %.3g, bound %.3g)" % (
            name, off, len(chunks), pen, ref, abs(float(pen) - ref) / ref, tol))
        assert np.isfinite(pen) and abs(float(pen) - ref) <= tol * ref, (name, off, pen, ref)
        # penalty only: g untouched in bits, the same P bits
        gb2 = g.to(dev)
        pen0 = _run(K, _args(K, pb, gb2, off, n, ranges, state, partials, add_grad=0), state)
        assert pen0.tobytes() == pen.tobytes() and np.array_equal(_bits(gb2), _bits(g)), (name, off)


def test_kernel_zero_signs():
    """sgn(0) = sgn(-0) = 0 and |-0| = 0: an all-zero range changes no gradient value and adds 0."""
    K = _K()
    dev = torch.device("cuda")
    state = torch.zeros(K.REG_STATE_WORDS, dtype=torch.float32, device=dev)
    partials = torch.zeros(4, dtype=torch.float32, device=dev)
    p = torch.zeros(PAD + 64)
    p[PAD + 1:PAD + 20:2] = -0.0
    g = torch.randn(PAD + 64, generator=torch.Generator().manual_seed(1))
    pb, gb = p.to(dev), g.to(dev)
    ranges = [(0, 40, 0.5, 0.25)]
    pen = _run(K, _args(K, pb, gb, 0, 40, ranges, state, partials), state)
    assert float(pen) == 0.0 and torch.equal(gb.cpu(), g)


def test_kernel_is_deterministic():
    """20 launches over several workgroups: identical P and gradient bits, the ticket zero after each."""
    K = _K()
    dev = torch.device("cuda")
    ranges = _range_sets(K)["gap"] + [(7 * K.REG_CHUNK + 1, 12 * K.REG_CHUNK + 3, _f32(1e-3), _f32(1e-2))]
    p, g, n = _make(ranges, 1, seed=9)
    pb = p.to(dev)
    state = torch.zeros(K.REG_STATE_WORDS, dtype=torch.float32, device=dev)
    partials = torch.zeros(16, dtype=torch.float32, device=dev)
    seen = set()
    for _ in range(20):
        gb = g.to(dev)
        a = _args(K, pb, gb, 1, n, ranges, state, partials)
        assert K.reg_blocks(a) == 10
        pen = _run(K, a, state)                       # (asserts the ticket)
        seen.add((pen.tobytes(), _bits(gb).tobytes()))
    assert len(seen) == 1


def test_kernel_host_checks():
    K = _K()
    dev = torch.device("cuda")
    a = K.RegArgs()
    with pytest.raises(Exception, match="MAX_REG_RANGES"):
        a.set_ranges([(4 * i, 4 * i + 2, 0.1, 0.1) for i in range(K.MAX_REG_RANGES + 1)])
    assert K.MAX_REG_RANGES >= 16
    a.set_ranges([(4 * i, 4 * i + 2, 0.1, 0.1) for i in range(K.MAX_REG_RANGES)])
    assert a.nranges == K.MAX_REG_RANGES
    for bad in ([(0, 4, -0.1, 0.0)], [(0, 4, 0.0, float("nan"))], [(4, 8, 0.1, 0.0), (6, 9, 0.1, 0.0)]):
        with pytest.raises(Exception):
            K.RegArgs().set_ranges(bad)
    state = torch.zeros(K.REG_STATE_WORDS, dtype=torch.float32, device=dev)
    buf = torch.zeros(64, device=dev)
    one = torch.zeros(1, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    b = _args(K, buf, buf, 0, 40, [(0, 48, 0.1, 0.1)], state, one)           # a range past n
    with pytest.raises(Exception):
        K.weight_reg(b, s)
    b = _args(K, buf, buf, 0, 40, [(0, 40, 0.1, 0.1)], state, one)
    b.npartials = 0                                                          # too few partials
    with pytest.raises(Exception, match="partials"):
        K.weight_reg(b, s)
    b = _args(K, buf, buf, 0, 40, [(0, 40, 0.1, 0.1)], state, one)
    b.g = buf.data_ptr() + 4 * (PAD + 1)                                     # g off p's 16-byte phase
    with pytest.raises(Exception, match="16-byte"):
        K.weight_reg(b, s)
    torch.cuda.synchronize()
    assert int(state.cpu().view(torch.int32)[K.REG_TICKET]) == 0


# ------------------------------------------------------------------------------------ 2. the metric words
def _slots(K, st):
    o = K.STEP_STATE_METRICS_OFFSET // 8
    return st.view(torch.int64)[o:o + 4 * K.STEP_STATE_METRIC_SLOTS].view(-1, 4).cpu().numpy().copy()


def test_metric_words_take_rows_times_penalty():
    K = _K()
    dev = torch.device("cuda")
    st = torch.zeros(K.STEP_STATE_BYTES, dtype=torch.uint8, device=dev)
    state = torch.zeros(K.REG_STATE_WORDS, dtype=torch.float32, device=dev)
    ranges = _range_sets(K)["adjacent"]
    p, g, n = _make(ranges, 0, seed=2)
    pb, gb = p.to(dev), g.to(dev)
    partials = torch.zeros(4, dtype=torch.float32, device=dev)
    total = 0
    for rows in (24.0, 1.0, 13.0):
        pen = _run(K, _args(K, pb, gb, 0, n, ranges, state, partials, st=st, rows=rows, add_grad=0), state)
        total += int(round(float(pen) * rows * 4294967296.0))            # (exact in float64: 24 + 5 + 32 bits)
        sl = _slots(K, st)
        assert int(sl[0, 0]) == total and not sl[1:].any() and not sl[0, 1:].any(), (rows, sl[0], total)
    assert total > 0


def test_infinite_weight_reports_nan():
    """P * rows non-finite (or >= 2^30): the spare word is bumped instead, and the host reports NaN
    exactly as it does for the head's own overflow."""
    K = _K()
    set_random_seed(3)
    m = M.tiny(optim.SGD(lr=0.0), device="cuda")
    ex = m._executor
    ex.reset_metrics()
    dev = ex.device
    ranges = [(0, 40, 0.0, 0.5)]
    p = torch.ones(PAD + 64)
    p[PAD + 17] = float("inf")
    pb = p.to(dev)
    partials = torch.zeros(2, dtype=torch.float32, device=dev)
    a = _args(K, pb, pb, 0, 40, ranges, ex.reg_state, partials, st=ex.state, rows=8.0, add_grad=0)
    pen = _run(K, a, ex.reg_state)
    assert not np.isfinite(pen)                        # (inf, or NaN from the other coefficient's 0 * inf)
    sl = _slots(K, ex.state)
    assert int(sl[0, 0]) == 0 and int(sl[0, 3]) == 1
    assert math.isnan(ex.read_metrics()[0])
    # finite but out of the fixed point's range
    ex.reset_metrics()
    p[PAD + 17] = 1e6                                  # 0.5 * 1e12 * 8 rows >= 2^30
    pb2 = p.to(dev)
    a = _args(K, pb2, pb2, 0, 40, ranges, ex.reg_state, partials, st=ex.state, rows=8.0, add_grad=0)
    assert np.isfinite(_run(K, a, ex.reg_state))
    assert int(_slots(K, ex.state)[0, 3]) == 1 and math.isnan(ex.read_metrics()[0])
    ex.reset_metrics()
    assert ex.read_metrics()[0] == 0.0


# ------------------------------------------------------------------------------------ 3. the step, bit level
def _model(kind, opt, device="cuda", drop=0.2, reg=True):
    return (M.tiny if kind == "tiny" else M.odd)(opt, device=device, drop=drop, reg=reg)


@pytest.mark.parametrize("kind", ["tiny", "odd"])
def test_step_gradient_is_the_twins_plus_the_term(kind, monkeypatch):
    """SGD with lr = 0 (the weights never move): after each of 2 steps the regularized model's
    store.grad equals the float32 formula applied to an unregularized twin's store.grad (the same
    plan structure, seed and batches) bit for bit, and its batch loss is the twin's plus P."""
    monkeypatch.setenv("INTML_TUNE", UNFUSED)
    set_random_seed(31)
    a = _model(kind, optim.SGD(lr=0.0))
    set_random_seed(31)
    b = _model(kind, optim.SGD(lr=0.0), reg=False)
    assert a._seed == b._seed
    b.set_weights(a.get_weights())
    n = a.store.numel
    assert n % 4 != 0
    ranges = a.regularized_ranges()
    assert len(ranges) == 6 and b.regularized_ranges() == [] and b._executor.reg_state is None
    if kind == "odd":                                 # (range borders that are no multiples of 4)
        assert any(lo % 4 for lo, _, _, _ in ranges) and any(hi % 4 for _, hi, _, _ in ranges)
    x, y = _data(a, 64, seed=3)
    w = a.store.master[:n].cpu().numpy()
    pen64 = G.penalty(ranges, w)
    rows = 32
    for t in range(2):
        out = []
        for m in (a, b):
            ex = m._executor
            d = ex.upload(x, y)
            ex.reset_metrics()
            ex.train_step(d, torch.arange(d.n, device=ex.device), rows * t, rows)
            torch.cuda.synchronize()
            out.append((m.store.grad[:n].cpu().numpy(), ex._metrics()))
        (ga, ma), (gb, mb) = out
        assert np.array_equal(a.store.master[:n].cpu().numpy(), w)
        assert np.array_equal(ga.view(np.int32), G.grad_f32(ranges, w, gb).view(np.int32)), (kind, t)
        assert not np.array_equal(ga, gb)
        pen = float(a._executor.reg_state[a._executor.K.REG_PENALTY].item())
        assert abs(pen - pen64) <= (_chain(a._executor.K, 1) + 2) * 2.0 ** -24 * pen64
        # the loss sums (rows * batch loss): the twin's plus rows * P within one fixed-point unit per row
        assert ma[2] == mb[2] == rows and ma[1] == mb[1]
        assert abs(ma[0] - (mb[0] + pen * rows)) <= rows * 2.0 ** -32, (kind, t, ma, mb, pen)
    names = [l.name for l in a._executor._plans[(rows, "train")].launches]
    assert [nm for nm in names if nm != "weight_reg"] == [l.name for l in b._executor._plans[(rows, "train")].launches]


# ------------------------------------------------------------------------------------ 4. the step, end to end
def _pair(kind, mk, **kw):
    set_random_seed(1234)
    g = _model(kind, mk(**kw), "cuda")
    set_random_seed(1234)
    c = _model(kind, mk(**kw), "cpu")
    assert g._seed == c._seed
    for a, b in zip(g.get_weights(), c.get_weights()):
        np.testing.assert_array_equal(a, b)
    return g, c


def _three_steps(g, c, x, y):
    for m in (g, c):
        ex = m._executor
        d = ex.upload(x, y)
        perm = torch.arange(d.n, device=ex.device)
        for k in range(3):
            ex.train_step(d, perm, 32 * k, 32)
    torch.cuda.synchronize()
    n = g.store.numel
    return g.store.master[:n].cpu().numpy(), c.store.master[:n].numpy()


@pytest.mark.parametrize("kind", ["tiny", "odd"])
@pytest.mark.parametrize("name", sorted(KINDS))
def test_three_steps_track_the_cpu_reference(name, kind):
    """The bound tests/test_hip_model.py::test_multiple_steps_track_reference applies to the same
    comparison without regularizers (relative L2 error of all weights < 1e-2): the regularization
    arithmetic is fp32 on both sides and earns no extra margin."""
    g, c = _pair(kind, KINDS[name])
    x, y = _data(g, 96, seed=3)
    w0 = g.store.master[:g.store.numel].cpu().numpy()
    wg, wc = _three_steps(g, c, x, y)
    print("%s %s: rel err %.3g, moved %.3g" % (name, kind, _rel(wg, wc), _rel(wg, w0)))
    assert _rel(wg, wc) < 1e-2
    plan = g._executor._plans[(32, "train")]
    assert [l.name for l in plan.launches].count("weight_reg") == 1 and not plan.optim_fused
    arena = g._executor.arena.clone()                  # the packs mirror the master
    g._executor.params_changed()
    torch.cuda.synchronize()
    assert torch.equal(arena, g._executor.arena)


@pytest.mark.parametrize("kind", ["tiny", "odd"])
@pytest.mark.parametrize("name", ["Adam", "SGD", "Adamax"])
def test_clipnorm_with_l2_tracks_the_cpu_reference(name, kind):
    g, c = _pair(kind, KINDS[name], clipnorm=CLIPNORM)
    x, y = _data(g, 96, seed=3)
    ex = g._executor
    n = g.store.numel
    d = ex.upload(x, y)
    dc = c._executor.upload(x, y)
    for k in range(3):
        w = g.store.master[:n].cpu().double().numpy()
        ex.train_step(d, torch.arange(d.n, device=ex.device), 32 * k, 32)
        c._executor.train_step(dc, torch.arange(dc.n), 32 * k, 32)
        torch.cuda.synchronize()
        # one GPU: store.grad holds the regularized, unclipped gradient; its norm is what clipped
        gr = g.store.grad[:n].cpu().double().numpy()
        _, info = C.clip(gr, clipnorm=CLIPNORM)
        assert info["fired"] and info["norm"] > 2 * CLIPNORM, (name, kind, k, info)
        dn = float(ex.clip_state[ex.K.CLIP_NORM].item())
        assert abs(dn - info["norm"]) < 1e-5 * info["norm"], (dn, info)
        assert float(ex.clip_state[ex.K.CLIP_FACTOR].item()) < 1.0
        # ... and it carries the term: without it the norm is another one
        assert abs(C.global_norm(gr - G.grad_term(g.regularized_ranges(), w)) - info["norm"]) > 1e-3 * info["norm"]
    wg, wc = g.store.master[:n].cpu().numpy(), c.store.master[:n].numpy()
    print("%s %s clipnorm: rel err %.3g" % (name, kind, _rel(wg, wc)))
    assert _rel(wg, wc) < 1e-2
    names = [l.name for l in ex._plans[(32, "train")].launches]
    assert names[-2:] == ["weight_reg", "grad_sqnorm"]


def test_evaluation_losses_contain_the_penalty():
    """evaluate (ragged last batch), test_on_batch, val_loss and sample weights against an
    unregularized twin at the same weights: the twin's loss + P, acc untouched.  Both sides run
    the same kernels on the same bf16 data, so the bound is the fixed point's and fp32 P's."""
    set_random_seed(6)
    m = M.tiny(optim.SGD(lr=0.0), device="cuda")
    twin = M.tiny(optim.SGD(lr=0.0), device="cuda", reg=False)
    twin.set_weights(m.get_weights())
    x, y, _ = synthetic_rpv(40, size=16, channels=3, seed=8)
    n = m.store.numel
    pen = G.penalty(m.regularized_ranges(), m.store.master[:n].cpu().numpy())
    # (fp32 P against float64: the kernel's addition-chain bound; 1e-6 for the fp32 / fixed-point loss sums)
    tol = (_chain(m._executor.K, 1) + 2) * 2.0 ** -24 * pen + 1e-6
    a, b = m.evaluate(x, y, batch_size=16, verbose=0), twin.evaluate(x, y, batch_size=16, verbose=0)      # 16 + 16 + 8
    assert abs(a[0] - (b[0] + pen)) <= tol and a[1] == b[1], (a, b, pen)
    a, b = m.test_on_batch(x[:16], y[:16]), twin.test_on_batch(x[:16], y[:16])
    assert abs(a[0] - (b[0] + pen)) <= tol and a[1] == b[1]
    sw = np.linspace(0.0, 3.0, 16).astype(np.float32)
    a, b = m.test_on_batch(x[:16], y[:16], sample_weight=sw), twin.test_on_batch(x[:16], y[:16], sample_weight=sw)
    assert abs(a[0] - (b[0] + pen)) <= tol               # the penalty is not sample-weighted
    h = m.fit(x, y, batch_size=16, epochs=1, verbose=0, shuffle=False, validation_data=(x[:24], y[:24]))
    ht = twin.fit(x, y, batch_size=16, epochs=1, verbose=0, shuffle=False, validation_data=(x[:24], y[:24]))
    for key in ("loss", "val_loss"):
        assert abs(h.history[key][0] - (ht.history[key][0] + pen)) <= tol, (key, h.history, ht.history, pen)
    assert h.history["val_acc"] == ht.history["val_acc"]
    names = {k: [l.name for l in p.launches] for k, p in m._executor._plans.items()}
    assert all(v.count("weight_reg") == 1 and v[-1] == "weight_reg" for k, v in names.items() if k[1] == "eval"), names
    assert any(k[1] == "eval" for k in names)
    m.predict(x[:16], batch_size=16)
    pred = [l.name for l in m._executor._plans[(16, "predict")].launches]
    assert "weight_reg" not in pred, pred


@pytest.mark.parametrize("name", ["Adam", "SGD"])
def test_graph_of_8_steps_equals_8_single_steps(name):
    """The ticket, P and the loss words must be right across the steps inside one graph."""
    res = []
    for chunks in ([1] * 8, [8]):
        set_random_seed(21)
        m = M.tiny(KINDS[name](decay=0.01), device="cuda", drop=0.2)
        x, y = _data(m, 256, seed=4)
        ex = m._executor
        d = ex.upload(x, y)
        perm = torch.randperm(d.n, generator=torch.Generator().manual_seed(3)).to(ex.device)
        ex.reset_metrics()
        pos = 0
        for k in chunks:
            ex.train_steps(d, perm, pos, 32, k)
            pos += 32 * k
        torch.cuda.synchronize()
        n = m.store.numel
        res.append(([m.store.master[:n].clone(), m.store.grad[:n].clone()] + [s.clone() for s in ex.optimizer_state()],
                    ex._metrics(), int(m.optimizer.iterations), ex.reg_state.clone()))
        assert float(ex.reg_state[ex.K.REG_PENALTY].item()) > 0
    for a, b in zip(res[0][0], res[1][0]):
        assert torch.equal(a, b)
    assert res[0][1] == res[1][1] and res[0][1][2] == 256
    assert torch.equal(res[0][3], res[1][3]) and res[0][2] == res[1][2] == 8


# ------------------------------------------------------------------------------------ 5. the plan
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


@pytest.mark.parametrize("name", ["Adam", "Adamax"])
def test_regularized_plan_is_gated_like_a_clipping_one(name, monkeypatch):
    from cori_intml_examples_amd.apps import zoo
    for tv in ("", "dense_opt=1"):
        monkeypatch.setenv("INTML_TUNE", tv)
        set_random_seed(57)
        m = zoo.rpv_cnn((64, 64, 3), conv_sizes=[16, 32, 64], fc_sizes=[128], dropout=0.2, optimizer=KINDS[name](),
                        lr=None, device="cuda", l2=1e-4)
        names = _plan_names(m)
        plan = m._executor._plans[(128, "train")]
        assert plan.early_red == {} and plan.dense_fused_opt == [] and not plan.dense_opt_ok and not plan.optim_fused
        assert names["train"].count("weight_reg") == 1 and names["train"][-1] == "weight_reg"
        assert names["eval"].count("weight_reg") == 1 and names["eval"][-1] == "weight_reg"
        assert "weight_reg" not in names["predict"]
        # ... the structure of the fuse_optim=0 step plus the one launch
        monkeypatch.setenv("INTML_TUNE", UNFUSED)
        set_random_seed(57)
        u = zoo.rpv_cnn((64, 64, 3), conv_sizes=[16, 32, 64], fc_sizes=[128], dropout=0.2, optimizer=KINDS[name](),
                        lr=None, device="cuda")
        un = _plan_names(u)
        for mode in ("train", "eval", "predict"):
            assert [nm for nm in names[mode] if nm != "weight_reg"] == un[mode], mode
        assert len(m.regularized_ranges()) == 5


def test_plan_without_regularizers_is_unchanged(monkeypatch):
    """The "nothing changed" claim: l2 = 0 and explicit None / L1L2(0, 0) regularizer arguments
    record exactly the launch lists of a model built with the arguments absent."""
    from cori_intml_examples_amd import regularizers
    from cori_intml_examples_amd.apps import zoo
    from cori_intml_examples_amd.models import Conv2D, Dense, Dropout, Flatten, Input, MaxPooling2D, Model
    monkeypatch.delenv("INTML_TUNE", raising=False)
    set_random_seed(57)
    absent = _build("rpv_bench", "cuda", opt="Adam", drop=0.2, cin=3, hw=64)
    ref = _plan_names(absent)
    plan = absent._executor._plans[(128, "train")]
    assert plan.early_red and plan.optim_fused and ref["train"].count("reduce_b0") == 1
    assert not [nm for mode in ref for nm in ref[mode] if "weight_reg" in nm]
    ex = absent._executor
    assert ex.regs == [] and ex.reg_state is None and ex.reg_partials is None
    set_random_seed(57)
    zero = zoo.rpv_cnn((64, 64, 3), conv_sizes=[16, 32, 64], fc_sizes=[128], dropout=0.2, optimizer="Adam", lr=1e-3,
                       device="cuda", l2=0.0)
    assert _plan_names(zero) == ref
    set_random_seed(57)
    none = {"kernel_regularizer": None, "bias_regularizer": regularizers.L1L2(0, 0), "activity_regularizer": None}
    inp = Input(shape=(64, 64, 3))
    h = inp
    for c in (16, 32, 64):
        h = MaxPooling2D((2, 2))(Conv2D(c, (3, 3), activation="relu", padding="same", **none)(h))
    h = Flatten()(Dropout(0.2)(h))
    h = Dropout(0.2)(Dense(128, activation="relu", **none)(h))
    m = Model(inp, Dense(1, activation="sigmoid", **none)(h), device="cuda")
    m.compile(optimizer=optim.Adam(lr=1e-3), loss="binary_crossentropy", metrics=["accuracy"])
    assert _plan_names(m) == ref and m._executor.reg_state is None


def test_too_many_regularized_tensors_is_a_host_error():
    from cori_intml_examples_amd import regularizers
    from cori_intml_examples_amd.models import Dense, Sequential
    K = _K()
    m = Sequential(device="cuda")
    for i in range(K.MAX_REG_RANGES // 2 + 1):
        m.add(Dense(4, activation="relu", kernel_regularizer=regularizers.l2(0.01), bias_regularizer=regularizers.l1(0.01),
                    **({"input_shape": (8,)} if i == 0 else {})))
    m.add(Dense(1, activation="sigmoid"))
    with pytest.raises(ValueError, match="MAX_REG_RANGES = %d" % K.MAX_REG_RANGES):
        m.compile(optimizer="Adam", loss="binary_crossentropy")


# ------------------------------------------------------------------------------------ 6. data parallel
def test_data_parallel_step_at_one_rank(tmp_path):
    out = tmp_path / "dp.json"
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("WORLD_SIZE", "RANK", "INTML_DP_BACKEND", "INTML_COMM", "INTML_XGMI", "INTML_TUNE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "reg_dp_worker_gpu.py"), str(out)],
                       env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rep = json.load(open(out))
    print(json.dumps(rep, indent=1))
    assert rep["native"], rep
    for case in ("Adam", "Adamax+clipnorm"):
        k = rep[case]
        clip = "clipnorm" in case
        assert k["moved"] > 1e-4 and not k["base_fused"] and k["base_penalty"] > 0, k
        assert k["base_launches"] == ["reduce_b0", "weight_reg"] + (["grad_sqnorm"] if clip else []), k
        for mode in ("captured", "segmented"):
            c = k[mode]
            assert c["reducer"] == "NativeGradReducer" and c["plane"] == "rccl" and not c["xgmi"], c
            assert c["comm_in_graph"] == (mode == "captured") and c["early_red"] == 0 and c["buckets"] == 1, c
            assert not [nm for nm in c["launches"] if "xgmi" in nm or "xchg" in nm], c
            # the order: local reduction, the regularizers' term, [norm, in-place clip,] all-reduce, update
            want = ["reduce_b0", "weight_reg_b0"] + (["grad_sqnorm_b0", "grad_clip_apply_b0"] if clip else [])
            if mode == "captured":
                want += ["allreduce_b0", "optim_b0"]
            assert c["launches"] == want, c
            assert c["iterations"] == 4 and c["penalty"] > 0, c
            print(case, mode, "bit-identical to the single-GPU regularized run:", c["identical"])
            assert max(c["max_abs_diff"]) < k["bound"], (case, mode, c)
            assert abs(c["penalty"] - k["base_penalty"]) <= 1e-4 * k["base_penalty"], (case, mode, c)
        for plane in ("xgmi", "hybrid"):
            msg = k["forced_" + plane]
            # (the refused model's own layers: three convs and two denses, auto-named)
            assert repr(plane) in msg and "regularizer" in msg, k
            assert len(re.findall(r"conv2d_\d+", msg)) == 3 and len(re.findall(r"dense_\d+", msg)) == 2, k
        assert len(k["layers"]) == 5
    assert rep["history_data_plane"].startswith("NativeGradReducer:rccl"), rep["history_data_plane"]
    assert rep["history_loss_finite"]


# ------------------------------------------------------------------------------------ 7. checkpoint
def test_gpu_checkpoint_loads_on_cpu_and_continues(tmp_path):
    x, y, _ = synthetic_rpv(96, channels=3, size=16, seed=1)
    set_random_seed(8)
    m = M.tiny(optim.Adam(lr=0.01), device="cuda")
    m.fit(x[:64], y[:64], batch_size=16, epochs=1, verbose=0, shuffle=False)
    p = str(tmp_path / "g.h5")
    m.save(p)
    c = load_model(p, device="cpu")
    assert c.store.master.device.type == "cpu" and c.optimizer.iterations == m.optimizer.iterations == 4
    assert c.regularized_ranges() == m.regularized_ranges() and len(c.regularized_ranges()) == 6
    assert [l.get_config() for l in c.layers] == [l.get_config() for l in m.layers]
    for a, b in zip(m.get_weights(), c.get_weights()):
        np.testing.assert_array_equal(a, b)
    # it continues: the CPU model's next regularized step from the GPU model's state
    n = c.store.numel
    pen = G.penalty(c.regularized_ranges(), c.store.master[:n].numpy())
    w0 = c.store.master[:n].clone()
    lc, lg = c.train_on_batch(x[64:], y[64:]), m.train_on_batch(x[64:], y[64:])
    torch.cuda.synchronize()
    assert lc[0] > pen > 0 and abs(lc[0] - lg[0]) < 2e-2 * lg[0]
    assert float((c.store.master[:n] - w0).abs().max()) > 1e-4
    assert _rel(m.store.master[:n].cpu().numpy(), c.store.master[:n].numpy()) < 1e-2
