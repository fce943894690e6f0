"""AveragePooling2D / GlobalAveragePooling2D / GlobalMaxPooling2D on the GPU: the pool.hip kernels
alone against the float64 oracle (values, indices, layout, guard regions, dropout, determinism,
the launchers' checks), and whole models against the CPU executor (three optimizer steps, one-step
gradients under ref_bf16, evaluate / predict, graph replay, checkpoints, unchanged plans, gating,
data parallel at one rank)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cori_intml_examples_amd import optim
from cori_intml_examples_amd.io.keras_h5 import load_model
from cori_intml_examples_amd.models.step_program import dropout_pair
from cori_intml_examples_amd.ops.rng import dropout_keep
from cori_intml_examples_amd.utils import set_random_seed

from helpers import act_oracle as A
from helpers import pool_models as M
from helpers import pool_oracle as O
from test_hip_model import _build, _data, _rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

PERLAYER = "conv_stack=0"                  # the structure an average-pooled or globally pooled model takes
NAN_BITS = 0x7FC1                          # what every output buffer and guard region is filled with
CHANNELS = [(3, 8), (16, 16), (20, 24)]    # (C, Cs)
OFF = 8                                    # payloads start 16 bytes into a 256-byte-aligned allocation
SEED, STREAM, RATE = 1234567, 3, 0.25


def _K():
    from cori_intml_examples_amd.ops.hip import kernels
    return kernels()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Buf:
    """A bf16 (or int32) payload ``OFF`` elements (int32: 4, both 16 bytes) into a sentinel-filled
    allocation with 64 guard elements behind it."""

    def __init__(self, shape, bits=None, int32=False):
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        self.int32 = int32
        self.off = 4 if int32 else OFF
        full = np.full(self.off + self.n + 64, -7 if int32 else NAN_BITS, np.int64)
        if bits is not None:
            full[self.off:self.off + self.n] = np.asarray(bits, np.int64).reshape(-1)
        self.init = full.copy()
        if int32:
            self.t = torch.tensor(full.astype(np.int32)).cuda()
        else:
            self.t = torch.tensor(full.astype(np.uint16).view(np.int16)).cuda()
        self.ptr = self.t.data_ptr() + (4 if int32 else 2) * self.off
        assert self.ptr % 16 == 0 and self.ptr % 32 != 0

    def raw(self):
        v = self.t.cpu().numpy().astype(np.int64)
        return v if self.int32 else v & 0xFFFF

    def get(self):
        """The payload (bf16 bits or ints), after checking that both guard regions are untouched."""
        v = self.raw()
        assert np.array_equal(v[:self.off], self.init[:self.off]) and np.array_equal(v[self.off + self.n:],
                                                                                   self.init[self.off + self.n:])
        return v[self.off:self.off + self.n].reshape(self.shape)


def _bits(v64):
    return A.to_bf16_bits(np.asarray(v64, np.float64))


def _vals(bits):
    return A.bf16_values(bits).astype(np.float64)


def _draw(rs, shape, C, pad_bits=NAN_BITS):
    """bf16 bits [.., Cs] of N(0, 2) draws in the C real channels (away from subnormals: |v| > 2^-20 or
    0 never occurs in practice; asserted), ``pad_bits`` in the pad channels."""
    b = _bits(rs.randn(*shape) * 2.0)
    v = np.abs(_vals(b))
    assert np.all(v > 2.0 ** -60)
    b[..., C:] = pad_bits
    return b


def _ulp(v64):
    """One bf16 ulp at |v| (the spacing of bf16 values in v's binade; 2^-133 at 0)."""
    v = np.abs(np.asarray(v64, np.float64))
    e = np.floor(np.log2(np.maximum(v, 2.0 ** -126)))
    return 2.0 ** (e - 7)


def _within_ulp(got_bits, want64, n=1):
    d = np.abs(A.ordinal(got_bits) - A.ordinal(_bits(want64)))
    return int(d.max(initial=0)) <= n, int(d.max(initial=0))


def _state(K, step):
    st = torch.zeros(K.STEP_STATE_BYTES, dtype=torch.uint8, device="cuda")
    st.view(torch.int32)[0] = step
    return st


def _pool_args(K, mode, B, H, W, C, Cs, x=0, out=0, idx=0):
    a = K.PoolArgs()
    a.mode, a.B, a.H, a.W, a.C, a.Cs = mode, B, H, W, C, Cs
    a.x, a.out, a.idx = x, out, idx
    return a


def _repeat_identical(launch, buf, times=4):
    """``times`` launches into the same (re-filled) buffer give bit-identical contents."""
    seen = []
    for _ in range(times):
        buf.t.copy_(torch.tensor(buf.init.astype(np.int32 if buf.int32 else np.uint16).view(
            np.int32 if buf.int32 else np.int16)).cuda())
        launch()
        torch.cuda.synchronize()
        seen.append(buf.raw().copy())
    assert all(np.array_equal(seen[0], s) for s in seen[1:])


# ------------------------------------------------------------------------------------ 1. AVG2
@pytest.mark.parametrize("C,Cs", CHANNELS)
@pytest.mark.parametrize("H,W", [(2, 2), (5, 7), (8, 6)])
def test_avg2_forward_and_backward(H, W, C, Cs):
    K, B = _K(), 3
    Hp, Wp = H // 2, W // 2
    rs = np.random.RandomState(H * 100 + W * 10 + C)
    xb = _draw(rs, (B, H, W, Cs), C)
    x64 = _vals(xb)[..., :C]
    want = O.avg2_fwd(x64)
    xin = Buf(xb.shape, xb)
    thr, scale = dropout_pair(RATE)
    for step in (None, 5):
        out = Buf((B, Hp, Wp, Cs))
        a = _pool_args(K, K.POOL_AVG2, B, H, W, C, Cs, xin.ptr, out.ptr)
        keep = np.ones((B, Hp, Wp, C), bool)
        if step is not None:
            st = _state(K, step)
            a.drop_thr, a.drop_scale, a.seed, a.stream_id, a.st = thr, scale, SEED, STREAM, st.data_ptr()
            keep = dropout_keep(B * Hp * Wp * C, RATE, SEED, STREAM, step).numpy().reshape(B, Hp, Wp, C)
        K.pool_fwd(a, _stream())
        torch.cuda.synchronize()
        got = out.get()
        assert np.all(got[..., C:] == 0)                                  # pad channels: +0
        assert np.all(got[..., :C][~keep] == 0)                           # dropped: +0
        sc = float(np.float32(scale)) if step is not None else 1.0
        ok, d = _within_ulp(got[..., :C][keep], (want * sc)[keep])
        assert ok, (H, W, C, step, d)
        nz = np.abs(want) > 1e-30
        assert np.all((got[..., :C] != 0)[keep & nz])                     # the kept set is dropout_keep's
        xin.get()                                                         # the input is not written
        _repeat_identical(lambda: K.pool_fwd(a, _stream()), out)
    # backward: 0.25 * dP is exact in bf16, so the gradient is exact; zeros in the leftover row / column
    dpb = _draw(rs, (B, Hp, Wp, Cs), C, pad_bits=0)
    linb = _draw(rs, (B, H, W, Cs), C)
    dp, lin = Buf(dpb.shape, dpb), Buf(linb.shape, linb)
    dp64, lin64 = _vals(dpb)[..., :C], _vals(linb)[..., :C]
    for relu in (0, 1):
        dz = Buf((B, H, W, Cs))
        a = _pool_args(K, K.POOL_AVG2, B, H, W, C, Cs)
        a.dp, a.dz, a.relu = dp.ptr, dz.ptr, relu
        if relu:
            a.lin = lin.ptr
        K.pool_bwd(a, _stream())
        torch.cuda.synchronize()
        got = dz.get()
        want = O.avg2_bwd(dp64, (H, W), lin64 if relu else None)
        assert np.array_equal(_vals(got[..., :C]), want), (H, W, C, relu)
        assert np.all(got[..., C:] == 0)
        assert np.all(got[:, 2 * Hp:] == 0) and np.all(got[:, :, 2 * Wp:] == 0)
        if relu:
            assert np.all(got[..., :C][lin64 <= 0] == 0) and (lin64 <= 0).mean() > 0.2
        dp.get(), lin.get()
        _repeat_identical(lambda: K.pool_bwd(a, _stream()), dz)


# ------------------------------------------------------------------------------------ 2. global forward
def _global_input(rs, B, H, W, C, Cs):
    """Random draws with crafted channels: 0 a maximum duplicated at two positions, 1 all negative
    (GAVG: +-100 cancelling to about 0.1), 2 all equal."""
    n = H * W
    x = rs.randn(B, n, Cs) * 2.0
    x[:, :, 0] = np.minimum(x[:, :, 0], 3.0)
    x[:, n // 3, 0] = x[:, n - 1, 0] = 7.0
    x[:, :, 2] = 3.0
    return x


@pytest.mark.parametrize("C,Cs", CHANNELS)
@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (7, 5), (16, 16)])
@pytest.mark.parametrize("B", [1, 5])
def test_global_forward(B, H, W, C, Cs):
    K, n = _K(), H * W
    rs = np.random.RandomState(B * 1000 + n * 10 + C)
    x = _global_input(rs, B, H, W, C, Cs)
    for mode in ("avg", "max"):
        xm = x.copy()
        if mode == "avg":
            # +-100 pairs and a small remainder: the mean is about 0.1 / n, every partial sum about 100
            pairs = 2 * ((n - 1) // 2)
            xm[:, :pairs, 1] = np.where(np.arange(pairs) % 2 == 0, 100.0, -100.0)
            xm[:, pairs:, 1] = 0.0625
            xm[:, n - 1, 1] = 0.125
        else:
            xm[:, :, 1] = -np.abs(xm[:, :, 1]) - 1.0                       # all negative
        xb = _bits(xm)
        xb[..., C:] = NAN_BITS
        x64 = _vals(xb).reshape(B, H, W, Cs)[..., :C]
        xin, out = Buf((B, H, W, Cs), xb), Buf((B, Cs))
        idx = Buf((B, Cs), int32=True) if mode == "max" else None
        a = _pool_args(K, K.POOL_GAVG if mode == "avg" else K.POOL_GMAX, B, H, W, C, Cs, xin.ptr, out.ptr,
                       idx.ptr if idx else 0)
        K.pool_fwd(a, _stream())
        torch.cuda.synchronize()
        got = out.get()
        assert np.all(got[:, C:] == 0)
        assert not np.any(A.is_nan_bits(got))
        if mode == "avg":
            want = O.gavg_fwd(x64)
            # 1 bf16 ulp of the oracle value + the kernel's fp32 chain: n * 2^-24 * sum |x_i| / n
            bound = _ulp(want) + n * 2.0 ** -24 * np.abs(x64).reshape(B, n, C).sum(1) / n
            err = np.abs(_vals(got[:, :C]) - want)
            print("gavg B=%d %dx%d C=%d: max err / bound %.3g, cancelling channel %.6g (oracle %.6g)" % (
                B, H, W, C, (err / bound).max(), _vals(got[0, 1]), want[0, 1]))
            assert np.all(err <= bound), (err / bound).max()
            assert np.all(np.abs(want[:, 1]) < 0.2) and (n < 3 or np.abs(x64[..., 1]).max() == 100.0)
        else:
            want, at = O.gmax_fwd(x64)
            assert np.array_equal(_vals(got[:, :C]), want)
            gi = idx.get()
            assert np.array_equal(gi[:, :C], at) and np.all(gi[:, C:] == 0)
            assert np.all(want[:, 1] < 0) and np.all(gi[:, 2] == 0)        # all negative; all equal -> the first
            if n >= 3:
                assert np.all(want[:, 0] == 7.0) and np.all(gi[:, 0] == n // 3)   # the first of the two maxima
            # an evaluation step has no index buffer: the same values
            out2 = Buf((B, Cs))
            a.out, a.idx = out2.ptr, 0
            K.pool_fwd(a, _stream())
            torch.cuda.synchronize()
            assert np.array_equal(out2.get(), got)
            a.out, a.idx = out.ptr, idx.ptr
            _repeat_identical(lambda: K.pool_fwd(a, _stream()), idx)
        _repeat_identical(lambda: K.pool_fwd(a, _stream()), out)
        xin.get()


@pytest.mark.parametrize("mode", ["avg", "max"])
def test_global_forward_dropout(mode):
    K, (B, H, W, C, Cs) = _K(), (5, 7, 5, 20, 24)
    rs = np.random.RandomState(11)
    xb = _draw(rs, (B, H, W, Cs), C)
    x64 = _vals(xb)[..., :C]
    want = O.gavg_fwd(x64) if mode == "avg" else O.gmax_fwd(x64)[0]
    thr, scale = dropout_pair(RATE)
    xin = Buf(xb.shape, xb)
    for step in (1, 77):
        out = Buf((B, Cs))
        idx = Buf((B, Cs), int32=True)
        a = _pool_args(K, K.POOL_GAVG if mode == "avg" else K.POOL_GMAX, B, H, W, C, Cs, xin.ptr, out.ptr,
                       idx.ptr if mode == "max" else 0)
        st = _state(K, step)
        a.drop_thr, a.drop_scale, a.seed, a.stream_id, a.st = thr, scale, SEED, STREAM, st.data_ptr()
        K.pool_fwd(a, _stream())
        torch.cuda.synchronize()
        keep = dropout_keep(B * C, RATE, SEED, STREAM, step).numpy().reshape(B, C)
        assert 0.5 < keep.mean() < 0.95
        got = out.get()
        assert np.all(got[:, C:] == 0) and np.all(got[:, :C][~keep] == 0)
        assert np.all(got[:, :C][keep] != 0)
        ok, d = _within_ulp(got[:, :C][keep], (want * float(np.float32(scale)))[keep], 1 if mode == "max" else 2)
        assert ok, d
        if mode == "max":                                                  # the index does not depend on the mask
            assert np.array_equal(idx.get()[:, :C], O.gmax_fwd(x64)[1])


# ------------------------------------------------------------------------------------ 3. global backward
@pytest.mark.parametrize("C,Cs", CHANNELS)
@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (7, 5), (16, 16)])
def test_global_backward_routes_through_the_feeding_stage(H, W, C, Cs):
    """The gradient of every element of the feeding stage's output grid, stored through that stage's
    BwdThrough: its dropout mask (regenerated at element (b, y, x) * C + c), its relu mask from its
    saved output, one bf16 rounding.  (A max-pooled feeding stage stores at its pooled resolution,
    like here; its codes are applied when its own dgrad / wgrad load that buffer.)"""
    K, B, n = _K(), 5, H * W
    rs = np.random.RandomState(n * 10 + C)
    dgb = _draw(rs, (B, Cs), C, pad_bits=0)
    dg64 = _vals(dgb)[:, :C]
    prevb = _draw(rs, (B, H, W, Cs), C)
    prev64 = _vals(prevb)[..., :C]
    at = rs.randint(0, n, (B, Cs))
    at[:, C:] = 0
    dg, prev, idx = Buf(dgb.shape, dgb), Buf(prevb.shape, prevb), Buf((B, Cs), at, int32=True)
    thr, scale = dropout_pair(RATE)
    step = 9
    st = _state(K, step)
    keep = dropout_keep(B * n * C, RATE, SEED, STREAM, step).numpy().reshape(B, H, W, C)
    for mode in ("avg", "max"):
        for relu, drop, wt in ((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 1)):
            dy = Buf((B, H, W, Cs))
            a = _pool_args(K, K.POOL_GAVG if mode == "avg" else K.POOL_GMAX, B, H, W, C, Cs,
                           idx=idx.ptr if mode == "max" else 0)
            a.dp, a.st = dg.ptr, st.data_ptr()
            bt = K.BwdThrough()
            bt.pH, bt.pW, bt.pC, bt.pCs, bt.cH, bt.cW = H, W, C, Cs, H, W
            bt.dy, bt.prev_relu, bt.wt = dy.ptr, relu, wt
            if relu:
                bt.prev_out = prev.ptr
            if drop:
                bt.drop_thr, bt.drop_scale, bt.seed, bt.stream_id = thr, scale, SEED, STREAM
            a.bt = bt
            K.pool_bwd(a, _stream())
            torch.cuda.synchronize()
            got = dy.get()
            g = O.gavg_bwd(dg64, (H, W)) if mode == "avg" else O.gmax_bwd(dg64, at[:, :C], (H, W))
            want = O.through(g, keep if drop else None, float(np.float32(scale)), prev64 if relu else None)
            assert np.all(got[..., C:] == 0)
            zero = want == 0
            assert np.all(_vals(got[..., :C])[zero] == 0), (mode, relu, drop)
            if mode == "max" and not drop:
                assert np.array_equal(_vals(got[..., :C]), want)          # a pure routing: exact
            else:
                ok, d = _within_ulp(got[..., :C][~zero], want[~zero])
                assert ok, (mode, relu, drop, d)
            if mode == "max":
                assert (np.count_nonzero(_vals(got[..., :C]).reshape(B, n, C), axis=1) <= 1).all()
            dg.get(), prev.get(), idx.get()
    _repeat_identical(lambda: K.pool_bwd(a, _stream()), dy)


# ------------------------------------------------------------------------------------ 4. launcher checks
def test_launcher_host_checks():
    K = _K()
    z = lambda *s, dt=torch.bfloat16: torch.zeros(*s, dtype=dt, device="cuda")
    x, out, idx = z(2, 4, 6, 16), z(2, 4, 6, 16), z(2, 16, dt=torch.int32)
    dp, dz = z(2, 2, 3, 16), z(2, 4, 6, 16)

    def fwd(mode=None, **kw):
        a = _pool_args(K, K.POOL_AVG2 if mode is None else mode, 2, 4, 6, 12, 16, x.data_ptr(), out.data_ptr())
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def bwd(mode=None, **kw):
        a = _pool_args(K, K.POOL_AVG2 if mode is None else mode, 2, 4, 6, 12, 16)
        a.dp, a.dz = dp.data_ptr(), dz.data_ptr()
        if mode not in (None, K.POOL_AVG2):
            bt = K.BwdThrough()
            bt.pH, bt.pW, bt.pC, bt.pCs, bt.dy = 4, 6, 12, 16, dz.data_ptr()
            for k in [k for k in kw if k.startswith("bt_")]:
                setattr(bt, k[3:], kw.pop(k))
            a.bt = bt
            a.idx = idx.data_ptr() if mode == K.POOL_GMAX else 0
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def bad(fn, a):
        with pytest.raises(ValueError):
            fn(a, _stream())
    for make, fn in ((fwd, K.pool_fwd), (bwd, K.pool_bwd)):
        for kw in ({"mode": 0}, {"mode": 9}, {"Cs": 12}, {"Cs": 0}, {"C": 17}, {"C": 0}, {"B": -1}, {"H": 0}, {"W": -2},
                   {"H": 1}):
            bad(fn, make(**kw))
    for kw in ({"x": 0}, {"x": x.data_ptr() + 2}, {"out": 0}, {"out": out.data_ptr() + 6}, {"idx": idx.data_ptr()},
               {"drop_thr": 5, "drop_scale": 0.5}, {"drop_thr": 5, "drop_scale": float("inf")}):
        bad(K.pool_fwd, fwd(**kw))
    bad(K.pool_fwd, fwd(K.POOL_GMAX, idx=idx.data_ptr() + 4))
    for kw in ({"dp": 0}, {"dp": dp.data_ptr() + 2}, {"dz": 0}, {"dz": dz.data_ptr() + 8}, {"relu": 1},
               {"relu": 1, "lin": x.data_ptr() + 2}):
        bad(K.pool_bwd, bwd(**kw))
    for mode in (K.POOL_GAVG, K.POOL_GMAX):
        for kw in ({"bt_pH": 5}, {"bt_pW": 3}, {"bt_pC": 11}, {"bt_pCs": 24}, {"bt_dy": 0}, {"bt_dy": dz.data_ptr() + 2},
                   {"bt_prev_relu": 1}, {"bt_prev_relu": 1, "bt_prev_out": x.data_ptr() + 2},
                   {"bt_drop_thr": 5, "bt_drop_scale": 0.0}, {"dp": 0}):
            bad(K.pool_bwd, bwd(mode, **kw))
    bad(K.pool_bwd, bwd(K.POOL_GMAX, idx=0))
    bad(K.pool_bwd, bwd(K.POOL_GMAX, idx=idx.data_ptr() + 4))
    # valid launches over zero buffers (and an empty batch: nothing to launch) leave zeros
    K.pool_fwd(fwd(B=0), _stream())
    K.pool_fwd(fwd(), _stream())
    K.pool_fwd(fwd(K.POOL_GAVG), _stream())
    K.pool_fwd(fwd(K.POOL_GMAX, idx=idx.data_ptr()), _stream())
    K.pool_bwd(bwd(), _stream())
    K.pool_bwd(bwd(K.POOL_GAVG), _stream())
    K.pool_bwd(bwd(K.POOL_GMAX), _stream())
    torch.cuda.synchronize()
    for t in (x, out, dp, dz):
        assert float(t.float().abs().sum()) == 0.0
    assert int(idx.abs().sum()) == 0


# ------------------------------------------------------------------------------------ 5. models
def _pair(kind, mk, drop=0.2):
    set_random_seed(1234)
    g = M.build(kind, mk(), "cuda", drop=drop)
    set_random_seed(1234)
    c = M.build(kind, mk(), "cpu", drop=drop)
    assert g._seed == c._seed
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


def _names(m, bs, mode="train"):
    return [l.name for l in m._executor._plans[(bs, mode)].launches]


OPTS = {"Adam": optim.Adam, "AMSGrad": lambda: optim.Adam(amsgrad=True), "SGDm": lambda: optim.SGD(lr=0.01, momentum=0.9)}


@pytest.mark.parametrize("kind,opt", [(k, "Adam") for k in M.KINDS] + [("avg_odd_gap", "AMSGrad"), ("max_gmp", "SGDm")])
def test_three_steps_track_the_cpu_reference(kind, opt):
    """tests/test_hip_model.py::test_multiple_steps_track_reference's bound (relative L2 error of all
    weights <= 1e-2) after three optimizer steps over batches of 6, 6 and 4 rows, dropout 0.2, fp32
    CPU executor.  AMSGrad is the stand-alone optimizer kind, SGD runs with momentum."""
    g, c = _pair(kind, OPTS[opt])
    x, y = _data(g, 16, seed=3)
    n = g.store.numel
    w0 = g.store.master[:n].cpu().numpy()
    wg, wc = _three_steps(g, c, x, y)
    train = [s.offset for s in g.store.specs if getattr(s, "trainable", True)]
    print("%s %s: rel err %.3g, moved %.3g" % (kind, opt, _rel(wg, wc), _rel(wg, w0)))
    assert _rel(wg, wc) <= 1e-2 and _rel(wg, w0) > 1e-4 and train
    names = _names(g, 6)
    navg = len([s for s in g._executor.plan.convs if s.pool_kind == "avg"])
    assert len([nm for nm in names if nm.startswith("pool_fwd_")]) == navg == len([nm for nm in names if nm.startswith("pool_bwd_")])
    assert ("gpool_fwd" in names) == ("gpool_bwd" in names) == (g._executor.plan.gpool is not None)
    arena = g._executor.arena.clone()                  # the packs mirror the master
    g._executor.params_changed()
    torch.cuda.synchronize()
    assert torch.equal(arena, g._executor.arena)


@pytest.mark.parametrize("kind", M.KINDS)
def test_grads_match_the_bf16_reference(kind, monkeypatch):
    """tests/test_hip_model.py::test_grads_match_bf16_reference's standard (per tensor: relative
    error <= 5e-2, cosine > 0.995) against the CPU executor with the GPU's bf16 storage points."""
    monkeypatch.setenv("INTML_TUNE", "ref_bf16=1")
    g, c = _pair(kind, lambda: optim.SGD(lr=0.0))
    assert c._executor.emulate_bf16
    x, y = _data(g, 48)
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
        if not getattr(s, "trainable", True):
            continue
        a, b = gg[s.offset:s.offset + s.numel], cg[s.offset:s.offset + s.numel]
        err = _rel(a, b)
        cos = float(np.dot(a, b) / max(np.linalg.norm(a) * np.linalg.norm(b), 1e-30))
        worst.append((err, cos, s.name))
    print("%s: worst grad rel err %.3g (cos %.6f) at %s" % ((kind,) + max(worst)))
    for err, cos, nm in worst:
        assert err <= 5e-2 and cos > 0.995, "%s: grad rel err %.3g cos %.6f" % (nm, err, cos)
    lg, lc = g._executor.read_metrics()[0], c._executor.read_metrics()[0]
    assert abs(lg - lc) < 1e-3 * max(1.0, abs(lc)), (lg, lc)


@pytest.mark.parametrize("kind", ["avg_odd_gap", "max_gmp", "tanh_avg"])
def test_predict_and_evaluate_match(kind):
    g, c = _pair(kind, optim.Adam)
    x, y = _data(g, 21, seed=5)
    pg, pc = g.predict(x, batch_size=8), c.predict(x, batch_size=8)
    assert pg.shape == pc.shape and np.abs(pg - pc).max() < 2e-2
    eg, ec = g.evaluate(x, y, batch_size=8, verbose=0), c.evaluate(x, y, batch_size=8, verbose=0)
    assert abs(eg[0] - ec[0]) < 2e-2 * max(1, ec[0])
    plans = g._executor._plans
    assert {"eval", "predict"} <= {k[1] for k in plans}
    for k, p in plans.items():
        names = [l.name for l in p.launches]
        assert not [n for n in names if "pool_bwd" in n]
        pools = [l for l in p.launches if l.name.startswith(("pool_fwd_", "gpool_fwd"))]
        assert pools and all(l.args["pool"].drop_thr == 0 and l.args["pool"].idx == 0 for l in pools)


def test_graph_of_8_steps_equals_8_single_steps():
    res = []
    for chunks in ([1] * 8, [8]):
        set_random_seed(21)
        m = M.avg_odd_gap(optim.Adam(decay=0.01), device="cuda", drop=0.2)
        x, y = _data(m, 64, seed=4)
        ex = m._executor
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
    for a, b in zip(res[0][0], res[1][0]):
        assert torch.equal(a, b)
    assert res[0][1] == res[1][1] and res[0][1][2] == 64 and res[0][2] == res[1][2] == 8


def test_eager_launches_equal_the_graph_replay(monkeypatch):
    """INTML_GRAPHS=0 issues the same launches eagerly: bit-identical weights (GlobalMaxPooling2D model)."""
    res = []
    for graphs in ("1", "0"):
        monkeypatch.setenv("INTML_GRAPHS", graphs)
        set_random_seed(22)
        m = M.max_gmp(optim.Adam(), device="cuda", drop=0.2)
        x, y = _data(m, 64, seed=4)
        ex = m._executor
        assert ex.use_graphs == (graphs == "1")
        d = ex.upload(x, y)
        perm = torch.arange(d.n, device=ex.device)
        for k in range(8):
            ex.train_step(d, perm, 8 * k, 8)
        torch.cuda.synchronize()
        res.append(m.store.master[:m.store.numel].clone())
    assert torch.equal(res[0], res[1])


def test_gpu_checkpoint_loads_on_cpu_and_continues(tmp_path):
    set_random_seed(8)
    m = M.avg_odd_gap(optim.Adam(lr=0.01), "cuda", drop=0.1)
    x, y = _data(m, 48, seed=1)
    m.fit(x[:32], y[:32], batch_size=8, epochs=1, verbose=0, shuffle=False)
    p = str(tmp_path / "g.h5")
    m.save(p)
    c = load_model(p, device="cpu")
    assert c.store.master.device.type == "cpu" and c.optimizer.iterations == m.optimizer.iterations == 4
    assert [l.get_config() for l in c.layers] == [l.get_config() for l in m.layers]
    assert [s.pool_kind for s in c._executor.plan.convs] == ["avg", "avg"] and c._executor.plan.gpool.mode == "avg"
    for a, b in zip(m.get_weights(), c.get_weights()):
        np.testing.assert_array_equal(a, b)
    assert np.abs(c.predict(x[32:], batch_size=16) - m.predict(x[32:], batch_size=16)).max() < 2e-2
    n = c.store.numel
    w0 = c.store.master[:n].clone()
    lc, lg = c.train_on_batch(x[32:], y[32:]), m.train_on_batch(x[32:], y[32:])
    torch.cuda.synchronize()
    assert abs(lc[0] - lg[0]) < 2e-2 * max(1.0, lg[0])
    assert float((c.store.master[:n] - w0).abs().max()) > 1e-4
    assert _rel(m.store.master[:n].cpu().numpy(), c.store.master[:n].numpy()) < 1e-2


def test_average_pooling_on_a_batchnorm_stage_raises():
    from cori_intml_examples_amd.models import (Activation, AveragePooling2D, BatchNormalization, Conv2D, Dense, Flatten,
                                                Input, Model)
    inp = Input(shape=(8, 8, 3))
    h = AveragePooling2D()(Activation("relu")(BatchNormalization()(Conv2D(4, (3, 3))(inp))))
    m = Model(inp, Dense(1, activation="sigmoid")(Flatten()(h)), device="cuda")
    with pytest.raises(NotImplementedError) as e:
        m.compile(optimizer="Adam", loss="binary_crossentropy")
    assert "average_pooling2d_1" in str(e.value) and "batch_normalization_1" in str(e.value)


# ------------------------------------------------------------------------------------ 6. plans
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


def _rpv(**kw):
    from cori_intml_examples_amd.apps import zoo
    set_random_seed(57)
    return zoo.rpv_cnn((64, 64, 3), conv_sizes=[16, 32, 64], fc_sizes=[128], dropout=0.2, optimizer="Adam", lr=1e-3,
                       device="cuda", **kw)


# the default RPV training step: 8 launches, the conv stack first, no prologue
RPV_TRAIN = ["conv_stack_fwd", "dense_fwd0", "head", "dense_bwd0", "wgrad_dgrad_conv2", "wgrad_dgrad_conv1",
             "wgrad_conv0", "reduce_b0"]
MNIST_TRAIN = ["conv_stack_fwd", "dense_fwd0", "head", "dense_bwd0", "wgrad_dgrad_conv1", "wgrad_conv0", "reduce_b0"]


def test_plans_without_new_pooling_are_unchanged(monkeypatch):
    """Models without the new layers record the launch lists they record without this feature: the
    default RPV step (8 launches with the conv stack) and the default MNIST step, pinned by name as
    tests/test_step_program.py records them, and for the MNIST, legacy, tanh and BatchNormalization
    models the builders' defaults against pool="max", global_pool=None given explicitly, none with
    a pool_* / gpool_* launch or a pooling buffer."""
    from cori_intml_examples_amd.apps import zoo
    monkeypatch.delenv("INTML_TUNE", raising=False)
    set_random_seed(57)
    absent = _build("rpv_bench", "cuda", opt="Adam", drop=0.2, cin=3, hw=64)
    ref = _plan_names(absent)
    plan = absent._executor._plans[(128, "train")]
    assert plan.early_red and plan.optim_fused and plan.pro_free and not plan.avg and plan.gp is None
    print(ref["train"])
    assert ref["train"] == RPV_TRAIN and len(ref["train"]) == 8
    assert ref["eval"][0] == ref["predict"][0] == "conv_stack_fwd"
    assert _plan_names(_rpv(pool="max", global_pool=None)) == ref
    builds = [lambda **kw: zoo.mnist_cnn(32, 64, 128, dropout=0.4, optimizer="Adam", lr=1e-3, device="cuda", **kw),
              lambda **kw: zoo.rpv_legacy_cnn((32, 32, 1), optimizer="Adam", lr=1e-3, h1=8, h2=16, h3=16, h4=16, h5=32,
                                              device="cuda", **kw),
              lambda **kw: _rpv(activation="tanh", **kw), lambda **kw: _rpv(batch_norm=True, **kw)]
    for build in builds:
        set_random_seed(57)
        a = _plan_names(build(), 32)
        set_random_seed(57)
        b = _plan_names(build(pool="max", global_pool=None), 32)
        assert a == b
        assert not [nm for mode in a for nm in a[mode] if "pool_" in nm]
    assert _plan_names(_build("mnist_bench", "cuda", opt="Adam", drop=0.4, cin=1, hw=28))["train"] == MNIST_TRAIN


def test_pooling_takes_the_per_layer_structure(monkeypatch):
    monkeypatch.delenv("INTML_TUNE", raising=False)
    avg = _plan_names(_rpv(pool="avg"))
    gap = _plan_names(_rpv(global_pool="avg"))
    both = _plan_names(_rpv(pool="avg", global_pool="max", activation="tanh"))
    for names in (avg, gap, both):
        for mode in names:
            assert "conv_stack_fwd" not in names[mode] and names[mode][0] == "prologue"
    pools = lambda ns: [n for n in ns if "pool_" in n]
    assert pools(avg["train"]) == ["pool_fwd_c0", "pool_fwd_c1", "pool_fwd_c2", "pool_bwd_c2", "pool_bwd_c1", "pool_bwd_c0"]
    assert pools(avg["eval"]) == pools(avg["predict"]) == ["pool_fwd_c0", "pool_fwd_c1", "pool_fwd_c2"]
    assert pools(gap["train"]) == ["gpool_fwd", "gpool_bwd"] and pools(gap["eval"]) == pools(gap["predict"]) == ["gpool_fwd"]
    tr = avg["train"]
    for i, nm in enumerate(tr):
        if nm.startswith("pool_fwd_c"):
            assert tr[i - 1] == "conv_fwd" + nm[-1]
        if nm.startswith("pool_bwd_c"):
            assert tr[i - 1] == "head" or tr[i - 1].startswith(("dense_dx", "dense_bwd", "dgrad_conv", "wgrad_dgrad_conv"))
            assert tr[i + 1].startswith(("wgrad_dgrad_conv", "wgrad_conv")) and tr[i + 1].endswith(nm[-1])
    tr = gap["train"]
    i = tr.index("gpool_fwd")
    assert tr[i - 1] == "conv_fwd2" and tr[i + 1] == "dense_fwd0"
    i = tr.index("gpool_bwd")
    assert tr[i - 1].startswith(("dense_dx0", "dense_bwd0")) and tr[i + 1].startswith(("wgrad_dgrad_conv2", "wgrad_conv2"))
    # tanh + avg + global max: conv -> act_fwd -> pool_fwd, ... gpool_bwd -> pool_bwd -> act_bwd -> wgrad / dgrad
    tr = both["train"]
    for c in "012":
        i = tr.index("conv_fwd" + c)
        assert tr[i + 1:i + 3] == ["act_fwd_c" + c, "pool_fwd_c" + c]
        i = tr.index("pool_bwd_c" + c)
        assert tr[i + 1] == "act_bwd_c" + c and tr[i + 2].endswith("conv" + c)
    assert tr[tr.index("gpool_bwd") + 1] == "pool_bwd_c2" and tr[tr.index("pool_fwd_c2") + 1] == "gpool_fwd"
    # ... the per-layer relu structure plus exactly those launches
    monkeypatch.setenv("INTML_TUNE", PERLAYER)
    un = _plan_names(_rpv())
    for mode in avg:
        assert [n for n in avg[mode] if "pool_" not in n] == un[mode], mode
    # (a global pooling model's dense layer is 64 wide, not 4096: the same launch names all the same)
    for mode in gap:
        assert [n for n in gap[mode] if "pool_" not in n] == un[mode], mode


# ------------------------------------------------------------------------------------ 7. data parallel
def test_data_parallel_step_at_one_rank(tmp_path):
    out = tmp_path / "dp.json"
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("WORLD_SIZE", "RANK", "INTML_DP_BACKEND", "INTML_COMM", "INTML_XGMI", "INTML_TUNE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pool_dp_worker_gpu.py"), str(out)],
                       env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rep = json.load(open(out))
    print(json.dumps(rep, indent=1))
    assert rep["native"] and rep["moved"] > 1e-4, rep
    pools = [n for n in rep["base_launches"] if "pool_" in n]
    assert pools == ["pool_fwd_c0", "pool_fwd_c1", "gpool_fwd", "gpool_bwd", "pool_bwd_c1", "pool_bwd_c0"]
    for mode in ("captured", "segmented"):
        c = rep[mode]
        assert c["reducer"] == "NativeGradReducer" and c["comm_in_graph"] == (mode == "captured"), c
        assert [n for n in c["launches"] if "pool_" in n] == pools, c
        assert c["iterations"] == 4 and all(c["identical"]), (mode, c)
