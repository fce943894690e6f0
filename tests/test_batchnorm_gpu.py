"""BatchNormalization on the GPU: the four bn.hip kernels alone in NaN / sentinel-filled buffers
against the float64 oracle (statistics within the bound of the kernel's own addition chain, outputs
within one bf16 ulp, pool routing with negative gamma, the backward sums and dz), and the whole step
(the CPU reference executor, moving statistics, evaluate / predict, graph replay, clipping and
regularizers, plan gating, data parallel at one rank, the xGMI gate, checkpoints)."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cori_intml_examples_amd import optim, regularizers
from cori_intml_examples_amd.io.datasets import synthetic_rpv
from cori_intml_examples_amd.io.keras_h5 import load_model
from cori_intml_examples_amd.models.step_program import dropout_pair
from cori_intml_examples_amd.ops.rng import dropout_keep
from cori_intml_examples_amd.utils import set_random_seed

from helpers import bn_models as M
from helpers import bn_oracle as O
from test_hip_model import _build, _data, _rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

U = 2.0 ** -24                           # unit roundoff of fp32
EPS = 1e-3
PERLAYER = "conv_stack=0,fuse_head=0"


def _K():
    from cori_intml_examples_amd.ops.hip import kernels
    return kernels()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def r8(c):
    return (c + 7) // 8 * 8


# ------------------------------------------------------------------------------------ kernel harness
class Stage:
    """One BN stage's buffers, NaN / sentinel filled, and its BnArgs."""

    def __init__(self, z, C, gamma=None, beta=None, relu=False, pool=False, momentum=0.0, drop=0.0, mm=None, mv=None):
        K = _K()
        self.K, self.C = K, C
        shape = tuple(z.shape)
        Cs = shape[-1]
        assert Cs == r8(C)
        self.conv = len(shape) == 4
        self.rows = int(np.prod(shape[:-1]))
        zt = torch.as_tensor(np.asarray(z, np.float32)).to(torch.bfloat16)
        assert torch.equal(zt.float(), torch.as_tensor(np.asarray(z, np.float32))), "inputs must be exact in bf16"
        zt[..., C:] = 0
        self.z = zt.cuda().contiguous()
        chunk, nchunks, lg = K.bn_plan(self.rows, Cs)
        self.plan = (chunk, nchunks, lg)
        f32 = dict(dtype=torch.float32, device="cuda")
        nan = float("nan")
        self.part = torch.full((2, nchunks, Cs), nan, **f32)
        self.saved = torch.full((2, Cs), nan, **f32)
        self.slab = torch.full((nchunks, 2, C), nan, **f32)       # per chunk: dgamma[C], dbeta[C]
        self.gamma = torch.as_tensor(np.asarray(gamma, np.float32)).cuda() if gamma is not None else None
        self.beta = torch.as_tensor(np.asarray(beta, np.float32)).cuda() if beta is not None else None
        self.mm = torch.as_tensor(np.asarray(mm if mm is not None else np.zeros(C), np.float32)).cuda()
        self.mv = torch.as_tensor(np.asarray(mv if mv is not None else np.ones(C), np.float32)).cuda()
        if self.conv and pool:
            B, H, W, _ = shape
            oshape = (B, H // 2, W // 2, Cs)
        else:
            oshape = shape
        self.out = torch.full(oshape, nan, dtype=torch.bfloat16, device="cuda")
        self.code = torch.full(oshape, 0xEE, dtype=torch.uint8, device="cuda") if pool else None
        self.dz = torch.full(shape, nan, dtype=torch.bfloat16, device="cuda")
        self.dp = None
        a = K.BnArgs()
        a.z, a.rows, a.C, a.Cs = self.z.data_ptr(), self.rows, C, Cs
        a.chunk, a.nchunks, a.gp_log2 = chunk, nchunks, lg
        if self.conv:
            a.B, a.Ho, a.Wo = shape[0], shape[1], shape[2]
            a.Hp, a.Wp, a.pool = (shape[1] // 2, shape[2] // 2, 1) if pool else (shape[1], shape[2], 0)
        else:
            a.B = shape[0]
        a.part, a.saved, a.slab = self.part.data_ptr(), self.saved.data_ptr(), self.slab.data_ptr()
        if self.gamma is not None:
            a.gamma = self.gamma.data_ptr()
        if self.beta is not None:
            a.beta = self.beta.data_ptr()
        a.moving_mean, a.moving_var = self.mm.data_ptr(), self.mv.data_ptr()
        a.eps, a.momentum = EPS, momentum
        a.unbias = self.rows / (self.rows - (1.0 + EPS))
        a.training, a.relu = 1, int(relu)
        a.out = self.out.data_ptr()
        if pool:
            a.code = self.code.data_ptr()
        if drop:
            a.drop_thr, a.drop_scale = dropout_pair(drop)
            a.seed, a.stream_id = 77, 3
        a.dz = self.dz.data_ptr()
        self.a = a

    def forward(self, training=True):
        self.a.training = int(training)
        if training:
            self.K.bn_stats(self.a, _stream())
        self.K.bn_apply_fwd(self.a, _stream())
        torch.cuda.synchronize()

    def backward(self, dp):
        self.dp = torch.as_tensor(np.asarray(dp, np.float32)).to(torch.bfloat16).cuda().contiguous()
        assert self.dp.shape == self.out.shape
        self.a.dp = self.dp.data_ptr()
        self.K.bn_bwd_reduce(self.a, _stream())
        self.K.bn_bwd_apply(self.a, _stream())
        torch.cuda.synchronize()

    # the kernel's addition chains (bn.hip): a thread adds ceil(chunk / R) rows, the workgroup tree
    # adds log2(R) levels; the chunk combine has ceil(nchunks / R) + log2(R) steps of about four
    # roundings each
    def depths(self):
        chunk, nchunks, lg = self.plan
        R = self.K.BN_THREADS >> lg
        d_chunk = math.ceil(min(chunk, self.rows) / R) + int(math.log2(R))
        d_comb = 4 * (math.ceil(nchunks / R) + int(math.log2(R)))
        return d_chunk, d_comb


def _grid_values(rng, shape, lo=-16, hi=16, step=0.25):
    """Random multiples of ``step``: exact in bf16, distinct values at least one step apart."""
    return rng.integers(int(lo / step), int(hi / step), size=shape).astype(np.float64) * step


def _inputs(B, H, W, C, seed, dense=False):
    """z with a far-off-centre channel: channel 1 holds 64 + 0.5 k, k = 0..4 (exact in bf16; |mean| / std
    is about 90)."""
    rng = np.random.default_rng(seed)
    shape = (B, r8(C)) if dense else (B, H, W, r8(C))
    z = O.bf16_round(rng.normal(0.3, 1.5, size=shape))
    if C > 1:
        k = rng.integers(0, 5, size=shape[:-1])
        z[..., 1] = 64.0 + 0.5 * k
    z[..., C:] = 0.0
    return z


SHAPES = [(3, 5, 5), (3, 21, 21), (3, 37, 37), (2, 64, 66)]       # 1, 2, 5 and 9 partials (chunks of 1024 rows)


@pytest.mark.parametrize("C", [3, 16, 20])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_statistics_and_outputs_against_the_oracle(shape, C):
    """momentum = 0, so the moving statistics ARE the batch mean and variance * m / (m - (1 + eps)).
    The bounds are those of the kernel's chain: (depth) * 2^-24 * sum |terms| / m -- for the
    variance with the CENTRED terms (z - mean)^2, which a cancelling E[z^2] - E[z]^2 misses by orders
    of magnitude on channel 1 (its E[z^2] is about 4300, its variance 0.5)."""
    B, H, W = shape
    z = _inputs(B, H, W, C, seed=C * 100 + H)
    rng = np.random.default_rng(5)
    gamma, beta = rng.normal(0.5, 1.0, C), rng.normal(0, 1, C)
    gamma[0] = -abs(gamma[0]) - 0.1
    st = Stage(z, C, gamma, beta, relu=True, pool=True)
    parts = {1024 * 0 + 75: 1, 1323: 2, 4107: 5, 8448: 9}
    assert st.plan[1] == parts[st.rows], st.plan
    st.forward()
    g32, b32 = st.gamma.cpu().double().numpy(), st.beta.cpu().double().numpy()
    zr = z[..., :C]
    u, xhat, mean, var, m = O.forward_train(zr, g32, b32, EPS)
    d_chunk, d_comb = st.depths()
    bound_mean = (d_chunk + d_comb + 2) * U * np.abs(zr).reshape(-1, C).sum(0) / m
    bound_var = ((d_chunk + d_comb + 8) * U * var + bound_mean ** 2) + 3 * U * var
    got_mean = st.mm.cpu().double().numpy()
    got_var = st.mv.cpu().double().numpy() / float(np.float32(st.a.unbias))
    print("C=%d %s: |mean err| / bound %.3g, |var err| / bound %.3g (channel 1: var %.6g got %.6g)" % (
        C, shape, (np.abs(got_mean - mean) / bound_mean).max(), (np.abs(got_var - var) / bound_var).max(), var[1], got_var[1]))
    assert np.all(np.abs(got_mean - mean) <= bound_mean)
    assert np.all(np.abs(got_var - var) <= bound_var)
    saved = st.saved.cpu().double().numpy()
    assert np.array_equal(saved[0, :C], got_mean)
    assert np.allclose(saved[1, :C], 1 / np.sqrt(var + EPS), rtol=1e-5, atol=0)     # (half the variance's bound)
    # outputs: relu(u) pooled, one bf16 rounding
    want = O.maxpool2x2(np.maximum(u, 0.0))[0]
    out = st.out.float().cpu().double().numpy()
    assert np.all(np.isfinite(out))
    err = np.abs(out[..., :C] - want)
    # (+ the fp32 evaluation of u from the fp32 mean, which matters only where relu(u) is about 0)
    inv = 1 / np.sqrt(var + EPS)
    slack = (np.abs(g32) * ((bound_mean + U * np.abs(mean)) * inv + 8 * U * np.abs(xhat).reshape(-1, C).max(0))
             + 4 * U * np.abs(b32))
    assert np.all(err <= O.bf16_ulp(want) + slack), (err - O.bf16_ulp(want) - slack).max()
    assert np.all(out[..., C:] == 0) and np.all(st.code.cpu().numpy()[..., C:] == 0)       # padding lanes
    assert st.code.cpu().numpy().max() <= 3
    # repeated launches: bit-identical
    first = (st.out.clone(), st.code.clone(), st.saved.clone(), st.part.clone())
    st.forward()
    for a, b in zip(first, (st.out, st.code, st.saved, st.part)):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_one_row_gives_zero_variance_and_beta():
    """m = 1: var = 0 exactly, xhat = 0, u = beta; the moving variance receives 0 * (1 - momentum)."""
    C = 5
    z = np.zeros((1, 8))
    z[0, :C] = [3.0, -2.5, 100.0, 0.0, 1e-3 * 0 + 7.0]
    beta = np.array([0.5, -1.0, 2.0, 0.0, 3.0])
    st = Stage(z, C, np.full(C, 1.5), beta, momentum=0.5, mv=np.full(C, 2.0), mm=np.full(C, 1.0))
    st.forward()
    assert np.array_equal(st.out.float().cpu().numpy()[0, :C], beta.astype(np.float32))
    assert np.array_equal(st.mv.cpu().numpy(), np.full(C, 1.0, np.float32))        # 2 * 0.5 + 0 * 0.5
    assert np.array_equal(st.mm.cpu().numpy(), (0.5 + 0.5 * z[0, :C]).astype(np.float32))
    st.backward(np.ones((1, 8)))
    assert np.all(st.dz.float().cpu().numpy() == 0)


@pytest.mark.parametrize("dense", [False, True])
def test_unpooled_dropout_and_evaluation_forms(dense):
    """Un-pooled stage (a dense layer's, and a conv's with an odd channel count): the dropout of the
    fused epilogues' counter RNG, and the evaluation form, which reads the moving statistics and
    writes nothing but the output."""
    C = 20
    z = _inputs(37, 3, 3, C, seed=9, dense=dense)
    rng = np.random.default_rng(2)
    gamma, beta = rng.normal(0, 1, C), rng.normal(0, 1, C)
    mm, mv = rng.normal(0, 1, C), rng.uniform(0.5, 2, C)
    st = Stage(z, C, gamma, beta, momentum=0.9, drop=0.25, mm=mm, mv=mv)
    st.forward()
    g32, b32 = st.gamma.cpu().double().numpy(), st.beta.cpu().double().numpy()
    u, _, mean, var, m = O.forward_train(z[..., :C], g32, b32, EPS)
    keep = dropout_keep(u.size, 0.25, 77, 3, 0).numpy().reshape(u.shape)
    want = np.where(keep, u * float(np.float32(dropout_pair(0.25)[1])), 0.0)
    out = st.out.float().cpu().double().numpy()
    assert np.all(np.abs(out[..., :C] - want) <= O.bf16_ulp(want))
    assert np.all(out[..., C:] == 0)
    wm, wv = O.moving_update(np.float32(mm), np.float32(mv), mean, var, m, np.float32(0.9), EPS)
    # (fp32 sums of 37 or 333 terms of size about 2, then times 1 - momentum)
    assert np.allclose(st.mm.cpu().numpy(), wm, rtol=2e-6, atol=2e-6)
    assert np.allclose(st.mv.cpu().numpy(), wv, rtol=2e-6, atol=2e-6)
    # evaluation form
    mm1, mv1 = st.mm.clone(), st.mv.clone()
    st.saved.fill_(float("nan"))
    st.out.fill_(float("nan"))
    st.a.drop_thr = 0                                          # (an evaluation step drops nothing)
    st.forward(training=False)
    assert torch.equal(mm1, st.mm) and torch.equal(mv1, st.mv) and bool(torch.isnan(st.saved).all())
    want = O.forward_eval(z[..., :C], g32, b32, mm1.cpu().double().numpy(), mv1.cpu().double().numpy(), EPS)
    out = st.out.float().cpu().double().numpy()
    assert np.all(np.abs(out[..., :C] - want) <= O.bf16_ulp(want)) and np.all(out[..., C:] == 0)


@pytest.mark.parametrize("C", [3, 20])
def test_pool_routing_with_negative_gamma(C):
    """z on a grid of 0.25 (exact in bf16): within a window the candidates are exactly tied (then
    the first position wins, for either sign of gamma) or at least 0.25 apart, far beyond the fp32
    rounding of u -- so the codes must equal the oracle's exactly; channels with a negative gamma
    must differ from a pool-first computation."""
    rng = np.random.default_rng(C)
    B, H, W = 3, 9, 11
    z = np.zeros((B, H, W, r8(C)))
    z[..., :C] = _grid_values(rng, (B, H, W, C), -2, 2)            # 16 values: many ties
    gamma = np.where(np.arange(C) % 2 == 0, -1.25, 0.75)
    beta = rng.normal(0, 1, C)
    st = Stage(z, C, gamma, beta, pool=True)
    st.forward()
    u = O.forward_train(z[..., :C], gamma, np.float32(beta).astype(np.float64), EPS)[0]
    want, code = O.maxpool2x2(u)
    got = st.code.cpu().numpy()[..., :C]
    assert np.array_equal(got, code)
    assert np.all(np.abs(st.out.float().cpu().double().numpy()[..., :C] - want) <= O.bf16_ulp(want))
    first = O.maxpool2x2(z[..., :C])[1]                       # "pool first": the argmax of z
    neg = np.arange(C) % 2 == 0
    assert (got[..., neg] != first[..., neg]).mean() > 0.3 and np.array_equal(got[..., ~neg], first[..., ~neg])
    tied = (np.sort(np.stack([z[:, dy:8:2, dx:10:2, :C] for dy in (0, 1) for dx in (0, 1)], 3), 3)[..., -1, :]
            == np.sort(np.stack([z[:, dy:8:2, dx:10:2, :C] for dy in (0, 1) for dx in (0, 1)], 3), 3)[..., -2, :])
    assert tied.mean() > 0.05                                 # the inputs do hold tied maxima


@pytest.mark.parametrize("pool", [True, False])
@pytest.mark.parametrize("shape,C", [((3, 5, 5), 3), ((3, 21, 21), 16), ((3, 37, 37), 20)], ids=["75x3", "1323x16", "4107x20"])
def test_backward_sums_and_dz(shape, C, pool):
    """dbeta / dgamma (the slabs summed in float64) within their addition-chain bound, and dz within
    one bf16 ulp of the oracle plus what those bounds propagate.  Odd sizes: the last row and column
    are outside every window -- counted in the statistics, du = 0 there, dz != 0."""
    B, H, W = shape
    rng = np.random.default_rng(C + H)
    z = np.zeros((B, H, W, r8(C)))
    z[..., :C] = _grid_values(rng, (B, H, W, C))
    if C > 1:
        z[..., 1] = 64.0 + 0.5 * rng.integers(0, 5, size=(B, H, W))
    gamma, beta = rng.normal(0.3, 1.0, C), rng.normal(0, 1, C)
    st = Stage(z, C, gamma, beta, pool=pool)
    st.forward()
    g64 = st.gamma.cpu().double().numpy()
    u, xhat, mean, var, m = O.forward_train(z[..., :C], g64, st.beta.cpu().double().numpy(), EPS)
    dp = O.bf16_round(rng.normal(0, 1, size=tuple(st.out.shape)))
    dp[..., C:] = 0
    st.backward(dp)
    if pool:
        code = O.maxpool2x2(u)[1]
        assert np.array_equal(code, st.code.cpu().numpy()[..., :C])
        du = O.route(dp[..., :C], code, (H, W))
        assert np.all(du[:, 2 * (H // 2):, :, :] == 0) and np.all(du[:, :, 2 * (W // 2):, :] == 0)
    else:
        du = dp[..., :C]
    dz, dgamma, dbeta = O.backward(du, xhat, g64, var, EPS)
    slab = st.slab.cpu().double().numpy()
    assert np.all(np.isfinite(slab))
    got_dg, got_db = slab[:, 0].sum(0), slab[:, 1].sum(0)
    d_chunk, d_comb = st.depths()
    inv = 1 / np.sqrt(var + EPS)
    # xhat in fp32 from the kernel's fp32 mean: |z - mean| rounding, the mean's own error and rounding
    bound_mean = (d_chunk + d_comb + 2) * U * np.abs(z[..., :C]).reshape(-1, C).sum(0) / m
    err_xhat = (bound_mean + U * np.abs(mean)) * inv + 4 * U * np.abs(xhat)
    bound_db = (d_chunk + 1) * U * np.abs(du).reshape(-1, C).sum(0)
    bound_dg = ((d_chunk + 3) * U * np.abs(du * xhat).reshape(-1, C).sum(0) + (np.abs(du) * err_xhat).reshape(-1, C).sum(0))
    print("%s C=%d pool=%d: dbeta err / bound %.3g, dgamma err / bound %.3g" % (
        shape, C, pool, (np.abs(got_db - dbeta) / np.maximum(bound_db, 1e-300)).max(),
        (np.abs(got_dg - dgamma) / np.maximum(bound_dg, 1e-300)).max()))
    assert np.all(np.abs(got_db - dbeta) <= bound_db)
    assert np.all(np.abs(got_dg - dgamma) <= bound_dg)
    ginv = np.abs(g64) * inv
    d_sum = d_comb + 2                                      # the fixed-order sum of the slabs
    prop = ginv * ((bound_db + d_sum * U * np.abs(dbeta)) / m + np.abs(xhat) * (bound_dg + d_sum * U * np.abs(dgamma)) / m
                   + err_xhat * np.abs(dgamma) / m + 8 * U * (np.abs(du) + np.abs(dbeta) / m + np.abs(xhat * dgamma) / m))
    got = st.dz.float().cpu().double().numpy()
    assert np.all(np.isfinite(got)) and np.all(got[..., C:] == 0)
    err = np.abs(got[..., :C] - dz)
    assert np.all(err <= O.bf16_ulp(dz) + prop), (err - O.bf16_ulp(dz) - prop).max()
    if pool and H % 2:
        assert np.abs(got[:, H - 1, :, :C]).max() > 0 and np.abs(got[:, :, W - 1, :C]).max() > 0
    first = (st.slab.clone(), st.dz.clone())
    st.backward(dp)
    assert torch.equal(first[0], st.slab) and torch.equal(first[1].view(torch.int16), st.dz.view(torch.int16))


def test_launchers_refuse_bad_arguments():
    K = _K()
    st = Stage(_inputs(3, 5, 5, 3, seed=1), 3, np.ones(3), np.zeros(3), pool=True)
    st.forward()
    st.backward(np.zeros(tuple(st.out.shape)))

    def bad(fn, **kw):
        old = {k: getattr(st.a, k) for k in kw}
        for k, v in kw.items():
            setattr(st.a, k, v)
        with pytest.raises(ValueError):
            fn(st.a, _stream())
        for k, v in old.items():
            setattr(st.a, k, v)

    for fn in (K.bn_stats, K.bn_apply_fwd, K.bn_bwd_reduce, K.bn_bwd_apply):
        bad(fn, Cs=12)
        bad(fn, C=9)
        bad(fn, rows=0)
        bad(fn, chunk=512)
        bad(fn, nchunks=2)
        bad(fn, z=0)
        bad(fn, Hp=3)
        bad(fn, rows=76)
    bad(K.bn_apply_fwd, eps=0.0)
    bad(K.bn_apply_fwd, momentum=1.0)
    bad(K.bn_apply_fwd, out=0)
    bad(K.bn_apply_fwd, code=0)
    bad(K.bn_apply_fwd, part=0)
    bad(K.bn_stats, part=4)
    bad(K.bn_bwd_reduce, dp=0)
    bad(K.bn_bwd_reduce, slab=0)
    bad(K.bn_bwd_apply, dz=0)
    bad(K.bn_bwd_apply, saved=0)
    assert K.bn_plan(75, 8) == (K.BN_MIN_CHUNK, 1, 0) and K.bn_plan(4107, 24) == (1024, 5, 2)
    assert K.bn_plan(1 << 20, 512) == (4096, 256, 5)
    with pytest.raises(ValueError):
        K.bn_plan(0, 8)


# ------------------------------------------------------------------------------------ the whole step
ACTS = ["relu", "tanh", ("LeakyReLU", 0.3)]
_ids = lambda c: c if isinstance(c, str) else "%s%g" % c
BS = 6


def _pair(kind, act, mk, drop=0.2, **kw):
    set_random_seed(1234)
    g = M.build(kind, mk(), "cuda", drop=drop, act=act, **kw)
    set_random_seed(1234)
    c = M.build(kind, mk(), "cpu", drop=drop, act=act, **kw)
    assert g._seed == c._seed
    # gamma / beta off their initial ones / zeros (a negative gamma too), so they matter
    rng = np.random.default_rng(3)
    ws = []
    for w, s in zip(c.get_weights(), c.store.specs):
        if s.short == "gamma":
            w = rng.normal(0.8, 0.5, w.shape).astype(np.float32)
            w[0] = -abs(w[0]) - 0.2
        elif s.short == "beta":
            w = rng.normal(0, 0.3, w.shape).astype(np.float32)
        ws.append(w)
    g.set_weights(ws)
    c.set_weights(ws)
    return g, c


def _steps(models, x, y, sizes=(BS, BS, 4)):
    """Batches of 6, 6 and a ragged last one of 4."""
    for m in models:
        ex = m._executor
        d = ex.upload(x, y)
        perm = torch.arange(d.n, device=ex.device)
        pos = 0
        for bs in sizes:
            ex.train_step(d, perm, pos, bs)
            pos += bs
    torch.cuda.synchronize()


def _moving(m):
    return np.concatenate([m.store.view(s.layer, s.short).detach().cpu().numpy().reshape(-1)
                           for s in m.store.specs if not s.trainable])


def _bn_names(names):
    return [n for n in names if n.startswith("bn_")]


@pytest.mark.parametrize("kind", ["tiny", "odd"])
@pytest.mark.parametrize("act,mk", [(a, optim.Adam) for a in ACTS]
                         + [("relu", lambda: optim.SGD(momentum=0.9)), ("relu", lambda: optim.Adam(amsgrad=True))],
                         ids=[_ids(a) + "-Adam" for a in ACTS] + ["relu-SGDm", "relu-AMSGrad"])
def test_three_steps_track_the_cpu_reference(act, mk, kind):
    """tests/test_hip_model.py::test_multiple_steps_track_reference's bound (relative L2 error of
    all weights < 1e-2) with BatchNormalization stages, dropout 0.2, batches of 6, 6 and 4; the
    moving statistics after the three steps under the same bound.

    The stand-alone kind is AMSGrad.  The bias ahead of a BN has the exact gradient 0 (BN removes
    it), so what it receives is rounding noise, uncorrelated between the fp32 CPU executor and the
    bf16 GPU step; an optimizer that normalises every element by its own gradient history turns
    that noise into steps of the full learning rate.  At Adam's and AMSGrad's 1e-3 this is a
    fifth of the error budget (measured 1.6e-3 to 1.9e-3); Adagrad's default 1e-2 moves those
    biases ten times as far (measured 1.5e-2 tiny, 5.7e-2 odd, with every loss-relevant gradient
    matching to 1e-5), which says nothing about the kernels.  SGD with momentum runs at Keras'
    default lr = 0.01; at lr = 0.05 the odd model, whose dense BN normalises over 6 and 4 rows,
    measured 2.9e-2 (it moved 7.7e-2), the tiny model 6.4e-3."""
    g, c = _pair(kind, act, mk)
    x, y = _data(g, 16, seed=3)
    n = g.store.numel
    w0 = g.store.master[:n].cpu().numpy()
    _steps((g, c), x, y)
    wg, wc = g.store.master[:n].cpu().numpy(), c.store.master[:n].numpy()
    mg, mc = _moving(g), _moving(c)
    print("%s %s: weights rel err %.3g (moved %.3g), moving statistics rel err %.3g" % (
        _ids(act), kind, _rel(wg, wc), _rel(wg, w0), _rel(mg, mc)))
    assert _rel(wg, wc) < 1e-2
    assert _rel(mg, mc) < 1e-2
    assert not np.array_equal(mc, _moving(M.build(kind, mk(), "cpu", act=act)))
    names = [l.name for l in g._executor._plans[(BS, "train")].launches]
    nbn = 4 if kind == "tiny" else 3
    assert len(_bn_names(names)) == 4 * nbn, names
    arena = g._executor.arena.clone()                  # the packs mirror the master
    g._executor.params_changed()
    torch.cuda.synchronize()
    assert torch.equal(arena, g._executor.arena)


@pytest.mark.parametrize("kind", ["tiny", "odd"])
@pytest.mark.parametrize("act", ACTS, ids=_ids)
def test_grads_match_the_bf16_reference(act, kind, monkeypatch):
    """tests/test_hip_model.py::test_grads_match_bf16_reference's standard (per tensor: relative
    error < 5e-2, cosine > 0.995) against the CPU executor with the GPU's bf16 storage points."""
    monkeypatch.setenv("INTML_TUNE", "ref_bf16=1")
    g, c = _pair(kind, act, lambda: optim.SGD(lr=0.0))
    assert c._executor.emulate_bf16
    x, y = _data(g, BS)
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
        if not s.trainable:
            continue
        a, b = gg[s.offset:s.offset + s.numel], cg[s.offset:s.offset + s.numel]
        err = _rel(a, b)
        cos = float(np.dot(a, b) / max(np.linalg.norm(a) * np.linalg.norm(b), 1e-30))
        worst.append((err, cos, s.name))
        print("%s %s %s: grad rel err %.3g cos %.6f (norm %.3g)" % (_ids(act), kind, s.name, err, cos, np.linalg.norm(b)))
    print("%s %s: worst grad rel err %.3g (cos %.6f) at %s" % ((_ids(act), kind) + max(worst)))
    for err, cos, nm in worst:
        assert err < 5e-2 and cos > 0.995, "%s: grad rel err %.3g cos %.6f" % (nm, err, cos)
    lg, lc = g._executor.read_metrics()[0], c._executor.read_metrics()[0]
    assert abs(lg - lc) < 1e-3 * max(1.0, abs(lc)), (lg, lc)
    assert _rel(_moving(g), _moving(c)) < 1e-2


@pytest.mark.parametrize("kind,act", [("tiny", "relu"), ("odd", "tanh")])
def test_evaluate_and_predict_use_the_moving_statistics(kind, act):
    g, c = _pair(kind, act, optim.Adam)
    x, y = _data(g, 23, seed=5)
    _steps((g, c), x, y)
    c.set_weights(g.get_weights())                     # the same weights AND moving statistics
    before = g.store.master.clone()
    pg, pc = g.predict(x, batch_size=BS), c.predict(x, batch_size=BS)
    assert pg.shape == pc.shape and np.abs(pg - pc).max() < 2e-2
    eg, ec = g.evaluate(x, y, batch_size=BS, verbose=0), c.evaluate(x, y, batch_size=BS, verbose=0)
    assert abs(eg[0] - ec[0]) < 2e-2 * max(1, ec[0])
    torch.cuda.synchronize()
    assert torch.equal(before, g.store.master)         # nothing is updated
    # rows are normalised one by one: a prediction does not depend on its batch
    assert np.array_equal(g.predict(x[:5], batch_size=5), g.predict(x, batch_size=BS)[:5])
    for k, p in g._executor._plans.items():
        if k[1] != "train":
            names = [l.name for l in p.launches]
            assert _bn_names(names) and all(n.startswith("bn_apply_fwd_") for n in _bn_names(names)), names
            assert all(l.args["bn"].training == 0 and l.args["bn"].drop_thr == 0 for l in p.launches if l.name.startswith("bn_"))


def test_graph_of_8_steps_equals_8_single_steps():
    res = []
    for chunks in ([1] * 8, [8]):
        set_random_seed(21)
        m = M.tiny(optim.Adam(decay=0.01), device="cuda", drop=0.2, act="relu")
        x, y = _data(m, 8 * BS, seed=4)
        ex = m._executor
        d = ex.upload(x, y)
        perm = torch.randperm(d.n, generator=torch.Generator().manual_seed(3)).to(ex.device)
        ex.reset_metrics()
        pos = 0
        for k in chunks:
            ex.train_steps(d, perm, pos, BS, k)
            pos += BS * k
        torch.cuda.synchronize()
        n = m.store.numel
        res.append(([m.store.master.clone(), m.store.grad[:n].clone()] + [s.clone() for s in ex.optimizer_state()],
                    ex._metrics(), int(m.optimizer.iterations)))
    for a, b in zip(res[0][0], res[1][0]):
        assert torch.equal(a, b)
    assert res[0][1] == res[1][1] and res[0][1][2] == 8 * BS and res[0][2] == res[1][2] == 8
    assert not torch.equal(res[0][0][0][m.store.capacity:], torch.zeros_like(res[0][0][0][m.store.capacity:]))


def test_clipnorm_and_l2_with_batchnorm_track_the_cpu_reference():
    """clipnorm (gamma / beta gradients are part of the global norm) and an l2 kernel regularizer
    together with BN, against the CPU executor under the three-step bound."""
    from cori_intml_examples_amd.models import (Activation, BatchNormalization, Conv2D, Dense, Dropout, Flatten, Input,
                                                MaxPooling2D, Model)

    def build(device):
        set_random_seed(77)
        inp = Input(shape=(12, 12, 3))
        h = Conv2D(6, (3, 3), padding="same", kernel_regularizer=regularizers.l2(0.01))(inp)
        h = MaxPooling2D()(Activation("relu")(BatchNormalization()(h)))
        h = Flatten()(h)
        h = Dropout(0.2)(Activation("relu")(BatchNormalization()(Dense(12, kernel_regularizer=regularizers.l2(0.01))(h))))
        m = Model(inp, Dense(1, activation="sigmoid")(h), device=device)
        m.compile(optimizer=optim.Adam(lr=0.01, clipnorm=0.05), loss="binary_crossentropy", metrics=["accuracy"])
        return m

    g, c = build("cuda"), build("cpu")
    x, y, _ = synthetic_rpv(16, channels=3, size=12, seed=1)
    _steps((g, c), x, y)
    n = g.store.numel
    wg, wc = g.store.master[:n].cpu().numpy(), c.store.master[:n].numpy()
    print("clipnorm + l2 + BN: rel err %.3g, moving %.3g" % (_rel(wg, wc), _rel(_moving(g), _moving(c))))
    assert _rel(wg, wc) < 1e-2 and _rel(_moving(g), _moving(c)) < 1e-2
    names = [l.name for l in g._executor._plans[(BS, "train")].launches]
    assert "weight_reg" in names and "grad_sqnorm" in names and len(_bn_names(names)) == 8
    assert float(g._executor.clip_state[g._executor.K.CLIP_FACTOR]) < 1.0       # the clip was active


# ------------------------------------------------------------------------------------ gating
def _plan_names(m, bs=128):
    x, y = _data(m, bs, seed=21)
    ex = m._executor
    d = ex.upload(x, y)
    ex.train_steps(d, torch.arange(d.n, device=ex.device), 0, bs, 1)
    ex.eval_step(d, 0, bs)
    ex.predict_step(d, 0, bs)
    torch.cuda.synchronize()
    assert np.isfinite(m.store.master.sum().item())
    return {mode: [l.name for l in ex._plans[(bs, mode)].launches] for mode in ("train", "eval", "predict")}


def _rpv(**kw):
    from cori_intml_examples_amd.apps import zoo
    set_random_seed(57)
    return zoo.rpv_cnn((64, 64, 3), conv_sizes=[16, 32, 64], fc_sizes=[128], dropout=0.2, optimizer="Adam", lr=1e-3,
                       device="cuda", **kw)


def test_plans_without_batchnorm_are_unchanged(monkeypatch):
    """A model without BN records the launch lists it records today (the fused stack, the early
    reduction, the fused optimizer), batch_norm=False is that model, and its store is unchanged."""
    monkeypatch.delenv("INTML_TUNE", raising=False)
    set_random_seed(57)
    absent = _build("rpv_bench", "cuda", opt="Adam", drop=0.2, cin=3, hw=64)
    ref = _plan_names(absent)
    plan = absent._executor._plans[(128, "train")]
    assert plan.early_red and plan.optim_fused and plan.pro_free and not plan.bn
    assert not [nm for mode in ref for nm in ref[mode] if nm.startswith("bn_")]
    assert ref["train"][0] == "conv_stack_fwd" and "dense_epi0" not in ref["train"]
    off = _rpv(batch_norm=False)
    assert _plan_names(off) == ref
    assert off.store.total == off.store.capacity == absent.store.capacity and off.store.master.numel() == off.store.capacity


def test_batchnorm_takes_the_per_layer_structure(monkeypatch):
    monkeypatch.delenv("INTML_TUNE", raising=False)
    names = _plan_names(_rpv(batch_norm=True))
    for mode in names:
        assert "conv_stack_fwd" not in names[mode] and "prologue" in names[mode]
    fwd = [n for t in ("c0", "c1", "c2", "d0") for n in ("bn_stats_" + t, "bn_apply_fwd_" + t)]
    bwd = [n for t in ("d0", "c2", "c1", "c0") for n in ("bn_bwd_reduce_" + t, "bn_bwd_apply_" + t)]
    assert _bn_names(names["train"]) == fwd + bwd
    assert _bn_names(names["eval"]) == _bn_names(names["predict"]) == fwd[1::2]
    tr = names["train"]
    assert "dense_epi0" in tr                          # the head does not run the last dense's epilogue
    for i, nm in enumerate(tr):
        if nm.startswith("bn_stats_"):
            assert tr[i - 1].startswith(("conv_fwd", "dense_epi")) and tr[i + 1].startswith("bn_apply_fwd_")
        if nm.startswith("bn_bwd_reduce_"):
            assert tr[i - 1] == "head" or tr[i - 1].startswith(("dense_dx", "dense_bwd", "dgrad_conv", "wgrad_dgrad_conv"))
            assert tr[i + 1].startswith("bn_bwd_apply_")
    # ... the per-layer relu structure plus the sixteen launches
    monkeypatch.setenv("INTML_TUNE", PERLAYER)
    un = _plan_names(_rpv())
    for mode in names:
        assert [n for n in names[mode] if not n.startswith("bn_")] == un[mode], mode


# ------------------------------------------------------------------------------------ data parallel
def test_data_parallel_step_at_one_rank(tmp_path):
    out = tmp_path / "dp.json"
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("WORLD_SIZE", "RANK", "INTML_DP_BACKEND", "INTML_COMM", "INTML_XGMI", "INTML_TUNE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bn_dp_worker_gpu.py"), str(out)],
                       env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rep = json.load(open(out))
    print(json.dumps(rep, indent=1))
    assert rep["native"] and rep["moved"] > 1e-4 and rep["moving_moved"] > 1e-4, rep
    assert len(_bn_names(rep["base_launches"])) == 16
    for mode in ("captured", "segmented"):
        c = rep[mode]
        assert c["reducer"] == "NativeGradReducer" and c["plane"] == "rccl", c
        assert c["comm_in_graph"] == (mode == "captured"), c
        assert _bn_names(c["launches"]) == _bn_names(rep["base_launches"]), c
        assert c["iterations"] == 4 and all(c["identical"]), (mode, c)
    # the xGMI planes are gated: a ValueError naming the BN layers and the plane when forced
    assert "batch_normalization_1" in rep["xgmi_error"] and "'xgmi'" in rep["xgmi_error"], rep["xgmi_error"]
    assert rep["auto_plane"] == "rccl"


# ------------------------------------------------------------------------------------ checkpoint
def test_gpu_checkpoint_loads_on_cpu_and_continues(tmp_path):
    x, y, _ = synthetic_rpv(96, channels=3, size=16, seed=1)
    set_random_seed(8)
    m = M.tiny(optim.Adam(lr=0.01), device="cuda", drop=0.1, act="relu", momentum=0.9)
    m.fit(x[:64], y[:64], batch_size=16, epochs=1, verbose=0, shuffle=False)
    p = str(tmp_path / "g.h5")
    m.save(p)
    c = load_model(p, device="cpu")
    assert c.store.master.device.type == "cpu" and c.optimizer.iterations == m.optimizer.iterations == 4
    assert [l.get_config() for l in c.layers] == [l.get_config() for l in m.layers]
    assert [s.bn.momentum for s in c._executor.plan.convs] == [0.9] * 3
    for a, b in zip(m.get_weights(), c.get_weights()):
        np.testing.assert_array_equal(a, b)
    assert np.abs(_moving(c) - _moving(M.tiny(optim.Adam(), act="relu"))).max() > 1e-3       # trained statistics
    assert np.abs(c.predict(x[64:], batch_size=32) - m.predict(x[64:], batch_size=32)).max() < 2e-2
    n = c.store.numel
    w0 = c.store.master[:n].clone()
    lc, lg = c.train_on_batch(x[64:], y[64:]), m.train_on_batch(x[64:], y[64:])
    torch.cuda.synchronize()
    assert abs(lc[0] - lg[0]) < 2e-2 * max(1.0, lg[0])
    assert float((c.store.master[:n] - w0).abs().max()) > 1e-4
    # (the loaded model draws a dropout seed of its own: only the first BN, ahead of every dropout,
    # sees the same batch on both sides)
    first = lambda mod: np.concatenate([w.reshape(-1) for w in mod.layers[2].get_weights()[2:]])
    print("first BN's moving statistics after one more batch: rel err %.3g" % _rel(first(m), first(c)))
    assert type(m.layers[2]).__name__ == "BatchNormalization" and _rel(first(m), first(c)) < 1e-2
