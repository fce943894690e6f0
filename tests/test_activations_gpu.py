"""Hidden activations on the GPU: act_fwd_kernel / act_bwd_kernel over every bf16 bit pattern
against the float64 oracle, their layout and dropout, the launchers' checks, and the whole step
(twin identity with relu, the CPU reference executor, pool order, eval / predict, graph replay,
gating, data parallel at one rank, checkpoints)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cori_intml_examples_amd import optim
from cori_intml_examples_amd.io.datasets import synthetic_rpv
from cori_intml_examples_amd.io.keras_h5 import load_model
from cori_intml_examples_amd.models.step_program import dropout_pair
from cori_intml_examples_amd.ops.rng import dropout_keep
from cori_intml_examples_amd.utils import set_random_seed

from helpers import act_models as M
from helpers import act_oracle as O
from test_hip_model import _build, _data, _rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

TINY = 2.0 ** -126                       # below it the hardware may flush: magnitude and sign only
PERLAYER = "conv_stack=0,fuse_head=0"
# the end-to-end cases: the seven strings, LeakyReLU(0.3) and ELU(0.5) layers
E2E = list(O.STRINGS) + [("LeakyReLU", 0.3), ("ELU", 0.5)]
_ids = lambda c: c if isinstance(c, str) else "%s%g" % c


def _K():
    from cori_intml_examples_amd.ops.hip import kernels
    return kernels()


def _bf16(bits):
    """int bit patterns -> bf16 CUDA tensor."""
    return torch.tensor(np.asarray(bits, np.int64).astype(np.uint16).view(np.int16)).view(torch.bfloat16).cuda()


def _args(K, name, alpha, x_ptr, rows, C, Cs, y_ptr=0):
    a = K.ActArgs()
    a.x, a.y = x_ptr, y_ptr
    a.rows, a.C, a.Cs = rows, C, Cs
    a.act, a.alpha = K.ACT_CODES[name], alpha
    return a


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _check_values(got_bits, want64, what):
    """got (bf16 bits) against the float64 oracle: NaN where the oracle is NaN; magnitude <= 2^-126
    and not the opposite sign where the oracle is below 2^-126; inf where it is inf; else within
    1 bf16 ulp of the oracle rounded to bf16."""
    got_bits, want64 = np.asarray(got_bits).reshape(-1), np.asarray(want64, np.float64).reshape(-1)
    got = O.bf16_values(got_bits).astype(np.float64)
    nan = np.isnan(want64)
    assert np.all(O.is_nan_bits(got_bits[nan])), what
    assert not np.any(O.is_nan_bits(got_bits[~nan])), what
    tiny = ~nan & (np.abs(want64) < TINY)
    assert np.all(np.abs(got[tiny]) <= TINY) and np.all(got[tiny] * want64[tiny] >= 0), what
    inf = ~nan & np.isinf(want64)
    assert np.array_equal(got[inf], want64[inf]), what
    rest = ~nan & ~tiny & ~inf
    d = np.abs(O.ordinal(got_bits[rest]) - O.ordinal(O.to_bf16_bits(want64[rest])))
    assert d.max(initial=0) <= 1, (what, int(d.max()), int((d > 1).sum()))
    return int(d.max(initial=0))


# ------------------------------------------------------------------------------------ 1. forward, exhaustive
@pytest.mark.parametrize("name,alpha", O.CASES)
def test_forward_all_bf16_inputs(name, alpha):
    K = _K()
    bits, x = O.all_bf16()
    buf = _bf16(bits)
    K.act_fwd(_args(K, name, alpha, buf.data_ptr(), 8192, 8, 8), _stream())
    torch.cuda.synchronize()
    got = O.bits_of(buf)
    with np.errstate(invalid="ignore"):                        # (signalling NaN patterns among the inputs)
        want = O.act(name, alpha, x.astype(np.float64))
    worst = _check_values(got, want, name)
    print("%s alpha %g: worst %d ulp" % (name, alpha, worst))
    # the limits at +-inf
    lo, hi = O.act(name, alpha, np.array([-np.inf, np.inf]))
    gv = O.bf16_values(got).astype(np.float64)
    for b, lim in ((0xFF80, lo), (0x7F80, hi)):
        assert gv[b] == lim or abs(O.ordinal(got[b]) - O.ordinal(O.to_bf16_bits(lim))) <= 1, (name, b, gv[b], lim)
    # non-decreasing over the sorted finite inputs
    fin = np.isfinite(x)
    order = np.argsort(x[fin], kind="stable")
    assert np.all(np.diff(O.ordinal(got[fin][order])) >= 0), name


# ------------------------------------------------------------------------------------ 2. forward, layout and dropout
def _ragged(C, off, seed):
    """(whole buffer's bits [N], payload slice, real-channel mask [rows, Cs]) of a [37, Cs] stage
    buffer that starts ``off`` elements into a sentinel-filled allocation."""
    rows, Cs = 37, -(-C // 8) * 8
    n = off + rows * Cs + 64
    bits = (np.arange(n, dtype=np.int64) * 7919 + 0x1234) & 0x7F7F           # finite sentinels
    rs = np.random.RandomState(seed)
    xs = O.to_bf16_bits(rs.randn(rows, C) * 2.0)
    pay = bits[off:off + rows * Cs].reshape(rows, Cs)
    pay[:, :C] = xs
    real = np.zeros((rows, Cs), bool)
    real[:, :C] = True
    return bits, slice(off, off + rows * Cs), real, rows, Cs


@pytest.mark.parametrize("name,alpha", O.CASES)
def test_forward_layout_and_dropout(name, alpha):
    K = _K()
    rate, seed, stream_id = 0.25, 1234567, 3
    thr, scale = dropout_pair(rate)
    st = torch.zeros(K.STEP_STATE_BYTES, dtype=torch.uint8, device="cuda")
    for C in (5, 12, 20):
        for off in (0, 8):                                # 0 and 16 bytes
            bits, sl, real, rows, Cs = _ragged(C, off, seed=C + off)
            x64 = O.bf16_values(bits[sl]).astype(np.float64).reshape(rows, Cs)
            a64 = O.act(name, alpha, x64)
            for step in (None, 1, 77):
                buf = _bf16(bits)
                a = _args(K, name, alpha, buf.data_ptr() + 2 * off, rows, C, Cs)
                keep = np.ones((rows, C), bool)
                if step is not None:
                    st.view(torch.int32)[0] = step
                    a.drop_thr, a.drop_scale, a.seed, a.stream_id, a.st = thr, scale, seed, stream_id, st.data_ptr()
                    keep = dropout_keep(rows * C, rate, seed, stream_id, step).numpy().reshape(rows, C)
                    assert 0.6 < keep.mean() < 0.9
                K.act_fwd(a, _stream())
                torch.cuda.synchronize()
                got = O.bits_of(buf)
                out = got[sl].reshape(rows, Cs)
                # pad channels and everything outside the buffer: bit for bit as they were
                assert np.array_equal(got[:sl.start], bits[:sl.start]) and np.array_equal(got[sl.stop:], bits[sl.stop:])
                assert np.array_equal(out[~real], bits[sl].reshape(rows, Cs)[~real]), (name, C, off)
                o = out[:, :C]
                assert np.all(o[~keep] == 0), (name, C, off, step)                   # dropped: +0
                sc = float(np.float32(scale)) if step is not None else 1.0
                _check_values(o[keep], a64[:, :C][keep] * sc, (name, C, off, step))
                if step is not None:         # the kept set is dropout_keep's: a kept non-zero value is not zero
                    nz = np.abs(a64[:, :C]) > 1e-30
                    assert np.all((o != 0)[keep & nz])
                # a second launch from the same input is bit-identical
                buf2 = _bf16(bits)
                a.x = buf2.data_ptr() + 2 * off
                K.act_fwd(a, _stream())
                torch.cuda.synchronize()
                assert torch.equal(buf.view(torch.int16), buf2.view(torch.int16))


# ------------------------------------------------------------------------------------ 3. backward
@pytest.mark.parametrize("name,alpha", O.CASES)
def test_backward_all_bf16_outputs(name, alpha):
    K = _K()
    bits, yp = O.all_bf16()
    ybuf = _bf16(bits)
    lo, hi = O.out_range(name, alpha)
    for rate in (0.0, 0.25):
        ys = np.float32(1.0 - rate)
        g = torch.ones(8192, 8, dtype=torch.bfloat16, device="cuda")
        a = _args(K, name, alpha, g.data_ptr(), 8192, 8, 8, ybuf.data_ptr())
        a.y_scale = float(ys)
        K.act_bwd(a, _stream())
        torch.cuda.synchronize()
        got = O.bits_of(g).reshape(-1)
        gv = O.bf16_values(got).astype(np.float64)
        with np.errstate(invalid="ignore"):
            y = (yp * ys).astype(np.float64)                   # fp32 product, as the kernel forms it
        ok = ~np.isnan(y)
        assert np.all(np.isfinite(gv[ok])) and np.all(gv[ok] >= 0), (name, rate)
        inr = ok & (y >= lo) & (y <= hi)
        worst = _check_values(got[inr], O.act_grad_from_output(name, alpha, y[inr]), (name, rate))
        print("%s alpha %g rate %g: %d outputs in range, worst %d ulp" % (name, alpha, rate, int(inr.sum()), worst))
    assert torch.equal(ybuf.view(torch.int16), _bf16(bits).view(torch.int16))      # the saved output is read only


@pytest.mark.parametrize("name,alpha", O.CASES)
def test_backward_layout(name, alpha):
    K = _K()
    for C in (5, 12, 20):
        for off in (0, 8):
            for rate in (0.0, 0.25):
                gbits, sl, real, rows, Cs = _ragged(C, off, seed=100 + C + off)
                ybits, _, _, _, _ = _ragged(C, off, seed=200 + C + off)
                # saved outputs from the function's range, carrying the dropout scale
                xs = O.bf16_values(ybits[sl]).astype(np.float64).reshape(rows, Cs)[:, :C]
                sc = float(np.float32(1.0 / (1.0 - rate)))
                ypay = ybits[sl].reshape(rows, Cs)
                ypay[:, :C] = O.to_bf16_bits(O.act(name, alpha, xs) * sc).reshape(rows, C)
                g, y = _bf16(gbits), _bf16(ybits)
                a = _args(K, name, alpha, g.data_ptr() + 2 * off, rows, C, Cs, y.data_ptr() + 2 * off)
                a.y_scale = float(np.float32(1.0 - rate))
                K.act_bwd(a, _stream())
                torch.cuda.synchronize()
                got = O.bits_of(g)
                assert np.array_equal(got[:sl.start], gbits[:sl.start]) and np.array_equal(got[sl.stop:], gbits[sl.stop:])
                out = got[sl].reshape(rows, Cs)
                assert np.array_equal(out[~real], gbits[sl].reshape(rows, Cs)[~real])
                assert np.array_equal(O.bits_of(y), ybits)
                y32 = O.bf16_values(ypay[:, :C]) * np.float32(1.0 - rate)
                g64 = O.bf16_values(gbits[sl]).astype(np.float64).reshape(rows, Cs)[:, :C]
                _check_values(out[:, :C], g64 * O.act_grad_from_output(name, alpha, y32.astype(np.float64)),
                              (name, C, off, rate))


# ------------------------------------------------------------------------------------ 4. launcher checks
def test_launcher_host_checks():
    K = _K()
    buf = torch.zeros(64, 16, dtype=torch.bfloat16, device="cuda")
    y = torch.zeros(64, 16, dtype=torch.bfloat16, device="cuda")
    p, q = buf.data_ptr(), y.data_ptr()

    def bad(fn, **kw):
        a = _args(K, "tanh", 0.0, p, 64, 12, 16, q)
        for k, v in kw.items():
            setattr(a, k, v)
        with pytest.raises(ValueError):
            fn(a, _stream())
    for fn in (K.act_fwd, K.act_bwd):
        bad(fn, act=0)
        bad(fn, act=99)
        bad(fn, Cs=12)
        bad(fn, Cs=0)
        bad(fn, C=17)
        bad(fn, C=0)
        bad(fn, x=0)
        bad(fn, x=p + 2)
        bad(fn, rows=-1)
        bad(fn, act=K.ACT_CODES["leaky_relu"], alpha=-0.1)
        bad(fn, act=K.ACT_CODES["elu"], alpha=float("nan"))
    bad(K.act_bwd, y=0)
    bad(K.act_bwd, y=q + 4)
    bad(K.act_bwd, y_scale=0.0)
    K.act_fwd(_args(K, "tanh", 0.0, p, 0, 12, 16), _stream())          # no rows: nothing to launch
    K.act_fwd(_args(K, "tanh", 0.0, p, 64, 12, 16), _stream())
    K.act_bwd(_args(K, "tanh", 0.0, p, 64, 12, 16, q), _stream())
    torch.cuda.synchronize()
    assert float(buf.float().abs().sum()) == 0.0
    assert sorted(K.ACT_CODES) == sorted(["leaky_relu"] + list(O.STRINGS))


# ------------------------------------------------------------------------------------ 5. twin: LeakyReLU(0) is relu
def _names(m, bs, mode="train"):
    return [l.name for l in m._executor._plans[(bs, mode)].launches]


@pytest.mark.parametrize("kind", ["tiny", "odd"])
def test_leaky_relu_zero_equals_the_relu_twin(kind, monkeypatch):
    """LeakyReLU(alpha=0) through the activation launches against activation="relu" through the
    fused epilogues and BwdThrough, both in the per-layer structure: losses and every weight after
    2 SGD steps are equal as floats, and the launch lists differ by the act_* launches only --
    which pins where each of the four kinds of launch sits, with no tolerance."""
    res = []
    for act, tv in ((("LeakyReLU", 0.0), ""), ("relu", PERLAYER)):
        monkeypatch.setenv("INTML_TUNE", tv)
        set_random_seed(11)
        m = M.build(kind, optim.SGD(lr=0.05), "cuda", drop=0.0, act=act)
        if res:
            m.set_weights(res[0][3])
        w0 = m.get_weights()
        x, y = _data(m, 64, seed=3)
        ex = m._executor
        d = ex.upload(x, y)
        ex.reset_metrics()
        losses = []
        for t in range(2):
            ex.train_step(d, torch.arange(d.n, device=ex.device), 32 * t, 32)
            torch.cuda.synchronize()
            losses.append(tuple(ex._metrics()))
        n = m.store.numel
        res.append((losses, m.store.master[:n].cpu().numpy(), _names(m, 32), w0))
    (la, wa, na, w0), (lb, wb, nb, _) = res
    assert la == lb, (la, lb)
    assert np.array_equal(wa, wb)
    assert not np.array_equal(wa, np.concatenate([w.reshape(-1) for w in w0]))
    acts = [nm for nm in na if nm.startswith("act_")]
    assert len(acts) == 8 and not [nm for nm in nb if nm.startswith("act_")], (na, nb)
    assert [nm for nm in na if not nm.startswith("act_")] == nb, (na, nb)
    # each act_bwd sits directly behind the launch that stored its gradient buffer
    for i, nm in enumerate(na):
        if nm.startswith("act_bwd_"):
            prev = na[i - 1]
            assert prev == "head" or prev.startswith(("dense_dx", "dense_bwd", "dgrad_conv", "wgrad_dgrad_conv")), na
        if nm.startswith("act_fwd_"):
            assert na[i - 1].startswith(("conv_fwd", "dense_epi")), na


# ------------------------------------------------------------------------------------ 6. end to end
def _pair(kind, act, mk, drop=0.2):
    set_random_seed(1234)
    g = M.build(kind, mk(), "cuda", drop=drop, act=act)
    set_random_seed(1234)
    c = M.build(kind, mk(), "cpu", drop=drop, act=act)
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
@pytest.mark.parametrize("act", E2E, ids=_ids)
def test_three_adam_steps_track_the_cpu_reference(act, kind):
    """tests/test_hip_model.py::test_multiple_steps_track_reference's bound (relative L2 error of
    all weights < 1e-2) for every activation, dropout 0.2; the CPU executor activates before it
    pools (Keras' order), the GPU after."""
    g, c = _pair(kind, act, optim.Adam)
    x, y = _data(g, 96, seed=3)
    w0 = g.store.master[:g.store.numel].cpu().numpy()
    wg, wc = _three_steps(g, c, x, y)
    print("%s %s: rel err %.3g, moved %.3g" % (_ids(act), kind, _rel(wg, wc), _rel(wg, w0)))
    assert _rel(wg, wc) < 1e-2
    names = _names(g, 32)
    assert len([n for n in names if n.startswith("act_fwd_")]) == 4 == len([n for n in names if n.startswith("act_bwd_")])
    arena = g._executor.arena.clone()                  # the packs mirror the master
    g._executor.params_changed()
    torch.cuda.synchronize()
    assert torch.equal(arena, g._executor.arena)


@pytest.mark.parametrize("kind", ["tiny", "odd"])
@pytest.mark.parametrize("act", E2E, ids=_ids)
def test_grads_match_the_bf16_reference(act, kind, monkeypatch):
    """tests/test_hip_model.py::test_grads_match_bf16_reference's standard (per tensor: relative
    error < 5e-2, cosine > 0.995) against the CPU executor with the GPU's bf16 storage points."""
    monkeypatch.setenv("INTML_TUNE", "ref_bf16=1")
    g, c = _pair(kind, act, lambda: optim.SGD(lr=0.0))
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
        a, b = gg[s.offset:s.offset + s.numel], cg[s.offset:s.offset + s.numel]
        err = _rel(a, b)
        cos = float(np.dot(a, b) / max(np.linalg.norm(a) * np.linalg.norm(b), 1e-30))
        worst.append((err, cos, s.name))
    print("%s %s: worst grad rel err %.3g (cos %.6f) at %s" % ((_ids(act), kind) + max(worst)))
    for err, cos, nm in worst:
        assert err < 5e-2 and cos > 0.995, "%s: grad rel err %.3g cos %.6f" % (nm, err, cos)
    lg, lc = g._executor.read_metrics()[0], c._executor.read_metrics()[0]
    assert abs(lg - lc) < 1e-3 * max(1.0, abs(lc)), (lg, lc)


# ------------------------------------------------------------------------------------ 7. pool order
@pytest.mark.parametrize("act", ["tanh", "sigmoid"])
def test_pooling_before_activating_equals_keras_order(act):
    """Every conv of the tiny model is pooled.  The reference here is an independently written
    autograd model that activates and THEN pools; the CPU executor must agree with it in fp32, and
    the GPU (which pools the linear conv, then activates) must track it within test 6's bound."""
    g, c = _pair("tiny", act, optim.Adam)
    x, y = _data(g, 96, seed=3)
    wg, wc = _three_steps(g, c, x, y)
    print("%s: rel err %.3g" % (act, _rel(wg, wc)))
    assert _rel(wg, wc) < 1e-2
    set_random_seed(1234)
    c1 = M.build("tiny", optim.SGD(lr=0.0), "cpu", drop=0.2, act=act)
    assert c1._seed == c._seed
    ex = c1._executor
    d = ex.upload(x, y)
    ex.train_step(d, torch.arange(d.n), 0, 32)
    got = [c1.store.view(l, n, grad=True).numpy() for l in c1.layers for n, _, _ in l.weight_specs()]
    _, want = M.torch_loss_grads(c1, x[:32], y[:32], step=1)
    for a, b in zip(got, want):
        assert np.linalg.norm(a - b) <= 1e-4 * np.linalg.norm(b) + 1e-7


# ------------------------------------------------------------------------------------ 8. eval / predict
@pytest.mark.parametrize("kind,act", [("tiny", "tanh"), ("odd", ("ELU", 0.5)), ("odd", "softsign")])
def test_predict_and_evaluate_match(kind, act):
    g, c = _pair(kind, act, optim.Adam)
    x, y = _data(g, 77, seed=5)
    pg, pc = g.predict(x, batch_size=32), c.predict(x, batch_size=32)
    assert pg.shape == pc.shape and np.abs(pg - pc).max() < 2e-2
    eg, ec = g.evaluate(x, y, batch_size=32, verbose=0), c.evaluate(x, y, batch_size=32, verbose=0)
    assert abs(eg[0] - ec[0]) < 2e-2 * max(1, ec[0])
    plans = g._executor._plans
    modes = {k[1] for k in plans}
    assert {"eval", "predict"} <= modes
    for k, p in plans.items():
        names = [l.name for l in p.launches]
        assert len([n for n in names if n.startswith("act_fwd_")]) == 4 and not [n for n in names if "act_bwd" in n]
        assert all(l.args["act"].drop_thr == 0 for l in p.launches if l.name.startswith("act_fwd_"))


# ------------------------------------------------------------------------------------ 9. graph replay
def test_graph_of_8_steps_equals_8_single_steps():
    res = []
    for chunks in ([1] * 8, [8]):
        set_random_seed(21)
        m = M.tiny(optim.Adam(decay=0.01), device="cuda", drop=0.2, act="tanh")
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
                    ex._metrics(), int(m.optimizer.iterations)))
    for a, b in zip(res[0][0], res[1][0]):
        assert torch.equal(a, b)
    assert res[0][1] == res[1][1] and res[0][1][2] == 256 and res[0][2] == res[1][2] == 8


# ------------------------------------------------------------------------------------ 10. gating
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


def test_conv_activation_leaves_the_fused_stack(monkeypatch):
    from cori_intml_examples_amd.apps import zoo
    monkeypatch.delenv("INTML_TUNE", raising=False)
    set_random_seed(57)
    m = zoo.rpv_cnn((64, 64, 3), conv_sizes=[16, 32, 64], fc_sizes=[128], dropout=0.2, optimizer="Adam", lr=1e-3,
                    device="cuda", activation="tanh")
    names = _plan_names(m)
    for mode in names:
        assert "conv_stack_fwd" not in names[mode] and "prologue" in names[mode]
        assert [n for n in names[mode] if n.startswith("act_fwd_")] == ["act_fwd_c0", "act_fwd_c1", "act_fwd_c2", "act_fwd_d0"]
    assert [n for n in names["train"] if n.startswith("act_bwd_")] == ["act_bwd_d0", "act_bwd_c2", "act_bwd_c1", "act_bwd_c0"]
    assert "dense_epi0" in names["train"]              # the head does not run the last dense's epilogue
    assert not m._executor._plans[(128, "train")].pro_free
    # ... the per-layer relu structure plus the eight launches
    monkeypatch.setenv("INTML_TUNE", PERLAYER)
    set_random_seed(57)
    u = zoo.rpv_cnn((64, 64, 3), conv_sizes=[16, 32, 64], fc_sizes=[128], dropout=0.2, optimizer="Adam", lr=1e-3,
                    device="cuda")
    un = _plan_names(u)
    for mode in names:
        assert [n for n in names[mode] if not n.startswith("act_")] == un[mode], mode


def test_dense_activation_keeps_the_stack_and_the_prologue_free_step(monkeypatch):
    from cori_intml_examples_amd.models import Conv2D, Dense, Dropout, Flatten, Input, MaxPooling2D, Model
    monkeypatch.delenv("INTML_TUNE", raising=False)
    set_random_seed(57)
    inp = Input(shape=(64, 64, 3))
    h = inp
    for c in (16, 32, 64):
        h = MaxPooling2D((2, 2))(Conv2D(c, (3, 3), activation="relu", padding="same")(h))
    h = Flatten()(Dropout(0.2)(h))
    h = Dropout(0.2)(Dense(128, activation="tanh")(h))
    m = Model(inp, Dense(1, activation="sigmoid")(h), device="cuda")
    m.compile(optimizer=optim.Adam(lr=1e-3), loss="binary_crossentropy", metrics=["accuracy"])
    names = _plan_names(m)
    plan = m._executor._plans[(128, "train")]
    assert plan.pro_free and "prologue" not in names["train"] and names["train"][0] == "conv_stack_fwd"
    assert [n for n in names["train"] if n.startswith("act_")] == ["act_fwd_d0", "act_bwd_d0"]
    i = names["train"].index("act_fwd_d0")
    assert names["train"][i - 1] == "dense_epi0" and names["train"][i + 1] == "head"
    assert names["train"][names["train"].index("act_bwd_d0") - 1] == "head"


def test_relu_plans_are_unchanged(monkeypatch):
    """The "nothing changed" claim: the default builders and activation="relu" record exactly the
    same launch lists, with no act_* launch, the early reduction and the fused optimizer."""
    from cori_intml_examples_amd.apps import zoo
    monkeypatch.delenv("INTML_TUNE", raising=False)
    set_random_seed(57)
    absent = _build("rpv_bench", "cuda", opt="Adam", drop=0.2, cin=3, hw=64)
    ref = _plan_names(absent)
    plan = absent._executor._plans[(128, "train")]
    assert plan.early_red and plan.optim_fused and plan.pro_free
    assert not [nm for mode in ref for nm in ref[mode] if nm.startswith("act_")]
    assert ref["train"][0] == "conv_stack_fwd" and "dense_epi0" not in ref["train"]
    set_random_seed(57)
    relu = zoo.rpv_cnn((64, 64, 3), conv_sizes=[16, 32, 64], fc_sizes=[128], dropout=0.2, optimizer="Adam", lr=1e-3,
                       device="cuda", activation="relu")
    assert _plan_names(relu) == ref
    p2 = relu._executor._plans[(128, "train")]
    assert p2.early_red and p2.optim_fused


# ------------------------------------------------------------------------------------ 11. data parallel
def test_data_parallel_step_at_one_rank(tmp_path):
    out = tmp_path / "dp.json"
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("WORLD_SIZE", "RANK", "INTML_DP_BACKEND", "INTML_COMM", "INTML_XGMI", "INTML_TUNE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "act_dp_worker_gpu.py"), str(out)],
                       env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rep = json.load(open(out))
    print(json.dumps(rep, indent=1))
    assert rep["native"] and rep["moved"] > 1e-4, rep
    assert len([n for n in rep["base_launches"] if n.startswith("act_")]) == 8
    for mode in ("captured", "segmented"):
        c = rep[mode]
        assert c["reducer"] == "NativeGradReducer" and c["comm_in_graph"] == (mode == "captured"), c
        acts = [n for n in c["launches"] if n.startswith("act_")]
        assert acts == [n for n in rep["base_launches"] if n.startswith("act_")], c
        assert c["iterations"] == 4 and all(c["identical"]), (mode, c)


# ------------------------------------------------------------------------------------ 12. checkpoint
def test_gpu_checkpoint_loads_on_cpu_and_continues(tmp_path):
    from cori_intml_examples_amd.models import Conv2D, Dense, Dropout, Flatten, Input, LeakyReLU, MaxPooling2D, Model
    x, y, _ = synthetic_rpv(96, channels=3, size=16, seed=1)
    set_random_seed(8)
    inp = Input(shape=(16, 16, 3))
    h = MaxPooling2D()(LeakyReLU(0.2)(Conv2D(4, (3, 3), padding="same")(inp)))
    h = MaxPooling2D()(Conv2D(8, (3, 3), padding="same", activation="elu")(h))
    h = Flatten()(Dropout(0.1)(h))
    h = Dense(16, activation="elu")(h)
    m = Model(inp, Dense(1, activation="sigmoid")(h), device="cuda")
    m.compile(optimizer=optim.Adam(lr=0.01), loss="binary_crossentropy", metrics=["accuracy"])
    m.fit(x[:64], y[:64], batch_size=16, epochs=1, verbose=0, shuffle=False)
    p = str(tmp_path / "g.h5")
    m.save(p)
    c = load_model(p, device="cpu")
    assert c.store.master.device.type == "cpu" and c.optimizer.iterations == m.optimizer.iterations == 4
    assert [l.get_config() for l in c.layers] == [l.get_config() for l in m.layers]
    assert [(s.act, s.act_alpha) for s in c._executor.plan.convs] == [("leaky_relu", float(np.float32(0.2))), ("elu", 1.0)]
    for a, b in zip(m.get_weights(), c.get_weights()):
        np.testing.assert_array_equal(a, b)
    assert np.abs(c.predict(x[64:], batch_size=32) - m.predict(x[64:], batch_size=32)).max() < 2e-2
    n = c.store.numel
    w0 = c.store.master[:n].clone()
    lc, lg = c.train_on_batch(x[64:], y[64:]), m.train_on_batch(x[64:], y[64:])
    torch.cuda.synchronize()
    assert abs(lc[0] - lg[0]) < 2e-2 * max(1.0, lg[0])
    assert float((c.store.master[:n] - w0).abs().max()) > 1e-4
    assert _rel(m.store.master[:n].cpu().numpy(), c.store.master[:n].numpy()) < 1e-2
